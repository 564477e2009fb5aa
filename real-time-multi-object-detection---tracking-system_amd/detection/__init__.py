from .detector import Detections, Detector
from .left_objects import LeftObjectDetector, LeftObjectEvent, LeftObjectResult
from .motion import MotionDetector, MotionResult
from .sliced import SlicedDetector

__all__ = ["Detector", "Detections", "SlicedDetector", "MotionDetector", "MotionResult", "LeftObjectDetector", "LeftObjectEvent", "LeftObjectResult"]
