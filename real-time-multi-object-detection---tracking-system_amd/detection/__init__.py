from .detector import Detections, Detector
from .motion import MotionDetector, MotionResult
from .sliced import SlicedDetector

__all__ = ["Detector", "Detections", "SlicedDetector", "MotionDetector", "MotionResult"]
