from .detector import Detections, Detector
from .sliced import SlicedDetector

__all__ = ["Detector", "Detections", "SlicedDetector"]
