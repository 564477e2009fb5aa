from .botsort import BotSortTracker
from .crosscam import CrossCameraLinker, HandoffEvent
from .deepsort import DeepSortTracker
from .gmc import CameraMotionEstimator
from .ocsort import OcSortTracker
from .reid import ReidEmbedder
from .search import AppearanceIndex, Hit
from .swapguard import IdSwapGuard, SwapEvent
from .tracker import MultiObjectTracker, Track

__all__ = ["AppearanceIndex", "BotSortTracker", "CameraMotionEstimator", "CrossCameraLinker", "DeepSortTracker", "HandoffEvent", "Hit", "IdSwapGuard", "MultiObjectTracker", "OcSortTracker", "ReidEmbedder", "SwapEvent", "Track"]
