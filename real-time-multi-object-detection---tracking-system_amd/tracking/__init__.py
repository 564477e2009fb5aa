from .botsort import BotSortTracker
from .deepsort import DeepSortTracker
from .gmc import CameraMotionEstimator
from .ocsort import OcSortTracker
from .reid import ReidEmbedder
from .swapguard import IdSwapGuard, SwapEvent
from .tracker import MultiObjectTracker, Track

__all__ = ["BotSortTracker", "CameraMotionEstimator", "DeepSortTracker", "IdSwapGuard", "MultiObjectTracker", "OcSortTracker", "ReidEmbedder", "SwapEvent", "Track"]
