from .deepsort import DeepSortTracker
from .reid import ReidEmbedder
from .swapguard import IdSwapGuard, SwapEvent
from .tracker import MultiObjectTracker, Track

__all__ = ["DeepSortTracker", "IdSwapGuard", "MultiObjectTracker", "ReidEmbedder", "SwapEvent", "Track"]
