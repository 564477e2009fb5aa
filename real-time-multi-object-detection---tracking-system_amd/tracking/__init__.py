from .botsort import BotSortTracker
from .deepsort import DeepSortTracker
from .ocsort import OcSortTracker
from .reid import ReidEmbedder
from .swapguard import IdSwapGuard, SwapEvent
from .tracker import MultiObjectTracker, Track

__all__ = ["BotSortTracker", "DeepSortTracker", "IdSwapGuard", "MultiObjectTracker", "OcSortTracker", "ReidEmbedder", "SwapEvent", "Track"]
