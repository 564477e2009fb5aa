from .deepsort import DeepSortTracker
from .reid import ReidEmbedder
from .tracker import MultiObjectTracker, Track

__all__ = ["DeepSortTracker", "MultiObjectTracker", "ReidEmbedder", "Track"]
