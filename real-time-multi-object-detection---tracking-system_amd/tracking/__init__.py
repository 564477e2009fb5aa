from .deepsort import DeepSortTracker
from .tracker import MultiObjectTracker, Track

__all__ = ["DeepSortTracker", "MultiObjectTracker", "Track"]
