from .compose import Cell, Compositor, Output
from .heatmap import Heatmap
from .jpeg import JpegEncoder, MjpegRecorder, MjpegWriter, multipart_chunk
from .privacy import PrivacyMask
from .renderer import FrameRenderer
from .snapshots import SnapshotGallery, SnapshotRetired, SnapshotUpdate

__all__ = ["FrameRenderer", "JpegEncoder", "MjpegWriter", "MjpegRecorder", "multipart_chunk", "PrivacyMask", "Heatmap", "SnapshotGallery",
           "SnapshotUpdate", "SnapshotRetired", "Compositor", "Cell", "Output"]
