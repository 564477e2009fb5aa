from .renderer import FrameRenderer

__all__ = ["FrameRenderer"]
