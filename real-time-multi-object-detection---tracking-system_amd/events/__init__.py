from .colours import ColourAttributes, TrackColours
from .crossing import CrossingCounter, CrossingEvent
from .speed import SpeedEstimator, SpeedEvent
from .zone_engine import Zone, ZoneEvent, ZoneEventEngine

__all__ = ["ZoneEventEngine", "ZoneEvent", "Zone", "CrossingCounter", "CrossingEvent", "SpeedEstimator", "SpeedEvent", "ColourAttributes", "TrackColours"]
