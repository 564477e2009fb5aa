#!/usr/bin/env python3
"""yolov8*.pt (Ultralytics checkpoint) -> RTMODTW1 fused-weight file, without Ultralytics.
    python tools/convert_weights.py yolov8s.pt weights/yolov8s.rtw
torchreid osnet_x0_25 checkpoint (the DeepSORT embedder of config/default.yaml:60) -> RTREID01 file, without torchreid:
    python tools/convert_weights.py --reid osnet_x0_25.pth weights/osnet_x0_25.rtreid
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtmodt_amd  # noqa: E402,F401

pkg = sys.modules["rtmodt_amd"]
args = [a for a in sys.argv[1:] if a != "--reid"]
if len(args) < 2:
    sys.exit(__doc__)
if "--reid" in sys.argv[1:]:
    if not args[1].endswith(pkg.reid_weights.SUFFIX):
        sys.exit(f"the output of --reid is a {pkg.reid_weights.SUFFIX} file")
    print(f"wrote {args[1]}: OSNet x0.25, digest {pkg.reid_weights.convert_pt(args[0], args[1])}")
else:
    scale, nc = pkg.weights.convert_pt(args[0], args[1], args[2] if len(args) > 2 else None)
    print(f"wrote {args[1]}: YOLOv8{scale}, nc={nc}")
