#!/bin/bash
# The measurements of profiles/yuv420/README.md, one GPU step each under its own time limit, stopping at the first failure:
#   bash tools/yuv420_measure.sh [outdir]
# (host-fed and HBM-resident A/Bs alternate BGR24 and NV12 inside one process; the kernel times come from rocprofv3 kernel traces,
#  one run per source size, in runs of their own)
set -u
O=${1:-/tmp/rtmodt_yuv420}
mkdir -p "$O"
export TMPDIR=${TMPDIR:-/tmp}
timeout -k 10 500 python tools/yuv420_ab.py --leg host > "$O/leg_host_1080p.json" &&
timeout -k 10 500 python tools/yuv420_ab.py --leg hbm > "$O/leg_hbm_640.json" &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/k1080" -- \
    python tools/yuv420_ab.py --leg kernel --src 1080x1920 --steps 20 --warmup 3 > "$O/kernel_leg_1080p.json" &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/k640" -- \
    python tools/yuv420_ab.py --leg kernel --src 640x640 --steps 20 --warmup 3 > "$O/kernel_leg_640.json" || exit 1
rm -f "$O"/k1080/*/*_kernel_trace.csv "$O"/k640/*/*_kernel_trace.csv
grep -h letterbox "$O"/k1080/*/*_kernel_stats.csv "$O"/k640/*/*_kernel_stats.csv
