"""Times JpegDecoder.decode_batch on 8 x 1080p frames (structured synthetic background with +-6 levels of sensor noise): the files this
tree's own encoder writes (4:2:0, one restart interval per MCU row) at quality 95 and 85, and the same frames saved by Pillow at the
same qualities WITHOUT restart markers (one interval per frame: one GPU lane decodes it).  Per set: the kernels' HIP-event time and
the whole call into device frames (host parse, staging, upload of the files, kernels, statuses back).  Beside them, from the same run:
Pillow (libjpeg-turbo) decoding the same files on one CPU thread, and the page-locked upload of the 50 MB of raw BGR24 that the
compressed upload replaces.  Medians of 5 after 2 warm-up calls.  Every decoded batch is compared with Pillow's pixels.  Prints one
JSON line.

    python tools/jpeg_decode_time.py [--out profiles/jpegdec/jpegdec_time.json]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rtmodt_amd  # noqa: E402,F401

pkg = sys.modules["rtmodt_amd"]
N, H, W, REPS, WARM = 8, 1080, 1920, 5, 2


def stats(us):
    return {"p50": float(np.median(us)), "min": float(np.min(us)), "max": float(np.max(us))}


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    base = pkg.synth.structured_frames(N, H, W).astype(np.int16) + rng.integers(-6, 7, (N, H, W, 3), dtype=np.int16)
    frames = np.clip(base, 0, 255).astype(np.uint8)
    res = {"frames": N, "size": f"{W}x{H}", "reps": REPS, "raw_bytes": int(frames.nbytes)}

    # the yardstick the compressed upload replaces: 50 MB of BGR24 from page-locked memory
    pinned = pkg._ffi.PinnedArray(frames.shape, np.uint8)
    np.copyto(pinned.array, frames)
    dev = pkg._ffi.DeviceBuffer(frames.nbytes)
    up = []
    for _ in range(WARM + REPS):
        t0 = time.perf_counter()
        pkg._ffi.check(pkg._ffi.lib().rtmodt_memcpy_h2d(0, C.c_void_p(dev.ptr), C.c_void_p(pinned.ptr), frames.nbytes))
        up.append((time.perf_counter() - t0) * 1e6)
    res["raw_pinned_upload_us"] = stats(up[WARM:])

    dec = pkg.JpegDecoder(max_height=H, max_width=W, max_batch=N, max_file_bytes=4 << 20)
    ok = True
    for q in (95, 85):
        enc = pkg.JpegEncoder(q, max_height=H, max_width=W, max_batch=N)
        marked = enc.encode_batch([f for f in frames])
        enc.close()
        plain = []
        for f in frames:
            b = io.BytesIO()
            Image.fromarray(f[..., ::-1]).save(b, "JPEG", quality=q, subsampling=2, optimize=False)
            plain.append(b.getvalue())
        for name, files in (("restart_per_mcu_row", marked), ("no_restart_markers", plain)):
            wall, kern = [], []
            for _ in range(WARM + REPS):
                t0 = time.perf_counter()
                _, status = dec.decode_batch(files, out=dev, height=H, width=W)
                wall.append((time.perf_counter() - t0) * 1e6)
                kern.append(dec.last_kernel_ms() * 1e3)
            got = dev.download().reshape(N, H, W, 3)
            pil = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                want = [np.asarray(Image.open(io.BytesIO(f))) for f in files]
                pil.append((time.perf_counter() - t0) * 1e6)
            exact = bool(status.tolist() == [0] * N and all(np.array_equal(got[i], want[i][..., ::-1]) for i in range(N)))
            ok &= exact
            res[f"q{q}_{name}"] = {"kernel_us": stats(kern[WARM:]), "call_with_upload_us": stats(wall[WARM:]),
                                   "file_bytes_total": int(sum(len(f) for f in files)), "pillow_1thread_us_per_batch": stats(pil),
                                   "equals_libjpeg_turbo": exact}
    dec.close()
    dev.free()
    pinned.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
