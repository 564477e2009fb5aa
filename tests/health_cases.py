"""Deterministic scenes for the camera-health tests (tests/test_health_cpu.py, tests/test_gpu_health.py): a textured scene with coarse
structure, and what a covered, defocused, re-aimed, dark, dazzled or frozen camera makes of it."""
import numpy as np

#: the sequence's stretches, (what the camera shows, frames); the timers the GPU tests run it with
STRETCHES = (("healthy", 6), ("covered", 8), ("healthy", 4), ("blurred", 5), ("healthy", 4), ("shifted", 5), ("healthy", 4), ("dark", 5), ("bright", 5),
             ("healthy", 3), ("repeated", 5))
N_FRAMES = sum(n for _, n in STRETCHES)
TIMERS = dict(warmup=4, hold_frames=3, clear_frames=2, freeze_frames=3, min_ref_edges=4)


def scene(h, w, seed):
    """A flat wall with rectangles of other brightness (coarse structure, sparse enough that a shifted copy does not cover it by
    chance) under a fixed per-pixel texture of +-12 (fine detail) -> int64 (h, w, 3)."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 110, np.int64)
    for _ in range(max(3, h * w // 1600)):
        rh, rw = int(rng.integers(max(2, h // 12), max(3, h // 4) + 1)), int(rng.integers(max(2, w // 16), max(3, w // 5) + 1))
        y0, x0 = int(rng.integers(0, max(1, h - rh))), int(rng.integers(0, max(1, w - rw)))
        img[y0:y0 + rh, x0:x0 + rw] = int(rng.choice([45, 65, 170, 200]))
    img = img + rng.integers(-12, 13, (h, w))
    return np.stack([img, img + 3, img - 5], -1)


def noisy(img, rng, amp=2):
    return np.clip(img + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def box_blur(img, k=5):
    """A k x k box mean with replicated borders (integer arithmetic)."""
    r = k // 2
    p = np.pad(np.asarray(img, np.int64), ((r, r), (r, r), (0, 0)), mode="edge")
    h, w = img.shape[:2]
    acc = np.zeros(np.asarray(img).shape, np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += p[dy:dy + h, dx:dx + w]
    return (acc + k * k // 2) // (k * k)


def shifted(img):
    """The scene a camera sees after it was turned by a third of the picture's width."""
    return np.roll(img, max(1, img.shape[1] // 3), axis=1)


def covered(h, w):
    return np.full((h, w, 3), 90, np.int64)


def view(kind, base, h, w):
    return {"healthy": base, "repeated": base, "covered": covered(h, w), "blurred": box_blur(base), "shifted": shifted(base),
            "dark": np.full((h, w, 3), 5, np.int64), "bright": np.full((h, w, 3), 250, np.int64)}[kind]


def sequence(h, w, seed, stretches=STRETCHES):
    """-> (frames, kinds): uint8 (h, w, 3) frames with fresh noise of +-2 on every frame but the `repeated` ones, which repeat the
    frame before them bit for bit."""
    rng = np.random.default_rng(seed + 7)
    base = scene(h, w, seed)
    frames, kinds = [], []
    for kind, n in stretches:
        v = view(kind, base, h, w)
        for _ in range(n):
            frames.append(frames[-1] if kind == "repeated" and frames else noisy(v, rng))
            kinds.append(kind)
    return frames, kinds
