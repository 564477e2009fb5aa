"""CPU: the scenarios of tests/grid_limit_cases.py on the restatements alone (motion_ref, leftobj_ref, health_ref).  Every test states
the conditions under which its scenario reaches the shared code it was written for -- the second pass of ccl_scan_chunks, the cut of
ccl_emit_chunk on and inside a chunk, the links ccl_link_cell leaves to a neighbour, the reader's and the filter's tiles at 1080p and
at 32768 px -- so that an edit of a generator cannot quietly empty it.  tests/test_gpu_grid_limits.py drives the same scenarios on the
kernels."""
import numpy as np
import pytest

import grid_limit_cases as G
import health_ref as HR
import leftobj_ref as LR
import motion_ref as MR

BIG = G.geometry(G.BIG_H, G.BIG_W, 1)


def motion_on_mask(mask, h, w, **cfg):
    ref = MR.Ref(1, h, w, **cfg)
    G.motion_load(ref, ref.gh, ref.gw)
    out = ref.step(0, G.motion_frame(mask, ref.c["scale"], h, w))
    assert np.array_equal(ref.masks[0], mask)
    return out


def leftobj_on_mask(mask, h, w, **cfg):
    ref = LR.Ref(1, h, w, **cfg)
    G.lo_load_ref(ref, G.lo_model(mask, ref.c["static_frames"]))
    out = ref.step(0, G.lo_frame(mask, h, w))
    assert np.array_equal(ref.masks[0], mask)
    return out


def test_the_constants_are_the_headers():
    """geometry() restates grid_host.h's GridGeom: its constants are read out of the headers it restates."""
    import glob
    import os
    import re
    csrc = glob.glob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "*", "csrc"))[0]
    text = lambda name: open(os.path.join(csrc, name)).read()                # noqa: E731
    value = lambda name, const: int(re.search(r"\b" + const + r" = (\d+)", text(name)).group(1))      # noqa: E731
    assert value("ccl_dev.h", "CCL_CHUNK") == G.CHUNK and "(cells + 4095) / 4096" in text("grid_host.h")
    assert (value("cell_grid.h", "CG_ROWS"), value("grid_host.h", "GRID_TW"), value("grid_host.h", "GRID_TH")) == (G.READER_ROWS, G.FILTER_TW, G.FILTER_TH)
    assert value("motion_model.h", "MO_MAX_DIM") == G.MAX_SIDE
    assert "return scale >= 4 ? 1 : 4 / scale" in text("cell_grid.h") and "64 * cg_cpt(scale)" in text("cell_grid.h")


def test_the_big_grid():
    assert (BIG["gw"], BIG["gh"], BIG["cells"], BIG["n_chunks"]) == (1024, 1025, 1049600, 257)
    assert BIG["n_chunks"] > 256 and BIG["cells"] - 256 * G.CHUNK == 1024 == G.CHUNK // 4          # a second pass; the last chunk a quarter full
    assert (2 ** 20) // BIG["gw"] == 1024 and (2 ** 20) % BIG["gw"] == 0                            # cell 2^20 is cell (0, 1024)
    assert BIG["reader_tiles"] == (4, 257) and BIG["filter_tiles"] == (16, 65)


# ---------------------------------------------------------------------------------------------------------------- 1. chunk_edges
@pytest.mark.parametrize("module", ["motion", "leftobj"])
def test_chunk_edges(module):
    mask = G.edge_mask()
    limits = G.EDGE_MOTION if module == "motion" else G.EDGE_LEFTOBJ
    cuts = G.edge_cuts(**limits)
    comps = MR.components(mask)
    table = sorted((y * G.BIG_W + x, len(G.KINDS[k])) for x, y, k in G.EDGE_PIECES)
    assert [(c[0], c[1]) for c in comps] == table                            # no two pieces touch: every piece is a component of its own
    firsts = {c[0] for c in comps}
    assert {0, 4095, 4096, 2 ** 20, BIG["cells"] - 2} <= firsts and mask[-1, -1] and mask[4, 1023]
    bar = [c for c in comps if c[1] == 5][0]
    assert bar[0] // G.CHUNK == 255 and (bar[3], bar[5]) == (1020, 1024)     # the root in chunk 255, the last cell in chunk 256
    totals, per = set(), None
    for name in "abcd":
        if module == "motion":
            out = motion_on_mask(mask, G.BIG_H, G.BIG_W, scale=1, max_regions=cuts[name], **G.EDGE_MOTION, **G.MOTION_MASK_CFG)
            stored = [(r[0] + r[1] * G.BIG_W, r[4]) for r in out["regions"]]                      # at scale 1 the box's corner is the root's row
            roots_all = [c for c in comps if c[1] >= limits["min_area"]]
        else:
            out = leftobj_on_mask(mask, G.BIG_H, G.BIG_W, max_regions=cuts[name], max_objects=32, **dict(G.LO_MASK_CFG, **G.EDGE_LEFTOBJ))
            stored = [(g["root"], g["area"]) for g in out["regions"]]
            assert all((g["age_min"], g["age_max"]) == (4 + min(a), 4 + max(a)) for g in out["regions"]
                       for a in [[(x + dx + 2 * (y + dy)) % 5 for x, y, k in G.EDGE_PIECES if y * G.BIG_W + x == g["root"] for dx, dy in G.KINDS[k]]])
            roots_all = [c for c in comps if limits["min_area"] <= c[1] <= limits["max_area"]]
        qualifying = [(c[0], c[1]) for c in roots_all]
        assert qualifying == G.edge_roots(**limits)
        per = G.chunk_counts([r for r, _ in qualifying], BIG["n_chunks"])
        first = np.concatenate(([0], np.cumsum(per)))                        # what ccl_scan_chunks leaves: the rank of a chunk's first region
        assert per[255] > 0 and per[256] > 1 and per[100] > 0 and per[0] > 0 and per[1] > 0
        n = cuts[name]
        assert stored == qualifying[:n]                                      # (every piece's first cell is its box's corner)
        if name == "a":
            assert first[255] == n and per[255] > 0                          # chunk 255 has first == max_regions: it emits nothing
        elif name == "b":
            assert first[256] == n
        elif name == "c":
            assert first[256] < n < first[257]
        else:
            assert n > first[257] and len(out["regions"]) == first[257]
        totals.add(out["n_regions_total"])
    assert totals == {int(per.sum())}
    # decoys directly before and after a qualifying root, in raster order
    order = [(c[0], limits["min_area"] <= c[1] <= limits.get("max_area", 2 ** 24)) for c in comps]
    flips = sum(1 for (_, p), (_, q) in zip(order, order[1:]) if p != q)
    assert flips >= 12 and not order[-2][1] and order[-1][1]


# ---------------------------------------------------------------------------------------------------------------- 2. speckle_wide
def test_speckle_wide():
    for f in range(G.SPECKLE_FRAMES):
        mask = (G.speckle_cells(f) > G.FLAT).astype(np.uint8)
        comps = MR.components(mask)
        per = G.chunk_counts([c[0] for c in comps], BIG["n_chunks"])
        assert (per[:256] > 0).all() and len(comps) > 10000, (f, len(comps))
        for max_regions in G.SPECKLE_MAX_REGIONS:
            ref = MR.Ref(1, G.BIG_H, G.BIG_W, max_regions=max_regions, **G.SPECKLE_CFG)
            G.motion_load(ref, ref.gh, ref.gw)
            out = ref.step(0, G.MC.cells_to_frame(G.speckle_cells(f), 1, G.BIG_H, G.BIG_W))
            assert out["n_regions_total"] == len(comps) and len(out["regions"]) == max_regions and out["status"] == MR.MOTION
            assert np.array_equal(ref.masks[0], mask)


# ---------------------------------------------------------------------------------------------------------------- 3. shapes_big
@pytest.mark.parametrize("shape", G.SHAPES)
def test_shapes_big(shape):
    cells = G.big_shape(shape)
    n = int(cells.sum())
    assert n > 1000 and cells[0, 0]
    out = motion_on_mask(cells, G.BIG_H, G.BIG_W, scale=1, min_area=1, **G.MOTION_MASK_CFG)
    assert out["n_regions_total"] == 1 and out["regions"] == [(0, 0, G.BIG_W, G.BIG_H, n)] and out["n_fg"] == n
    out = leftobj_on_mask(cells, G.BIG_H, G.BIG_W, max_regions=4, max_objects=4, **G.LO_MASK_CFG)
    assert out["n_regions_total"] == 1 and len(out["regions"]) == 1
    g = out["regions"][0]
    assert (g["area"], g["age_min"], g["age_max"], g["cells"], g["box"], g["root"]) == (n, 4, 8, (0, 0, G.BIG_W - 1, G.BIG_H - 1), (0, 0, G.BIG_W, G.BIG_H), 0)
    # a full mask is a scene change under every scene_pm (1000 n_fg >= scene_pm cells); the others stay below the default 600
    assert out["status"] == (LR.SCENE_CHANGE if shape == "full" else LR.STATIC)
    assert (1000 * n >= 600 * BIG["cells"]) == (shape == "full")
    assert g["kind"] == (LR.UNKNOWN if shape == "full" else LR.ABANDONED)                        # (a full mask has no edge)
    comp = MR.components(1 - cells)
    assert len(comp) == {"spiral": 1, "comb": 512, "diagonal": 1, "full": 0}[shape]


# ---------------------------------------------------------------------------------------------------------------- 4. dense
@pytest.mark.parametrize("fill", G.FILLS)
def test_dense(fill):
    for seed in G.SEEDS:
        mask = G.dense_mask(fill, seed)
        comps = MR.components(mask)
        assert comps == MR.components_flood(mask)
        n = int(mask.sum())
        assert abs(n - fill * mask.size) < 0.01 * mask.size
        if fill in (0.42, 0.50):                                             # the regime of the 8-connected percolation threshold
            assert max(c[1] for c in comps) > n // 4 and len(comps) > 50, (fill, seed, max(c[1] for c in comps), n, len(comps))
        # cells with N and W both set: the links ccl_link_cell leaves to a neighbour
        both = int((mask[1:, 1:] & mask[:-1, 1:] & mask[1:, :-1]).sum())
        assert both > 0.8 * fill ** 3 * mask.size
        out = motion_on_mask(mask, G.MID_H, G.MID_W, **G.DENSE_MOTION)
        big = [c for c in comps if c[1] >= 2]
        assert out["n_regions_total"] == len(big) and len(out["regions"]) == min(256, len(big)) and len(big) < len(comps)
        assert out["status"] == (MR.SCENE_CHANGE if fill == 0.70 else MR.MOTION)
        lo = leftobj_on_mask(mask, G.MID_H, G.MID_W, **G.DENSE_LEFTOBJ)
        assert lo["n_regions_total"] == len(big) and [g["root"] for g in lo["regions"]] == [c[0] for c in big[:256]]
        assert lo["status"] == (LR.SCENE_CHANGE if fill == 0.70 else LR.STATIC)


# ---------------------------------------------------------------------------------------------------------------- 5. streams_big
def test_streams_big():
    mid = G.geometry(G.MID_H, G.MID_W, 1)
    assert mid["n_chunks"] == 20
    for call, streams in enumerate(G.STREAM_LISTS):
        counts = [len([c for c in MR.components(G.stream_mask_big(call, s)) if c[1] >= 2]) for s in streams]
        assert len(set(counts)) == len(counts) and min(counts) > 0, counts        # each stream of a call another region count
        counts = [len([c for c in MR.components(G.stream_mask_mid(call, s)) if c[1] >= 2]) for s in streams]
        assert len(set(counts)) == len(counts) and min(counts) > 0, counts
    assert sorted(G.STREAM_LISTS[0]) == [0, 1, 2] and G.STREAM_LISTS[0] != [0, 1, 2] and [len(l) for l in G.STREAM_LISTS] == [3, 1, 2, 3]
    # the slot of a stream in the call differs from the stream: the chunk table goes by the first, the cell state by the second
    assert all(any(i != s for i, s in enumerate(l)) for l in G.STREAM_LISTS[:3])


# ---------------------------------------------------------------------------------------------------------------- 6. production
def test_production_motion():
    geo = G.geometry(G.PROD_H, G.PROD_W, 4)
    assert (geo["gw"], geo["gh"], geo["n_chunks"], geo["reader_tiles"], geo["filter_tiles"]) == (480, 270, 32, (8, 68), (8, 17))
    assert G.PROD_PITCH == 5760 and G.PROD_PITCH % 4 == 0 and G.PROD_ODD[0] % 4 and G.PROD_ODD[1] % 4
    ref = MR.Ref(1, G.PROD_H, G.PROD_W)
    assert ref.c == MR.config()
    outs = [ref.step(0, f) for f in G.motion_frames(G.PROD_H, G.PROD_W, 1, G.MOTION_PICK)]
    W_, S_, M_ = MR.WARMUP, MR.STILL, MR.MOTION
    assert [o["status"] for o in outs] == [W_] * 8 + [S_] + [M_] * 2 + [S_] * 2
    assert [o["n_regions_total"] for o in outs] == [0] * 9 + [1, 1, 0, 0]


def test_production_motion_scale_1():
    geo = G.geometry(G.PROD_H, G.PROD_W, 1)
    assert geo["n_chunks"] == 507 and geo["reader_tiles"] == (8, 270) and geo["filter_tiles"] == (30, 68)
    ref = MR.Ref(1, G.PROD_H, G.PROD_W, **G.MOTION_SCALE1)
    outs = [ref.step(0, f) for f in G.motion_frames(G.PROD_H, G.PROD_W, 2, G.MOTION_SCALE1_PICK, low=True)]
    assert [o["status"] for o in outs] == [MR.WARMUP] * 2 + [MR.STILL, MR.MOTION, MR.STILL]
    first, second = outs[3]["regions"]                                       # one region in each pass of the scan over the chunk counts
    assert outs[3]["n_regions_total"] == 2 and (first[0] + first[1] * G.PROD_W) // G.CHUNK < 256 < (second[0] + second[1] * G.PROD_W) // G.CHUNK


def test_production_leftobj():
    ref = LR.Ref(1, G.PROD_H, G.PROD_W, **G.LEFTOBJ_PROD)
    outs = [ref.step(0, f) for f in G.leftobj_frames(G.PROD_H, G.PROD_W, 3, G.LEFTOBJ_PICK)]
    W_, C_, S_ = LR.WARMUP, LR.CLEAR, LR.STATIC
    born = G.LC.PLACE + 4
    # static static_frames after PLACE (the walker is ridden out); taken away, the cells miss twice (occlusion 2) and are lost on the third
    assert [o["status"] for o in outs] == [W_] * 4 + [C_] * (born - 4) + [S_] * 4 + [S_] * 2 + [C_] * 2
    assert [(f, e["oid"], e["kind"]) for f, o in enumerate(outs) for e in o["events"]] == [(born + 2, 1, LR.ABANDONED)]
    assert outs[-1]["n_static"] == 0 and outs[born]["n_regions_total"] == 1
    # the default configuration over the first frames: the warm-up of 8, then the block is foreground and 100 frames short of static
    ref = LR.Ref(1, G.PROD_H, G.PROD_W)
    assert ref.c == LR.config()
    outs = [ref.step(0, f) for f in G.leftobj_frames(G.PROD_H, G.PROD_W, 3, G.LEFTOBJ_PICK[:G.DEFAULT_FRAMES])]
    assert [o["status"] for o in outs] == [W_] * 8 + [C_] * 2 and outs[-1]["n_fg"] > 1000 and outs[-1]["n_static"] == 0


def test_production_health():
    cfg = dict(G.HC.TIMERS)
    ref = HR.Ref(1, G.PROD_H, G.PROD_W, **cfg)
    assert ref.c["scale"] == 4
    outs = [ref.step(0, f) for f in G.health_frames(G.PROD_H, G.PROD_W, 5)]
    events = [e for o in outs for e in o["events"]]
    assert events == [(HR.COVERED, HR.RAISED, 6), (HR.COVERED, HR.CLEARED, 9)]
    assert not any(o["raw"] & HR.NO_STRUCTURE for o in outs) and outs[-1]["active"] == 0
    # the default configuration: its warm-up of 25 frames learns from every frame, the covered ones too
    ref = HR.Ref(1, G.PROD_H, G.PROD_W)
    assert ref.c == HR.config()
    outs = [ref.step(0, f) for f in G.health_frames(G.PROD_H, G.PROD_W, 5)[:G.DEFAULT_FRAMES]]
    assert [o["learned"] for o in outs] == [HR.LEARN_SET] + [HR.LEARN_AVERAGE] * (G.DEFAULT_FRAMES - 1) and not any(o["events"] for o in outs)
    assert outs[3]["n_edge"] > 100 > outs[5]["n_edge"]


# ---------------------------------------------------------------------------------------------------------------- 7. max_side
@pytest.mark.parametrize("scale", G.SIDE_SCALES)
@pytest.mark.parametrize("h,w", G.SIDE_SHAPES)
def test_max_side(h, w, scale):
    geo = G.geometry(h, w, scale)
    long_cells = G.MAX_SIDE // scale
    assert max(geo["gh"], geo["gw"]) == long_cells and min(geo["gh"], geo["gw"]) == (4 if scale == 1 else 1)
    assert geo["n_chunks"] == (32 if scale == 1 else 1)
    if w > h:
        assert geo["reader_tiles"][0] == (128 if scale == 1 else 64) and geo["filter_tiles"][0] == long_cells // 64
    else:
        assert geo["reader_tiles"][1] == long_cells // 4 and geo["filter_tiles"][1] == long_cells // 16
    (a0, a1), (b0, b1) = G.SIDE_RECTS
    assert b1 == G.MAX_SIDE
    cpt = 1 if scale >= 4 else 4 // scale
    edges = (64 * cpt, G.FILTER_TW) if w > h else (G.READER_ROWS, G.FILTER_TH)   # the reader's and the filter's tile, in cells along the long side

    def straddles(mask, step):
        """A multiple of ``step`` with a mask cell on either side of it, along the long side."""
        line = np.asarray(mask).any(axis=0 if w > h else 1)
        m = np.arange(step, len(line), step)
        return bool((line[m - 1] & line[m]).any())
    # motion
    ref = MR.Ref(1, h, w, scale=scale, **G.SIDE_MOTION)
    outs, masks = [], []
    for f in G.side_motion_frames(h, w):
        outs.append(ref.step(0, f))
        masks.append(ref.masks[0].copy())
    assert all(straddles(masks[3], e) for e in edges) and masks[4].any(axis=0 if w > h else 1)[-1] and not any(straddles(masks[2], e) for e in edges)
    assert [o["status"] for o in outs] == [MR.WARMUP] * 2 + [MR.STILL, MR.MOTION, MR.MOTION, MR.STILL]
    box = lambda r: (r[0], r[2]) if w > h else (r[1], r[3])                 # noqa: E731
    assert [o["n_regions_total"] for o in outs[3:5]] == [1, 1]
    r0, r1 = box(outs[3]["bbox"]), box(outs[4]["bbox"])
    assert r0[0] <= a0 and r0[1] >= a1 and r1[0] <= b0 and r1[1] == G.MAX_SIDE    # (dilated by a cell; the second ends on the last pixel)
    # left objects
    ref = LR.Ref(1, h, w, scale=scale, **G.SIDE_LEFTOBJ)
    outs, last_mask = [], None
    for k, f in enumerate(G.side_leftobj_frames(h, w)):
        outs.append(ref.step(0, f))
        if k == 5:
            last_mask = ref.masks[0].copy()
    assert [o["status"] for o in outs] == [LR.WARMUP, LR.CLEAR, LR.CLEAR] + [LR.STATIC] * 3 + [LR.CLEAR] * 2
    assert [o["n_regions_total"] for o in outs[3:6]] == [2, 2, 2] and sorted(e["kind"] for o in outs for e in o["events"]) == [LR.ABANDONED] * 2
    assert box(outs[5]["regions"][1]["box"])[1] == G.MAX_SIDE
    assert all(straddles(last_mask, e) for e in edges) and last_mask.any(axis=0 if w > h else 1)[-1]
    # health
    ref = HR.Ref(1, h, w, scale=scale, **G.SIDE_HEALTH)
    outs = [ref.step(0, f) for f in G.side_health_frames(h, w)]
    events = [e[:2] for o in outs for e in o["events"]]
    if scale == 1:
        assert (HR.COVERED, HR.RAISED) in events and (HR.COVERED, HR.CLEARED) in events and not any(o["raw"] & HR.NO_STRUCTURE for o in outs)
    else:
        assert any(o["raw"] & HR.NO_STRUCTURE for o in outs)                # a grid one cell high (or wide) has no interior cell
    assert (HR.FROZEN, HR.RAISED) in events and outs[0]["n_changed"] == geo["cells"]
