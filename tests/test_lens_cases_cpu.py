"""CPU, restatement only: the cases of tests/lens_cases.py reach the tiles, waves, runs and kinds of pixel that
tests/test_gpu_lens_tiles.py relies on (without this a GPU test could pass on a case that never leaves the kernel's first tile or never
blends a border); the byte comparisons see each fault of the tile arithmetic the GPU tests are there for; and the restatement itself
stays inside the float64 bound the GPU test asserts of the kernel."""
import numpy as np
import pytest

import lens_cases as L
import lens_ref as R

IDS = [c.name for c in L.CASES]

# (tile columns, row bands, the most live lanes of a wave, the live lanes of a wave in the last tile column)
GEOMETRY = {
    "two_tiles_plus_1": (2, 3, 64, 1), "three_tiles_odd": (3, 3, 64, 3), "exact_tiles": (2, 2, 64, 64), "wide_260": (2, 2, 64, 1),
    "one_row": (5, 1, 64, 2), "tall": (1, 258, 2, 2), "tiny_src_1x1": (2, 2, 64, 11), "tiny_src_2x2": (2, 1, 64, 2),
    "max_width": (64, 1, 64, 64), "max_height": (1, 4096, 1, 1), "hostile_map_wide": (3, 3, 64, 3),
}


# ---------------------------------------------------------------------------------------------------------------- 1. census
@pytest.mark.parametrize("case", L.CASES, ids=IDS)
def test_case_reaches_its_tiles_and_kinds(case):
    assert L.geometry(case) == GEOMETRY[case.name]
    cs = L.census(case)
    assert len(cs) == GEOMETRY[case.name][0]
    print(f"{case.name}: (whole, partial, outside) per tile column {cs if len(cs) <= 5 else cs[:2] + ['...'] + cs[-2:]}")
    for t, got in enumerate(cs):
        need = case.promise.last if case.promise.last is not None and t == len(cs) - 1 else case.promise.each
        assert all(g >= n for g, n in zip(got, need)), (case.name, t, got, need)
    if case.promise == L.GENERIC:
        assert all(min(got) >= 8 for got in cs)


def test_cases_keep_what_their_rows_promise():
    B, oh, ow = L.BY_NAME, lambda n: L.BY_NAME[n].out[0], lambda n: L.BY_NAME[n].out[1]
    generic = [c.name for c in L.CASES if c.promise == L.GENERIC]
    assert {"three_tiles_odd", "exact_tiles", "wide_260", "tall", "hostile_map_wide"} <= set(generic)
    # two_tiles_plus_1: the second tile column is one pixel wide -- a partial run of 1 -- and holds every kind of pixel
    assert ow("two_tiles_plus_1") == L.TILE_W + 1 and min(L.census(B["two_tiles_plus_1"])[1]) >= 1
    assert ow("three_tiles_odd") % L.RUN == 1 and oh("three_tiles_odd") % L.TILE_H == 1
    assert ow("exact_tiles") % L.TILE_W == 0 and oh("exact_tiles") % L.TILE_H == 0
    # wide_260: full runs in tile 1 (260 % 4 == 0); pitch 780 is a multiple of 4 (WIDE), 781 is not
    assert ow("wide_260") % L.RUN == 0 and ow("wide_260") > L.TILE_W and B["wide_260"].dextras == (0, 1) and (3 * ow("wide_260")) % 4 == 0
    assert 7 in B["three_tiles_odd"].dextras and 9 in B["three_tiles_odd"].dextras and (3 * 521 + 9) % 4 == 0 and (3 * 521 + 7) % 4 != 0
    assert oh("one_row") == 1 and all(min(got) >= 1 for got in L.census(B["one_row"]))
    assert ow("tall") % L.RUN != 0 and ow("tall") < L.RUN * 2                                     # every row ends (and nearly begins) with a partial run
    for name in ("tiny_src_1x1", "tiny_src_2x2"):                                                 # no whole pixel anywhere: every tap blends the border
        assert sum(got[0] for got in L.census(B[name])) == 0
    # the largest extents: a tap of non-zero weight on the source's last column / row, whole pixels in nearly every tile column / row band
    for name, axis in (("max_width", 0), ("max_height", 1)):
        c = B[name]
        assert c.src[1 - axis] == c.out[1 - axis] == L.MAX_DIM == 16384
        q, inside = L.table(name)[axis], L.table(name)[2] == 0
        p0, a = q >> R.BITS, q & (R.ONE - 1)
        assert (inside & ((p0 == L.MAX_DIM - 1) | ((p0 == L.MAX_DIM - 2) & (a > 0)))).any() and (inside & (p0 <= 0)).any()
        whole, partial, outside = L.kinds(c)
        assert whole.sum() >= 8 and partial.sum() >= 8 and outside.sum() >= 8
        bands = whole.reshape(3, 64, 256).any(axis=(0, 2)) if axis == 0 else whole.reshape(4096, 4, 3).any(axis=(1, 2))
        assert bands.sum() >= 0.9 * len(bands) and not bands.all()                                # ... and the outermost ones are all border
        assert c.src[0] * c.src[1] * 3 < 150 * 1024
    # hostile map: NaN and both infinities in EVERY tile column, +-2^20 in the first two (the third is 9 pixels wide), all OUTSIDE;
    # ordinary pixels of every kind beside them (the census)
    c = B["hostile_map_wide"]
    mx, my = c.map
    o = L.table(c.name)[2]
    for at in range(0, c.out[1], L.TILE_W):
        sl = np.s_[:, at:at + L.TILE_W]
        limits = (lambda a: a == np.float32(2.0 ** 20), lambda a: a == np.float32(-2.0 ** 20)) if at < 2 * L.TILE_W else ()
        for bad in (np.isnan, np.isposinf, np.isneginf) + limits:
            hit = bad(mx[sl]) | bad(my[sl])
            assert hit.any() and o[sl][hit].all(), at


# ---------------------------------------------------------------------------------------------------------------- 2. mutations
def content(case):
    return L.random_frames(1, case.src, 900 + case.out[1])[0]


@pytest.mark.parametrize("name", ["three_tiles_odd", "exact_tiles", "two_tiles_plus_1", "one_row", "wide_260"])
def test_emulation_without_a_fault_is_the_restatement(name):
    case = L.BY_NAME[name]
    frame = content(case)
    assert np.array_equal(L.emulate(case, frame), L.expected_buffer(case, frame))


# Where a fault cannot show, by arithmetic and whatever the content: a square grid of tiles (3 x 3, 2 x 2) is only permuted by the swap
# of the row band and the tile column, every tile is still made once and right; an out_w that is a multiple of 4 has a table stride of
# out_w and no partial run.  Those pairs are asserted to be the identity, so that nobody counts on them; every fault is seen on
# three_tiles_odd or, the swap, on the cases whose grid is not square (two_tiles_plus_1: 2 x 3, one_row: 5 x 1).
SEEN = [(m, "three_tiles_odd") for m in L.MUTATIONS if m != "band_swapped"] + [("tile_ignored", "exact_tiles"), ("wide_swapped", "exact_tiles"),
        ("band_swapped", "two_tiles_plus_1"), ("band_swapped", "one_row")]
BLIND = [("band_swapped", "three_tiles_odd"), ("band_swapped", "exact_tiles"), ("stride_out_w", "exact_tiles"), ("full_last_run", "exact_tiles")]


@pytest.mark.parametrize("fault,name", SEEN, ids=[f"{m}-{n}" for m, n in SEEN])
def test_byte_comparison_sees_tile_faults(fault, name):
    case = L.BY_NAME[name]
    frame = content(case)
    want, got = L.expected_buffer(case, frame), L.emulate(case, frame, fault)
    wrong = np.flatnonzero(want != got)
    print(f"{fault} on {name}: {len(wrong)} bytes differ, the first at {wrong[:1].tolist()}")
    assert len(wrong) >= 1
    if fault == "full_last_run":                                                                  # seen through the guard bytes alone
        assert (want[wrong] == L.SENT).all()


@pytest.mark.parametrize("fault,name", BLIND, ids=[f"{m}-{n}" for m, n in BLIND])
def test_faults_these_geometries_cannot_show(fault, name):
    case = L.BY_NAME[name]
    tiles_x, bands = L.geometry(case)[:2]
    assert tiles_x == bands if fault == "band_swapped" else case.out[1] % L.RUN == 0
    frame = content(case)
    assert np.array_equal(L.emulate(case, frame, fault), L.expected_buffer(case, frame))


def test_every_mutation_is_seen_on_a_case_the_gpu_runs():
    assert {m for m, _ in SEEN} == set(L.MUTATIONS) and {n for _, n in SEEN} <= set(IDS)
    assert {"three_tiles_odd", "exact_tiles"} <= {n for _, n in SEEN}


# ---------------------------------------------------------------------------------------------------------------- 3. float64 bound
FLOAT64_CASES = ("three_tiles_odd", "wide_260", "exact_tiles")


@pytest.mark.parametrize("name", FLOAT64_CASES)
def test_restatement_stays_inside_the_float64_bound(name):
    case = L.BY_NAME[name]
    frame, G = L.smooth_frame(case.src)
    assert G == 7
    out = R.sample(frame, L.table(name), L.BORDER)
    worst, n_inner, n_off = L.float64_check(case.lens, case.src, case.out, frame, G, out, L.BORDER)
    print(f"{name}: worst {worst:.4f} over {n_inner} inner pixels, bound {L.float64_bound(G):.4f}; {n_off} pixels off the source")
    assert n_inner >= 500 and n_off >= 100
    inner = L.float64_reference(case.lens, case.src, case.out, frame)[1]
    for t in range(L.geometry(case)[0]):                                                          # inner pixels in every tile column
        assert inner[:, t * L.TILE_W:(t + 1) * L.TILE_W].sum() >= 8


@pytest.mark.parametrize("lens", R.LENSES)
def test_restatement_stays_inside_the_float64_bound_for_every_lens(lens):
    for src, out, sx, sy in (((11, 300), (9, 521), 0.62, 1.9), ((13, 523), (6, 260), 1.9, 4.3), ((23, 37), (5, 257), 0.15, 4.0)):
        m = L.axis_lens(lens, src, out, sx, sy)
        frame, G = L.smooth_frame(src)
        out_px = R.sample(frame, R.build_model(m, src, out), L.BORDER)
        worst, n_inner, _ = L.float64_check(m, src, out, frame, G, out_px, L.BORDER)
        print(f"{lens} {src} -> {out}: worst {worst:.4f} over {n_inner} pixels, bound {L.float64_bound(G):.4f}")
        assert n_inner >= 100


def test_float64_check_sees_a_wrong_position():
    """A table moved by one fractional step (1 / 32 pixel) in x stays inside the bound only by luck: moved by a whole pixel it does not."""
    case = L.BY_NAME["three_tiles_odd"]
    frame, G = L.smooth_frame(case.src)
    qx, qy, o = L.table(case.name)
    out = R.sample(frame, (np.where(o == 0, qx + R.ONE, 0), qy, o), L.BORDER)
    with pytest.raises(AssertionError):
        L.float64_check(case.lens, case.src, case.out, frame, G, out, L.BORDER)
