"""The host-built footprint table of k_remap_lds (remap_tile_table) against what the kernel reads.

k_remap_lds stages, per 128 x 8 output tile, the source rectangle [x0a, x0a + 16 * pieces) x [y0, y0 + rows) of a table entry
with 16-byte global loads and then takes every tap from that copy.  The blended pixels stay right when an entry is wrong (the
LDS offsets are relative to the same entry), so image parity cannot see a footprint that leaves the source rows or misses a
tap; these tests can.  `read_boxes` restates, from the KERNEL (not from the table's code), which source bytes a tile's threads
read; every entry must be legal for the staging loads and must contain that set.  No GPU: orbx_debug_remap_footprints is host
code."""
import ctypes as C

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

TILE_W, TILE_H, MAX_PIECES = 128, 8, 256


def _cv_round32(m):
    """cvRound(32 * m) as the kernel does it: float product, round to nearest even, INT_MIN for NaN / out of range."""
    t = m.astype(np.float32) * np.float32(32)
    ok = np.abs(t) < 2147483648.0
    return np.where(ok, np.rint(np.where(ok, t, 0)), -2147483648).astype(np.int64)


def read_boxes(mx, my, sw, sh):
    """Bounding box (c0, c1, r0, r1: inclusive, arrays [tiles_x, tiles_y]) of the source bytes the threads of every output tile
    read.  A thread owns 4 consecutive output pixels of one row; positions past the right / bottom edge repeat the edge's map
    entry.  Per pixel: sx = clamp(cvRound(32 x) >> 5, +-2^15), the tap column clamped to [0, sw - 2], the tap rows to
    [0, sh - 1].  Per thread: bx / by = the smallest tap column / first tap row of its pixels; if (bx & ~3) + 12 <= sw it may
    read the 12-byte window from bx & ~3 on rows by .. min(by + 2, sh - 1); the byte path reads columns sxk, sxk + 1 on rows
    sy0k, sy1k of every pixel."""
    dh, dw = mx.shape
    tx_n, ty_n = (dw + TILE_W - 1) // TILE_W, (dh + TILE_H - 1) // TILE_H
    ys = np.minimum(np.arange(ty_n * TILE_H), dh - 1)
    xs = np.minimum(np.arange(tx_n * TILE_W), dw - 1)
    fsx, fsy = _cv_round32(mx[np.ix_(ys, xs)]), _cv_round32(my[np.ix_(ys, xs)])
    sx, sy = np.clip(fsx >> 5, -32768, 32767), np.clip(fsy >> 5, -32768, 32767)
    sxk = np.clip(sx, 0, sw - 2)
    sy0k, sy1k = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)

    def per_thread(a, f):   # (rows, threads) from (rows, 4 * threads)
        return f(a.reshape(a.shape[0], -1, 4), axis=2)

    bx, by = per_thread(sxk, np.min), per_thread(sy0k, np.min)
    c0, c1 = bx.copy(), per_thread(sxk, np.max) + 1          # byte reads
    r0, r1 = by.copy(), per_thread(sy1k, np.max)
    win = (bx & ~3) + 12 <= sw                                # the window
    c0 = np.where(win, np.minimum(c0, bx & ~3), c0)
    c1 = np.where(win, np.maximum(c1, (bx & ~3) + 11), c1)
    r1 = np.where(win, np.maximum(r1, np.minimum(by + 2, sh - 1)), r1)

    def per_tile(a, f):     # (tiles_x, tiles_y) from (rows, threads): 8 rows x 32 threads per tile
        return f(a.reshape(ty_n, TILE_H, tx_n, TILE_W // 4), axis=(1, 3)).T

    return per_tile(c0, np.min), per_tile(c1, np.max), per_tile(r0, np.min), per_tile(r1, np.max)


def pieces_needed(box):
    """16-byte pieces the smallest legal footprint around a tile's read set takes (two pieces per row at least)."""
    c0, c1, r0, r1 = box
    per_row = np.maximum(((c1 + 16) & ~15) - (c0 & ~15), 32) // 16
    return per_row * (r1 - r0 + 1)


def check_table(tab, mapsx, mapsy, sw, sh, what):
    assert tab is not None, "%s: no table" % (what,)
    for m in range(len(mapsx)):
        c0, c1, r0, r1 = read_boxes(mapsx[m], mapsy[m], sw, sh)
        e = tab[m].astype(np.int64)
        x0a, y0, pieces, rows, magic = e[..., 0], e[..., 1], e[..., 2], e[..., 3], e[..., 4]

        def all_tiles(cond, name):
            bad = np.argwhere(~cond)
            assert not len(bad), "%s, map %d: %s fails at tile (tx, ty) = %s: entry %s, reads columns %d..%d rows %d..%d" % (
                what, m, name, tuple(bad[0]), e[tuple(bad[0])][:5].tolist(), c0[tuple(bad[0])], c1[tuple(bad[0])],
                r0[tuple(bad[0])], r1[tuple(bad[0])])

        all_tiles(x0a >= 0, "x0a >= 0")
        all_tiles(x0a % 16 == 0, "x0a % 16 == 0")
        all_tiles(pieces >= 2, "pieces >= 2")
        all_tiles(x0a + 16 * pieces <= sw, "x0a + 16 * pieces <= src_w")
        all_tiles(y0 >= 0, "y0 >= 0")
        all_tiles(rows >= 1, "rows >= 1")
        all_tiles(y0 + rows <= sh, "y0 + rows <= src_h")
        all_tiles(pieces * rows <= MAX_PIECES, "pieces * rows <= 256")
        all_tiles((magic & 0xffffffff) == ((1 << 32) + np.maximum(pieces, 1) - 1) // np.maximum(pieces, 1), "entry[4] == ceil(2^32 / pieces)")
        all_tiles(~e[..., 5:].any(axis=-1), "entry[5..7] == 0")
        all_tiles((c0 >= x0a) & (c1 < x0a + 16 * pieces), "read columns inside the footprint")
        all_tiles((r0 >= y0) & (r1 < y0 + rows), "read rows inside the footprint")


def _table(mapsx, mapsy, sw, sh):
    return orbx.remap_footprints(np.stack(mapsx), np.stack(mapsy), sw, sh)


def _grid(dw, dh):
    return np.meshgrid(np.arange(dw, dtype=np.float32), np.arange(dh, dtype=np.float32))


def _stretch(dw, dh, sw, sh):   # the whole source over the whole output
    u, v = _grid(dw, dh)
    return (u * np.float32(sw / dw)).astype(np.float32), (v * np.float32(sh / dh)).astype(np.float32)


# ---- the two maps that made the parent's table leave the rows -------------------------------------------------------------------
def test_identity_with_first_tile_left_of_the_source():
    u, v = _grid(512, 512)
    mx, my = u.copy(), v.copy()
    mx[:8, :128] = -20.0
    tab = _table([mx], [my], 512, 512)
    check_table(tab, [mx], [my], 512, 512, "identity, first tile at x = -20")
    assert tab[0, 0, 0, :4].tolist() == [0, 0, 2, 10]   # widened to the right: columns 0..31 of rows 0..9


def test_sideways_shift_with_a_black_left_border():
    u, v = _grid(512, 512)
    mx, my = (u - 140).astype(np.float32), v
    tab = _table([mx], [my], 512, 512)
    check_table(tab, [mx], [my], 512, 512, "(u - 140, v)")
    assert (tab[0, 0, :, 0] == 0).all() and (tab[0, 0, :, 2] == 2).all()   # the 64 tiles of the border: columns 0..31


# ---- tiles off the source, one border at a time and all at once; tiles across the first / last column ------------------------------
BORDER_SIZES = [((256, 64), (300, 37)), ((752, 480), (720, 460)), ((32, 20), (150, 13))]   # src_w = 32: x0a has one legal value


def _off_source(kind, sw, sh, dw, dh):
    mx, my = _stretch(dw, dh, sw, sh)
    u, _ = _grid(dw, dh)
    lastx, lasty = (dw - 1) // TILE_W * TILE_W, (dh - 1) // TILE_H * TILE_H   # the (partial) last tile column / row
    if kind in ("left", "all"):
        mx[:, :TILE_W] = -300.0
    if kind in ("right", "all"):
        mx[:, lastx:] = sw + 300.0
    if kind in ("above", "all"):
        my[:TILE_H] = -50.0
    if kind in ("below", "all"):
        my[lasty:] = sh + 50.0
    if kind == "straddle0":
        mx[:, :TILE_W] = (u[:, :TILE_W] * 0.1 - 3).astype(np.float32)
    if kind == "straddle_last":
        mx[:, lastx:] = (sw - 4 + (u[:, lastx:] - lastx) * 0.1).astype(np.float32)
    return mx, my


@pytest.mark.parametrize("kind", ["left", "right", "above", "below", "all", "straddle0", "straddle_last"])
def test_tiles_off_the_source(kind):
    for (sw, sh), (dw, dh) in BORDER_SIZES:
        mx, my = _off_source(kind, sw, sh, dw, dh)
        check_table(_table([mx], [my], sw, sh), [mx], [my], sw, sh, (kind, sw, sh, dw, dh))
        # two maps: the off-source map second, an ordinary one first
        ox, oy = _stretch(dw, dh, sw, sh)
        check_table(_table([ox, mx], [oy, my], sw, sh), [ox, mx], [oy, my], sw, sh, (kind, "two maps", sw, sh, dw, dh))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 1e12, -1e12])
def test_tiles_of_non_finite_and_huge_entries(value):
    for (sw, sh), (dw, dh) in BORDER_SIZES:
        for axis in (0, 1):
            maps = list(_stretch(dw, dh, sw, sh))
            maps[axis][TILE_H:2 * TILE_H, :TILE_W] = value          # a whole tile
            maps[1 - axis][0, 0] = value                              # and one entry of another
            check_table(_table([maps[0]], [maps[1]], sw, sh), [maps[0]], [maps[1]], sw, sh, (value, axis, sw, sh, dw, dh))


def test_rectification_maps_at_the_sizes_of_the_gpu_tests():
    for (sw, sh), (dw, dh), nmaps in (((752, 480), (720, 460), 2), ((1280, 720), (1280, 720), 2), ((640, 480), (601, 353), 1),
                                      ((256, 64), (130, 9), 1), ((512, 512), (512, 512), 2), ((752, 480), (752, 480), 1)):
        maps = [synth.rectify_maps(dw, dh, sw, sh, seed=10 + m) for m in range(nmaps)]
        mapsx, mapsy = [a for a, _ in maps], [b for _, b in maps]
        tab = _table(mapsx, mapsy, sw, sh)
        if tab is None:   # refused: only because a tile's read set does not fit
            assert max(pieces_needed(read_boxes(mapsx[m], mapsy[m], sw, sh)).max() for m in range(nmaps)) > MAX_PIECES, (sw, sh, dw, dh)
        else:
            check_table(tab, mapsx, mapsy, sw, sh, ("rectify", sw, sh, dw, dh))


# ---- a seeded sweep over the map kinds of test_fuzz_preproc_plans -----------------------------------------------------------------
def _sweep_case(case):
    rng = np.random.default_rng(77000 + case)
    sw, sh = 16 * int(rng.integers(2, 50)), int(rng.integers(12, 400))
    dw, dh = int(rng.integers(5, 700)), int(rng.integers(3, 400))
    nmaps = int(rng.integers(1, 3))
    u, v = _grid(dw, dh)
    kind = case % 4
    maps = []
    for m in range(nmaps):
        if kind == 0:
            maps.append(synth.rectify_maps(dw, dh, sw, sh, seed=case + m, k1=float(rng.uniform(-0.3, 0.1)), rot_deg=tuple(rng.uniform(-1, 1, 3))))
        elif kind == 1:
            sc = float(rng.choice([0.6, 0.9, 1.0, 1.3, 2.2]))
            maps.append(((u * sc + v * 0.05 - 2 + m).astype(np.float32), (v * sc - u * 0.03 + 1).astype(np.float32)))
        elif kind == 2:   # a seam and a region outside the source
            mx, my = (u * (sw / max(dw, 1)) + 0.4).astype(np.float32), (v * (sh / max(dh, 1)) - 0.6).astype(np.float32)
            mx[:, dw // 2:] += 7.25
            my[: max(dh // 5, 1)] = -9.0
            maps.append((mx, my))
        else:
            maps.append(((u + rng.integers(0, 33, (dh, dw)) / 32).astype(np.float32), (v + rng.integers(0, 33, (dh, dw)) / 32).astype(np.float32)))
    return kind, sw, sh, [a for a, _ in maps], [b for _, b in maps]


def test_seeded_sweep_of_plan_maps():
    built = [0, 0, 0, 0]
    for case in range(60):
        kind, sw, sh, mapsx, mapsy = _sweep_case(case)
        tab = _table(mapsx, mapsy, sw, sh)
        if tab is None:   # a refusal must be explained by the read set itself: some tile needs more than 256 pieces
            need = max(int(pieces_needed(read_boxes(mapsx[m], mapsy[m], sw, sh)).max()) for m in range(len(mapsx)))
            assert need > MAX_PIECES, "case %d (kind %d, %dx%d): table refused although the largest tile needs %d pieces" % (
                case, kind, sw, sh, need)
            continue
        built[kind] += 1
        check_table(tab, mapsx, mapsy, sw, sh, ("sweep", case, kind, sw, sh))
    print("sweep: %d of 60 cases yield a table (rectify %d, scale / shear %d, seam %d, 1/32 fractions %d)" % (sum(built), *built))
    assert sum(built) >= 30


# ---- refusals and the argument checks -----------------------------------------------------------------------------------------
def _raw(mx, my, sw, sh, table, cap, n_maps=1):
    gx, gy = C.c_int(-1), C.c_int(-1)
    dh, dw = mx.shape[-2:]
    rc = orbx.lib().orbx_debug_remap_footprints(mx.ctypes.data_as(C.c_void_p), my.ctypes.data_as(C.c_void_p), dw, dw, dh, sw, sh, n_maps,
                                                None if table is None else table.ctypes.data_as(C.c_void_p), cap, C.byref(gx), C.byref(gy))
    return rc, gx.value, gy.value


def test_sources_the_staging_loads_cannot_take_are_refused():
    for sw in (8, 16, 24, 31, 33, 40, 100, 750):
        mx, my = _stretch(70, 20, sw, 30)
        assert orbx.remap_footprints(mx, my, sw, 30) is None, sw
    mx, my = _stretch(70, 20, 32, 30)
    assert orbx.remap_footprints(mx, my, 32, 30) is not None


def test_a_tile_that_does_not_fit_is_refused_and_nothing_is_written_past_cap():
    rng = np.random.default_rng(3)
    sw, sh, dw, dh = 640, 480, 300, 37
    mx = rng.uniform(0, sw, (dh, dw)).astype(np.float32)   # every tile reads from all over the source
    my = rng.uniform(0, sh, (dh, dw)).astype(np.float32)
    assert pieces_needed(read_boxes(mx, my, sw, sh)).max() > MAX_PIECES
    n = 8 * 3 * 5
    table = np.full(n + 64, -7, np.int32)
    assert _raw(mx, my, sw, sh, table, n) == (0, 3, 5)
    assert (table == -7).all()
    # a table that is built fills exactly its entries
    sw, sh = 256, 64
    mx, my = _stretch(dw, dh, sw, sh)
    assert _raw(mx, my, sw, sh, table, n) == (1, 3, 5)
    assert (table[n:] == -7).all() and np.array_equal(table[:n].reshape(1, 3, 5, 8), orbx.remap_footprints(mx, my, sw, sh))
    table[:] = -7
    assert _raw(mx, my, sw, sh, table, n - 1)[0] == -3 and (table == -7).all()   # ORBX_E_CAPACITY, nothing written
    assert _raw(mx, my, sw, sh, None, n)[0] == -2                                  # ORBX_E_BADARG
    assert _raw(mx, my, 0, sh, table, n)[0] == -2
    assert _raw(mx, my, sw, sh, table, n, n_maps=0)[0] == -2
