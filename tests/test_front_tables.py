"""The tables that stand in for the fronts of k_detect and k_resize, field by field (no GPU).

orbx_extractor_configure builds one record per FAST cell (what k_detect's front used to derive per wave: the cell loop's bounds
of src/ORBextractor.cc:892-971 and the constants of the stage-1 rounds) and one record per 256 x 16 destination tile plus one
block per tile row of every resize level (the bounds k_resize's front used to derive from the cv::resize tables).
orbx_debug_front_tables returns both for a frame size without touching a device; here every field is compared with a Python
restatement of the rules.  A wrong field would still be caught by the GPU parity tests only where the images happen to
exercise it, so the table itself is held here."""
import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

f32 = np.float32
REJECT, WIDE, LEVEL0 = 1, 2, 4          # cell flags
T_FAST, T_WHOLE = 1, 2                  # tile flags

# (w, h, nlevels).  The four sizes of the benchmark configurations, then one geometry per compiled LDS tile pitch of k_detect
# (44, 48, 52, 56) and one that falls to the run-time pitch, found by a host search over widths <= 400 (levels reduced where the
# smallest level would have no cell, or where it alone would widen the pitch), then two sizes for the cell kinds that need a
# large level: a rejected last-column cell needs >= 31 cell columns, a last-row cell shorter than a round >= 25 cell rows.
SIZES = [(1280, 720, 8), (640, 480, 8), (752, 480, 8), (512, 512, 8),
         (383, 100, 2), (357, 166, 6), (340, 199, 7), (364, 239, 8), (241, 239, 8),
         (1118, 165, 2), (470, 897, 2)]
PITCH = {(383, 100, 2): 44, (357, 166, 6): 48, (340, 199, 7): 52, (364, 239, 8): 56, (241, 239, 8): 76,
         (1118, 165, 2): 44, (470, 897, 2): 48, (1280, 720, 8): 48}


def align_up(v, a):
    return (v + a - 1) // a * a


def levels(w, h, nl, sf=1.2):
    """Per-level geometry as ORBextractor's constructor and ComputePyramid / ComputeKeyPointsOctTree derive it
    (src/ORBextractor.cc:408-420, 1111-1113, 895-907), with the buffer layout of the handle."""
    sfd = float(f32(sf))
    scale = [f32(1)]
    for _ in range(1, nl):
        scale.append(f32(float(scale[-1]) * sfd))
    out, off, cell_off, cells, xc, yc = [], 0, 0, 0, 0, 0
    for l in range(nl):
        inv = f32(1) / scale[l]
        lw, lh = int(np.rint(f32(w) * inv)), int(np.rint(f32(h) * inv))
        width, height = f32(lw - 32), f32(lh - 32)
        ncols, nrows = int(width / f32(35)), int(height / f32(35))
        wcell, hcell = int(np.ceil(width / f32(ncols))), int(np.ceil(height / f32(nrows)))
        cap = ((wcell + 1) // 2) * ((hcell + 1) // 2)
        out.append(dict(w=lw, h=lh, pitch=align_up(lw, 64), off=off, ncols=ncols, nrows=nrows, wcell=wcell, hcell=hcell,
                        cell_start=cells, cell_cap=cap, cell_off=cell_off, xcoef=xc, ycoef=yc))
        off = align_up(off + align_up(lw, 64) * lh, 256)
        cell_off += ncols * nrows * cap
        cells += ncols * nrows
        xc += align_up(lw, 256)
        yc += lh
    return out


def expected_cell(L, l, ci, cj, tile_p):
    """The record of cell (ci, cj) of level l from the reference's loop: iniY / maxY / iniX / maxX with their `continue`s and
    clamps (:909-924), then the round constants as the kernel's front stated them."""
    max_bx, max_by = L["w"] - 16, L["h"] - 16
    ini_y = 16 + ci * L["hcell"]
    max_y = ini_y + L["hcell"] + 6
    ini_x = 16 + cj * L["wcell"]
    max_x = ini_x + L["wcell"] + 6
    rec = np.zeros(16, np.uint64)
    flags = (l << 8) | (L["w"] << 16) | (LEVEL0 if l == 0 else 0)
    if max_y > max_by:
        max_y = max_by
    if max_x > max_bx:
        max_x = max_bx
    rw, rh = max_x - ini_x, max_y - ini_y
    dw, dh = rw - 6, rh - 6
    if ini_y >= max_by - 3 or ini_x >= max_bx - 6 or dw <= 0 or dh <= 0:
        rec[2] = flags | REJECT
        return rec
    if ini_x + tile_p <= L["w"]:
        flags |= WIDE
    qpr = -(-dw // 4)
    dq = 64 // qpr
    rounds = -(-dh // dq)
    act = min((dh - (rounds - 1) * dq) * qpr, 64)
    mask = (1 << act) - 1
    vlast = dw - 4 * (qpr - 1)
    assert 1 <= vlast <= 4 and 1 <= qpr <= 63 and dq >= 1 and 0 < act
    rec[0] = ini_x | (ini_y << 16)
    rec[1] = rw | (rh << 16)
    rec[2] = flags
    rec[3] = L["pitch"]
    rec[4] = L["off"] + ini_y * L["pitch"] + ini_x
    rec[5] = L["cell_off"] + (ci * L["ncols"] + cj) * L["cell_cap"]
    rec[6] = L["cell_cap"]
    rec[7] = qpr | (dq << 8) | ((64 - dq * qpr) << 16)
    rec[8] = 64 * rounds
    rec[9] = ((tile_p // 4) * (dh + 2) + 3) // 4
    rec[10], rec[11] = mask & 0xFFFFFFFF, mask >> 32
    rec[12] = 0 if vlast > 1 else 0x7C000000
    rec[13] = (0 if vlast > 2 else 0x7C00) | (0 if vlast > 3 else 0x7C000000)
    rec[14] = int(np.array(f32(1) / f32(qpr)).view(np.uint32))
    return rec


def resize_axis(dst, src):
    """cv::resize INTER_LINEAR 8U coefficient tables of one axis (resize.cpp: fx = (dx + 0.5) * scale - 0.5, floor, the
    two clamps, cvRound(f * 2048) as shorts)."""
    sc = 1.0 / (float(dst) / float(src))
    idx, a0, a1 = [], [], []
    for d in range(dst):
        f = f32((d + 0.5) * sc - 0.5)
        s = int(np.floor(f))
        f = f32(f - f32(s))
        idx.append(s)
        a0.append(int(np.clip(np.rint(f32((f32(1) - f) * f32(2048))), -32768, 32767)))
        a1.append(int(np.clip(np.rint(f32(f * f32(2048))), -32768, 32767)))
    return idx, a0, a1


def expected_tiles(lv, l):
    """Tile records and tile-row blocks of level l from the axis tables: the footprint of a 256 x 16 tile is the source rows /
    columns its taps touch, clamped to the source level as cv::resize clamps them."""
    D, S = lv[l], lv[l - 1]
    sx, _, _ = resize_axis(D["w"], S["w"])
    sy, b0, b1 = resize_axis(D["h"], S["h"])
    nbx, nby = -(-D["w"] // 256), -(-D["h"] // 16)
    tiles = np.zeros((nby, nbx, 8), np.uint64)
    rows = np.zeros((nby, 4, 4, 4), np.uint64)
    cl = lambda v, hi: min(max(v, 0), hi)
    for tby in range(nby):
        y0, y1 = tby * 16, min(tby * 16 + 16, D["h"]) - 1
        rb = min(cl(sy[y], S["h"] - 1) for y in range(y0, y1 + 1))
        re = max(cl(sy[y] + 1, S["h"] - 1) for y in range(y0, y1 + 1))
        for tbx in range(nbx):
            x0, x1 = tbx * 256, min(tbx * 256 + 256, D["w"]) - 1
            cols = [cl(sx[x], S["w"] - 1) for x in range(x0, x1 + 1)]
            cb = min(cols) & ~3
            ce = min(max(cols) + 1, S["w"] - 1)
            ndw = (ce - cb) // 4 + 1
            whole = l > 1 or cb + 4 * ndw <= S["w"]
            fast = whole and 64 < ndw <= 85 and re - rb + 1 <= 24 and rb + 28 <= S["h"]
            tiles[tby, tbx] = [D["xcoef"] + x0, x0 | ((y1 - y0 + 1) << 16), rb | ((re - rb + 1) << 16), cb | (ndw << 16),
                               (T_FAST if fast else 0) | (T_WHOLE if whole else 0), y0 * D["pitch"], tby, 0]
        for w in range(4):
            for k in range(4):
                dy = min(y0 + w + 4 * k, D["h"] - 1)
                r0, r1 = cl(sy[dy], S["h"] - 1), cl(sy[dy] + 1, S["h"] - 1)
                assert rb <= r0 <= r1 <= re
                rows[tby, w, k] = [(b0[dy] & 0xFFFF) | ((b1[dy] & 0xFFFF) << 16), (r0 - rb) * 512, (r1 - rb) * 512, 0]
    return tiles, rows


@pytest.mark.parametrize("w,h,nl", SIZES)
def test_cell_records(w, h, nl):
    cells, _, tile_p, tile_h = orbx.front_tables(1000, 1.2, nl, 20, 7, w, h)
    lv = levels(w, h, nl)
    max_cw, max_ch = max(L["wcell"] for L in lv), max(L["hcell"] for L in lv)
    assert tile_p == 4 * ((max_cw + 3) // 4 + 2) and tile_h == max_ch + 6
    if (w, h, nl) in PITCH:
        assert tile_p == PITCH[(w, h, nl)]
    assert len(cells) == sum(L["ncols"] * L["nrows"] for L in lv)
    for l, L in enumerate(lv):
        for ci in range(L["nrows"]):
            for cj in range(L["ncols"]):
                got = cells[L["cell_start"] + ci * L["ncols"] + cj]
                want = expected_cell(L, l, ci, cj, tile_p)
                assert np.array_equal(got.astype(np.uint64), want), (l, ci, cj, got, want)
                if not want[2] & REJECT:   # what the kernel relies on: the ROI fits the LDS tile and lies inside the level
                    x, y, rw, rh = int(got[0] & 0xFFFF), int(got[0] >> 16), int(got[1] & 0xFFFF), int(got[1] >> 16)
                    assert x + rw <= L["w"] and y + rh <= L["h"] and rh <= tile_h and 4 * ((rw + 3) // 4) <= tile_p


def test_cell_kinds_occur():
    """The sizes above reach every kind of cell the front distinguishes."""
    seen = set()
    for (w, h, nl) in SIZES:
        cells, _, tile_p, _ = orbx.front_tables(1000, 1.2, nl, 20, 7, w, h)
        fl = cells[:, 2]
        ok = (fl & REJECT) == 0
        dw, dh = (cells[:, 1] & 0xFFFF).astype(int) - 6, (cells[:, 1] >> 16).astype(int) - 6
        dq = ((cells[:, 7] >> 8) & 0xFF).astype(int)
        seen |= {"rejected"} if (~ok).any() else set()
        seen |= {"narrow"} if (ok & ((fl & WIDE) == 0)).any() else set()
        seen |= {"short last row"} if (ok & (dh < dq)).any() else set()
        seen |= {"wider than 58"} if (ok & (dw > 58)).any() else set()
        seen.add(tile_p if tile_p in (44, 48, 52, 56) else 0)
    assert seen == {"rejected", "narrow", "short last row", "wider than 58", 44, 48, 52, 56, 0}


@pytest.mark.parametrize("w,h,nl", SIZES)
def test_tile_records(w, h, nl):
    _, tab, _, _ = orbx.front_tables(1000, 1.2, nl, 20, 7, w, h)
    lv = levels(w, h, nl)
    pos = 0
    for l in range(1, nl):
        tiles, rows = expected_tiles(lv, l)
        got_t = tab[pos:pos + tiles.size].reshape(tiles.shape)
        pos += tiles.size
        got_r = tab[pos:pos + rows.size].reshape(rows.shape)
        pos += rows.size
        assert np.array_equal(got_t.astype(np.uint64), tiles), (l, np.argwhere(got_t != tiles)[:4])
        assert np.array_equal(got_r.astype(np.uint64), rows), (l, np.argwhere(got_r != rows)[:4])
    assert pos == len(tab)


def test_sizes_only_and_capacity():
    import ctypes as C
    prm = orbx._Params(1000, 1.2, 8, 20, 7)
    info = np.zeros(4, np.int32)
    lib = orbx.lib()
    assert lib.orbx_debug_front_tables(C.byref(prm), 640, 480, None, 0, None, 0, orbx._p(info)) == 0
    n, m = int(info[0]), int(info[1])
    cells = np.full(n * 16 + 3, 0xABCD, np.uint32)
    assert lib.orbx_debug_front_tables(C.byref(prm), 640, 480, orbx._p(cells), n * 16 - 1, None, 0, orbx._p(info)) < 0
    assert (cells == 0xABCD).all()
    assert lib.orbx_debug_front_tables(C.byref(prm), 640, 480, orbx._p(cells), n * 16, None, 0, orbx._p(info)) == 0
    assert (cells[n * 16:] == 0xABCD).all() and m > 0
    assert lib.orbx_debug_front_tables(C.byref(prm), 60, 60, None, 0, None, 0, orbx._p(info)) < 0   # no 35 px cell fits
