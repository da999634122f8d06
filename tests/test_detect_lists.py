"""k_detect's survivor / corner lists with branch-free appends and loop-invariant stage-1 masks.

The stage-1 rounds append survivors with a select instead of an exec-mask branch (lanes without a survivor store to a dump
slot in tile bytes 0 - 1), mask the pixels outside the detectable window through per-lane thresholds and mask lanes only in
the last round; the contrast pass does the same for its score bytes and corner entries.  These tests pin the list paths the
change touches, bit-exact against the CPU oracle on every tile pitch:
- a cell whose survivors fill the list exactly (sEnd + round == listTotal: no flush in that round, a flush in the next);
- corner-list overflow (tile-scan NMS fallback) with the list at its minimum;
- a last stage-1 round with a partial row group (dh not a multiple of the rows per round);
- cells redone at minThFAST;
- frames whose top-left ROI bytes (the dump slot) are extreme, so that a read of the slot or a dumped entry would show.
"""
import math

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

# w, h, nlevels, tile pitch (4 * (ceil(maxCellW / 4) + 2), orbx_api.hip)
GEOMETRIES = [
    (600, 450, 4, 44),
    (300, 225, 4, 48),
    (328, 246, 4, 52),
    (344, 258, 5, 56),
    (384, 288, 8, 60),   # run-time pitch
]
ROW_ROUND_PITCHES = (44, 48, 56)   # kRowRounds in orbx_detect.hip: a round is dq = 64 // qpr whole detect rows
INI_TH, MIN_TH = 20, 7


def _level0_cells(w, h):
    """Level-0 FAST cells as k_detect clips them: [(iniX, iniY, dw, dh)] (orbx_api.hip / orbx_detect.hip geometry)."""
    width, height = np.float32(w - 32), np.float32(h - 32)
    nc, nr = int(width / np.float32(35)), int(height / np.float32(35))
    wc, hc = math.ceil(width / nc), math.ceil(height / nr)
    cells = []
    for i in range(nr):
        for j in range(nc):
            ix, iy = 16 + j * wc, 16 + i * hc
            mx, my = min(ix + wc + 6, w - 16), min(iy + hc + 6, h - 16)
            dw, dh = mx - ix - 6, my - iy - 6
            if iy >= h - 16 - 3 or ix >= w - 16 - 6 or dw <= 0 or dh <= 0:
                continue
            cells.append((ix, iy, dw, dh))
    return cells


def _compass(img, t):
    """Stage 1's compass pre-test for every pixel with a full ring: bright or dark pair of adjacent compass pixels."""
    a = img.astype(np.int32)
    c = a[3:-3, 3:-3]
    v0, v8 = a[6:, 3:-3], a[:-6, 3:-3]
    v4, v12 = a[3:-3, 6:], a[3:-3, :-6]
    bright = np.minimum(np.maximum(v0, v8), np.maximum(v4, v12)) > c + t
    dark = np.maximum(np.minimum(v0, v8), np.minimum(v4, v12)) < c - t
    out = np.zeros(a.shape, bool)
    out[3:-3, 3:-3] = bright | dark
    return out


def _round_totals(surv, cell, tp):
    """Cumulative stage-1 survivors of a cell at the end of each round, in the kernel's round order."""
    ix, iy, dw, dh = cell
    win = surv[iy + 3: iy + 3 + dh, ix + 3: ix + 3 + dw]
    qpr = (dw + 3) // 4
    padded = np.zeros((dh, 4 * qpr), bool)
    padded[:, :dw] = win
    per_quad = padded.reshape(dh, qpr, 4).sum(2).reshape(-1)   # row-major quads
    if tp in ROW_ROUND_PITCHES:
        dq = 64 // qpr
        per_round = [per_quad[r * dq * qpr: (r + 1) * dq * qpr].sum() for r in range(-(-dh // dq))]
    else:
        per_round = [per_quad[q: q + 64].sum() for q in range(0, len(per_quad), 64)]
    return np.cumsum(per_round)


def _exact_fill_cap(img, w, h, tp):
    """A list size in [320, 704] that some level-0 cell's survivors reach exactly at the end of a round before any flush."""
    surv = _compass(img, INI_TH)
    for cell in _level0_cells(w, h):
        for total in _round_totals(surv, cell, tp)[:-1]:   # not the last round: the next round must flush
            if 320 <= total <= 704:
                return int(total)
    return None


def _partial_last_round(w, h, tp):
    """Level-0 cells whose last stage-1 round holds fewer rows (kRowRounds) or quads (flat rounds) than the others."""
    n = 0
    for _, _, dw, dh in _level0_cells(w, h):
        qpr = (dw + 3) // 4
        if tp in ROW_ROUND_PITCHES:
            n += dh % (64 // qpr) != 0
        else:
            n += (qpr * dh) % 64 != 0
    return n


def _noise_frame(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _dump_probe_frame(w, h, seed):
    """A natural frame whose pixels at the top-left ROI corner of every level-0 cell (tile bytes 0 - 1, the dump slot) alternate
    between 0 and 255: if anything read the slot back, the scores around it would differ from the oracle's."""
    img = synth.mono_frame(w, h, seed)
    for ix, iy, _, _ in _level0_cells(w, h):
        img[iy, ix] = 0 if (ix + iy) % 2 else 255
        img[iy, ix + 1] = 255 - img[iy, ix]
    return img


def _kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 28)


def _check(ex, oe, img, nl):
    mono, k, d = ex(img)
    omono, ok_, od = oe.extract(img)
    for l in range(nl):
        c = oe.detect_candidates(l)
        want = np.stack([c["x"], c["y"], c["response"]], 1).astype(np.int32)
        got = ex.debug_candidates(l)
        want = want[np.lexsort(want.T[::-1])]
        got = got[np.lexsort(got.T[::-1])]
        assert np.array_equal(got, want), "candidates level %d" % l
    assert mono == omono and len(k) == len(ok_)
    assert np.array_equal(_kp_bytes(k), _kp_bytes(ok_)) and np.array_equal(d, od)
    return len(k)


@pytest.mark.parametrize("w,h,nl,tp", GEOMETRIES)
def test_every_geometry_has_a_partial_last_round(w, h, nl, tp):
    assert _partial_last_round(w, h, tp) > 0


@pytest.mark.parametrize("w,h,nl,tp", GEOMETRIES)
def test_noise_frames_fill_the_list_exactly(w, h, nl, tp):
    assert _exact_fill_cap(_noise_frame(w, h, tp), w, h, tp) is not None


def test_round_totals_match_a_plain_count():
    w, h, tp = 300, 225, 48
    img = _noise_frame(w, h, 1)
    surv = _compass(img, INI_TH)
    for cell in _level0_cells(w, h)[:5]:
        ix, iy, dw, dh = cell
        assert _round_totals(surv, cell, tp)[-1] == surv[iy + 3: iy + 3 + dh, ix + 3: ix + 3 + dw].sum()


@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nl,tp", GEOMETRIES)
def test_list_filled_exactly_at_list_total(gpu, oracle, w, h, nl, tp):
    img = _noise_frame(w, h, tp)
    cap = _exact_fill_cap(img, w, h, tp)
    ex = orbx.ORBextractor(1000, 1.2, nl, INI_TH, MIN_TH, max_width=w, max_height=h)
    oe = oracle.OracleExtractor(1000, 1.2, nl, INI_TH, MIN_TH)
    try:
        for c in (cap, cap - 1, cap + 1):
            orbx.lib().orbx_debug_set_detect_list_cap(c)
            assert _check(ex, oe, img, nl) > 0
    finally:
        orbx.lib().orbx_debug_set_detect_list_cap(1024)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nl,tp", GEOMETRIES)
def test_corner_overflow_partial_rounds_and_min_threshold(gpu, oracle, w, h, nl, tp):
    """Noise at the smallest list (corner overflow, tile-scan NMS), a natural frame with a low-contrast quarter (minThFAST
    redo cells) and the dump-slot probe, at the smallest and the full list."""
    noise = _noise_frame(w, h, 100 + tp)
    nat = synth.mono_frame(w, h, 70 + tp)
    nat[: h // 2, : w // 2] = nat[: h // 2, : w // 2] // 10 + 120
    probe = _dump_probe_frame(w, h, 80 + tp)
    ex = orbx.ORBextractor(1000, 1.2, nl, INI_TH, MIN_TH, max_width=w, max_height=h)
    oe = oracle.OracleExtractor(1000, 1.2, nl, INI_TH, MIN_TH)
    try:
        for cap in (320, 704):
            orbx.lib().orbx_debug_set_detect_list_cap(cap)
            for img in (noise, nat, probe):
                assert _check(ex, oe, img, nl) > 0
    finally:
        orbx.lib().orbx_debug_set_detect_list_cap(1024)
