"""k_detect's contrast pass scores one survivor per lane with both polarities in the halves of one packed network.

Bit-exact against the CPU oracle on every tile pitch the kernel is instantiated for (44 / 48 / 52 / 56 and the run-time one),
on geometries with odd cell rows and columns, on frames where many pixels pass BOTH compass tests (a bright and a dark pair
of compass pixels), and through the list-flush / corner-overflow paths (LDS list shrunk by the test hook).
"""
import math

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

# w, h, nlevels -> the LDS tile pitch 4 * (ceil(maxCellW / 4) + 2) of orbx_api.hip's geometry
GEOMETRIES = [
    (600, 450, 4, 44),
    (300, 225, 4, 48),
    (328, 246, 4, 52),
    (344, 258, 5, 56),
    (384, 288, 8, 60),   # no compile-time instantiation: run-time pitch
]


def _tile_pitch(w, h, nl, sf=1.2):
    """orbx_api.hip's cell geometry: (tile pitch, any level with an odd number of cell rows or columns)."""
    max_cw, odd, scale = 0, False, 1.0
    for _ in range(nl):
        inv = np.float32(1.0 / scale)
        lw, lh = int(np.round(np.float32(w) * inv)), int(np.round(np.float32(h) * inv))
        width, height = np.float32(lw - 32), np.float32(lh - 32)
        nc, nr = int(width / np.float32(35)), int(height / np.float32(35))
        odd |= nc % 2 == 1 or nr % 2 == 1
        max_cw = max(max_cw, math.ceil(width / nc))
        scale *= sf
    return 4 * ((max_cw + 3) // 4 + 2), odd


def _both_polarity_frame(w, h, stream):
    """A natural frame with diagonal sawtooth stripes over its right half: next to a stripe edge ring pixels 0 and 4 are
    bright while 8 and 12 are dark, so the pixel passes the bright AND the dark compass test."""
    img = synth.mono_frame(w, h, stream)
    y, x = np.mgrid[0:h, 0:w]
    saw = ((x + y) * 23 % 256).astype(np.uint8)
    img[:, w // 2:] = saw[:, w // 2:]
    return img


def _both_compass_count(img, t):
    a = img.astype(np.int32)
    c = a[3:-3, 3:-3]
    v0, v8 = a[6:, 3:-3], a[:-6, 3:-3]
    v4, v12 = a[3:-3, 6:], a[3:-3, :-6]
    bright = np.minimum(np.maximum(v0, v8), np.maximum(v4, v12)) > c + t
    dark = np.maximum(np.minimum(v0, v8), np.minimum(v4, v12)) < c - t
    return int((bright & dark).sum())


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


def test_geometries_cover_every_pitch_and_odd_cell_grids():
    pitches = []
    for w, h, nl, tp in GEOMETRIES:
        p, odd = _tile_pitch(w, h, nl)
        assert p == tp, (w, h, nl, p)
        pitches.append(p)
        assert odd, (w, h, nl)
    assert {44, 48, 52, 56} <= set(pitches) and any(p not in (44, 48, 52, 56) for p in pitches)


def test_both_polarity_frames_have_such_pixels():
    img = _both_polarity_frame(344, 258, 3)
    assert _both_compass_count(img, 20) > 1000


@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nl,tp", GEOMETRIES)
def test_every_tile_pitch_natural_and_both_polarity(gpu, oracle, w, h, nl, tp):
    ex = orbx.ORBextractor(1000, 1.2, nl, 20, 7, max_width=w, max_height=h)
    oe = oracle.OracleExtractor(1000, 1.2, nl, 20, 7)
    nat = synth.mono_frame(w, h, 40 + tp)
    nat[: h // 3, : w // 3] = nat[: h // 3, : w // 3] // 8 + 100      # low-contrast corner: minThFAST redo cells
    assert _check(ex, oe, nat, nl) > 0
    assert _check(ex, oe, _both_polarity_frame(w, h, 50 + tp), nl) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nl,tp", [GEOMETRIES[0], GEOMETRIES[3], GEOMETRIES[4]])
def test_list_flush_and_corner_overflow_on_every_path(gpu, oracle, w, h, nl, tp):
    """White noise and the both-polarity stripes with the LDS list at its minimum (320 entries: mid-cell flushes, the
    corner limit and the tile-scan NMS) and at its full size (704)."""
    rng = np.random.default_rng(tp)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    stripes = _both_polarity_frame(w, h, 60 + tp)
    stripes[: h // 2] = noise[: h // 2]
    ex = orbx.ORBextractor(1000, 1.2, nl, 20, 7, max_width=w, max_height=h)
    oe = oracle.OracleExtractor(1000, 1.2, nl, 20, 7)
    try:
        for cap in (320, 704):
            orbx.lib().orbx_debug_set_detect_list_cap(cap)
            for img in (noise, stripes):
                assert _check(ex, oe, img, nl) > 0
    finally:
        orbx.lib().orbx_debug_set_detect_list_cap(1024)
