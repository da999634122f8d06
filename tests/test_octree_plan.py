"""k_octree's plan (orbx_debug_octree_plan; host only): the class of every level (the threads of its workgroup that work) and the
dynamic LDS of the batch's launch.  The LDS lower bound is a Python copy of oct_layout (orbx_octree.hip) evaluated for the level alone, with the level
quotas of ORBextractor's constructor (src/ORBextractor.cc:431-445) and the FAST cell grid of ComputeKeyPointsOctTree (:888-894)."""
import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

K_MAX_INI = 8     # orbx_internal.h: kMaxIni
LDS_LIMIT = 160 * 1024 - 2048

SIZES = [
    # w, h, nfeatures, nlevels
    (1280, 720, 1500, 8),
    (640, 480, 1000, 8),
    (512, 512, 1500, 8),
    (752, 480, 1000, 8),
    (96, 72, 100, 1),      # (levels as small as one FAST cell: 72 px leave room for one level only)
    (160, 120, 300, 3),
]


def _cv_round(x):
    return int(np.rint(np.float64(x)))


def _level_dims(w, h, nlevels, sf=1.2):
    scale = [np.float32(1)]
    for _ in range(1, nlevels):
        scale.append(np.float32(scale[-1] * np.float32(sf)))
    inv = [np.float32(1) / s for s in scale]
    return [(_cv_round(np.float32(w) * i), _cv_round(np.float32(h) * i)) for i in inv]


def _quotas(nf, nlevels, sf=1.2):
    factor = np.float32(1) / np.float32(sf)
    n = np.float32(nf) * (np.float32(1) - factor) / (np.float32(1) - np.float32(np.power(np.float64(factor), np.float64(nlevels))))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(_cv_round(n))
        total += out[-1]
        n = np.float32(n * factor)
    out.append(max(nf - total, 0))
    return out


def _layout_total(maxn, maxcells, rep):
    def a8(b):
        return (b + 7) & ~7
    t = 2 * (4 * a8(maxn * 2) + a8(maxn * 4))
    t += a8(max(maxn * 16, 4096)) + a8(max(maxn * 16 * rep, 16400))
    t += 4 * a8(maxn * 8) + a8(maxn * 2) + a8(maxn * 4) + a8(256 * 8 + 64) + a8((maxcells + 1) * 4)
    return t


def _cells(w, h):
    return int(np.float32(w - 32) / np.float32(35)) * int(np.float32(h - 32) / np.float32(35))


def _lds_of(quota, cells):   # octree_lds_bytes of a launch whose largest quota / cell grid are these
    maxn = quota + 4 * K_MAX_INI + 8
    rep = 2 if _layout_total(maxn, cells, 2) <= 78 * 1024 else 1
    return _layout_total(maxn, cells, rep)


def test_python_copy_of_the_quotas_is_the_oracle_s(oracle):
    for w, h, nf, nl in SIZES:
        assert _quotas(nf, nl) == list(oracle.OracleExtractor(nf, 1.2, nl, 20, 7).tables()["nfeat"]), (nf, nl)


@pytest.mark.parametrize("w,h,nf,nl", SIZES)
def test_plan_invariants(w, h, nf, nl):
    nt, lds = orbx.octree_plan(nf, 1.2, nl, 20, 7, w, h)
    nt, lds = nt.tolist(), lds.tolist()
    assert len(nt) == nl and all(c in (128, 256, 512) for c in nt), nt
    assert all(nt[l] >= nt[l + 1] for l in range(nl - 1)), nt            # non-increasing ...
    for c in set(nt):                                                     # ... hence every class is one contiguous level range
        ls = [l for l in range(nl) if nt[l] == c]
        assert ls == list(range(ls[0], ls[-1] + 1)), nt
    quota, cells = _quotas(nf, nl), [_cells(*d) for d in _level_dims(w, h, nl)]
    for l in range(nl):
        assert _lds_of(quota[l], cells[l]) <= lds[l] <= LDS_LIMIT, (l, lds)
    # one launch serves every level of a batch: its LDS is that of the largest quota and the largest cell grid, no more
    assert set(lds) == {_lds_of(max(quota), max(cells))}, lds


def test_plan_of_the_benchmark_size_is_pinned():
    """1280 x 720, 8 levels of 1.2: levels 0 - 2 with 512 threads, 3 - 6 with 256, 7 with 128: the densest benchmark frame has 9229 /
    5398 / 1950 candidates at the densest level of each class, 1.5 x under 16384 / 8192 / 4096 (level 6 has up to 3010: 1.36 x
    under 4096, hence 256; DESIGN.md 4 has every level)."""
    nt, _ = orbx.octree_plan(1500, 1.2, 8, 20, 7, 1280, 720)
    assert nt.tolist() == [512] * 3 + [256] * 4 + [128]


def test_plan_rejects_bad_arguments():
    with pytest.raises(orbx.OrbxError):
        orbx.octree_plan(1500, 1.2, 8, 20, 7, 0, 720)
    with pytest.raises(orbx.OrbxError):
        orbx.octree_plan(1500, 1.2, 8, 20, 7, 96, 72)      # level 1 is smaller than one FAST cell
