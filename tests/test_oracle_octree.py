"""A second, literal restatement of ORBextractor::DistributeOctTree (src/ORBextractor.cc:490-757) in pure Python --
std::list emulated by a Python list with push_front / erase, DivideNode and the loops transcribed statement by
statement -- checked against the C++ oracle on random candidate sets.  The only shared piece is libstdc++'s std::sort
(called through the oracle library) because the tie order of an unstable sort cannot be restated independently."""
import numpy as np
import pytest

from octree_cases import distribute_octtree_py   # the restatement itself (tests/octree_cases.py; it also takes a trace)


def _cands(rng, W, H, n, clustered):
    if clustered:
        cx, cy = rng.uniform(0, W, 6), rng.uniform(0, H, 6)
        which = rng.integers(0, 6, n)
        x = np.clip(cx[which] + rng.normal(0, W / 15, n), 0, W - 1)
        y = np.clip(cy[which] + rng.normal(0, H / 15, n), 0, H - 1)
    else:
        x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    pts = np.unique(np.stack([np.floor(x), np.floor(y)], 1).astype(np.int64), axis=0)  # FAST never yields a pixel twice
    rng.shuffle(pts)
    resp = rng.integers(7, 60, len(pts))  # few distinct responses: "first maximum wins" matters
    return pts, resp


@pytest.mark.parametrize("W,H,N,n,clustered,seed", [
    (1248, 688, 326, 6000, False, 1), (1248, 688, 326, 6000, True, 2), (608, 448, 217, 2500, False, 3),
    (720, 448, 217, 900, True, 4), (325, 169, 91, 400, False, 5), (325, 169, 91, 1500, True, 6),
    (1008, 568, 271, 150, False, 7), (480, 480, 100, 3000, True, 8), (1248, 688, 30, 2000, False, 9),
    (300, 120, 60, 700, True, 10),
])
def test_python_restatement_of_distribute_octtree_matches_oracle(oracle, W, H, N, n, clustered, seed):
    rng = np.random.default_rng(seed)
    pts, resp = _cands(rng, W, H, n, clustered)
    keys = [(float(p[0]), float(p[1]), float(r)) for p, r in zip(pts, resp)]
    exp = distribute_octtree_py(oracle, keys, 16, 16 + W, 16, 16 + H, N)
    cand = np.zeros(len(pts), oracle.KP_DTYPE)
    cand["x"], cand["y"], cand["response"], cand["size"], cand["angle"], cand["class_id"] = pts[:, 0], pts[:, 1], resp, 7, -1, -1
    ex = oracle.OracleExtractor(1000)
    got = ex.distribute(cand, 16, 16 + W, 16, 16 + H, N)
    assert len(got) == len(exp) and len(got) >= min(N, 1)
    assert [(float(k["x"]), float(k["y"]), float(k["response"])) for k in got] == exp
