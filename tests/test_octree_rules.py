"""k_octree against named rules of DistributeOctTree (src/ORBextractor.cc:490-757), on crafted candidate sets (tests/octree_cases.py)
instead of whatever candidates an image happens to produce, and its std::sort replica on crafted sort inputs.

CPU (no marker): every case reaches the rule it was designed for -- asserted from the trace of the pure-Python restatement, so a
case that misses its branch FAILS -- and the C++ oracle agrees with the restatement; the Python port of the introsort agrees with
libstdc++ and with the host replica, and its trace shows the heapsorts and the three pending segments the inputs were built for.

GPU: orbx_debug_octree runs k_octree alone on the candidates, in batches of three images that carry different cases of one window
size (per-image strides; with hook 0 the batch's launch of the plan), for every class (128 / 256 / 512 threads and the plan) and
every candidate path (histogram variant, global-memory candidates, per-pass sweeps).  The selected (x, y, response) per level, in
list order, and the counts equal the oracle's exactly.  orbx_debug_introsort_device_nt sorts the crafted inputs with 64, 128, 256
and 512 threads.  Everything is bit-exact.

Derived constants stated where they are used: see test_large_quota_uses_one_counter_replica and test_path_table_forms."""
import ctypes as C

import numpy as np
import pytest

import octree_cases as oc

CLASSES = (128, 256, 512, 0)   # orbx_debug_set_octree_class: 0 = the plan
PATHS = (0, 1, 2)              # orbx_debug_set_octree_global: histogram variant, global-memory candidates, per-pass sweeps
SORT_NT = (64, 128, 256, 512)  # orbx_debug_introsort_device_nt: introsort_wave | introsort_block with that many threads

CASES = oc.all_cases()
GROUPS = oc.groups()
_expected = {}


def expected(oracle, case):
    """oracle.distribute of a case, candidates in the reference's order: [(x, y, response)] relative to the window.  Computed once."""
    if case.name not in _expected:
        k = case.canonical()
        cand = np.zeros(len(k), oracle.KP_DTYPE)
        if k:
            a = np.array(k, np.float32)
            cand["x"], cand["y"], cand["response"] = a[:, 0], a[:, 1], a[:, 2]
        cand["size"], cand["angle"], cand["class_id"] = 7, -1, -1
        got = oracle.OracleExtractor(1000).distribute(cand, 16, 16 + case.W, 16, 16 + case.H, case.N)
        _expected[case.name] = [(int(g["x"]), int(g["y"]), int(g["response"])) for g in got]
    return _expected[case.name]


def std_sort(oracle, v):
    a = np.array(v, np.uint64)
    oracle.lib().oro_std_sort_keys(a.ctypes.data_as(C.c_void_p), len(a))
    return [int(x) for x in a]


# ================================================================================================ CPU
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_reaches_its_rule_and_oracle_equals_restatement(oracle, case):
    t = {}
    out = oc.distribute_octtree_py(oracle, case.keys(), 16, 16 + case.W, 16, 16 + case.H, case.N, t)
    assert expected(oracle, case) == [(int(x), int(y), int(r)) for x, y, r in out]
    assert case.prop(t, out, case), (case.name, case.why, {k: v for k, v in t.items() if k != "rounds"},
                                     [(len(r["keys"]), r["broke"], r["size"], r["children"]) for r in t["rounds"]])
    if case.stable_differs is not None:   # the tie cases: the order std::sort leaves equal keys in decides the selection
        stable = oc.distribute_octtree_py(oracle, case.keys(), 16, 16 + case.W, 16, 16 + case.H, case.N, sort=oc.stable_sort_nodes)
        assert (stable != out) == case.stable_differs, case.name


def test_cases_cover_every_group_of_the_issue():
    """The census of the case list: every root count, every list size of the sort with every tie pattern, and at least one batch
    of three different cases for the windows that have three."""
    names = {c.name for c in CASES}
    assert {"roots%d_bounds" % n for n in range(2, 9)} <= names and {"roots1_random", "no_candidate", "one_candidate", "fewer_than_roots"} <= names
    assert {"sort%d_%s" % (m, v) for m in oc.SORT_SIZES for v in oc.SORT_VARIANTS} <= names
    assert all(len({c.name for c in oc.batches(g)[0]}) == min(3, len(g)) for g in GROUPS.values())
    assert max(c.W for c in CASES) <= 700 and max(c.H for c in CASES) <= 320


KILLERS = oc.killer_inputs()
PENDING = oc.three_pending_inputs()
RANKS = oc.rank_inputs()
SORT_INPUTS = [(n, v) for n, v, _ in KILLERS] + PENDING + RANKS


def test_sort_port_equals_libstdcxx_and_host_replica(oracle):
    import orb_slam3_fast_amd as orbx
    for name, v in SORT_INPUTS:
        want = std_sort(oracle, v)
        assert oc.introsort_py(v) == want, name
        a = np.array(v, np.uint64)
        orbx.lib().orbx_debug_introsort(a.ctypes.data_as(C.c_void_p), len(a))
        assert [int(x) for x in a] == want, name


def test_killer_inputs_reach_every_heapsort():
    """McIlroy's adversary exhausts the depth budget 2 floor(log2 n): the port hands one segment of n - 4 floor(log2 n) elements
    (two leave per partition) to heapsort.  20 and 40 are introsort_seg_reg's d == 0 (the whole input is one register segment), 76
    and 100 introsort_block's depth == 0 behind partition_reg2 (65 .. 128), 268 and 964 behind partition_wave; with one wave (nt =
    64) all six are introsort_wave's."""
    for name, v, seg in KILLERS:
        t = {}
        oc.introsort_py(v, t)
        if seg is not None:
            n = len(v)
            assert seg == oc.KILLER_SIZES[n] == n - 4 * (n.bit_length() - 1)
            assert t["heapsorts"] == [seg] and t["partitions"] == 2 * (n.bit_length() - 1), (name, t)
    assert sorted(oc.KILLER_SIZES.values()) == [20, 40, 76, 100, 268, 964]


def test_pending_inputs_reach_three_stack_entries():
    assert len(PENDING) >= 6
    for name, v in PENDING:
        t = {}
        oc.introsort_py(v, t)
        assert 52 <= len(v) <= 64 and t["max_pending"] == 3, (name, t)
    assert any(len({x >> 28 for x in v}) < len(v) for _, v in PENDING)    # some with tied keys
    assert any(len({x >> 28 for x in v}) == len(v) for _, v in PENDING)   # some permutations


def test_rank_sizes_straddle_the_lane_thresholds():
    """per = 4 / 2 / 1 lanes per element of introsort_block's final rank by 4 n <= nt and 2 n <= nt: both sides of both, per class."""
    for nt in (128, 256, 512):
        assert {nt // 4, nt // 4 + 1, nt // 2, nt // 2 + 1} <= set(oc.RANK_SIZES)
    assert all(len({x >> 28 for x in v}) < max(len(v), 2) or len(v) <= 2 for n, v in RANKS if n.startswith("two"))


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def gpu():
    import orb_slam3_fast_amd as orbx
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return orbx


def _run_group(orbx, oracle, cases, W, H, N, classes=CLASSES, paths=PATHS):
    ex = orbx.ORBextractor(N, 1.2, 1, 20, 7, max_width=W + 32, max_height=H + 32, max_batch=3)
    assert ex.features_per_level()[0] == N == oracle.OracleExtractor(N, 1.2, 1, 20, 7).tables()["nfeat"][0]   # one level: quota == nfeatures
    L = orbx.lib()
    try:
        for batch in oc.batches(cases):
            cand = [[oc.device_order(c, slot)] for slot, c in enumerate(batch)]
            want = [[(x + 16, y + 16, r) for x, y, r in expected(oracle, c)] for c in batch]
            for nt in classes:
                for path in paths:
                    L.orbx_debug_set_octree_class(nt)
                    L.orbx_debug_set_octree_global(path)
                    got = ex.debug_octree(W + 32, H + 32, cand)
                    for slot, c in enumerate(batch):
                        tag = (c.name, "slot", slot, "class", nt, "path", path)
                        assert len(got[slot][0]) == len(want[slot]), tag
                        assert [tuple(int(v) for v in k) for k in got[slot][0]] == want[slot], tag
                        st = ex.level_stats(slot)
                        assert st[2][0] == len(c.pts) and st[3][0] == len(want[slot]), tag
        return ex, batch, cand
    finally:
        L.orbx_debug_set_octree_class(0)
        L.orbx_debug_set_octree_global(0)


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(GROUPS), ids=lambda k: "%dx%d_N%d" % k)
def test_octree_on_crafted_candidates(gpu, oracle, key):
    W, H, N = key
    _run_group(gpu, oracle, GROUPS[key], W, H, N)


def test_large_quota_uses_one_counter_replica():
    """N = 800 (run above as the group 256x256_N800) is the quota at which k_octree keeps ONE counter replica, hence nrepB == 1 in
    the winner sweeps: oct_layout(maxn, cells, 2) with maxn = N + 4 * 8 + 8 = 840 takes 2 * (4 * 2 + 4) * 840 (node tables) + 16 *
    840 (cnt4) + 16 * 2 * 840 (counters, 2 replicas) + 4 * 8 * 840 (scan, cpos, e[2]) + 2 * 840 + 4 * 840 + 2112 = 94 512 bytes
    before the cell prefix, over oct_rep's 78 KB = 79 872; the plan reports the launch's LDS with one replica: 20 160 + 16 400 (the
    histogram variant's floor) + 13 440 + 26 880 + 5 040 + 2 112 + 4 * (49 + 1) rounded to 8 = 84 232.  At N = 503, the largest
    other quota here, two replicas fit: 110 * 543 + 2112 = 61 842."""
    import orb_slam3_fast_amd as orbx
    _, lds = orbx.octree_plan(800, 1.2, 1, 20, 7, 256 + 32, 256 + 32)
    assert int(lds[0]) == 84232
    _, lds = orbx.octree_plan(503, 1.2, 1, 20, 7, 256 + 32, 256 + 32)
    assert int(lds[0]) > 110 * 543 and int(lds[0]) <= 78 * 1024


def test_path_table_forms():
    """The histogram variant's sweep reads per-coordinate path tables when 2 (W + H) + 8 bytes fit the LDS that is idle then, 30 *
    maxn bytes (cpos + e[0] + e[1] + mark + bestk = 8 + 8 + 8 + 2 + 4 bytes per node; maxn = N + 40): on the 669 x 288 window that
    is 1 922 bytes against 30 * 60 = 1 800 at N = 20 (the arithmetic form) and 30 * 140 = 4 200 at N = 100 (the tables).  Both groups
    run in test_octree_on_crafted_candidates on the GPU; this pins the arithmetic that makes them two forms."""
    assert 2 * (oc.TAB_W + oc.TAB_H) + 8 == 1922 and 30 * (20 + 40) < 1922 <= 30 * (100 + 40)
    assert (oc.TAB_W, oc.TAB_H, 20) in GROUPS and (oc.TAB_W, oc.TAB_H, 100) in GROUPS


@pytest.mark.gpu
def test_injected_candidates_round_trip(gpu, oracle):
    """orbx_debug_candidates after the entry returns the injected set, in the gather's order (cell by cell, arrival order inside)."""
    W, H, N = oc.TAB_W, oc.TAB_H, 100
    ex, batch, cand = _run_group(gpu, oracle, GROUPS[(W, H, N)], W, H, N, classes=(0,), paths=(0,))
    _, _, wCell, hCell = oc.cell_grid(W, H)
    nCols = oc.cell_grid(W, H)[0]
    for slot, c in enumerate(batch):
        got = [tuple(int(v) for v in k) for k in ex.debug_candidates(0, slot)]
        assert got == sorted(cand[slot][0], key=lambda p: (p[1] - 3) // hCell * nCols + (p[0] - 3) // wCell)   # (a stable sort)


@pytest.mark.gpu
def test_two_levels_of_different_classes_in_one_launch(gpu, oracle):
    """A 352 x 272 frame with two levels: the plan gives level 0 (320 x 240 window, 76 800 px^2) 256 threads and level 1 (261 x 195)
    128, so hook 0 runs two classes in one launch of three images."""
    orbx = gpu
    w, h, nf = 352, 272, 300
    nt, _ = orbx.octree_plan(nf, 1.2, 2, 20, 7, w, h)
    assert nt.tolist() == [256, 128]
    ox = oracle.OracleExtractor(nf, 1.2, 2, 20, 7)
    tab = ox.tables()
    ex = orbx.ORBextractor(nf, 1.2, 2, 20, 7, max_width=w, max_height=h, max_batch=3)
    assert np.array_equal(ex.features_per_level(), tab["nfeat"])
    sizes = [(int(np.rint(np.float32(w) * tab["inv_scale"][l])) - 32, int(np.rint(np.float32(h) * tab["inv_scale"][l])) - 32) for l in range(2)]
    assert sizes == [(320, 240), (261, 195)]
    rng = np.random.default_rng(21)
    cases = [[oc.Case("two_levels_%d_%d" % (i, l), W, H, int(tab["nfeat"][l]), oc._rand(rng, (900, 40, 400)[i], 3, W - 3, 3, H - 3), "", None)
              for l, (W, H) in enumerate(sizes)] for i in range(3)]
    cand = [[oc.device_order(c, i) for c in per_level] for i, per_level in enumerate(cases)]
    L = orbx.lib()
    try:
        for hook in (0, 512):
            L.orbx_debug_set_octree_class(hook)
            got = ex.debug_octree(w, h, cand)
            for i in range(3):
                st = ex.level_stats(i)
                assert (st[0].tolist(), st[1].tolist()) == ([s[0] + 32 for s in sizes], [s[1] + 32 for s in sizes])
                for l in range(2):
                    want = [(x + 16, y + 16, r) for x, y, r in expected(oracle, cases[i][l])]
                    assert [tuple(int(v) for v in k) for k in got[i][l]] == want, (hook, i, l)
    finally:
        L.orbx_debug_set_octree_class(0)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", SORT_NT)
def test_device_sort_on_crafted_inputs(gpu, oracle, nt):
    for name, v in SORT_INPUTS:
        got = gpu.introsort_device(v, nt)
        assert [int(x) for x in got] == std_sort(oracle, v), (name, nt)
