"""k_stereo_sort (the row sort in front of the batched ComputeStereoMatches, src/Frame.cc:930-949) on crafted keypoints: the
sizes around its index-permutation path (up to 2048 keypoints per image: source indices permuted in 4 KB of LDS, the sorted
arrays gathered through them) and its direct-scatter path (2049 and more), through the batched stereo entry and the crafted
helpers of tests/stereo_cases.py / tests/test_stereo_gates.py.

Two kinds of sets:
  * in-bounds sets (every row band and SAD window inside the image, stereo_cases.check_reads_in_bounds): uRight / depth are
    compared bit for bit with the oracle's ComputeStereoMatches, and the sorted arrays (orbx_debug_stereo_sort) with a numpy
    model;
  * edge sets (rows 0 and imgH - 1, y values that clamp, octave 7 at the image edge): the reference indexes its row table with
    these rows unguarded (vRowIndices[yi], yi < 0 or >= rows), so the oracle is not run on them.  Every left descriptor is
    0x00.. and every right one 0xFF.. (Hamming 256): no keypoint reaches the SAD windows, every uRight / depth is -1, and the
    sorted arrays are compared with the model.

The frame is 160 x 132 with a (1.1, 8) pyramid: the smallest frame whose eighth level still holds one FAST cell (67 px), i.e.
the smallest on which a handle exists and octave 7 is a valid level.  133 row counters for 256 or 512 threads: most threads
of the prefix scan own no row.

The order of a row's records depends on the arrival order of LDS atomics: rows are compared as multisets, and every record's
index field must name the keypoint whose x, y, octave, band and descriptor the slot carries."""
import numpy as np
import pytest

import stereo_cases as sc
from test_stereo_gates import _same_bits, _upload

W, H, PYR = 160, 132, (1.1, 8)
NF = 2100          # result slots per image: 2049 keypoints fit
NPAIRS = 2
SHIFT = 6
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ sets
def _zero_points(k, d, rng):
    """(0, 0) keypoints (maxr = -1 for a right one, src/Frame.cc:943) at the front, in the middle and at the end."""
    z = np.zeros(1, sc.KP_DTYPE)
    z["size"], z["response"], z["class_id"] = 31.0, 50.0, -1
    m = len(k) // 2
    zd = lambda: rng.integers(0, 256, (1, 32), dtype=np.uint8)
    return np.concatenate([z, k[:m], z, k[m:], z]), np.concatenate([zd(), d[:m], zd(), d[m:], zd()])


def inbounds_set(seed, nL, nR, rows="spread", zeros=True):
    """nL left and nR right keypoints on one noise scene (R = L shifted by 6): min(nL, nR) partners, a quarter of them at
    octave 7, the rest unpartnered; rows = spread / one (every keypoint in row 60) / own (every keypoint in a row of its own)."""
    s = sc.Scene(seed, W, H, PYR, shift=SHIFT)
    s.speckle(0.3)      # (SADs of different sizes: a median of 0 would cut every match)
    rng = s.rng
    z = 3 if zeros else 0
    zL, zR = (z if nL >= 8 else 0), (z if nR >= 8 else 0)
    nl, nr = nL - zL, nR - zR
    own = iter(rng.permutation(np.arange(14, 118)))

    def place(octave):
        if rows == "one":
            y = 60.0 + float(rng.integers(0, 4)) * 0.25
        elif rows == "own":
            y = float(next(own)) + float(rng.integers(0, 4)) * 0.25
        else:
            y = float(rng.integers(14 * 4, 117 * 4)) * 0.25
        x = float(rng.integers(36 * 4, 112 * 4)) * 0.25
        return x, y

    for i in range(min(nl, nr)):
        octave = 7 if i % 4 == 3 else 0
        x, y = place(octave)
        s.pair(x, y, SHIFT, None, ham=int(rng.integers(0, 40)), octave=octave)
    for i in range(nl - min(nl, nr)):
        x, y = place(0)
        s.left(x, y, 0, s.desc())
    for i in range(nr - min(nl, nr)):
        x, y = place(0)
        s.right(x - SHIFT, y, 0, s.desc())
    L, R, kL, dL, kR, dR, bf, b, _ = s.finish()
    sc.check_reads_in_bounds((L, R, kL, dL, kR, dR, bf, b, {}), PYR)
    if zL:
        kL, dL = _zero_points(kL, dL, rng)
    if zR:
        kR, dR = _zero_points(kR, dR, rng)
    assert len(kL) == nL and len(kR) == nR
    return L, R, kL, dL, kR, dR


def _kps(xyo):
    a = np.zeros(len(xyo), sc.KP_DTYPE)
    for i, (x, y, o) in enumerate(xyo):
        a[i]["x"], a[i]["y"], a[i]["octave"] = x, y, o
    a["size"], a["response"], a["class_id"] = 31.0, 50.0, -1
    return a


def edge_set(kind, seed):
    """Keypoints the reference's row table has no row for; descriptors 0x00 (left) / 0xFF (right): nothing matches."""
    rng = np.random.default_rng(seed)
    xs = lambda n: [float(v) * 0.5 for v in rng.integers(0, 2 * W, n)]
    if kind == "one_row_own_row":      # left: 700 keypoints in row 0; right: one keypoint in every row 0 .. H - 1
        left = [(x, float(rng.integers(0, 4)) * 0.25, int(o)) for x, o in zip(xs(700), rng.integers(0, 8, 700))]
        right = [(x, float(r) + 0.5, 0) for x, r in zip(xs(H), rng.permutation(H))]
    elif kind == "last_row_clamps":    # left: row H - 1 and everything that clamps into rows 0 and H - 1; right: octaves 0 / 7 at the edges
        ys = [-0.25, -0.75, -3.5, -0.0, 0.0, 0.99, H - 1.0, H - 0.5, float(H), H + 0.5, H + 100.0, 1.0e6]
        left = [(x, ys[i % len(ys)], i % 8) for i, x in enumerate(xs(600))]
        ys = [0.0, 0.5, 1.0, H - 1.0, H - 0.5, 3.0, H - 4.0]
        right = [(x + 1.0, ys[i % len(ys)], (0, 7)[(i // len(ys)) % 2]) for i, x in enumerate(xs(70))]
        right = [(0.0, 0.0, 0)] + right[:35] + [(0.0, 0.0, 7)] + right[35:] + [(0.0, 0.0, 3)]
    else:
        raise KeyError(kind)
    kL, kR = _kps(left), _kps(right)
    return kL, np.zeros((len(kL), 32), np.uint8), kR, np.full((len(kR), 32), 255, np.uint8)


# every run: two pairs on one handle, (kind, arguments) per pair; the sizes of the issue: 0, 1, 63, 64, 65, 512, 513, 2048
# (the last index-permutation size) and 2049 (the first direct-scatter size), the two eyes of a pair always different
RUNS = {
    "n_0_1_63_64": [("in", (11, 0, 1)), ("in", (12, 63, 64))],
    "n_1_0_64_65": [("in", (13, 1, 0)), ("in", (14, 64, 65))],
    "n_65_512_513_2048": [("in", (15, 65, 512)), ("in", (16, 513, 2048))],
    "n_2048_2049": [("in", (17, 2048, 2049)), ("in", (18, 2049, 2048))],
    "one_row_and_own_rows": [("in", (19, 900, 700, "one")), ("in", (20, 100, 104, "own", False))],
    "edges": [("edge", ("one_row_own_row", 21)), ("edge", ("last_row_clamps", 22))],
}
_sets = {}


def _run_sets(name):
    """[(L, R, kL, dL, kR, dR, oracle-comparable)] of a run, built once and read-only."""
    if name not in _sets:
        out = []
        scene = sc.Scene(5, W, H, PYR, shift=SHIFT)
        for kind, args in RUNS[name]:
            if kind == "in":
                out.append(inbounds_set(*args) + (True,))
            else:
                out.append((scene.L, scene.R) + edge_set(*args) + (False,))
            for a in out[-1][:6]:
                a.setflags(write=False)
        _sets[name] = out
    return _sets[name]


@pytest.fixture(scope="module")
def refs(oracle):
    """(uRight, depth) of the C++ oracle per in-bounds set, computed once per run."""
    done = {}

    def get(name):
        if name not in done:
            res = []
            for L, R, kL, dL, kR, dR, comparable in _run_sets(name):
                if not comparable:
                    res.append((np.full(len(kL), -1, f32),) * 2)
                    continue
                eL, eR = oracle.OracleExtractor(100, *PYR), oracle.OracleExtractor(100, *PYR)
                eL.compute_pyramid(L)
                eR.compute_pyramid(R)
                res.append(oracle.stereo_match(eL, eR, kL, dL, kR, dR, sc.BF, sc.B))
            done[name] = res
        return done[name]

    yield get
    done.clear()


# ----------------------------------------------------------------------------------------------------------------- model
def band_words(k):
    """minr | maxr << 16 of the +-2 * scale row band (src/Frame.cc:943-948) in float32, maxr = -1 for a (0, 0) point."""
    scale, _ = sc.tables(*PYR)
    y = k["y"].astype(f32)
    r = (f32(2.0) * scale[k["octave"]]).astype(f32)
    maxr = np.ceil((y + r).astype(f32)).astype(np.int64)
    minr = np.floor((y - r).astype(f32)).astype(np.int64)
    maxr[(k["x"] == 0) & (k["y"] == 0)] = -1
    return ((minr & 0xFFFF) | ((maxr << 16) & 0xFFFF0000)).astype(np.uint32)


def rows_of(k):
    y = np.clip(k["y"].astype(np.float64), -1.0, float(H))      # (int)y truncates towards zero; then min / max into the image
    return np.clip(np.trunc(y).astype(np.int64), 0, H - 1)


def check_sorted(k, d, row_start, rec, dsc, tag):
    n = len(k)
    row = rows_of(k)
    counts = np.bincount(row, minlength=H)
    want = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    assert np.array_equal(row_start, want), (tag, "row table")
    rec, dsc = rec[:n], dsc[:n]
    idx = (rec[:, 2] >> 8).astype(np.int64)
    assert np.array_equal(np.sort(idx), np.arange(n)), (tag, "the index fields are not a permutation")
    # slot p lies in the row whose [row_start[r], row_start[r + 1]) holds it: with the permutation, every row's multiset
    assert np.array_equal(row[idx], np.repeat(np.arange(H), counts)), (tag, "a record outside its row")
    assert np.array_equal(rec[:, 0], k["x"].view(np.uint32)[idx]) and np.array_equal(rec[:, 1], k["y"].view(np.uint32)[idx]), tag
    assert np.array_equal(rec[:, 2] & 0xFF, k["octave"].astype(np.uint32)[idx]), tag
    assert np.array_equal(rec[:, 3], band_words(k)[idx]), (tag, "row band")
    assert np.array_equal(dsc, np.ascontiguousarray(d).view(np.uint32).reshape(n, 8)[idx]), (tag, "descriptor")


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def handle():
    import orb_slam3_fast_amd as orbx
    ex = orbx.ORBextractor(NF, PYR[0], PYR[1], 20, 7, max_width=W, max_height=H, max_batch=2 * NPAIRS)
    assert 2049 <= ex.capacity <= 4096
    yield ex
    ex.close()


def _associate(ex, sets):
    """The row-sorted form on the two pairs: (uRight, depth), then per pair the sorted arrays of both eyes."""
    import orb_slam3_fast_amd as orbx
    imgs = np.stack([s[0] for s in sets] + [s[1] for s in sets])
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    dbuf = DeviceBuffer.from_numpy(imgs)
    ex.extract_batch_device(dbuf.ptr.value, 2 * NPAIRS, W, H, W, W * H)
    ex.sync()
    for p, (_, _, kL, dL, kR, dR, _) in enumerate(sets):
        _upload(ex, p, kL, dL)
        _upload(ex, NPAIRS + p, kR, dR)
    L = orbx.lib()
    try:
        L.orbx_debug_set_stereo_direct(0)
        u, dep = orbx.ComputeStereoMatches(ex, ex, float(sc.BF), float(sc.B), first_left=0, first_right=NPAIRS, n_pairs=NPAIRS)
    finally:
        L.orbx_debug_set_stereo_direct(-1)
        dbuf.free()      # (level 0 of a device batch is the caller's frames: they stay until the association has read them)
    cap = ex.capacity
    tables = []
    for p in range(NPAIRS):
        rs, rec, dsc = np.zeros((2, H + 1), np.int32), np.zeros((2, cap, 4), np.uint32), np.zeros((2, cap, 8), np.uint32)
        assert orbx._check(L.orbx_debug_stereo_sort(ex._h, p, orbx._p(rs), orbx._p(rec), orbx._p(dsc), cap)) == cap
        tables.append((rs, rec, dsc))
    return u, dep, tables


def _check_run(name, refs, u, dep, tables):
    for p, ((_, _, kL, dL, kR, dR, comparable), (ou, od)) in enumerate(zip(_run_sets(name), refs(name))):
        n = len(kL)
        bad = np.nonzero(u[p, :n].view(np.uint32) != ou.view(np.uint32))[0]
        assert _same_bits(u[p, :n], ou), (name, p, bad[:8], u[p, bad[:8]], ou[bad[:8]], kL[bad[:8]])
        assert _same_bits(dep[p, :n], od), (name, p)
        if comparable and min(len(kL), len(kR)) >= 63:
            assert (ou >= 0).sum() > 0, (name, p)      # (the comparison decides something)
        rs, rec, dsc = tables[p]
        check_sorted(kL, dL, rs[0], rec[0], dsc[0], (name, p, "left"))
        check_sorted(kR, dR, rs[1], rec[1], dsc[1], (name, p, "right"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUNS))
def test_stereo_sort_crafted_sizes(refs, handle, name):
    u, dep, tables = _associate(handle, _run_sets(name))
    _check_run(name, refs, u, dep, tables)


@pytest.mark.gpu
def test_stereo_sort_on_poisoned_work_buffers(refs, handle):
    """The large run, then the small one in the same slots, each on work buffers poisoned beforehand: stale rows, records or
    anything read past n would change the row table, a row's multiset or a result bit."""
    from scratch_cases import POISON
    for byte, name in zip(POISON[1:], ("n_2048_2049", "n_0_1_63_64")):
        handle.debug_fill_work_buffers(byte)
        u, dep, tables = _associate(handle, _run_sets(name))
        _check_run(name, refs, u, dep, tables)


def test_sets_have_the_sizes_and_rows_they_are_named_for():
    """No GPU: the sets hold what the cases are about."""
    sizes = sorted({len(s[i]) for name in RUNS if name.startswith("n_") for s in _run_sets(name) for i in (2, 4)})
    assert sizes == [0, 1, 63, 64, 65, 512, 513, 2048, 2049]
    for name in RUNS:
        for s in _run_sets(name):
            assert len(s[2]) != len(s[4])
    one, own = _run_sets("one_row_and_own_rows")
    assert len(set(rows_of(one[2]))) <= 2 and len(set(rows_of(own[4])) - {0}) == len(own[4])   # (row 0: the (0, 0) points)
    e0, e1 = _run_sets("edges")
    assert set(rows_of(e0[2])) == {0} and sorted(rows_of(e0[4])) == list(range(H))
    r = rows_of(e1[2])
    assert set(r) == {0, H - 1} and (e1[2]["y"] < 0).any() and (e1[2]["y"] >= H).any()
    assert ((e1[4]["x"] == 0) & (e1[4]["y"] == 0)).nonzero()[0].tolist() == [0, 36, len(e1[4]) - 1]
    assert {0, 7} <= set(e1[4]["octave"]) and {0, H - 1} <= set(rows_of(e1[4]))
    w = band_words(e1[4])
    assert (w[[0, 36]] >> 16 == 0xFFFF).all() and ((w & 0xFFFF) > 0x8000).any()      # maxr = -1; a negative minr
