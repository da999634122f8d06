"""k_octree with workgroups of 128, 256 and 512 threads and the batch's launch that gives every level its class of the plan: every
class, under every candidate path (orbx_debug_set_octree_global 0 / 1 / 2), gives the oracle's keypoints -- the selection per level
and the final 28-byte records and descriptors, bit for bit.

Every case goes through the batched device entry with at least three images: launches of one or two images keep 512 threads at
every level, so only larger batches run the plan under hook 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orb_slam3_fast_amd as orbx
from orb_slam3_fast_amd import synth

CLASSES = (128, 256, 512, 0)   # orbx_debug_set_octree_class: 0 = the plan
PATHS = (0, 1, 2)              # orbx_debug_set_octree_global: histogram variant, global-memory candidates, per-pass sweeps
OCT_KMAX = 32                  # register-resident candidates per thread (orbx_octree.hip)


@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


def _kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 28)


def _want(oracle, imgs, nf, nl):
    """Oracle results of each distinct image, computed once: (mono, keypoints, descriptors, candidates per level, selected per level)."""
    out, seen = [], {}
    for img in imgs:
        key = id(img)
        if key not in seen:
            oe = oracle.OracleExtractor(nf, 1.2, nl, 20, 7)
            mono, k, d = oe.extract(img)
            ncand = np.array([len(oe.detect_candidates(l)["x"]) for l in range(nl)])
            seen[key] = (mono, k, d, ncand, np.bincount(k["octave"], minlength=nl))
        out.append(seen[key])
    return out


def _check_all(ex, imgs, want, nl, label, classes=CLASSES, paths=PATHS):
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    h, w = imgs[0].shape
    d = DeviceBuffer.from_numpy(np.stack(imgs))
    L = orbx.lib()
    try:
        for nt in classes:
            for path in paths:
                L.orbx_debug_set_octree_class(nt)
                L.orbx_debug_set_octree_global(path)
                ex.extract_batch_device(d.ptr.value, len(imgs), w, h, w, w * h)
                ex.sync()
                for i, (omono, ok_, od, ncand, nsel) in enumerate(want):
                    mono, k, dd = ex.download(i)
                    st = ex.level_stats(i)
                    tag = (label, nt, path, i)
                    assert np.array_equal(st[2], ncand), tag            # the candidates the quadtree was given
                    assert np.array_equal(st[3], nsel), tag             # its selection, per level
                    assert mono == omono and np.array_equal(_kp_bytes(k), _kp_bytes(ok_)) and np.array_equal(dd, od), tag
    finally:
        L.orbx_debug_set_octree_class(0)
        L.orbx_debug_set_octree_global(0)


def test_small_batch_textured_flat_and_single_blob(gpu, oracle):
    """Three 320 x 240 images, 8 levels, 500 features: a textured one; a flat one (n = 0 at every level, and the top levels have
    fewer FAST cells than any block has threads); one bright blob, so that some levels hold 1 - 3 candidates, fewer than roots."""
    w, h, nf, nl = 320, 240, 500, 8
    tex = synth.mono_frame(w, h, 31)
    flat = np.full((h, w), 120, np.uint8)
    blob = flat.copy()
    yy, xx = np.mgrid[0:h, 0:w]
    blob[(yy - 118) ** 2 + (xx - 171) ** 2 <= 5 ** 2] = 250
    imgs = [tex, flat, blob]
    want = _want(oracle, imgs, nf, nl)
    assert want[1][3].sum() == 0                                       # flat: no candidate at any level
    assert ((want[2][3] >= 1) & (want[2][3] <= 3)).any(), want[2][3]   # blob: levels with 1 - 3 candidates
    assert (want[0][3] > 128).any()                                    # textured: more candidates than a block has threads
    ex = orbx.ORBextractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=3)
    _check_all(ex, imgs, want, nl, "small")


@pytest.mark.parametrize("w,h,over", [(276, 207, 128), (372, 279, 256)])
def test_more_candidates_than_the_registers_of_a_class_hold(gpu, oracle, w, h, over):
    """Dense noise, the smallest 4 : 3 size (in steps of 4 px) whose level 0 holds more than OCT_KMAX * 128 = 4096 candidates, and
    the smallest with more than OCT_KMAX * 256 = 8192: with that class (or a smaller one) forced, the level hands over to the
    global-memory path -- the same hand-over a 512-thread block makes above 16384."""
    nf, nl = 1000, 6
    noise = np.random.default_rng(19).integers(0, 256, (h, w), dtype=np.uint8)
    imgs = [noise, noise, noise]
    want = _want(oracle, imgs, nf, nl)
    n0 = int(want[0][3][0])
    assert OCT_KMAX * over < n0 <= OCT_KMAX * over * 2, n0   # the case exercises this class's overflow and not the next one's
    ex = orbx.ORBextractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=3)
    _check_all(ex, imgs, want, nl, "overflow %d" % over)


def test_level_quota_met_exactly_and_missed_by_one(gpu, oracle):
    """nfeatures chosen so that the quota of level 7 equals the number of FAST candidates the oracle finds there (every candidate a
    node: the quadtree stops by its size), and is one more than it (the quota cannot be met: it stops because no node splits)."""
    w, h, nl = 640, 480, 8
    img = (synth.mono_frame(w, h, 44) // 4 + 90).astype(np.uint8)   # low contrast: tens of candidates at level 7, not hundreds
    probe = oracle.OracleExtractor(1000, 1.2, nl, 20, 7)
    probe.extract(img)
    c7 = len(probe.detect_candidates(nl - 1)["x"])
    assert 8 <= c7 <= 200
    imgs = [img, img, img]
    for target in (c7, c7 + 1):
        nf = next(n for n in range(10 * target, 40 * target)
                  if oracle.OracleExtractor(n, 1.2, nl, 20, 7).tables()["nfeat"][nl - 1] == target)
        want = _want(oracle, imgs, nf, nl)
        assert want[0][3][nl - 1] == c7 and oracle.OracleExtractor(nf, 1.2, nl, 20, 7).tables()["nfeat"][nl - 1] == target
        ex = orbx.ORBextractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=3)
        _check_all(ex, imgs, want, nl, "quota %d of %d" % (target, c7))


def test_the_plan_at_the_benchmark_size(gpu, oracle):
    """One 1280 x 720 stereo pair (in a batch of three images, so that the plan runs: levels of 512, 256 and 128 working threads in
    one launch): hook 0 against the oracle and against 512 threads at every level, bit for bit."""
    from orb_slam3_fast_amd.hipmem import DeviceBuffer
    w, h, nf, nl = 1280, 720, 1500, 8
    nt, _ = orbx.octree_plan(nf, 1.2, nl, 20, 7, w, h)
    assert len(set(nt.tolist())) == 3            # all three classes in the launch
    left, right = synth.stereo_pair(w, h, 9)
    imgs = [left, right, left]
    want = _want(oracle, imgs, nf, nl)
    ex = orbx.ORBextractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=3)
    d = DeviceBuffer.from_numpy(np.stack(imgs))
    L = orbx.lib()
    res = {}
    try:
        for hook in (0, 512):
            L.orbx_debug_set_octree_class(hook)
            ex.extract_batch_device(d.ptr.value, 3, w, h, w, w * h)
            ex.sync()
            res[hook] = [ex.download(i) for i in range(3)]
    finally:
        L.orbx_debug_set_octree_class(0)
    for i in range(3):
        assert res[0][i][0] == res[512][i][0] and res[0][i][1].tobytes() == res[512][i][1].tobytes()
        assert np.array_equal(res[0][i][2], res[512][i][2])
        omono, ok_, od = want[i][:3]
        assert res[0][i][0] == omono and np.array_equal(_kp_bytes(res[0][i][1]), _kp_bytes(ok_)) and np.array_equal(res[0][i][2], od)
