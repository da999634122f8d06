"""No entry may read device memory before something of the same call has written it.

The one-shot entries take their device memory from a pool that hands cached hipMalloc blocks back as they are, upload their
inputs through a staging buffer of which only the items' own bytes are rewritten, and the extractor handle's buffers only ever
grow: a kernel that read an accumulator, a counter, a status word or a list length that nothing of its chain had cleared would
see what an EARLIER call left there -- the same thing on every run of a suite that runs its files in one order, something else
in an application.  The tests here decide what that memory holds (orbx_debug_scratch_pool, orbx_debug_fill_work_buffers) and
require the same bytes out, whatever it was: zeros, NaN / -1 (0xFF) or large finite values (0x55).

  - every one-shot entry of include/orbx.h: tests/scratch_cases.py, protocol in scratch_cases.run_protocol;
  - the extractor handle: a device batch with its stereo association, bag of words and a device-side projection search; the
    single-frame host entries (also with their pipeline captured into a graph); a small frame after a dense one;
  - without a GPU: every exported entry is a case or excluded for a stated reason, every device buffer of the handle is
    classified, and the hooks check their arguments before they touch a device.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx
import scratch_cases as sc
from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ without a GPU
# Every exported entry that is not a case of the table, with the reason.  A new entry has to go into one of the two lists.
LIFECYCLE = "lifecycle: creates, configures, destroys or synchronises a handle"
GETTER = "getter: copies results or tables out, or hands out device pointers; launches nothing"
HOST = "host only: touches no device"
COMM = "comm: RCCL collectives on the caller's buffers"
PROFILING = "profiling and probes"
HANDLE = "batched entry on an extractor handle: the handle sequences below cover its buffers"
UPLOAD = "upload of the caller's data into a handle"
OUT_OF_SCOPE = "key-frame database and pre-processing handles: out of scope (their protocol state needs a classification of its own)"
EXCLUDED = {
    **{s: LIFECYCLE for s in ("orbx_extractor_create", "orbx_extractor_destroy", "orbx_sync", "orbx_stream_handle", "orbx_set_host_pyramid",
                              "orbx_set_opencv_compat", "orbx_vocabulary_create", "orbx_vocabulary_destroy", "orbx_vocabulary_load_text",
                              "orbx_merge_ba_stop_after_first")},
    **{s: GETTER for s in ("orbx_abi_version", "orbx_device_count", "orbx_last_error", "orbx_get_tables", "orbx_stage_name",
                           "orbx_vocabulary_info", "orbx_batch_download", "orbx_batch_download_async", "orbx_batch_results_device",
                           "orbx_bow_download", "orbx_bow_results_device", "orbx_fisheye_download", "orbx_fisheye_results_device",
                           "orbx_host_pyramid_level", "orbx_host_results", "orbx_level_stats", "orbx_pyramid_download", "orbx_pyramid_level",
                           "orbx_stereo_download", "orbx_stereo_results_device")},
    **{s: HOST for s in ("orbx_hamming256", "orbx_mlpnp_ransac_parameters", "orbx_sim3_ransac_parameters")},
    **{s: COMM for s in ("orbx_allgather_descriptors", "orbx_comm_adopt", "orbx_comm_create", "orbx_comm_destroy", "orbx_comm_size",
                         "orbx_comm_unique_id", "orbx_comm_wait")},
    **{s: PROFILING for s in ("orbx_clock_probe_finish", "orbx_clock_probe_start", "orbx_copy_probe", "orbx_profile_collect",
                              "orbx_profile_enable")},
    **{s: HANDLE for s in ("orbx_extract", "orbx_extract_batch", "orbx_extract_batch_device", "orbx_extract_stereo", "orbx_extract_rgbd",
                           "orbx_rgbd_depth_batch", "orbx_stereo_match_batch", "orbx_fisheye_stereo_match_batch", "orbx_bow_transform_batch",
                           "orbx_project_map_points_batch", "orbx_project_map_points_fisheye_batch", "orbx_project_last_frames_batch",
                           "orbx_search_by_projection_batch", "orbx_search_by_projection_frame_batch",
                           "orbx_search_by_projection_fisheye_batch", "orbx_search_by_projection_frame_fisheye_batch",
                           "orbx_search_for_initialization_batch", "orbx_search_by_bow_batch")},
    **{s: UPLOAD for s in ("orbx_map_upload", "orbx_last_frames_upload")},
    **{s: OUT_OF_SCOPE for s in ("orbx_kfdb_add", "orbx_kfdb_add_from_batch", "orbx_kfdb_clear", "orbx_kfdb_clear_map", "orbx_kfdb_create",
                                 "orbx_kfdb_create_sized", "orbx_kfdb_destroy", "orbx_kfdb_detect_n_best_candidates",
                                 "orbx_kfdb_detect_relocalization_candidates", "orbx_kfdb_detect_relocalization_candidates_batch",
                                 "orbx_kfdb_erase", "orbx_kfdb_profile", "orbx_kfdb_set_covisibles", "orbx_kfdb_size", "orbx_preproc_create",
                                 "orbx_preproc_destroy", "orbx_preproc_output_size", "orbx_preproc_run", "orbx_preproc_run_device",
                                 "orbx_extract_batch_raw_device")},
}
# the entries this file was written for: each must be a case (a table that lost one fails here, not silently)
REQUIRED = """orbx_bf_knn2 orbx_search_for_initialization orbx_features_in_area orbx_search_by_projection orbx_search_by_projection_frame
orbx_search_by_projection_keyframe orbx_search_for_triangulation orbx_search_for_triangulation_rig orbx_search_by_bow
orbx_search_by_bow_keyframes orbx_fuse_search orbx_fisheye_stereo_match orbx_search_by_projection_fisheye
orbx_search_by_projection_frame_fisheye orbx_undistort_keypoints orbx_bow_transform orbx_cvt_gray orbx_resize_linear orbx_remap_linear
orbx_clahe orbx_pose_optimization orbx_pose_optimization_batch orbx_pose_optimization_kb8 orbx_pose_optimization_fisheye_batch
orbx_reconstruct_two_views orbx_reconstruct_two_views_batch orbx_mlpnp_iterate orbx_mlpnp_iterate_batch orbx_sim3_iterate
orbx_sim3_iterate_batch orbx_optimize_sim3 orbx_optimize_sim3_batch orbx_pose_inertial_optimization_last_keyframe
orbx_pose_inertial_optimization_last_frame orbx_pose_inertial_optimization_last_keyframe_batch
orbx_pose_inertial_optimization_last_frame_batch orbx_local_bundle_adjustment orbx_local_bundle_adjustment_rig orbx_bundle_adjustment
orbx_bundle_adjustment_rig orbx_merge_bundle_adjustment orbx_merge_bundle_adjustment_rig orbx_optimize_pose_graph
orbx_pose_graph_evaluate orbx_triangulate_matches orbx_create_new_map_points""".split()
VARIANTS = ("orbx_search_by_projection_keyframe:small_capacity", "orbx_pose_inertial_optimization_last_keyframe:device_staging",
            "orbx_pose_inertial_optimization_last_frame:device_staging", "orbx_bundle_adjustment:past_128_keyframes",
            "orbx_optimize_pose_graph:chain")


def test_every_exported_entry_is_a_case_or_excluded_for_a_reason():
    lib = orbx.lib()
    syms = declared_symbols()
    assert len(syms) > 150 and all(hasattr(lib, s) for s in syms)
    entries = {sc.entry_of(n) for n in sc.CASES}
    for s in syms:
        if s.startswith("orbx_debug_"):
            assert s not in entries and s not in EXCLUDED, s          # the hooks are one class: no list of them to keep
            continue
        assert (s in entries) != (s in EXCLUDED), "%s is %s" % (s, "in both lists" if s in entries else "neither a case nor excluded")
    assert not (entries | set(EXCLUDED)) - set(syms), sorted((entries | set(EXCLUDED)) - set(syms))
    assert not set(REQUIRED) - entries, sorted(set(REQUIRED) - entries)
    assert not set(VARIANTS) - set(sc.CASES)
    assert all(isinstance(r, str) and r for r in EXCLUDED.values())


def test_every_extractor_buffer_is_classified():
    """csrc/orbx_host.h: every DevBuf member of orbx_extractor stands in ORBX_EXTRACTOR_BUFFERS exactly once, under one of the
    four classes, and the members the hook must leave alone are not WORK."""
    src = open(os.path.join(ROOT, "orb_slam3_fast_amd", "csrc", "orbx_host.h")).read()
    body = src[src.index("struct orbx_extractor {"):]
    body = body[:body.index("\n};")]
    members = []
    for decl in re.findall(r"^\s*DevBuf<[^;]*?>\s+([^;]+);", body, flags=re.M):
        members += [m.strip() for m in decl.split(",")]
    assert len(members) >= 60 and len(set(members)) == len(members)
    table = src[src.index("#define ORBX_EXTRACTOR_BUFFERS("):]
    table = re.sub(r"/\*.*?\*/", "", table[:table.index("\n\n")], flags=re.S)
    listed = re.findall(r"\b(WORK|TABLE|UPLOAD|STATE)\((\w+)\)", table)
    names = [m for _, m in listed]
    assert sorted(names) == sorted(members), (sorted(set(members) - set(names)), sorted(set(names) - set(members)))
    cls = dict((m, c) for c, m in listed)
    for m in ("d_xtab", "d_yrow", "d_rsRec", "d_cellRec", "d_yofs", "d_yab", "d_tailBands", "d_latBands"):
        assert cls[m] == "TABLE", m
    for m in ("d_mapPos", "d_mapDesc", "d_lfPos", "d_lfN", "d_poses", "d_posesQ", "d_posesK", "d_lap", "d_mapSkip"):
        assert cls[m] == "UPLOAD", m
    assert cls["d_packCtr"] == "STATE"
    for m in ("d_cand", "d_cellCand", "d_sel", "d_cellCount", "d_cellPrefix", "d_candCount", "d_selCount", "d_slot", "d_nOut", "d_mono",
              "d_kps", "d_desc", "d_stage", "d_pyr", "d_srec", "d_sdesc", "d_sad", "d_uR", "d_depth", "d_fl2r", "d_fcand", "d_bowWord",
              "d_bowWords", "d_views", "d_pviews", "d_fviewsL", "d_fviewsR", "d_blur"):
        assert cls[m] == "WORK", m


def test_hooks_check_their_arguments_before_any_device():
    L = orbx.lib()
    out = np.zeros(4, np.uint64)
    far = 1 << 20                                                    # a device that does not exist: never reached
    assert L.orbx_debug_scratch_pool(far, 3, 0, orbx._p(out)) == orbx.E_BADARG
    assert L.orbx_debug_scratch_pool(far, -1, 0, orbx._p(out)) == orbx.E_BADARG
    assert L.orbx_debug_scratch_pool(far, orbx.SCRATCH_STATS, 0, None) == orbx.E_BADARG
    assert L.orbx_debug_scratch_pool(far, orbx.SCRATCH_FILL, 0, None) == orbx.E_BADARG
    assert L.orbx_debug_scratch_pool(far, orbx.SCRATCH_FILL, 256, orbx._p(out)) == orbx.E_BADARG
    assert L.orbx_debug_scratch_pool(far, orbx.SCRATCH_FILL, -1, orbx._p(out)) == orbx.E_BADARG
    assert b"fill value" in L.orbx_last_error()
    assert L.orbx_debug_fill_work_buffers(None, 0) == orbx.E_BADARG and b"null handle" in L.orbx_last_error()
    assert not out.any()
    for op in (orbx.SCRATCH_STATS, orbx.SCRATCH_FILL, orbx.SCRATCH_TRIM):      # valid arguments and no such device
        rc = L.orbx_debug_scratch_pool(far, op, 0x55, orbx._p(out))
        assert rc == (orbx.E_NODEVICE if orbx.device_count() == 0 else orbx.E_BADARG), (op, rc)
    if orbx.device_count() == 0:
        with pytest.raises(orbx.OrbxError) as e:
            orbx.scratch_pool_stats()
        assert e.value.code == orbx.E_NODEVICE


def test_flatten_and_first_difference():
    a = dict(x=np.arange(6, dtype=np.float32).reshape(2, 3), n=3, s=[1.5, None], r=np.zeros(1, orbx.KP_DTYPE)[0])
    b = dict(a, x=a["x"].copy())
    assert sc.first_difference(sc.flatten(a), sc.flatten(b)) is None
    b["x"][1, 2] = np.nan
    assert "result['x'] differs" in sc.first_difference(sc.flatten(a), sc.flatten(b))
    assert "result['n']" in sc.first_difference(sc.flatten(a), sc.flatten(dict(a, n=4)))
    assert sc.first_difference(sc.flatten(a), sc.flatten(dict(a, extra=1))) == "the results are not made of the same outputs"
    assert sc.flatten(a["x"]) != sc.flatten(a["x"].astype(np.float64)) and sc.flatten(a["x"]) != sc.flatten(a["x"].reshape(3, 2))


# ------------------------------------------------------------------------------------------------ the pool itself
@pytest.fixture(scope="module")
def gpu():
    if orbx.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.mark.gpu
def test_pool_hook_counts_fills_and_trims(gpu):
    d = np.arange(64 * 32, dtype=np.uint8).reshape(64, 32)
    orbx.scratch_pool_trim()
    blocks, cached, takes, hits = orbx.scratch_pool_stats()
    assert (blocks, cached) == (0, 0) and orbx.scratch_pool_fill(0xFF) == 0
    orbx.bf_knn2(d, d)                                               # one Pack: one block of the 8 KiB class
    s1 = orbx.scratch_pool_stats()
    assert s1[0] >= 1 and s1[1] >= 4096 and s1[2] - takes >= 1 and s1[3] == hits          # allocated, not served
    assert orbx.scratch_pool_fill(0x55) == s1[1]
    orbx.bf_knn2(d, d)
    s2 = orbx.scratch_pool_stats()
    assert s2[:2] == s1[:2] and s2[2] - s1[2] == s2[3] - s1[3] >= 1                          # served from the cache
    orbx.scratch_pool_trim()
    assert orbx.scratch_pool_stats()[:2] == (0, 0)
    orbx.bf_knn2(d, d)
    s3 = orbx.scratch_pool_stats()
    assert s3[3] == s2[3] and s3[2] > s2[2]                                                    # fresh again after the trim


# ------------------------------------------------------------------------------------------------ the one-shot entries
IN_PROCESS = [n for n in sc.CASES if n not in sc.SMALL_CAPACITY]


@pytest.mark.gpu
@pytest.mark.parametrize("name", IN_PROCESS)
def test_one_shot_entry_on_poisoned_scratch(gpu, oracle, name):
    report = sc.run_protocol(name, oracle)
    assert not report, (name, report)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(sc.SMALL_CAPACITY))
def test_forced_retry_on_poisoned_scratch_in_a_fresh_process(gpu, name):
    """The knob is read once per process, hence the child: the same protocol on a case whose first attempt runs against a full
    candidate array and is repeated with the exact size."""
    code = ("import json, sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nfrom oracle import oracle_py\nimport scratch_cases as sc\n"
            "print(json.dumps(dict(report=sc.run_protocol(%r, oracle_py))))\n" % (ROOT, os.path.join(ROOT, "tests"), name))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **sc.SMALL_CAPACITY[name]), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["report"] == [], out.stdout[-1000:]


# ------------------------------------------------------------------------------------------------ the extractor handle
W, H, NF, NL = 160, 120, 300, 3          # the smallest size of tests/test_gpu_parity.py
BF, B = 0.12 * 532.03, 0.12


def _kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 28)


class Sequence:
    """One handle, a batch of two stereo pairs (L0 L1 R0 R1): extraction, stereo association, bag of words, and a device-side
    projection of an uploaded map with the search on its view lists.  run() downloads everything."""

    def __init__(self):
        from orb_slam3_fast_amd import synth
        from orb_slam3_fast_amd.hipmem import DeviceBuffer
        from test_projection_device import _scene
        self.pairs = [synth.stereo_pair(W, H, 40 + i) for i in range(2)]
        self.dev = DeviceBuffer.from_numpy(np.stack([p[0] for p in self.pairs] + [p[1] for p in self.pairs]))
        self.ex = orbx.ORBextractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=4)
        self.cols = synth.make_vocabulary(5, 3, seed=8, early_leaf_prob=0.08, stop_prob=0.04)
        self.voc = orbx.ORBVocabulary(5, 3, *self.cols)
        self.bounds = (0.0, 0.0, float(W), float(H))
        first = self.extract()
        rng = np.random.default_rng(31)
        self.poses, pos, nrm, mind, maxd, desc, flags = _scene(rng, W, H, 2, [f[1] for f in first[:2]], [f[2] for f in first[:2]], fx=110.0)
        self.map = (pos, nrm, mind, maxd, desc, flags)
        self.skip = (rng.random((2, len(pos))) < 0.05).astype(np.uint8)
        self.occ = (rng.random((2, self.ex.capacity)) < 0.04).astype(np.uint8)
        self.ex.map_upload(*self.map)                                # the caller's data: the hook leaves it alone

    def extract(self):
        self.ex.extract_batch_device(self.dev.ptr.value, 4, W, H, W, W * H)
        return [self.ex.download(i) for i in range(4)]

    def run(self):
        ex = self.ex
        frames = self.extract()
        u, dep = orbx.ComputeStereoMatches(ex, ex, BF, B, first_left=0, first_right=2, n_pairs=2)
        self.voc.transform_batch(ex, 1)
        bow = [orbx.ORBVocabulary.download(ex, i) for i in range(4)]
        views = ex.project_map_points(self.poses, self.bounds, 0.5, self.skip, want_views=True)
        found = orbx.ORBmatcher(0.8, True).SearchByProjectionBatchDevice(ex, 0, 2, self.bounds, self.occ, th=3.0, stereo_pair0=0)
        # (rows of uRight / depth past a left image's keypoint count are neither read nor written: include/orbx.h,
        # tests/test_rgbd.py::test_first_image_subrange_untouched_rows_and_invalidation; what is compared is what every parity test compares)
        n = [len(frames[i][1]) for i in range(2)]
        return dict(frames=frames, u=[u[i, :n[i]] for i in range(2)], dep=[dep[i, :n[i]] for i in range(2)], bow=bow, views=views, found=found)

    def check(self, r, oracle):
        ovoc = oracle.Vocabulary(5, 3, *self.cols)
        from test_bow import _same_transform
        oes = []
        for i in range(4):
            oe = oracle.OracleExtractor(NF, 1.2, NL, 20, 7)
            omono, ok, od = oe.extract(self.pairs[i % 2][i // 2])
            mono, k, d = r["frames"][i]
            assert mono == omono and np.array_equal(_kp_bytes(k), _kp_bytes(ok)) and np.array_equal(d, od), i
            _same_transform(r["bow"][i], ovoc.transform(od, 1))
            oes.append((oe, ok, od))
        sf = self.ex.GetScaleFactors()
        total = 0
        for i in range(2):
            (oL, okL, odL), (oR, okR, odR) = oes[i], oes[2 + i]
            ou, odp = oracle.stereo_match(oL, oR, okL, odL, okR, odR, BF, B)
            n = len(okL)
            assert sc.same(r["u"][i], ou) and sc.same(r["dep"][i], odp), i
            nm, match, occ = r["found"]
            on, om, oo = oracle.search_by_projection(okL, odL, r["u"][i], self.bounds, sf, r["views"][i], 3.0, False, 50.0, 0.8,
                                                     self.occ[i, :n])
            assert nm[i] == on and np.array_equal(match[i, :n], om) and np.array_equal(occ[i, :n], oo), i
            total += on
        assert total > 0 and len(oes[0][1]) > 30


@pytest.mark.gpu
def test_handle_sequence_on_poisoned_work_buffers(gpu, oracle):
    s = Sequence()
    a = s.run()
    s.check(a, oracle)
    flat = sc.flatten(a)
    for byte in (0xFF, 0x55):
        s.ex.debug_fill_work_buffers(byte)
        d = sc.first_difference(flat, sc.flatten(s.run()))
        assert d is None, "after a fill with 0x%02X: %s" % (byte, d)


def _host_entries():
    """orbx_extract and orbx_extract_stereo on one handle: clean, then after a fill with 0xFF and with 0x55.  Returns the
    differences (none expected) and the first result."""
    from orb_slam3_fast_amd import synth
    L, R = synth.stereo_pair(W, H, 66)
    ex = orbx.ORBextractor(NF, 1.2, NL, 20, 7, max_width=W, max_height=H, max_batch=2)

    def run():
        return dict(mono=ex(L, (0, 0)), lapped=ex(R, (20, 140)), stereo=ex.extract_stereo(L, R, bf=BF, b=B))
    a = run()
    flat, report = sc.flatten(a), []
    for byte in (0xFF, 0x55):
        ex.debug_fill_work_buffers(byte)
        d = sc.first_difference(flat, sc.flatten(run()))
        if d:
            report.append("after a fill with 0x%02X: %s" % (byte, d))
    return report, a, (L, R)


def _check_host_entries(a, L, R, oracle):
    oL, oR = oracle.OracleExtractor(NF, 1.2, NL, 20, 7), oracle.OracleExtractor(NF, 1.2, NL, 20, 7)
    for got, want in ((a["mono"], oL.extract(L, (0, 0))), (a["lapped"], oR.extract(R, (20, 140)))):
        assert got[0] == want[0] and np.array_equal(_kp_bytes(got[1]), _kp_bytes(want[1])) and np.array_equal(got[2], want[2])
    (mL, kL, dL), (mR, kR, dR), (u, dep) = a["stereo"]
    omL, okL, odL = oL.extract(L)
    omR, okR, odR = oR.extract(R)
    assert (mL, mR) == (omL, omR) and np.array_equal(_kp_bytes(kL), _kp_bytes(okL)) and np.array_equal(dR, odR)
    ou, od = oracle.stereo_match(oL, oR, okL, odL, okR, odR, np.float32(BF), np.float32(B))
    assert sc.same(u, ou) and sc.same(dep, od)


@pytest.mark.gpu
def test_single_frame_host_entries_on_poisoned_work_buffers(gpu, oracle):
    report, a, (L, R) = _host_entries()
    assert not report, report
    _check_host_entries(a, L, R, oracle)


@pytest.mark.gpu
def test_single_frame_host_entries_with_a_captured_pipeline_in_a_fresh_process(gpu):
    """ORBX_GRAPH=1 (read once per process) replays orbx_extract's pipeline from a captured graph.  The hook moves no buffer, so the
    graph stays valid; what it replays must not depend on the buffers' contents either."""
    code = ("import json, sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nfrom oracle import oracle_py\nimport test_scratch_reuse as t\n"
            "report, a, (L, R) = t._host_entries()\nt._check_host_entries(a, L, R, oracle_py)\nprint(json.dumps(dict(report=report)))\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ORBX_GRAPH="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["report"] == [], out.stdout[-1000:]


@pytest.mark.gpu
def test_small_flat_frame_after_a_dense_one_equals_a_fresh_handle(gpu, oracle):
    """A dense frame at the handle's maximum size leaves long lists and high counts in every buffer; after a fill, a much
    smaller low-contrast frame must come out as on a handle that has seen nothing else."""
    from orb_slam3_fast_amd import synth
    w, h = 640, 480
    rng = np.random.default_rng(5)
    dense = (rng.integers(0, 2, (h // 4, w // 4), dtype=np.uint8) * 255).repeat(4, 0).repeat(4, 1)       # corners everywhere
    small = (synth.mono_frame(384, 288, 16) // 8 + 90).astype(np.uint8)                                 # low contrast: min-threshold cells
    for byte in (0xFF, 0x55):
        ex = orbx.ORBextractor(800, 1.2, 8, 20, 7, max_width=w, max_height=h)
        mono, k, d = ex(dense, (0, 0))
        assert len(k) >= 400
        ex.debug_fill_work_buffers(byte)
        got = ex(small, (0, 0))
        fresh = orbx.ORBextractor(800, 1.2, 8, 20, 7, max_width=w, max_height=h)(small, (0, 0))
        assert sc.first_difference(sc.flatten(fresh), sc.flatten(got)) is None, byte
        want = oracle.OracleExtractor(800).extract(small, (0, 0))
        assert got[0] == want[0] and np.array_equal(_kp_bytes(got[1]), _kp_bytes(want[1])) and np.array_equal(got[2], want[2])
