"""bench.py prints exactly one JSON line with the contract's keys (tiny configurations of every mode)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline"}


def _run(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True)
    return r


def test_bench_refuses_to_run_without_a_gpu_or_prints_json():
    import orb_slam3_fast_amd as orbx
    r = _run(["--steps", "2", "--warmup", "1", "--pairs", "2", "--width", "320", "--height", "240", "--nfeatures", "300", "--cpu-pairs", "0"])
    if orbx.device_count() == 0:
        assert r.returncode != 0 and "needs a GPU" in (r.stderr + r.stdout)  # no CPU fallback
    else:
        assert r.returncode == 0


def test_gpus_n_never_comes_from_one_process():
    """`bench.py --gpus 2` started WITHOUT a launcher must either become 2 real ranks (torch.distributed.run re-exec, needs 2
    devices) or exit non-zero: a single process can never print an n_gpus = 2 line (round-2 VERDICT: it multiplied by N)."""
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--pairs", "2",
                        "--width", "320", "--height", "240", "--nfeatures", "300", "--cpu-pairs", "0", "--no-extras"],
                       cwd=ROOT, capture_output=True, text=True, env=env)
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    if have < 2:
        assert r.returncode == 2 and "refusing to run" in r.stderr and not lines
    else:
        d = json.loads(lines[-1])
        assert r.returncode == 0 and d["n_gpus"] == 2 and d["rccl_ranks"] == 2
    # and a launcher that provides ONE rank while the flag says 2 is refused too
    env1 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2"], cwd=ROOT,
                       capture_output=True, text=True, env=env1)
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout) and not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_self_launch_path_prints_the_contract_line():
    """--self-launch: bench.py re-executes itself under torch.distributed.run (here with ONE rank) and rank 0 prints the
    same single contract line; n_gpus / rccl_ranks are the size of the RCCL group that ran."""
    r = _run(["--self-launch", "--full", "--steps", "3", "--warmup", "1", "--pairs", "2", "--width", "320", "--height", "240",
              "--nfeatures", "300", "--cpu-pairs", "0", "--no-extras"])
    assert r.returncode == 0, r.stderr[-800:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["rccl_ranks"] == 1 and d["launcher"].startswith("self") and d["value"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["stereo", "mono", "fisheye"])
def test_bench_prints_one_contract_line(mode):
    size = ["--width", "256", "--height", "256"] if mode == "fisheye" else ["--width", "320", "--height", "240"]
    r = _run(["--full", "--mode", mode, "--steps", "3", "--warmup", "1", "--pairs", "2", "--nfeatures", "300", "--cpu-pairs",
              "4" if mode == "stereo" else "0", "--latency-frames", "12", "--h2d-steps", "4"] + size)
    assert r.returncode == 0, r.stderr[-600:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert KEYS <= set(d) and d["value"] > 0 and d["n_gpus"] == 1 and d["steps"] == 3 and d["scaling"] == "weak"
    assert d["rccl_ranks"] == 0 and d["launcher"] == "plain"
    assert d["vs_baseline"] is None and d["dtype"] == "u8" and d["data"] == "synthetic" and "workload" in d["config"]
    rf = d["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(rf) and rf["bound"] in ("hbm", "mfma")
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4
    assert d["config"]["distinct_streams_per_gpu"] == 2 and d["config"]["frames_in_ring"] == 3
    assert "streaming" in rf and "limited_by" in rf
    # the preheat (untimed steps before the warm-up: GPU clock ramp) is reported, the warm-up count stays the caller's
    assert d["warmup"] == 1 and d["preheat_steps"] >= len(lines) and d["preheat_steps"] % d["config"]["handles"] == 0
    assert rf["measured_copy_GBps"] is None or (rf["measured_copy_GBps"] > 100 and rf["frac_of_measured_copy"] > 0)
    if mode == "stereo":
        cb = d["cpu_baseline"]
        assert {"value", "unit", "cores", "kind", "sample"} <= set(cb) and cb["kind"] == "port" and cb["value"] > 0
        mt = d["cpu_mt"]
        assert mt["threads"] == 16 and mt["value"] > 0 and mt["extract_ms"]["mean"] > 0 and mt["stereo_ms"]["mean"] > 0
        for k in ("latency_ms", "latency_ctypes_ms", "latency_python_ms", "extract_ms", "stereo_ms"):   # C++ class / C ABI call / wrapper / REGISTER_TIMES brackets
            assert {"mean", "std", "p50", "p99", "frames"} <= set(d[k]) and d[k]["frames"] in (12, 50) and d[k]["mean"] > 0
        assert d["h2d_inclusive_value"] > 0 and d["h2d_inclusive"]["steps"] == 4
        assert d["h2d_inclusive"]["link_upload_GBps"] > 0 and d["h2d_inclusive"]["frac_of_link_bound"] > 0   # (tiny frames here: latency, not bandwidth)
        npair = d["natural_pair"]   # the Middlebury pair through the product path: the oracle's numbers (tests/test_natural_images.py)
        assert (npair["keypoints_left"], npair["keypoints_right"], npair["stereo_matches"]) == (1504, 1508, 595)
        assert d["latency_with_host_pyramid_ms"]["mean"] >= d["latency_ms"]["p50"] * 0.5   # (more work, never less: a loose bound, not a timing test)
        assert d["latency_with_host_pyramid_python_ms"]["mean"] > 0 and "C ABI" in d["latency_note"]
        assert d["latency_ctypes_ms"]["mean"] > 0 and d["latency_source"] in ("cpp_mirror", "ctypes")
        if d["latency_source"] == "cpp_mirror":   # (the C++ class, timed in C++: what latency_ms holds when g++ is on the box)
            assert d["latency_ms"] == d["latency_cpp_mirror_ms"] and d["latency_ms"]["mean"] > 0
    assert 0.5 < rf["shader_clock_ghz"] < 2.6    # measured, not assumed


@pytest.mark.gpu
def test_bench_c5_mode_prints_one_contract_line():
    r = _run(["--full", "--config", "C5", "--inflight", "2", "--steps", "4", "--warmup", "1", "--nfeatures", "300", "--width", "320",
              "--height", "240", "--ring", "2"])
    assert r.returncode == 0, r.stderr[-600:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert KEYS <= set(d) and d["value"] > 0 and d["config"]["workload"].startswith("C5")
    assert d["config"]["pairs_per_step_per_gpu"] == 16 and d["config"]["distinct_streams_per_gpu"] == 8
    assert d["config"]["allgather_bytes_per_step_per_gpu"] > 0
    # a collective inside the step: the preheat runs a FIXED number of steps (all ranks must issue the same all-gathers)
    nh = d["config"]["handles"]
    assert d["preheat_steps"] == nh * ((int(40.0 / 0.55 / nh) + 1))


def test_full_and_dump_outputs_are_options():
    """--full (everything beyond the headline) is off by default; --dump-outputs takes a directory.  No GPU touched."""
    r = _run(["--help"])
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_timed_step(tmp_path):
    """A plain run prints the headline line only (the legs and rooflines are --full's); --dump-outputs writes the last timed
    step's results as float32 .npy files, the same in two runs, and equal to the CPU oracle on that step's inputs."""
    import numpy as np
    import bench
    import orb_slam3_fast_amd as orbx
    from orb_slam3_fast_amd import synth
    from oracle import cpu_bench
    W, H, B, NF = 320, 240, 2, 300
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = _run(["--steps", "3", "--warmup", "1", "--pairs", str(B), "--width", str(W), "--height", str(H), "--nfeatures", str(NF),
                  "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-600:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
        assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["n_gpus"] == 1
        assert not {"roofline", "stages", "cpu_baseline", "latency_ms", "h2d_inclusive_value", "other_configs"} & set(line)
        files = sorted(os.listdir(d))
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        arrs = {f[:-4]: np.load(d / f) for f in files if f.endswith(".npy")}
        assert all(v.dtype in (np.float32, np.float64) for v in arrs.values())
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys()
    assert all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
    # the last timed step: max(warm-up 1, 4 handles) warm-up steps + 3 timed steps -> step 6, ring slot 6 mod 3 = 0
    gl, gr = synth.stereo_ring(W, H, bench.rank_streams(0, B), [0, 1, 2])
    ref = cpu_bench.oracle_pairs(gl[0], gr[0], NF, bench.BF, bench.BASE)
    kp = lambda k: np.stack([np.ascontiguousarray(k).view(orbx.KP_DTYPE)[f].astype(np.float32) for f in orbx.KP_DTYPE.names], 1)
    got = dumps[0]
    assert got["counts"].tolist() == [len(x[0]) for x in ref] + [len(x[2]) for x in ref]
    assert np.array_equal(got["keypoints"], np.concatenate([kp(x[0]) for x in ref] + [kp(x[2]) for x in ref]))
    assert np.array_equal(got["descriptors"], np.concatenate([x[1] for x in ref] + [x[3] for x in ref]).astype(np.float32))
    assert np.array_equal(got["uright"].view(np.uint32), np.concatenate([x[4] for x in ref]).view(np.uint32))
    assert np.array_equal(got["depth"].view(np.uint32), np.concatenate([x[5] for x in ref]).view(np.uint32))


def test_two_rank_launch_rank_logic_on_gloo():
    """bench.py's rank logic under the driver's own launch line with two ranks, up to the first HIP call --
    world size from the environment (n_gpus = the group that ran, never the flag), whole streams per rank, the same (handle, ring
    slot) order of steps on every rank (the all-gather ordering rule), barrier + max-over-ranks time, one line from rank 0.  gloo
    on CPU: the only step an 8-GPU node adds is RCCL itself."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "7", "--warmup", "3",
           "--dry-run-ranks", "--handles", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (r.stdout[-500:], r.stderr[-800:])
    d = json.loads(lines[0])
    assert d["dry_run"] and d["n_gpus"] == 2 and d["steps"] == 7 and d["scaling"] == "weak"
    p0, p1 = d["plans"]
    assert (p0["rank"], p1["rank"]) == (0, 1)
    assert not set(p0["streams"]) & set(p1["streams"]) and len(p0["streams"]) == len(p1["streams"]) == 32
    assert p0["steps"] == p1["steps"] and [h for h, _ in p0["steps"][:6]] == [0, 1, 2, 0, 1, 2]
    assert abs(d["elapsed_max_s"] - 0.002) < 1e-12                      # the slower rank's time
    assert abs(d["value"] - 2 * 32 * 7 / 0.002) < 1e-3                  # units of ALL ranks / max-over-ranks time
