"""ORB_SLAM3::KeyFrameDatabase of the C++ mirror (csrc/KeyFrameDatabase.h), driven by tests/cpp/kfdb_like.cpp in the shape of its
two call sites (src/Tracking.cc:3527, src/LoopClosing.cc:517).  The program is compiled by this test."""
import os
import subprocess

import numpy as np
import pytest

import orb_slam3_fast_amd as orbx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kfdb_like.cpp")


def build(out_dir):
    libdir = os.path.join(ROOT, "orb_slam3_fast_amd")
    exe = os.path.join(str(out_dir), "kfdb_like")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe, "-L" + libdir, "-lorbx", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_vocabulary(path, k, L, cols):
    """The DBoW2 text format (TemplatedVocabulary.h:1338-1421): k L scoring weighting, then one node per line."""
    parent, leaf, desc, weight = cols
    with open(path, "w") as f:
        f.write("%d %d 0 0\n" % (k, L))
        for i in range(1, len(parent)):
            f.write("%d %d %s %r\n" % (parent[i], leaf[i], " ".join(str(int(b)) for b in desc[i]), float(weight[i])))


def test_kfdb_like_compiles_and_fails_loudly_without_gpu(tmp_path):
    from test_kfdb import voc_cols
    exe = build(tmp_path)
    write_vocabulary(tmp_path / "voc.txt", 10, 3, voc_cols())
    r = subprocess.run([exe, str(tmp_path / "voc.txt")], capture_output=True, text=True)
    if orbx.device_count() == 0:
        assert r.returncode == 3 and "no-device error" in r.stdout
    else:
        assert r.returncode == 0, r.stdout + r.stderr


def write_scene(path, sc, mode, qmap, n_candidates, connected, bad, query):
    from test_kfdb import split
    with open(path, "wb") as o:
        np.array([len(sc.kfs), mode, qmap, n_candidates, len(connected), len(bad), len(query)], np.int32).tofile(o)
        for k in sc.kfs:
            w, v = split(k["bow"])
            np.array([k["id"], k["map"], len(w), len(k["cov"])], np.int32).tofile(o)
            w.tofile(o)
            v.tofile(o)
            np.array(k["cov"], np.int32).tofile(o)
        np.array(connected, np.int32).tofile(o)
        np.array(bad, np.int32).tofile(o)
        w, v = split(query)
        w.tofile(o)
        v.tofile(o)


def read_lists(path, count):
    raw = np.fromfile(path, np.int32)
    out, pos = [], 0
    for _ in range(count):
        n = int(raw[pos])
        out.append([int(x) for x in raw[pos + 1:pos + 1 + n]])
        pos += 1 + n
    assert pos == len(raw)
    return out


@pytest.mark.gpu
def test_kfdb_like_matches_the_python_entry(tmp_path):
    from test_kfdb import scene_nbest, scene_relocalisation, split, voc_cols
    assert orbx.device_count() > 0
    exe = build(tmp_path)
    write_vocabulary(tmp_path / "voc.txt", 10, 3, voc_cols())
    voc = orbx.ORBVocabulary(10, 3, *voc_cols())

    def run(name, *scene):
        write_scene(tmp_path / (name + ".raw"), *scene)
        r = subprocess.run([exe, str(tmp_path / "voc.txt"), str(tmp_path / (name + ".raw")), str(tmp_path / (name + ".out"))],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        return tmp_path / (name + ".out")

    sc, query, qmap = scene_relocalisation()
    want = sc.device(voc).DetectRelocalizationCandidates(split(query), qmap)
    assert read_lists(run("reloc", sc, 0, qmap, 0, [], [], query), 1) == [want] and len(want) >= 3
    sc, query, qmap, connected, bad, _ = scene_nbest()
    for n in (3, 1):
        loop, merge = sc.device(voc).DetectNBestCandidates(split(query), qmap, connected, n, bad)
        assert read_lists(run("nbest%d" % n, sc, 1, qmap, n, connected, bad, query), 2) == [loop, merge] and len(loop) == n
