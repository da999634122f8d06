"""The layout of orb_slam3_fast_amd/csrc that the build and the measurement builds rely on (text checks, no GPU, no compiler).

  - the Makefile compiles every .hip exactly once and every object waits for every orbx_*.h / .inc;
  - the measurement-build flags meet the preprocessor in orbx_prof.h only (kernels see constexpr bools), and the two ablation
    switches that produced wrong results are gone;
  - the environment is read by the one helper of orbx_host.h;
  - the five run-time switches nothing named are gone from the code, the headers, the tools and the tests.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_fast_amd", "csrc")


def _make_var(name):
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    return re.search(r"^%s\s*=\s*(.*)$" % name, text, re.M).group(1).split()


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")))


def test_every_hip_is_compiled_once():
    srcs = _make_var("SRCS")
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert sorted(srcs) == on_disk, "SRCS and csrc/*.hip differ: %s" % sorted(set(srcs) ^ set(on_disk))
    assert len(srcs) == len(set(srcs))


def test_every_header_is_a_prerequisite():
    hdrs = set(_make_var("HDRS"))
    want = {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "orbx_*.h")) + glob.glob(os.path.join(CSRC, "*.inc"))}
    assert want <= hdrs, "not in HDRS: %s" % sorted(want - hdrs)


def test_build_flags_meet_the_preprocessor_in_one_header():
    flag = re.compile(r"\b(\w+_PROF|DET_CLK|OCT_NO_SORT_PRINT|FE_ABLATE|REMAP_ABLATE)\b")
    hits = []
    for p in _sources():
        if os.path.basename(p) == "orbx_prof.h":
            continue
        for i, ln in enumerate(open(p).read().split("\n"), 1):
            if ln.lstrip().startswith("#") and flag.search(ln):
                hits.append("%s:%d: %s" % (os.path.basename(p), i, ln.strip()))
    assert not hits, "\n".join(hits)
    prof = open(os.path.join(CSRC, "orbx_prof.h")).read()
    for name in ("OCT_PROF", "OCT_WG_PROF", "OCT_NO_SORT_PRINT", "RS_PROF", "RT_PROF", "ST_PROF", "DET_PROF", "DET_CLK"):
        assert re.search(r"^#ifdef %s$" % name, prof, re.M), name


def test_one_reader_of_the_environment():
    hits = [(os.path.basename(p), open(p).read().count("getenv(")) for p in _sources()]
    assert [h for h in hits if h[1]] == [("orbx_host.h", 1)], [h for h in hits if h[1]]


def test_removed_switches_stay_removed():
    # (spelled in two pieces so that this file passes its own search)
    removed = ["ORBX_" + s for s in ("PYR_STREAM_WAIT", "UPLOAD_1D", "EARLY_COPYOUT", "GRAY_NAIVE", "RESIZE_PLAIN")]
    text_like = (".py", ".hip", ".h", ".inc", ".sh", ".cpp", ".hpp", ".md", ".txt", ".json", "Makefile")
    hits = []
    for top in ("orb_slam3_fast_amd", "include", "tools", "tests"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("__pycache__", "golden")]
            for f in files:
                if f.endswith(text_like):
                    s = open(os.path.join(d, f), errors="replace").read()
                    hits += ["%s: %s" % (os.path.relpath(os.path.join(d, f), ROOT), n) for n in removed if n in s]
    assert not hits, hits
