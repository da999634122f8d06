"""A second, literal restatement of Frame::ComputeStereoMatches (src/Frame.cc:921-1084) in Python / numpy float32,
transcribed statement by statement, checked bit for bit against the C++ oracle on seeded synthetic stereo pairs."""
import numpy as np
import pytest

from orb_slam3_fast_amd import synth
from stereo_cases import compute_stereo_matches_py   # (the restatement lives beside the crafted cases that also use it)

f32 = np.float32


@pytest.mark.parametrize("w,h,nf,stream", [(400, 300, 500, 201), (512, 384, 700, 202), (640, 480, 400, 203)])
def test_python_restatement_of_compute_stereo_matches_matches_oracle(oracle, w, h, nf, stream):
    L, R = synth.stereo_pair(w, h, stream)
    eL, eR = oracle.OracleExtractor(nf), oracle.OracleExtractor(nf)
    _, kL, dL = eL.extract(L)
    _, kR, dR = eR.extract(R)
    t = eL.tables()
    bf, b = f32(0.12) * f32(532.03), f32(0.12)
    pyrL, pyrR = [eL.level(l) for l in range(8)], [eR.level(l) for l in range(8)]
    eu, ed = compute_stereo_matches_py(pyrL, pyrR, kL, dL, kR, dR, t["scale"], t["inv_scale"], bf, b)
    ou, od = oracle.stereo_match(eL, eR, kL, dL, kR, dR, bf, b)
    assert (ou >= 0).sum() > 50
    assert eu.tobytes() == ou.tobytes() and ed.tobytes() == od.tobytes()
