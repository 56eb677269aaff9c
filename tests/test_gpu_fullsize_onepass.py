"""The one-pass arithmetic contract (`oc_hip_set_tuning("arith_onepass", 1)`) on the WHOLE queues of BASELINE configs B and C.

Same pairs, grids and FFTCC guesses as tests/test_gpu_fullsize.py (tests/fullsize/run_configs.py).  On every POI of the queue:
GPU == the CPU restatement (tests/cpp/icgn2d_onepass_twin.cpp) bit for bit, and against the oracle in the reference's loop order
(ORDER_SEQ) the bars test_gpu_fullsize.py applies to the other two contracts: identical failure codes, >= 99.5 % identical iteration
counts, >= 99.99 % of the POIs within 1e-4 px and none beyond 2e-4, |d ZNCC| <= 1e-5.
"""
import importlib.util
import os

import numpy as np
import pytest

import onepass_twin as twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _configs():
    spec = importlib.util.spec_from_file_location("run_configs", os.path.join(ROOT, "tests", "fullsize", "run_configs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(side, r, nside, engine, so=None):
    import torch
    import opencorr_amd as oc
    import oracle
    from opencorr_amd import synth
    dev = torch.device("cuda", 0)
    ref, tar = synth.speckle_pair_2d(side, side, seed=20260925, device=dev, second_order=so)
    xs, ys = synth.poi_grid_2d(side, side, nside, nside, r + 8)
    stream = torch.cuda.current_stream().cuda_stream
    f = oc.FFTCC2D(r, r)
    f.set_stream(stream)
    f.set_images(ref, tar)
    g = (oc.ICGN2D1 if engine == 1 else oc.ICGN2D2)(r, r, 0.001, 10.0)
    g.set_stream(stream)
    g.share_images(f)
    g.prepare()
    g.set_tuning("arith_onepass", 1)
    pois = torch.from_numpy(oc.make_pois2d(xs, ys)).to(dev)
    f.compute(pois)
    torch.cuda.synchronize()
    guesses = pois.cpu().numpy()
    g.compute(pois)
    torch.cuda.synchronize()
    got = pois.cpu().numpy()
    prep = oracle.Prepared2D(ref.cpu().numpy(), tar.cpu().numpy())
    dof = 6 if engine == 1 else 12
    want = twin.icgn2d(dof, prep, r, r, 0.001, 10.0, guesses.copy())
    seq = guesses.copy()
    (oracle.icgn2d1 if engine == 1 else oracle.icgn2d2)(prep, r, r, 0.001, 10.0, seq, order=oracle.ORDER_SEQ)
    rec = _configs().vs_reference_order(got, seq, [2, 8], 16, 17)
    rec["pois"] = len(got)
    rec["converged"] = int((got[:, 16] >= 0).sum())
    rec["mismatching_words"] = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(rec)
    return rec


def _check(rec, pois, min_converged):
    assert rec["pois"] == pois and rec["seq_sample"] == pois
    assert rec["mismatching_words"] == 0, rec
    assert rec["seq_flag_mismatches"] == 0, rec
    assert rec["seq_iteration_agreement"] >= 0.995, rec
    assert rec["seq_frac_within_1e4"] >= 0.9999 and rec["seq_max_abs_d_disp"] <= 2e-4 and rec["seq_max_abs_d_zncc"] <= 1e-5, rec
    assert rec["converged"] >= min_converged * pois, rec


def test_config_b_whole_queue_onepass():
    """B (the bench line): 4096^2, r = 16, 500 x 500 POIs, ICGN2D1."""
    _check(_run(4096, 16, 500, 1), 250000, 0.999)


def test_config_c_whole_queue_onepass():
    """C: 4096^2, r = 20, 316 x 316 POIs, ICGN2D2 (12 DoF), second-order displacement field."""
    _check(_run(4096, 20, 316, 2, so=dict(uxx=2e-6, vyy=-1e-6)), 99856, 0.99)
