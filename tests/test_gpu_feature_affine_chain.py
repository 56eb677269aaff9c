"""The feature-guided initial guess end to end on the GPU, device-resident throughout: SIFT3D -> DescriptorMatcher ->
FeatureAffine3D -> ICGN3D1 (the reference's examples/test_dvc_sift_icgn1.cpp) on a synthetic volume pair whose target is rotated
by 20 degrees about z and translated -- a deformation FFTCC cannot seed.  The same chain runs through the CPU twins
(tests/sift3d_features_twin.py, tests/match_twin.py, tests/feature_affine_twin.py, the oracle's ICGN3D1) and the two agree in
every bit of every record; every POI FeatureAffine accepts converges in ICGN3D1 onto the planted displacement.

The volume edge was sized with the twins on the CPU: SIZE^3 voxels give more than 200 matched pairs."""
import numpy as np
import pytest

import feature_affine_twin as fa_twin
import sift3d_features_twin as sift_twin

pytestmark = pytest.mark.gpu

SIZE = 80
ANGLE = np.deg2rad(20.0)
SHIFT = (1.5, -1.0, 0.5)
SETTINGS = dict(n_octave_layers=3, min_dimension=8, alpha=0.1, sigma_source=1.15, sigma_base=1.6, units=(1.0, 1.0, 1.0))
RADIUS = 8


def _pair():
    from opencorr_amd import synth
    c, s = float(np.cos(ANGLE)), float(np.sin(ANGLE))
    warp = dict(u=SHIFT[0], ux=c - 1, uy=-s, uz=0.0, v=SHIFT[1], vx=s, vy=c - 1, vz=0.0, w=SHIFT[2], wx=0.0, wy=0.0, wz=0.0)
    ref, tar = synth.speckle_pair_3d(SIZE, SIZE, SIZE, warp=warp)
    return np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(tar, np.float32)


def _planted(points):
    c, s = np.cos(ANGLE), np.sin(ANGLE)
    M = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    centre = (SIZE - 1) * 0.5
    return (points - centre) @ M.T + centre + np.array(SHIFT) - points


def test_sift3d_matcher_feature_affine_icgn3d1_chain():
    import torch
    import opencorr_amd as oc
    import oracle
    from opencorr_amd import synth
    P = oracle.P3
    ref, tar = _pair()
    xs, ys, zs = synth.poi_grid_3d(SIZE, SIZE, SIZE, 3, 3, 3, 24)
    pois = oracle.make_pois3d(xs, ys, zs)
    assert len(pois) == 27

    # the CPU twins
    ref_kp, tar_kp, _, _ = sift_twin.pipeline(ref, tar, SETTINGS)
    assert len(ref_kp) >= 200
    radius = fa_twin.default_radius(3, (RADIUS, RADIUS, RADIUS))
    want_fa = fa_twin.compute(ref_kp, tar_kp, pois, radius)
    want = want_fa.copy()
    oracle.icgn3d1(oracle.Prepared3D(ref, tar), RADIUS, RADIUS, RADIUS, 0.001, 10, want, order=oracle.GPU_ORDER_3D, lanes=oracle.GPU_LANES_3D)

    # the GPU chain: volumes, descriptors, keypoints, pairs and the queue stay on the device
    dev = torch.device("cuda", 0)
    sift = oc.SIFT3D()
    kp, desc = [], []
    for vol in (ref, tar):
        k, d = sift.extract(torch.from_numpy(vol).to(dev))
        kp.append(torch.from_numpy(np.ascontiguousarray(k["coor_img"])).to(dev))
        desc.append(d)
    sift.matcher.set_descriptors(0, desc[0])
    sift.matcher.set_descriptors(1, desc[1])
    ri, ti = sift.matcher.match(oc.DescriptorMatcher.MONODIRECTIONAL)
    assert ri.is_cuda and ri.shape[0] == len(ref_kp)
    fa = oc.FeatureAffine3D(RADIUS, RADIUS, RADIUS)
    fa.set_matched_pairs(kp[0], kp[1], ri, ti)
    fa.prepare()
    queue = torch.from_numpy(pois).to(dev)
    fa.compute(queue)
    fa.synchronize()
    got_fa = queue.cpu().numpy()
    icgn = oc.ICGN3D1(RADIUS, RADIUS, RADIUS, 0.001, 10)
    icgn.set_images(torch.from_numpy(ref).to(dev), torch.from_numpy(tar).to(dev))
    icgn.prepare()
    icgn.compute(queue)
    icgn.synchronize()
    got = queue.cpu().numpy()

    assert np.array_equal(got_fa.view(np.uint32), want_fa.view(np.uint32)), "FeatureAffine3D: GPU chain against the twins"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "ICGN3D1 after FeatureAffine3D: GPU chain against the twins"
    accepted = got_fa[:, P["zncc"]] == 0
    assert accepted.sum() >= 20
    assert (got[accepted, P["zncc"]] > 0.9).all() and (got[accepted, P["iteration"]] < 10).all(), "every accepted POI converges"
    truth = _planted(np.stack([xs, ys, zs], axis=1).astype(np.float64))
    found = got[accepted][:, [P["u"], P["v"], P["w"]]]
    assert np.abs(found - truth[accepted]).max() < 0.05
