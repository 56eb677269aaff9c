"""Builds tests/golden/rotation_sift2d.npz from the reference's own example data.

Needs the reference tree (REF below):
    python tests/golden/make_golden_sift2d.py

Inputs (all under /root/reference/examples/2d_dic/):
  rotation_000.tif, rotation_170.tif     8-bit gray, 512 x 512 (the second one as RGB with three equal channels)
  rotation_170_matched_kp.csv            ref x, ref y, tar x, tar y: the 7 665 matched pairs SIFT2D::compute() (src/oc_sift.cpp:60-131)
                                         found on that pair with the constructor's defaults and the real OpenCV
Only data is stored -- no reference source code: both images as uint8 and the distinct ref-side and tar-side positions (float64,
the CSV's six significant digits).  A keypoint's position is final after localisation (orientation only duplicates keypoints at
the same place), so every one of these positions must be among the detector's output: tests/test_sift2d_golden.py.
"""
import os

import numpy as np
from PIL import Image

REF = "/root/reference/examples/2d_dic"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rotation_sift2d.npz")


def main():
    ref = np.asarray(Image.open(os.path.join(REF, "rotation_000.tif")))
    tar = np.asarray(Image.open(os.path.join(REF, "rotation_170.tif")))
    if tar.ndim == 3:  # stored as RGB with three equal channels: cv::IMREAD_GRAYSCALE (src/oc_image.cpp:39) gives that value
        assert all(np.array_equal(tar[..., 0], tar[..., k]) for k in range(1, tar.shape[2]))
        tar = np.ascontiguousarray(tar[..., 0])
    assert ref.dtype == np.uint8 and ref.shape == (512, 512) and tar.dtype == np.uint8 and tar.shape == ref.shape
    table = np.genfromtxt(os.path.join(REF, "rotation_170_matched_kp.csv"), delimiter=",")
    if np.isnan(table[0]).any():
        table = table[1:]
    assert table.shape == (7665, 4), table.shape
    ref_xy = np.unique(table[:, :2], axis=0)
    tar_xy = np.unique(table[:, 2:], axis=0)
    assert len(ref_xy) == 6386
    np.savez_compressed(OUT, ref=ref, tar=tar, ref_xy=ref_xy, tar_xy=tar_xy)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(ref_xy), "ref positions,", len(tar_xy), "tar positions")


if __name__ == "__main__":
    main()
