"""Writes tests/golden/gt4_stereo_r16.npz: the stereo-DIC anchor of the reference's 3D-DIC examples as plain data.

    python tests/golden/make_golden_stereo.py /path/to/OpenCorr

Reads examples/3d_dic/GT4-0273_0_epipolar_sift_r16.csv of the reference tree (9 997 POI2DS rows, 26 columns, the table
IO2D::saveTable2DS wrote after EpipolarSearch + SIFT + ICGN + Stereovision::reconstruct + Strain on the GT4 image pair) and
stores it as float32 next to the numbers of that rig: the calibration of both cameras (the constants of
examples/test_3d_dic_epipolar_sift.cpp:60-100, carried here as data), the image size and the strain settings of
examples/test_3d_dic_strain.cpp:47-53.  No image is needed; the tests read only the .npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join("examples", "3d_dic", "GT4-0273_0_epipolar_sift_r16.csv")
COLUMNS = ["x", "y", "u", "v", "w", "r1r2 ZNCC", "r1t1 ZNCC", "r1t2 ZNCC", "r2_x", "r2_y", "t1_x", "t1_y", "t2_x", "t2_y",
           "ref_x", "ref_y", "ref_z", "tar_x", "tar_y", "tar_z", "exx", "eyy", "ezz", "exy", "eyz", "ezx"]

# fx, fy, fs, cx, cy, k1, k2, k3, k4, k5, k6, p1, p2 | tx, ty, tz, rx, ry, rz
CAM1_INTRINSICS = [6673.315918, 6669.302734, 0.0, 872.15778, 579.95532, 0.032258954, -1.01141417, 29.78838921, 0, 0, 0, 0, 0]
CAM1_EXTRINSICS = [0, 0, 0, 0, 0, 0]
CAM2_INTRINSICS = [6607.618164, 6602.857422, 0.0, 917.9733887, 531.6352539, 0.064598486, -4.531373978, 29.78838921, 0, 0, 0, 0, 0]
CAM2_EXTRINSICS = [122.24886, 1.8488892, 17.624638, 0.00307711, -0.33278773, 0.00524556]
HEIGHT, WIDTH = 1200, 1920
# subregion radius, neighbor_number_min, ZNCC threshold, approximation (1 = Cauchy)
STRAIN_SETTINGS = [20.0, 5.0, 0.9, 1.0]


def main(reference_root):
    path = os.path.join(reference_root, CSV)
    with open(path) as f:
        header = f.readline().strip().split(",")
    assert header == COLUMNS, header
    table = np.loadtxt(path, delimiter=",", skiprows=1, dtype=np.float64).astype(np.float32)
    assert table.shape == (9997, 26), table.shape
    out = os.path.join(HERE, "gt4_stereo_r16.npz")
    np.savez_compressed(out, table=table,
                        cam1_intrinsics=np.array(CAM1_INTRINSICS, dtype=np.float32), cam1_extrinsics=np.array(CAM1_EXTRINSICS, dtype=np.float32),
                        cam2_intrinsics=np.array(CAM2_INTRINSICS, dtype=np.float32), cam2_extrinsics=np.array(CAM2_EXTRINSICS, dtype=np.float32),
                        height=np.int32(HEIGHT), width=np.int32(WIDTH), strain_settings=np.array(STRAIN_SETTINGS, dtype=np.float32))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
