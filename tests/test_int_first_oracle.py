"""What the integer-translation sweep of icgn2d.hip ("icgn2d_int_first") rests on, pinned on the CPU oracle alone: at an
integer point the bicubic interpolant is ONE coefficient of the table -- coef[0][0], element 0 of the 16 -- because every other
term of the 16-term polynomial is a product with dx = 0 or dy = 0; and for a finite image that coefficient is the pixel
itself (the last row of BC is {0, 1, 0, 0}).  The GPU half lives in tests/test_gpu_int_first.py."""
import numpy as np


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_interpolant_at_integer_points_is_coefficient_00_and_the_pixel():
    import oracle
    h, w = 37, 45
    rng = np.random.default_rng(20261017)
    img = rng.uniform(0.0, 255.0, (h, w)).astype(np.float32)
    img[5, 7] = 0.0
    img[11, 13] = 1e-30          # tiny and huge finite values go through unchanged as well
    img[17, 19] = 3e30
    lut = oracle.bspline2d_lut(img)
    ys, xs = np.mgrid[1:h - 2, 1:w - 2]
    got = np.array([oracle.bspline2d_eval(lut, x, y) for y, x in zip(ys.ravel(), xs.ravel())], dtype=np.float32).reshape(ys.shape)
    assert np.array_equal(_bits(got), _bits(lut[1:h - 2, 1:w - 2, 0]))
    assert np.array_equal(_bits(got), _bits(img[1:h - 2, 1:w - 2]))
    # no negative zero among the interior coefficients (the sum that forms them starts from +0)
    assert not (_bits(lut[1:h - 2, 1:w - 2, 0]) == 0x80000000).any()


def test_table_border_is_zero_and_outside_is_the_sentinel():
    import oracle
    h, w = 24, 29
    img = np.random.default_rng(3).uniform(1.0, 255.0, (h, w)).astype(np.float32)
    lut = oracle.bspline2d_lut(img)
    border = np.ones((h, w), dtype=bool)
    border[1:h - 2, 1:w - 2] = False
    assert (_bits(lut[border]) == 0).all()
    # the range rule the sweep's test restates: x < 1, y < 1, x >= w - 2, y >= h - 2 are outside
    for x, y in ((0, 5), (5, 0), (w - 2, 5), (5, h - 2)):
        assert oracle.bspline2d_eval(lut, x, y) == -1.0
    for x, y in ((1, 1), (w - 3, h - 3)):
        assert oracle.bspline2d_eval(lut, x, y) == img[y, x]
