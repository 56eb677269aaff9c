"""What oc_hip_set_tuning answers, restated from the C-ABI's documented behaviour key by key -- independent of the table in
opencorr_amd/csrc/host/engine_tuning.h, which tests/test_engine_tuning_cpu.py (CPU) and tests/test_gpu_tuning_keys.py (the library
itself) compare with it.  set_tuning(kind, key, value, ab_build) -> (status, refusal, settings): the settings start from DEFAULTS and
a refused call leaves them there.
"""
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, 1, 5
FFTCC2D, ICGN2D1, ICGN2D2, FFTCC3D, ICGN3D1, NR2D1, ICLM2D1, ICLM2D2, STRAIN, REGION_FIT, CALIBRATION, STEREOVISION, MATCHER = range(1, 14)
KINDS = tuple(range(1, 14))

# (name in the check program's output, default) in the order it prints them
DEFAULTS = (("variant", -1), ("xcd", 1), ("tile_px", 128), ("setup_cache", 1), ("int_first", 1), ("split_chunks", 0), ("arith_fma", 0),
            ("arith_onepass", 0), ("arith_onepass3d", 0), ("fftcc2d_fused", 1), ("fftcc3d_fused", 1), ("planes_blocks", 0),
            ("fftcc3d_tile_vox", 64), ("icgn3d_tile_vox", 64), ("mapping", 0), ("match_splits", 0), ("single_combine", 1),
            ("host_chunk", 65536), ("group_allgather", 0), ("group_force_rccl", 0), ("self_adaptive", 0), ("lm", "100,0.1,10"))

# key -> the setting it writes
FIELD = {"icgn2d_variant": "variant", "icgn2d_xcd": "xcd", "xcd": "xcd", "icgn2d_tile_px": "tile_px", "icgn2d_setup_cache": "setup_cache",
         "icgn2d_int_first": "int_first", "icgn2d_split_chunks": "split_chunks", "arith_fma": "arith_fma", "arith_onepass": "arith_onepass",
         "arith_onepass3d": "arith_onepass3d", "fftcc2d_fused": "fftcc2d_fused", "fftcc3d_fused": "fftcc3d_fused",
         "fftcc3d_planes_blocks": "planes_blocks", "fftcc3d_tile_vox": "fftcc3d_tile_vox", "icgn3d_tile_vox": "icgn3d_tile_vox",
         "icgn3d_mapping": "mapping", "match_splits": "match_splits", "single_combine": "single_combine", "host_chunk": "host_chunk",
         "group_allgather": "group_allgather", "group_force_rccl": "group_force_rccl"}
KEYS = tuple(k for k in FIELD if k != "xcd")

SWITCHES = ("icgn2d_xcd", "xcd", "icgn2d_setup_cache", "icgn2d_int_first", "single_combine", "group_allgather", "group_force_rccl")
OFF_OR_AT_LEAST = {"icgn2d_tile_px": 16, "fftcc3d_tile_vox": 8, "icgn3d_tile_vox": 8, "host_chunk": 16384}
VARIANT_IDS = 12                      # "icgn2d_variant": -1 (automatic), 0 ... 11
VARIANTS_OF_THE_AB_BUILD = (0, 6, 8, 9)   # "measured losers that only the A/B build of the library contains"
FUSED_ARITHMETIC = (ICGN2D1, ICGN2D2, ICLM2D1, ICLM2D2, ICGN3D1, MATCHER)


def _answer(kind, key, value, ab_build):
    """(status, refusal, stored value)"""
    if key not in FIELD:
        return ERR_INVALID, "unknown_key", None
    if key in SWITCHES:
        return OK, "none", int(value != 0)
    if key in OFF_OR_AT_LEAST:
        if value < 0 or 0 < value < OFF_OR_AT_LEAST[key]:
            return ERR_INVALID, "out_of_range", None
        return OK, "none", value
    if key == "icgn2d_variant":
        if not -1 <= value < VARIANT_IDS:
            return ERR_INVALID, "out_of_range", None
        if value in VARIANTS_OF_THE_AB_BUILD and not ab_build:
            return ERR_UNSUPPORTED, "ab_only", None
        return OK, "none", value
    if key == "arith_fma":
        if value != 0 and kind not in FUSED_ARITHMETIC:
            return ERR_UNSUPPORTED, "wrong_kind", None
        return OK, "none", int(value != 0)
    if key == "arith_onepass":
        # ICGN2D1 / ICGN2D2 only; every other engine refuses 1 and accepts 0, and ICGN3D1 is told the name of its own key
        if value != 0 and kind == ICGN3D1:
            return ERR_UNSUPPORTED, "onepass_of_3d", None
        if value != 0 and kind not in (ICGN2D1, ICGN2D2):
            return ERR_UNSUPPORTED, "wrong_kind", None
        return OK, "none", int(value != 0)
    if key == "arith_onepass3d":
        if value != 0 and kind != ICGN3D1:
            return ERR_UNSUPPORTED, "wrong_kind", None
        return OK, "none", int(value != 0)
    if key == "match_splits":
        # the descriptor matcher's key: every other engine refuses it, whatever the value
        if kind != MATCHER:
            return ERR_UNSUPPORTED, "wrong_kind", None
        if not 0 <= value <= 64:
            return ERR_INVALID, "out_of_range", None
        return OK, "none", value
    if key == "icgn2d_split_chunks":
        # belongs to variant 8: the product build refuses every value but 0 before it looks at the range
        if value != 0 and not ab_build:
            return ERR_UNSUPPORTED, "ab_only", None
        if not 0 <= value <= 256:
            return ERR_INVALID, "out_of_range", None
        return OK, "none", value
    if key == "fftcc3d_planes_blocks":
        if not 0 <= value <= 4096:
            return ERR_INVALID, "out_of_range", None
        return OK, "none", value
    if key == "fftcc2d_fused":
        return OK, "none", value if value in (2, 3, 4, 5) else int(value != 0)
    if key == "fftcc3d_fused":
        if value == 2 and not ab_build:
            return ERR_UNSUPPORTED, "ab_only", None
        return OK, "none", 2 if value == 2 else int(value != 0)
    if key == "icgn3d_mapping":
        if value != 0 and not ab_build:
            return ERR_UNSUPPORTED, "ab_only", None
        return OK, "none", int(value != 0)
    raise AssertionError(key)


def set_tuning(kind, key, value, ab_build):
    status, refusal, stored = _answer(kind, key, value, bool(ab_build))
    settings = dict(DEFAULTS)
    if status == OK:
        settings[FIELD[key]] = stored
    return status, refusal, settings


def status(kind, key, value, ab_build=False):
    return _answer(kind, key, value, bool(ab_build))[0]


def line(kind, key, value, ab_build):
    """What tests/cpp/engine_tuning_check.cpp prints for the request."""
    st, refusal, settings = set_tuning(kind, key, value, ab_build)
    return "%d %s %s" % (st, refusal, format_settings(settings))


def format_settings(settings):
    return " ".join("%s=%s" % (name, settings[name]) for name, _ in DEFAULTS)


# values at and around every bound of the rules above (tests/test_gpu_tuning_keys.py)
BOUNDARY_VALUES = (-2, -1, 0, 1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 15, 16, 64, 65, 256, 257, 4096, 4097, 16383, 16384, 65536, 2 ** 31 - 1)
