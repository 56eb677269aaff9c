"""What an ICGN2D1 / ICGN2D2 / IC-LM call launches, restated in Python from the documentation of "icgn2d_variant",
"icgn2d_setup_cache", "arith_onepass" and "icgn2d_split_chunks" in include/opencorr_hip.h and from the layout comments of
opencorr_amd/csrc/icgn2d.hip -- NOT from opencorr_amd/csrc/host/icgn2d_plan.h, which tests/test_icgn2d_plan_cpu.py compares
against this file row by row.  The LDS arithmetic here is spelled out in bytes per pass; the header derives it from its shape
table.

A request is the tuple REQUEST_FIELDS; plan() returns the line tests/cpp/icgn2d_plan_check.cpp prints for it.
"""
REQUEST_FIELDS = ("dof", "lm", "onepass", "self_adaptive", "offsets", "variant", "rx", "ry", "count", "setup_cache", "split_chunks",
                  "ab_build", "band_supported")

BUDGET = 160 * 1024 - 2048      # dynamic LDS of a CU less the 2 KB kept for static LDS
MAX_GRID = 1 << 30              # POIs per launch
BIG_QUEUE = 32768
SPLIT_MIN_POIS = 16384

# bytes of LDS per pass of 64 samples and workgroup: float arrays per wave x waves x 256 B, plus the coordinate table (12 B per slot,
# 6 B for the compact one)
#   0: four arrays, one wave          1, 3: two arrays, one wave       2: two arrays, four waves      7: one array, four waves
#   4, 5, 8: one array, eight waves + table      6: one array, four waves + table      10, 11: one array, four waves + compact table
PASS_BYTES = {0: 4 * 256, 1: 2 * 256, 3: 2 * 256, 2: 2 * 4 * 256, 7: 4 * 256,
              4: 8 * 256 + 768, 5: 8 * 256 + 768, 8: 8 * 256 + 768, 6: 4 * 256 + 768, 10: 4 * 256 + 384, 11: 4 * 256 + 384}
TABLE_VARIANTS = (4, 5, 6, 8, 9, 10, 11)
AB_ONLY = (0, 6, 8, 9)
ONEPASS_PASS_BYTES = 3 * 256    # the one-pass kernel: a table of three floats per slot and nothing else


def max_samples(variant):
    """Whole passes one workgroup of the variant holds (variant 9, the band kernel, has a rule of its own: 0)."""
    return 0 if variant == 9 else BUDGET // PASS_BYTES[variant] * 64


def onepass_max_samples():
    return BUDGET // ONEPASS_PASS_BYTES * 64


def passes(rx, ry):
    return ((2 * rx + 1) * (2 * ry + 1) + 63) // 64


def compact_fits(variant, rx, ry):
    """10 / 11: at most 256 columns and rows, six / four workgroups inside a CU's LDS."""
    if variant not in (10, 11) or rx < 0 or ry < 0 or 2 * rx + 1 > 256 or 2 * ry + 1 > 256:
        return False
    return (6 if variant == 10 else 4) * PASS_BYTES[variant] * passes(rx, ry) <= BUDGET


def plan(dof, lm, onepass, self_adaptive, offsets, variant, rx, ry, count, setup_cache, split_chunks, ab_build, band_supported):
    onepass = onepass and not lm
    if onepass and offsets:
        return "refuse onepass_offsets 0"
    if onepass and self_adaptive:
        return "refuse onepass_self_adaptive 0"
    samples = (2 * rx + 1) * (2 * ry + 1)
    one_radius = not lm and not self_adaptive
    if variant in (10, 11) and not (one_radius and compact_fits(variant, rx, ry)):
        variant = -1
    chosen = variant < 0
    if chosen:
        # 6 DoF: 5 while three of its workgroups fit a CU (19 passes), 12 DoF: 4 while two fit (28 passes); big queues only
        if dof == 12:
            variant = 4 if passes(rx, ry) <= 28 and count >= BIG_QUEUE else 3
        else:
            variant = 5 if passes(rx, ry) <= 19 and count >= BIG_QUEUE else 2
        compact = 11 if dof == 12 else 10
        if variant in (4, 5) and one_radius and count >= BIG_QUEUE and compact_fits(compact, rx, ry):
            variant = compact
    if self_adaptive and (chosen or variant in TABLE_VARIANTS):
        # 7 (target array only) once three workgroups of variant 2 no longer fit a CU: from 27 passes up
        variant = 7 if 3 * PASS_BYTES[2] * passes(rx, ry) > BUDGET else (3 if dof == 12 else 2)
    if lm:
        variant = 1
    band = bool(ab_build and variant == 9 and not lm and not self_adaptive and band_supported)
    if variant == 9 and not band:
        variant = 3 if dof == 12 else 2
    if onepass:
        if samples > onepass_max_samples():
            return "refuse onepass_too_large %d" % onepass_max_samples()
        return "run %d onepass 0 0" % (5 if dof == 6 else 4)
    if not band and samples > max_samples(variant):
        variant = 1
    if not band and samples > max_samples(variant):
        return "refuse too_large %d" % max_samples(variant)
    records = variant == 8 and not lm
    if lm:
        path = "lm"
    elif band:
        path = "band"
    elif records and split_chunks >= 2 and min(count, MAX_GRID) >= SPLIT_MIN_POIS:
        path = "split_pipelined"
    else:
        path = "plain"
    cached = bool(setup_cache and not lm and not band and not offsets and not self_adaptive and variant in (4, 5, 10, 11)
                  and count <= MAX_GRID)
    return "run %d %s %d %d" % (variant, path, cached, records)
