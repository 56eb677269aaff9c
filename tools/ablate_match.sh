#!/bin/bash
# Ablation of match_top2_kernel (opencorr_amd/csrc/match.hip, OC_MATCH_ABLATE): what the distance kernel's time is made of.
#   bash tools/ablate_match.sh build     where hipcc and the product build's objects are: tools/ab_build/libmatch_ablate_<mask>.so
#   bash tools/ablate_match.sh run       on the GPU: tools/match_bench.py (no twin: the ablated results are wrong on purpose) per
#                                        library, records under $OUT/match_ablate_<mask>.json (OUT defaults to profiles)
# masks: 1 = no staging after a tile's first chunk, 2 = no top-2 fold, 3 = both
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT" || exit 1
MASKS=${MASKS:-1 2 3}
AB=tools/ab_build
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize"
case "$1" in
build)
    mkdir -p $AB
    OBJS=$(ls opencorr_amd/lib/*.o | grep -v "/match\.o") || exit 1
    for mask in $MASKS; do
        hipcc --offload-arch=gfx950 -c opencorr_amd/csrc/match.hip -o $AB/match_ablate_$mask.o $FLAGS -DOC_MATCH_ABLATE=$mask || exit 1
        hipcc --offload-arch=gfx950 -shared -o $AB/libmatch_ablate_$mask.so $OBJS $AB/match_ablate_$mask.o -L/opt/rocm/lib -lrocfft -ldl -lpthread || exit 1
    done
    ;;
run)
    OUT=${OUT:-profiles}
    mkdir -p "$OUT"
    for mask in $MASKS; do
        OPENCORR_HIP_LIB=$ROOT/$AB/libmatch_ablate_$mask.so timeout -k 10 120 python tools/match_bench.py --no-twin --reps 3 \
            --out "$OUT"/match_ablate_$mask.json || exit 1
    done
    ;;
*)
    echo "usage: bash tools/ablate_match.sh build|run" >&2
    exit 2
    ;;
esac
