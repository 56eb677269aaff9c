// volume_limits_check.cpp -- runs opencorr_amd/csrc/host/volume_limits.h on a CPU (tests/test_volume_limits_cpu.py).
//
// stdin, one request per line:  rx ry rz dy dx
// stdout, one answer per line:  <box span> <accepted: 0 | 1>
// With the argument "limit": the largest span ICGN3D1 serves.
#include <cstdio>
#include <cstring>

#include "../../opencorr_amd/csrc/host/volume_limits.h"

using namespace ochip_host;

static_assert(icgn3d_box_span(3, 3, 30, 5984, 5984) == 2148531270ull && icgn3d_volume_accepted(3, 3, 30, 5984, 5984), "between 2^31 and 2^32");
static_assert(!icgn3d_volume_accepted(3, 3, 7, 17514, 17517) && icgn3d_volume_accepted(3, 3, 7, 17513, 17517), "the first refused plane");

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "limit")) {
        std::printf("%llu\n", kIcgn3dMaxBoxSpan);
        return 0;
    }
    int rx, ry, rz, dy, dx, got;
    while ((got = std::scanf("%d %d %d %d %d", &rx, &ry, &rz, &dy, &dx)) == 5)
        std::printf("%llu %d\n", icgn3d_box_span(rx, ry, rz, dy, dx), (int)icgn3d_volume_accepted(rx, ry, rz, dy, dx));
    if (got != EOF) {
        std::fprintf(stderr, "malformed request line (%d of 5 fields)\n", got);
        return 2;
    }
    return 0;
}
