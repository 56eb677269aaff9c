// match_twin.cpp -- CPU restatement of the descriptor matcher's arithmetic contract (opencorr_amd/csrc/match.hip), written as the
// reference writes it: the sequential scan of SIFT3D::bruteforceMatch (src/oc_sift.cpp:625-674), j ascending, strict `<` against
// two FLT_MAX-initialised slots; the many-to-one elimination of monodirectionalMatch (:1251-1418) and the cross-check of
// bidirectionalMatch (:1420-1487).  The kernel finds the same two candidates as "the two smallest under (distance, j)": this file
// is the scan, so the GPU test compares the lexicographic form with the scan and not with itself.
//
// Build: g++ -O2 -ffp-contract=off -fopenmp (tests/match_twin.py).  fma = 0: product and sum round separately; fma = 1:
// std::fmaf(d, d, acc), what g++ -mfma makes of the reference's expression.
//
// Defined where the reference is not ("Descriptor matching"):
//   * every entry of matched_idx is written (-1 = the ratio test failed or there is no candidate);
//   * the element behind the last many-to-one group counts as different (:1335 reads one past the resized vector);
//   * all matches are processed when every reference keypoint passed the ratio test (:1310-1317 leaves matched_amount at 0);
//   * equal distances inside a group: the lower reference index is visited first (:1325 is an unstable sort).
//
// oc_twin_match_set_slip plants ONE deliberate error (tests/test_match_twin_cpu.py shows that the float64 model catches each):
// 1 = `<=` in place of `<` in the scan, 2 = the ratio left unsquared, 3 = ascending in place of descending output order.
#include <cfloat>
#include <cmath>
#include <vector>

namespace {

int g_slip = 0;

struct Slots {
    int idx[2];
    float dist[2];
};

inline float squared_distance(const float* a, const float* b, int dim, int fma) {
    float acc = 0.f;
    if (fma) {
        for (int k = 0; k < dim; k++) {
            const float d = a[k] - b[k];
            acc = std::fmaf(d, d, acc);
        }
    } else {
        for (int k = 0; k < dim; k++) {
            const float d = a[k] - b[k];
            acc = acc + d * d;
        }
    }
    return acc;
}

// :637-663
inline void offer(Slots& s, float dist, int j, bool or_equal) {
    if (or_equal ? dist <= s.dist[0] : dist < s.dist[0]) {
        s.idx[1] = s.idx[0];
        s.dist[1] = s.dist[0];
        s.idx[0] = j;
        s.dist[0] = dist;
    } else if (or_equal ? dist <= s.dist[1] : dist < s.dist[1]) {
        s.idx[1] = j;
        s.dist[1] = dist;
    }
}

inline float ratio_factor(float ratio) { return g_slip == 2 ? ratio : ratio * ratio; }  // :629

long nearest(const float* q, long nq, const float* c, long nc, int dim, float ratio, int fma, int* idx, float* best, float* second) {
    const float factor = ratio_factor(ratio);
    const bool or_equal = g_slip == 1;
    long matched = 0;
#pragma omp parallel for reduction(+ : matched) schedule(static)
    for (long i = 0; i < nq; i++) {
        Slots s = {{-1, -1}, {FLT_MAX, FLT_MAX}};
        for (long j = 0; j < nc; j++) offer(s, squared_distance(q + i * dim, c + j * dim, dim, fma), (int)j, or_equal);
        const bool pass = s.idx[0] >= 0 && s.dist[0] < factor * s.dist[1];  // :666
        idx[i] = pass ? s.idx[0] : -1;
        if (best) best[i] = s.dist[0];
        if (second) second[i] = s.dist[1];
        matched += pass ? 1 : 0;
    }
    return matched;
}

}  // namespace

extern "C" {

void oc_twin_match_set_slip(int slip) { g_slip = slip; }

long oc_twin_match_nearest(const float* query, long nq, const float* cand, long nc, int dim, float ratio, int fma, int* matched_idx,
                           float* best, float* second) {
    return nearest(query, nq, cand, nc, dim, ratio, fma, matched_idx, best, second);
}

// mode 0 = monodirectional, 1 = bidirectional; ref_idx / tar_idx hold min(nr, nt) entries; returns the number of pairs
long oc_twin_match_pairs(const float* ref, long nr, const float* tar, long nt, int dim, float ratio, int fma, int mode, int* ref_idx,
                         int* tar_idx) {
    if (nr == 0 || nt == 0) return 0;
    std::vector<int> r2t(nr);
    std::vector<float> dist(nr);
    nearest(ref, nr, tar, nt, dim, ratio, fma, r2t.data(), dist.data(), nullptr);
    long n = 0;
    if (mode == 1) {
        std::vector<int> t2r(nt);
        nearest(tar, nt, ref, nr, dim, ratio, fma, t2r.data(), nullptr, nullptr);
        for (long i = 0; i < nr; i++)  // :1436-1445, :1464-1481
            if (r2t[i] > -1 && t2r[r2t[i]] == (int)i) {
                ref_idx[n] = (int)i;
                tar_idx[n] = r2t[i];
                n++;
            }
        return n;
    }
    // the groups of :1330-1388: reference keypoints in ascending index offered to the two slots of their target
    const float factor = ratio_factor(ratio);
    std::vector<Slots> group(nt, Slots{{-1, -1}, {FLT_MAX, FLT_MAX}});
    for (long i = 0; i < nr; i++)
        if (r2t[i] > -1) offer(group[r2t[i]], dist[i], (int)i, false);
    // descending target index (:1325); the group's nearest stays when it passes the ratio test against the second (:1383)
    for (long p = 0; p < nt; p++) {
        const long j = g_slip == 3 ? p : nt - 1 - p;
        const Slots& s = group[j];
        if (s.idx[0] > -1 && s.dist[0] < factor * s.dist[1]) {
            ref_idx[n] = s.idx[0];
            tar_idx[n] = (int)j;
            n++;
        }
    }
    return n;
}

}  // extern "C"
