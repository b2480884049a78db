// rgldm.hip -- "redundant geometric local descriptor matching" (translation invariant) of two
// bead lists on MI355X: the candidate stage of the reference's descriptor-based registration.
//
// References (under the reference's src/main/java/):
//   spim/process/interestpointregistration/geometricdescriptor/RGLDMPairwise.java:34-77   the call, "Not enough detections"
//   .../geometricdescriptor/RGLDMMatcher.java:44-95     best / second best, the ratio test
//   .../geometricdescriptor/RGLDMMatcher.java:97-123    nn + re nearest neighbours per point
//   .../geometricdescriptor/RGLDMParameters.java        3 / 1 / 3 / 50
//   spim/process/interestpointregistration/Detection.java:96-117   the kNN metric (float)
//   mpicbg/pointdescriptor/AbstractPointDescriptor.java:63-112     neighbour - basis, min over pairings
//   mpicbg/pointdescriptor/matcher/SubsetMatcher.java:46-107       a-major pairings, computePD
//   mpicbg/pointdescriptor/similarity/SquareDistance.java:11-21    sum of squareDistance / 3.0
//
// Every sum is a plain double sum in the reference's order, so the result is bit-exact against
// a restatement.  What is rearranged, and why it changes no bit:
//   * the (nn+re)^2 square distances of a descriptor pair are computed once; a pairing adds nn
//     of them in its order (0 + s0 == s0)
//   * x -> x / 3.0 is monotone, so min over pairings of (sum / 3.0) is (min sum) / 3.0: one
//     division per descriptor pair
//   * a descriptor pair whose min sum exceeds the sum behind the current second best cannot
//     pass "difference < secondBest" (monotone again) and skips that division
//   k_pm_knn        (pointmatch.hip) per point the nn+re nearest others, neighbour - basis in double
//   k_rgldm_match   a lane owns one A descriptor in registers; B descriptors go through LDS in
//                   tiles and are read as broadcasts; grid.y splits B (partial best / second)
//   k_rgldm_merge   partials -> best by (value, index), second = 2nd smallest of the four
//   k_pm_compact    (pointmatch.hip) the candidates in ascending A order
// The call around them -- argument rules, staging, "not enough detections", the result copies --
// is pm_match_candidates (pointmatch.hpp), shared with geohash.hip.
// No atomics; every output is written with ordinary stores.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "pointmatch.hpp"

namespace spimdecon {
namespace {

constexpr int kRgATile = 128;    // A descriptors (lanes) per block of k_rgldm_match
constexpr int kRgBTile = 64;     // B descriptors per LDS tile
constexpr int kRgMaxM = 6;       // num_neighbors + redundancy
constexpr int kRgMaxComb = 20;   // C(6, 3)

// SubsetMatcher.computePD(M, NN, 0) (:79-107): the NN-subsets of 0..M-1 in lexicographic order
template <int NN>
struct RgComb {
    int n;
    int c[kRgMaxComb][NN];
};
template <int NN, int M>
constexpr RgComb<NN> rg_comb() {
    RgComb<NN> t{};
    int cur[NN] = {};
    for (int i = 0; i < NN; ++i) cur[i] = i;
    int n = 0;
    while (true) {
        for (int i = 0; i < NN; ++i) t.c[n][i] = cur[i];
        ++n;
        int i = NN - 1;
        while (i >= 0 && cur[i] == M - NN + i) --i;
        if (i < 0) break;
        ++cur[i];
        for (int j = i + 1; j < NN; ++j) cur[j] = cur[j - 1] + 1;
    }
    t.n = n;
    return t;
}

// One block: kRgATile A descriptors against the B descriptors of partition blockIdx.y.
// Partials are [partition][na].
template <int NN, int M>
__global__ __launch_bounds__(kRgATile) void k_rgldm_match(const double* __restrict__ rel_a, int na,
                                                          const double* __restrict__ rel_b, int nb, int chunk,
                                                          double* __restrict__ pbest, double* __restrict__ psecond,
                                                          int* __restrict__ pidx) {
    constexpr int D = M * 3;
    constexpr RgComb<NN> tab = rg_comb<NN, M>();
    __shared__ double sb[kRgBTile * D];
    const int i = int(blockIdx.x) * kRgATile + int(threadIdx.x);
    const int ic = min(i, na - 1);
    double a[D];
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = rel_a[int64_t(ic) * D + k];
    const int b0 = int(min(int64_t(blockIdx.y) * chunk, int64_t(nb)));
    const int b1 = int(min(int64_t(b0) + chunk, int64_t(nb)));

    double best = kJavaDoubleMax, second = kJavaDoubleMax;
    double best_sum = __builtin_inf(), second_sum = __builtin_inf();   // the sums behind them
    int best_idx = -1;
    for (int j0 = b0; j0 < b1; j0 += kRgBTile) {
        const int cnt = min(kRgBTile, b1 - j0);
        __syncthreads();
        for (int e = int(threadIdx.x); e < cnt * D; e += kRgATile) sb[e] = rel_b[int64_t(j0) * D + e];
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const double* b = sb + t * D;   // the same address in every lane: a broadcast
            double sq[M][M];                // Point.squareDistance of neighbour p of A and q of B
#pragma unroll
            for (int q = 0; q < M; ++q) {
                const double bx = b[3 * q], by = b[3 * q + 1], bz = b[3 * q + 2];
#pragma unroll
                for (int p = 0; p < M; ++p) {
                    const double dx = __dsub_rn(a[3 * p], bx), dy = __dsub_rn(a[3 * p + 1], by),
                                 dz = __dsub_rn(a[3 * p + 2], bz);
                    sq[p][q] = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                }
            }
            double ms = __builtin_inf();   // min over the pairings (a NaN sum never is "<": fmin drops it)
#pragma unroll
            for (int ca = 0; ca < tab.n; ++ca) {
#pragma unroll
                for (int cb = 0; cb < tab.n; ++cb) {
                    double s = sq[tab.c[ca][0]][tab.c[cb][0]];
#pragma unroll
                    for (int k = 1; k < NN; ++k) s = __dadd_rn(s, sq[tab.c[ca][k]][tab.c[cb][k]]);
                    ms = fmin(ms, s);
                }
            }
            if (!(ms <= second_sum)) continue;   // ms / 3.0 >= second: not "difference < secondBest"
            const double diff = fmin(__ddiv_rn(ms, 3.0), kJavaDoubleMax);   // (from Double.MAX_VALUE down)
            if (diff < second) {                 // RGLDMMatcher.java:64-80
                second = diff;
                second_sum = ms;
                if (second < best) {
                    const double tv = best, ts = best_sum;
                    best = second; best_sum = second_sum;
                    second = tv; second_sum = ts;
                    best_idx = j0 + t;
                }
            }
        }
    }
    if (i < na) {
        const int64_t o = int64_t(blockIdx.y) * na + i;
        pbest[o] = best;
        psecond[o] = second;
        pidx[o] = best_idx;
    }
}

// The partitions in ascending B order: the best by (value, index) -- strict < keeps the lower
// index --, the second as the second smallest of {best, second, best', second'}; then the
// ratio test (RGLDMMatcher.java:83).
__global__ __launch_bounds__(256) void k_rgldm_merge(int na, int nparts, const double* __restrict__ pbest,
                                                     const double* __restrict__ psecond,
                                                     const int* __restrict__ pidx, double thr, double ratio,
                                                     double* __restrict__ best_out, double* __restrict__ second_out,
                                                     int* __restrict__ idx_out, unsigned char* __restrict__ flag) {
    const int i = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (i >= na) return;
    double best = kJavaDoubleMax, second = kJavaDoubleMax;
    int idx = -1;
    for (int p = 0; p < nparts; ++p) {
        const int64_t o = int64_t(p) * na + i;
        const double b2 = pbest[o], s2 = psecond[o];
        if (b2 < best) {
            second = fmin(best, s2);
            best = b2;
            idx = pidx[o];
        } else {
            second = fmin(second, b2);
        }
    }
    best_out[i] = best;
    second_out[i] = second;
    idx_out[i] = idx;
    flag[i] = (best < thr && __dmul_rn(best, ratio) < second) ? 1 : 0;
}

// Per-device workspace, grown on demand and kept between calls.
struct RgWork : PmCandidateWork {
    DBuf<double> rel_a, rel_b, pbest, psecond;
    DBuf<int> nbr_a, nbr_b, pidx;
};

// every argument rule that needs no GPU; returns nn + re
int rg_check_params(const spim_rgldm_params* p) {
    SD_CHECK(p, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(p->num_neighbors >= 1 && p->redundancy >= 0, SPIMDECON_ERR_ARG,
             "rgldm: num_neighbors must be >= 1 and redundancy >= 0");
    SD_CHECK(int64_t(p->num_neighbors) + p->redundancy <= kRgMaxM, SPIMDECON_ERR_ARG,
             "rgldm: num_neighbors + redundancy beyond the supported maximum of 6");
    SD_CHECK(p->b_split >= 0, SPIMDECON_ERR_ARG, "rgldm: b_split must be >= 0");
    return p->num_neighbors + p->redundancy;
}

void rg_match_launch(int nn, int m, dim3 grid, hipStream_t s, const double* ra, int na, const double* rb, int nb,
                     int chunk, double* pbest, double* psecond, int* pidx) {
#define SD_RG_M(NNV, MV)                                                                                     \
    if (nn == NNV && m == MV) {                                                                              \
        hipLaunchKernelGGL((k_rgldm_match<NNV, MV>), grid, dim3(kRgATile), 0, s, ra, na, rb, nb, chunk, pbest, \
                           psecond, pidx);                                                                   \
        return;                                                                                              \
    }
    SD_RG_M(1, 1) SD_RG_M(1, 2) SD_RG_M(2, 2) SD_RG_M(1, 3) SD_RG_M(2, 3) SD_RG_M(3, 3)
    SD_RG_M(1, 4) SD_RG_M(2, 4) SD_RG_M(3, 4) SD_RG_M(4, 4)
    SD_RG_M(1, 5) SD_RG_M(2, 5) SD_RG_M(3, 5) SD_RG_M(4, 5) SD_RG_M(5, 5)
    SD_RG_M(1, 6) SD_RG_M(2, 6) SD_RG_M(3, 6) SD_RG_M(4, 6) SD_RG_M(5, 6) SD_RG_M(6, 6)
#undef SD_RG_M
    fail(SPIMDECON_ERR_ARG, "rgldm: unsupported neighbour count");
}

void rgldm_descriptors(const double* pts, int64_t n, const spim_rgldm_params* p, int32_t* neighbors, double* rel) {
    const int m = rg_check_params(p);
    pm_check_points(pts, n, "rgldm");
    SD_CHECK(neighbors && rel, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(n >= m + 1, SPIMDECON_ERR_ARG, "rgldm: a descriptor needs num_neighbors + redundancy + 1 points");
    with_work<RgWork>(p->device, [&](RgWork& w, hipStream_t s) {
        const double* d = pm_stage_points(pts, n, p->device, w.pts_a, w.bad, s, "rgldm");
        grow(w.nbr_a, size_t(n) * m);
        grow(w.rel_a, size_t(n) * m * 3);
        pm_knn(d, int(n), m, w.nbr_a.p, w.rel_a.p, s);
        SD_HIP(hipMemcpyAsync(neighbors, w.nbr_a.p, size_t(n) * m * sizeof(int), hipMemcpyDefault, s));
        SD_HIP(hipMemcpyAsync(rel, w.rel_a.p, size_t(n) * m * 3 * sizeof(double), hipMemcpyDefault, s));
        SD_HIP(hipStreamSynchronize(s));
    });
}

void rgldm_match(const double* a, int64_t na, const double* b, int64_t nb, const spim_rgldm_params* p,
                 int32_t* best_idx, double* best, double* second, int32_t* cand_a, int32_t* cand_b, int64_t cap,
                 int64_t* count) {
    const int m = rg_check_params(p);
    // fewer than m + 1 points: RGLDMPairwise.java:46-54, "Not enough detections to match": no candidates
    pm_match_candidates<RgWork>(
        "rgldm", m + 1, p->device, a, na, b, nb, best_idx, best, second, cand_a, cand_b, cap, count,
        [&](RgWork& w, const double* da, const double* db, hipStream_t s) {
            grow(w.nbr_a, size_t(na) * m);
            grow(w.rel_a, size_t(na) * m * 3);
            grow(w.nbr_b, size_t(nb) * m);
            grow(w.rel_b, size_t(nb) * m * 3);
            pm_knn(da, int(na), m, w.nbr_a.p, w.rel_a.p, s);
            pm_knn(db, int(nb), m, w.nbr_b.p, w.rel_b.p, s);
            // B split: 313 wavefronts of A (20,000 beads) do not fill the device; aim at ~8 waves per CU
            const int64_t ablocks = ceil_div(na, kRgATile);
            const PmSplit sp = pm_split(p->b_split, ablocks, nb, kRgBTile, 4 /* blocks of 2 waves */, p->device,
                                        "rgldm");
            grow(w.pbest, size_t(na) * sp.split);
            grow(w.psecond, size_t(na) * sp.split);
            grow(w.pidx, size_t(na) * sp.split);
            rg_match_launch(p->num_neighbors, m, dim3(unsigned(ablocks), unsigned(sp.split)), s, w.rel_a.p, int(na),
                            w.rel_b.p, int(nb), sp.chunk, w.pbest.p, w.psecond.p, w.pidx.p);
            SD_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_rgldm_merge, dim3(unsigned(ceil_div(na, 256))), dim3(256), 0, s, int(na),
                               int(sp.split), w.pbest.p, w.psecond.p, w.pidx.p, double(p->difference_threshold),
                               double(p->ratio_of_distance), w.best.p, w.second.p, w.idx.p, w.flag.p);
            SD_HIP(hipGetLastError());
        });
}

}  // namespace
}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" void spim_rgldm_params_default(spim_rgldm_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->num_neighbors = 3;            // RGLDMParameters.numNeighbors
    p->redundancy = 1;               // .redundancy
    p->ratio_of_distance = 3.0f;     // .ratioOfDistance
    p->difference_threshold = 50.0f; // .differenceThreshold
    p->b_split = 0;
    p->device = 0;
}

extern "C" void spim_rgldm_tiles(int32_t* a_tile, int32_t* b_tile) {
    if (a_tile) *a_tile = kRgATile;
    if (b_tile) *b_tile = kRgBTile;
}

extern "C" int spim_rgldm_descriptors(const double* pts, int64_t n, const spim_rgldm_params* p, int32_t* neighbors,
                                      double* rel) {
    return guarded([&] { rgldm_descriptors(pts, n, p, neighbors, rel); });
}

extern "C" int spim_rgldm_match(const double* a, int64_t na, const double* b, int64_t nb, const spim_rgldm_params* p,
                                int32_t* best_idx, double* best, double* second, int32_t* cand_a, int32_t* cand_b,
                                int64_t cap, int64_t* count) {
    return guarded([&] { rgldm_match(a, na, b, nb, p, best_idx, best, second, cand_a, cand_b, cap, count); });
}
