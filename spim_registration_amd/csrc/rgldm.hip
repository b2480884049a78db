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
//   k_rgldm_knn     per point the nn+re nearest others (brute force over LDS tiles, top-k in
//                   registers, ties by lower index), neighbour - basis in double
//   k_rgldm_match   a lane owns one A descriptor in registers; B descriptors go through LDS in
//                   tiles and are read as broadcasts; grid.y splits B (partial best / second)
//   k_rgldm_merge   partials -> best by (value, index), second = 2nd smallest of the four
//   k_rgldm_compact the candidates in ascending A order (one block, chunked prefix sum)
// No atomics; every output is written with ordinary stores.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>

#include "common.hpp"
#include "rgldm.hpp"

namespace spimdecon {

bool is_device_ptr(const void* p, int dev);   // dog.hip

namespace {

constexpr int kRgATile = 128;    // A descriptors (lanes) per block of k_rgldm_match
constexpr int kRgBTile = 64;     // B descriptors per LDS tile
constexpr int kRgKnnBlock = 256;
constexpr int kRgMaxM = 6;       // num_neighbors + redundancy
constexpr int kRgMaxComb = 20;   // C(6, 3)
constexpr int kRgScanBlock = 1024;
constexpr double kJavaDoubleMax = DBL_MAX;   // Double.MAX_VALUE

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

// flag[0] = 1 when a coordinate is not finite as double or as float (Detection.get rounds to float)
__global__ __launch_bounds__(256) void k_rgldm_finite(const double* __restrict__ p, int64_t n3,
                                                      int* __restrict__ flag) {
    int bad = 0;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n3; i += int64_t(gridDim.x) * 256) {
        const float f = float(p[i]);
        bad |= (f - f == 0.0f) ? 0 : 1;
    }
    if (bad) flag[0] = 1;   // (every writer stores the same value)
}

// Detection.distanceTo's argument: per-axis float differences, squared and summed in double
__device__ __forceinline__ double rg_knn_s(float ax, float ay, float az, float bx, float by, float bz) {
    const double x = double(__fsub_rn(bx, ax)), y = double(__fsub_rn(by, ay)), z = double(__fsub_rn(bz, az));
    return __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z));
}

template <int M>
__global__ __launch_bounds__(kRgKnnBlock) void k_rgldm_knn(const double* __restrict__ pts, int n,
                                                           int* __restrict__ neighbors,
                                                           double* __restrict__ rel) {
    __shared__ float tile[kRgKnnBlock * 3];
    const int i = int(blockIdx.x) * kRgKnnBlock + int(threadIdx.x);
    const int ic = min(i, n - 1);
    const float ax = float(pts[3 * int64_t(ic)]), ay = float(pts[3 * int64_t(ic) + 1]),
                az = float(pts[3 * int64_t(ic) + 2]);
    float dist[M];   // ascending; (float) Math.sqrt(...) as the kd-tree compares it
    int idx[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        dist[k] = __builtin_inff();
        idx[k] = -1;
    }
    double s_worst = __builtin_inf();   // the double sum behind dist[M - 1]
    for (int j0 = 0; j0 < n; j0 += kRgKnnBlock) {
        const int cnt = min(kRgKnnBlock, n - j0);
        __syncthreads();
        for (int e = int(threadIdx.x); e < cnt * 3; e += kRgKnnBlock) tile[e] = float(pts[3 * int64_t(j0) + e]);
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const int j = j0 + t;
            const double s = rg_knn_s(ax, ay, az, tile[3 * t], tile[3 * t + 1], tile[3 * t + 2]);
            // s > s_worst: the rounded root is no smaller than the worst kept (monotone): not "<"
            if (j == ic || !(s <= s_worst)) continue;
            const float d = float(__dsqrt_rn(s));
            if (!(d < dist[M - 1])) continue;
            dist[M - 1] = d;
            idx[M - 1] = j;
#pragma unroll
            for (int k = M - 1; k > 0; --k) {   // strict <: an equal distance stays behind the lower index
                if (dist[k] < dist[k - 1]) {
                    const float td = dist[k]; dist[k] = dist[k - 1]; dist[k - 1] = td;
                    const int ti = idx[k]; idx[k] = idx[k - 1]; idx[k - 1] = ti;
                }
            }
            if (idx[M - 1] >= 0) {
                // the sum of the worst kept is not tracked through the swaps: rebuild it
                const int w = idx[M - 1];
                s_worst = rg_knn_s(ax, ay, az, float(pts[3 * int64_t(w)]), float(pts[3 * int64_t(w) + 1]),
                                   float(pts[3 * int64_t(w) + 2]));
            }
        }
    }
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const int64_t o = int64_t(i) * M + k;
        const int w = idx[k];
        neighbors[o] = w;
        const int wc = w < 0 ? i : w;   // (fewer than M finite distances: no neighbour, NaN)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = __dsub_rn(pts[3 * int64_t(wc) + c], pts[3 * int64_t(i) + c]);
            rel[o * 3 + c] = w < 0 ? __builtin_nan("") : v;
        }
    }
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

// One block: thread t owns the chunk [t * per, (t + 1) * per) of A; an exclusive scan of the
// chunk counts gives each chunk's first output slot.  count[0] = all candidates (may exceed cap).
__global__ __launch_bounds__(kRgScanBlock) void k_rgldm_compact(int na, const unsigned char* __restrict__ flag,
                                                                const int* __restrict__ idx, int* __restrict__ cand_a,
                                                                int* __restrict__ cand_b, int64_t cap,
                                                                int64_t* __restrict__ count) {
    __shared__ int sums[kRgScanBlock];
    const int t = int(threadIdx.x);
    const int per = (na + kRgScanBlock - 1) / kRgScanBlock;
    const int64_t lo = int64_t(t) * per, hi = min(lo + per, int64_t(na));
    int c = 0;
    for (int64_t i = lo; i < hi; ++i) c += flag[i];
    sums[t] = c;
    __syncthreads();
    for (int o = 1; o < kRgScanBlock; o <<= 1) {   // inclusive scan
        const int v = t >= o ? sums[t - o] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int64_t pos = sums[t] - c;
    for (int64_t i = lo; i < hi; ++i) {
        if (!flag[i]) continue;
        if (pos < cap) {
            cand_a[pos] = int(i);
            cand_b[pos] = idx[i];
        }
        ++pos;
    }
    if (t == kRgScanBlock - 1) count[0] = sums[t];
}

__global__ __launch_bounds__(256) void k_rgldm_fill(int na, double* __restrict__ best, double* __restrict__ second,
                                                    int* __restrict__ idx) {
    const int i = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (i >= na) return;
    best[i] = kJavaDoubleMax;
    second[i] = kJavaDoubleMax;
    idx[i] = -1;
}

// Per-device workspace, grown on demand and kept between calls (never destroyed: no hipFree
// from a static destructor racing the runtime's teardown).
struct RgWork {
    std::mutex mu;
    hipStream_t stream = nullptr;
    DBuf<double> pts_a, pts_b, rel_a, rel_b, pbest, psecond, best, second;
    DBuf<int> nbr_a, nbr_b, pidx, idx, cand_a, cand_b, bad;
    DBuf<unsigned char> flag;
    DBuf<int64_t> count;
    hipStream_t get_stream() {
        if (!stream) SD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return stream;
    }
};
std::mutex g_rgwork_mu;
std::map<int, std::unique_ptr<RgWork>>& g_rgwork = *new std::map<int, std::unique_ptr<RgWork>>();
RgWork& rg_work(int dev) {
    std::lock_guard<std::mutex> lk(g_rgwork_mu);
    auto& w = g_rgwork[dev];
    if (!w) w.reset(new RgWork());
    return *w;
}
template <typename T>
void rg_grow(DBuf<T>& b, size_t n) {
    if (b.n < n) b.alloc(n);
}

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

void rg_check_points(const double* pts, int64_t n) {
    SD_CHECK(n >= 0 && (pts || n == 0), SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(n <= int64_t(INT32_MAX), SPIMDECON_ERR_ARG, "rgldm: more than 2^31 - 1 points");
}

// the points on the device (in place when they already are) and checked finite
const double* rg_stage(const double* pts, int64_t n, int dev, DBuf<double>& buf, DBuf<int>& bad_buf, hipStream_t s,
                       const char* who = "rgldm") {
    const double* d = pts;
    if (!is_device_ptr(pts, dev)) {
        rg_grow(buf, size_t(3 * n));
        SD_HIP(hipMemcpyAsync(buf.p, pts, size_t(3 * n) * sizeof(double), hipMemcpyDefault, s));
        d = buf.p;
    }
    rg_grow(bad_buf, 1);
    SD_HIP(hipMemsetAsync(bad_buf.p, 0, sizeof(int), s));
    const unsigned g = unsigned(std::min<int64_t>(ceil_div(3 * n, 256), 1024));
    hipLaunchKernelGGL(k_rgldm_finite, dim3(g), dim3(256), 0, s, d, 3 * n, bad_buf.p);
    SD_HIP(hipGetLastError());
    int bad = 0;
    SD_HIP(hipMemcpyAsync(&bad, bad_buf.p, sizeof(int), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
    SD_CHECK(!bad, SPIMDECON_ERR_ARG, std::string(who) + ": non-finite coordinates");
    return d;
}

void rg_knn(const double* dpts, int n, int m, int* nbr, double* rel, hipStream_t s) {
    const unsigned g = unsigned(ceil_div(n, kRgKnnBlock));
#define SD_RG_KNN(MV) \
    case MV: hipLaunchKernelGGL(k_rgldm_knn<MV>, dim3(g), dim3(kRgKnnBlock), 0, s, dpts, n, nbr, rel); break;
    switch (m) {
        SD_RG_KNN(1) SD_RG_KNN(2) SD_RG_KNN(3) SD_RG_KNN(4) SD_RG_KNN(5) SD_RG_KNN(6)
        default: fail(SPIMDECON_ERR_ARG, "rgldm: unsupported neighbour count");
    }
#undef SD_RG_KNN
    SD_HIP(hipGetLastError());
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
    rg_check_points(pts, n);
    SD_CHECK(neighbors && rel, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(n >= m + 1, SPIMDECON_ERR_ARG, "rgldm: a descriptor needs num_neighbors + redundancy + 1 points");
    check_device(p->device);
    DeviceGuard guard(p->device);
    RgWork& w = rg_work(p->device);
    std::lock_guard<std::mutex> lk(w.mu);
    hipStream_t s = w.get_stream();
    const double* d = rg_stage(pts, n, p->device, w.pts_a, w.bad, s);
    rg_grow(w.nbr_a, size_t(n) * m);
    rg_grow(w.rel_a, size_t(n) * m * 3);
    rg_knn(d, int(n), m, w.nbr_a.p, w.rel_a.p, s);
    SD_HIP(hipMemcpyAsync(neighbors, w.nbr_a.p, size_t(n) * m * sizeof(int), hipMemcpyDefault, s));
    SD_HIP(hipMemcpyAsync(rel, w.rel_a.p, size_t(n) * m * 3 * sizeof(double), hipMemcpyDefault, s));
    SD_HIP(hipStreamSynchronize(s));
}

void rgldm_match(const double* a, int64_t na, const double* b, int64_t nb, const spim_rgldm_params* p,
                 int32_t* best_idx, double* best, double* second, int32_t* cand_a, int32_t* cand_b, int64_t cap,
                 int64_t* count) {
    const int m = rg_check_params(p);
    rg_check_points(a, na);
    rg_check_points(b, nb);
    SD_CHECK(count && cap >= 0 && (cap == 0 || (cand_a && cand_b)), SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(na == 0 || (best_idx && best && second), SPIMDECON_ERR_ARG, "null argument");
    *count = 0;
    check_device(p->device);
    DeviceGuard guard(p->device);
    RgWork& w = rg_work(p->device);
    std::lock_guard<std::mutex> lk(w.mu);
    hipStream_t s = w.get_stream();
    const double* da = na ? rg_stage(a, na, p->device, w.pts_a, w.bad, s) : nullptr;
    const double* db = nb ? rg_stage(b, nb, p->device, w.pts_b, w.bad, s) : nullptr;
    if (na == 0) return;
    rg_grow(w.best, size_t(na));
    rg_grow(w.second, size_t(na));
    rg_grow(w.idx, size_t(na));
    const unsigned ga = unsigned(ceil_div(na, 256));
    if (na < m + 1 || nb < m + 1) {
        // RGLDMPairwise.java:46-54, "Not enough detections to match": no candidates
        hipLaunchKernelGGL(k_rgldm_fill, dim3(ga), dim3(256), 0, s, int(na), w.best.p, w.second.p, w.idx.p);
        SD_HIP(hipGetLastError());
    } else {
        rg_grow(w.nbr_a, size_t(na) * m);
        rg_grow(w.rel_a, size_t(na) * m * 3);
        rg_grow(w.nbr_b, size_t(nb) * m);
        rg_grow(w.rel_b, size_t(nb) * m * 3);
        rg_knn(da, int(na), m, w.nbr_a.p, w.rel_a.p, s);
        rg_knn(db, int(nb), m, w.nbr_b.p, w.rel_b.p, s);
        // B split: 313 wavefronts of A (20,000 beads) do not fill the device; aim at ~8 waves per CU
        const int64_t ablocks = ceil_div(na, kRgATile);
        int64_t split = p->b_split;
        if (split <= 0) {
            int cus = 0;
            SD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device));
            const int64_t want = int64_t(cus) * 4;   // blocks of 2 waves
            split = std::min<int64_t>(std::max<int64_t>(ceil_div(want, ablocks), 1), ceil_div(nb, kRgBTile));
        }
        split = std::min<int64_t>(split, 65535);
        const int chunk = int(ceil_div(nb, split));
        SD_CHECK(ablocks * split < (int64_t(1) << 31), SPIMDECON_ERR_ARG, "rgldm: too many blocks");
        rg_grow(w.pbest, size_t(na) * split);
        rg_grow(w.psecond, size_t(na) * split);
        rg_grow(w.pidx, size_t(na) * split);
        rg_match_launch(p->num_neighbors, m, dim3(unsigned(ablocks), unsigned(split)), s, w.rel_a.p, int(na),
                        w.rel_b.p, int(nb), chunk, w.pbest.p, w.psecond.p, w.pidx.p);
        SD_HIP(hipGetLastError());
        rg_grow(w.flag, size_t(na));
        hipLaunchKernelGGL(k_rgldm_merge, dim3(ga), dim3(256), 0, s, int(na), int(split), w.pbest.p, w.psecond.p,
                           w.pidx.p, double(p->difference_threshold), double(p->ratio_of_distance), w.best.p,
                           w.second.p, w.idx.p, w.flag.p);
        SD_HIP(hipGetLastError());
        rg_grow(w.count, 1);
        const int64_t dcap = std::min<int64_t>(cap, na);
        rg_grow(w.cand_a, size_t(std::max<int64_t>(dcap, 1)));
        rg_grow(w.cand_b, size_t(std::max<int64_t>(dcap, 1)));
        hipLaunchKernelGGL(k_rgldm_compact, dim3(1), dim3(kRgScanBlock), 0, s, int(na), w.flag.p, w.idx.p,
                           w.cand_a.p, w.cand_b.p, dcap, w.count.p);
        SD_HIP(hipGetLastError());
        SD_HIP(hipMemcpyAsync(count, w.count.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    }
    SD_HIP(hipMemcpyAsync(best_idx, w.idx.p, size_t(na) * sizeof(int), hipMemcpyDefault, s));
    SD_HIP(hipMemcpyAsync(best, w.best.p, size_t(na) * sizeof(double), hipMemcpyDefault, s));
    SD_HIP(hipMemcpyAsync(second, w.second.p, size_t(na) * sizeof(double), hipMemcpyDefault, s));
    SD_HIP(hipStreamSynchronize(s));
    SD_CHECK(*count <= cap, SPIMDECON_ERR_ARG,
             "rgldm: " + std::to_string(*count) + " candidates beyond the capacity " + std::to_string(cap));
    if (*count) {
        SD_HIP(hipMemcpyAsync(cand_a, w.cand_a.p, size_t(*count) * sizeof(int), hipMemcpyDefault, s));
        SD_HIP(hipMemcpyAsync(cand_b, w.cand_b.p, size_t(*count) * sizeof(int), hipMemcpyDefault, s));
        SD_HIP(hipStreamSynchronize(s));
    }
}

}  // namespace

// ---------------------------------------------------------------- shared with geohash.hip (rgldm.hpp)
const double* pm_stage_points(const double* pts, int64_t n, int dev, DBuf<double>& buf, DBuf<int>& bad,
                              hipStream_t s, const char* who) {
    rg_check_points(pts, n);
    return rg_stage(pts, n, dev, buf, bad, s, who);
}

void pm_knn(const double* dpts, int n, int m, int* nbr, double* rel, hipStream_t s) {
    rg_knn(dpts, n, m, nbr, rel, s);
}

void pm_compact(int na, const unsigned char* flag, const int* idx, int* cand_a, int* cand_b, int64_t cap,
                int64_t* count, hipStream_t s) {
    hipLaunchKernelGGL(k_rgldm_compact, dim3(1), dim3(kRgScanBlock), 0, s, na, flag, idx, cand_a, cand_b, cap, count);
    SD_HIP(hipGetLastError());
}

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
