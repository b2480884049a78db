// pointmatch.hip -- the stages that the point-list matchers share (pointmatch.hpp): the finite
// check, the neighbour search, the fill of "not enough detections" and the compaction, with
// the staging and the partition rule of the host.
//
// References (under the reference's src/main/java/):
//   spim/process/interestpointregistration/Detection.java:96-117   the kNN metric (float)
//   .../geometricdescriptor/RGLDMMatcher.java:97-123    nn + re nearest neighbours per point
//   .../geometrichashing/GeometricHasher.java:87-116    3 nearest neighbours per point
//   mpicbg/pointdescriptor/AbstractPointDescriptor.java:54-76      neighbour - basis in double
//
//   k_pm_finite   flag[0] = 1 when a coordinate is not finite as double or as float
//   k_pm_knn      per point the m nearest others (brute force over LDS tiles, top-k in
//                 registers, ties by lower index), neighbour - basis in double
//   k_pm_fill     best = second = Double.MAX_VALUE, idx = -1
//   k_pm_compact  the candidates in ascending A order (one block, chunked prefix sum)
// No atomics; every output is written with ordinary stores.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "pointmatch.hpp"

namespace spimdecon {
namespace {

constexpr int kRgKnnBlock = 256;
constexpr int kRgScanBlock = 1024;

// flag[0] = 1 when a coordinate is not finite as double or as float (Detection.get rounds to float)
__global__ __launch_bounds__(256) void k_pm_finite(const double* __restrict__ p, int64_t n3,
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
__global__ __launch_bounds__(kRgKnnBlock) void k_pm_knn(const double* __restrict__ pts, int n,
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

// One block: thread t owns the chunk [t * per, (t + 1) * per) of A; an exclusive scan of the
// chunk counts gives each chunk's first output slot.  count[0] = all candidates (may exceed cap).
__global__ __launch_bounds__(kRgScanBlock) void k_pm_compact(int na, const unsigned char* __restrict__ flag,
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

__global__ __launch_bounds__(256) void k_pm_fill(int na, double* __restrict__ best, double* __restrict__ second,
                                                 int* __restrict__ idx) {
    const int i = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (i >= na) return;
    best[i] = kJavaDoubleMax;
    second[i] = kJavaDoubleMax;
    idx[i] = -1;
}

}  // namespace

void pm_check_points(const double* pts, int64_t n, const char* who) {
    SD_CHECK(n >= 0 && (pts || n == 0), SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(n <= int64_t(INT32_MAX), SPIMDECON_ERR_ARG, std::string(who) + ": more than 2^31 - 1 points");
}

const double* pm_stage_points(const double* pts, int64_t n, int dev, DBuf<double>& buf, DBuf<int>& bad_buf,
                              hipStream_t s, const char* who) {
    const double* d = pts;
    if (!is_device_ptr(pts, dev)) {
        grow(buf, size_t(3 * n));
        SD_HIP(hipMemcpyAsync(buf.p, pts, size_t(3 * n) * sizeof(double), hipMemcpyDefault, s));
        d = buf.p;
    }
    grow(bad_buf, 1);
    SD_HIP(hipMemsetAsync(bad_buf.p, 0, sizeof(int), s));
    const unsigned g = unsigned(std::min<int64_t>(ceil_div(3 * n, 256), 1024));
    hipLaunchKernelGGL(k_pm_finite, dim3(g), dim3(256), 0, s, d, 3 * n, bad_buf.p);
    SD_HIP(hipGetLastError());
    int bad = 0;
    SD_HIP(hipMemcpyAsync(&bad, bad_buf.p, sizeof(int), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
    SD_CHECK(!bad, SPIMDECON_ERR_ARG, std::string(who) + ": non-finite coordinates");
    return d;
}

PmSplit pm_split(int64_t requested, int64_t row_blocks, int64_t n_cols, int col_tile, int blocks_per_cu, int dev,
                 const char* who) {
    int64_t split = requested;
    if (split <= 0) {
        int cus = 0;
        SD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int64_t want = int64_t(cus) * blocks_per_cu;
        split = std::min<int64_t>(std::max<int64_t>(ceil_div(want, row_blocks), 1), ceil_div(n_cols, col_tile));
    }
    split = std::min<int64_t>(split, 65535);
    const int chunk = int(ceil_div(n_cols, split));
    SD_CHECK(row_blocks * split < (int64_t(1) << 31), SPIMDECON_ERR_ARG, std::string(who) + ": too many blocks");
    return {split, chunk};
}

void pm_knn(const double* dpts, int n, int m, int* nbr, double* rel, hipStream_t s) {
    const unsigned g = unsigned(ceil_div(n, kRgKnnBlock));
#define SD_PM_KNN(MV) \
    case MV: hipLaunchKernelGGL(k_pm_knn<MV>, dim3(g), dim3(kRgKnnBlock), 0, s, dpts, n, nbr, rel); break;
    switch (m) {
        SD_PM_KNN(1) SD_PM_KNN(2) SD_PM_KNN(3) SD_PM_KNN(4) SD_PM_KNN(5) SD_PM_KNN(6)
        default: fail(SPIMDECON_ERR_ARG, "rgldm: unsupported neighbour count");
    }
#undef SD_PM_KNN
    SD_HIP(hipGetLastError());
}

void pm_compact(int na, const unsigned char* flag, const int* idx, int* cand_a, int* cand_b, int64_t cap,
                int64_t* count, hipStream_t s) {
    hipLaunchKernelGGL(k_pm_compact, dim3(1), dim3(kRgScanBlock), 0, s, na, flag, idx, cand_a, cand_b, cap, count);
    SD_HIP(hipGetLastError());
}

void pm_fill(int na, double* best, double* second, int* idx, hipStream_t s) {
    hipLaunchKernelGGL(k_pm_fill, dim3(unsigned(ceil_div(na, 256))), dim3(256), 0, s, na, best, second, idx);
    SD_HIP(hipGetLastError());
}

}  // namespace spimdecon
