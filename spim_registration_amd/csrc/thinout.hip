// thinout.hip -- "Thin out detections" on MI355X: per detection of one view the distance to
// its nearest other detection in calibrated units, the range rule that removes or keeps the
// detections whose distance lies in [min, max], and the 100-bin histogram of those distances.
//
// References (under the reference's src/main/java/):
//   spim/fiji/plugin/ThinOut_Detections.java:38-42     0 / 5 / remove
//   spim/fiji/plugin/ThinOut_Detections.java:73-166    thinOut: scale, nearest other, the range rule
//   spim/fiji/plugin/ThinOut_Detections.java:220-225   min >= max stops the dialog
//   spim/fiji/plugin/ThinOut_Detections.java:238-299   plotHistogram: the views of a channel pooled
//   spim/fiji/plugin/thinout/Histogram.java:56-90      getMinMax, binData
//
// Everything is double.  Every operation is one explicit round-to-nearest intrinsic in the
// source order of the Java code (which never contracts a multiply and an add), so distances,
// nearest indices, the kept list and the histogram are bit-exact against a restatement.
//   k_to_scale     one thread per point: c[d] = l[d] * voxel[d], padded to 32 bytes; the finite
//                  check of the scaled coordinates
//   k_to_nn        the self-join: a lane owns point i; the scaled list goes through LDS in tiles
//                  and is read as broadcasts; grid.y splits the list (partial nearest); no root
//   k_to_merge     partials in ascending order -> nearest, one root per point, the keep flag
//   k_pm_compact   (pointmatch.hip) the kept indices in ascending order: the reference's append order
//   k_to_minmax    per block the Math.min / Math.max of the selected distances and their number
//   k_to_hist      bin = (int) floor(((v - min) / size) * numBins); integer atomics, LDS then global
// No kernel waits on another block; every loop is bounded by a count the host passes.
//
// Stated deviations and unpinned points:
//   * The reference searches with imglib2's KDTree / KNearestNeighborSearchOnKDTree (k = 2, the
//     second nearest), whose jar is not in its tree.  The squared distance as the sum over x, y, z
//     from left to right, then Math.sqrt, is restated, not pinned; among equal sums the lower
//     index is the nearest here.
//   * Its result for a list of one point is unknown.  Here the distance is +inf and the nearest
//     -1: kept by remove-range, dropped by keep-range.
//   * plotHistogram's subsampling draws from a java.util.Random seeded with the clock; the draw is
//     the caller's here (a 0/1 selection mask).
//   * The parameter string of the new list (:147-150) is not produced.
//   * The histogram's bins live in LDS: more than kToMaxBins of them is SPIMDECON_ERR_ARG; a
//     distance that is not finite (the one-point list's) cannot be binned and is one too.
#include <algorithm>
#include <cmath>

#include "pointmatch.hpp"

// The host arithmetic of the histogram below (size, the bin centres) restates Java sums and
// products that are each rounded on their own: no multiply is contracted into an add in this
// file, whatever flags the library is built with.  (The kernels use explicit intrinsics.)
#pragma clang fp contract(off)

namespace spimdecon {
namespace {

constexpr int kToRBlock = 256;     // points (lanes) per block of k_to_nn
constexpr int kToCTile = 512;      // scaled points per LDS tile (16 KiB of double4)
constexpr int kToBlock = 256;
constexpr int kToHistBlocks = 256;   // the most blocks of k_to_minmax / k_to_hist (grid-stride)
constexpr int kToMaxBins = 4096;     // 16 KiB of LDS counters

// RealPoint(l[0] * voxel[0], l[1] * voxel[1], l[2] * voxel[2]) (:106-109).  bad[0] = 1 when a
// scaled coordinate is not finite.
__global__ __launch_bounds__(kToBlock) void k_to_scale(const double* __restrict__ pts, int n, double vx, double vy,
                                                       double vz, double4* __restrict__ c, int* __restrict__ bad) {
    const int i = int(blockIdx.x) * kToBlock + int(threadIdx.x);
    if (i >= n) return;
    const double x = __dmul_rn(pts[3 * int64_t(i)], vx), y = __dmul_rn(pts[3 * int64_t(i) + 1], vy),
                 z = __dmul_rn(pts[3 * int64_t(i) + 2], vz);
    if (!(x - x == 0.0) || !(y - y == 0.0) || !(z - z == 0.0)) bad[0] = 1;   // (every writer stores the same value)
    c[i] = make_double4(x, y, z, 0.0);
}

// One block: kToRBlock points against the points of partition blockIdx.y, in ascending index.
// s = ((dx * dx) + (dy * dy)) + (dz * dz) of c_i - c_j; the running minimum is replaced only on a
// strictly smaller s, so the lower j stays among equal s.  The self pair is left out by its
// global index, not by its value: a duplicate of point i is a neighbour at distance 0.
// Partials are [partition][n]; a partition with no other point leaves index -1.
__global__ __launch_bounds__(kToRBlock) void k_to_nn(const double4* __restrict__ c, int n, int chunk,
                                                     double* __restrict__ ps, int* __restrict__ pi) {
    __shared__ double4 tile[kToCTile];
    const int i = int(blockIdx.x) * kToRBlock + int(threadIdx.x);
    const int ic = min(i, n - 1);
    const double4 ci = c[ic];
    const int t0 = int(min(int64_t(blockIdx.y) * chunk, int64_t(n)));
    const int t1 = int(min(int64_t(t0) + chunk, int64_t(n)));
    double best_s = __builtin_inf();
    int best_i = -1;
    for (int j0 = t0; j0 < t1; j0 += kToCTile) {
        const int cnt = min(kToCTile, t1 - j0);
        __syncthreads();
        for (int e = int(threadIdx.x); e < cnt; e += kToRBlock) tile[e] = c[int64_t(j0) + e];
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < cnt; ++t) {   // tile[t]: the same address in every lane, a broadcast
            const double4 cj = tile[t];
            const double dx = __dsub_rn(ci.x, cj.x), dy = __dsub_rn(ci.y, cj.y), dz = __dsub_rn(ci.z, cj.z);
            const double s = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
            const int j = j0 + t;
            if (j == ic || (best_i >= 0 && !(s < best_s))) continue;
            best_s = s;
            best_i = j;
        }
    }
    if (i < n) {
        const int64_t o = int64_t(blockIdx.y) * n + i;
        ps[o] = best_s;
        pi[o] = best_i;
    }
}

// The partitions in ascending order, again replaced only on a strictly smaller s.  Then one
// root per point: a correctly rounded root is monotone (s <= s' gives sqrt(s) <= sqrt(s')), so
// sqrt(min_j s_ij) is min_j sqrt(s_ij) bit for bit -- the distance the reference's search
// compares -- and an index the strict rule passes over has no smaller root either.
// The range rule of :141; no other point: +inf and -1.
__global__ __launch_bounds__(kToBlock) void k_to_merge(int n, int nparts, const double* __restrict__ ps,
                                                       const int* __restrict__ pi, double dmin, double dmax,
                                                       int keep_range, double* __restrict__ dist,
                                                       int* __restrict__ nearest, unsigned char* __restrict__ keep) {
    const int i = int(blockIdx.x) * kToBlock + int(threadIdx.x);
    if (i >= n) return;
    double best_s = __builtin_inf();
    int best_i = -1;
    for (int p = 0; p < nparts; ++p) {
        const int64_t o = int64_t(p) * n + i;
        const int j = pi[o];
        if (j < 0) continue;
        const double s = ps[o];
        if (best_i >= 0 && !(s < best_s)) continue;
        best_s = s;
        best_i = j;
    }
    const double d = best_i >= 0 ? __dsqrt_rn(best_s) : __builtin_inf();
    dist[i] = d;
    nearest[i] = best_i;
    const bool k = keep_range ? (d >= dmin && d <= dmax) : (d < dmin || d > dmax);
    keep[i] = k ? 1 : 0;
}

// Math.min / Math.max of two doubles that are not NaN: -0.0 is smaller than 0.0
__device__ __host__ inline double java_min(double a, double b) {
    if (a < b) return a;
    if (b < a) return b;
    return __builtin_signbit(a) ? a : b;
}
__device__ __host__ inline double java_max(double a, double b) {
    if (a > b) return a;
    if (b > a) return b;
    return __builtin_signbit(a) ? b : a;
}

// Histogram.getMinMax over the selected values (sel null: all): per block part[2 b] = min,
// part[2 b + 1] = max (min and max are associative and commutative, so the order of the
// reduction does not show), cnt[b] = how many; a block without a selected value leaves 0 there.
// bad[0] = 1 when a selected value is not finite.
__global__ __launch_bounds__(kToBlock) void k_to_minmax(const double* __restrict__ v, int n,
                                                        const unsigned char* __restrict__ sel,
                                                        double* __restrict__ part, int* __restrict__ cnt,
                                                        int* __restrict__ bad) {
    __shared__ double smin[kToBlock], smax[kToBlock];
    __shared__ int scnt[kToBlock];
    const int t = int(threadIdx.x);
    double lo = __builtin_inf(), hi = -__builtin_inf();
    int c = 0;
    for (int64_t i = int64_t(blockIdx.x) * kToBlock + t; i < n; i += int64_t(gridDim.x) * kToBlock) {
        if (sel && !sel[i]) continue;
        const double x = v[i];
        if (!(x - x == 0.0)) {
            bad[0] = 1;   // (every writer stores the same value)
            continue;
        }
        lo = c ? java_min(lo, x) : x;
        hi = c ? java_max(hi, x) : x;
        ++c;
    }
    smin[t] = lo;
    smax[t] = hi;
    scnt[t] = c;
    __syncthreads();
    for (int o = kToBlock / 2; o > 0; o >>= 1) {
        if (t < o && scnt[t + o]) {
            smin[t] = scnt[t] ? java_min(smin[t], smin[t + o]) : smin[t + o];
            smax[t] = scnt[t] ? java_max(smax[t], smax[t + o]) : smax[t + o];
            scnt[t] += scnt[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        part[2 * blockIdx.x] = smin[0];
        part[2 * blockIdx.x + 1] = smax[0];
        cnt[blockIdx.x] = scnt[0];
    }
}

// Histogram.binData :79-80 per selected value.  Integer adds commute: the counts do not depend
// on the order.  bad[0] = 1 for a bin outside [0, num_bins): Java's ArrayIndexOutOfBoundsException.
__global__ __launch_bounds__(kToBlock) void k_to_hist(const double* __restrict__ v, int n,
                                                      const unsigned char* __restrict__ sel, double vmin,
                                                      double size, int num_bins, unsigned int* __restrict__ counts,
                                                      int* __restrict__ bad) {
    __shared__ unsigned int bins[kToMaxBins];
    const int t = int(threadIdx.x);
    for (int b = t; b < num_bins; b += kToBlock) bins[b] = 0;
    __syncthreads();
    const double nb = double(num_bins);
    for (int64_t i = int64_t(blockIdx.x) * kToBlock + t; i < n; i += int64_t(gridDim.x) * kToBlock) {
        if (sel && !sel[i]) continue;
        const double f = floor(__dmul_rn(__ddiv_rn(__dsub_rn(v[i], vmin), size), nb));
        if (!(f >= 0.0 && f < nb)) {
            bad[0] = 1;   // (every writer stores the same value)
            continue;
        }
        atomicAdd(&bins[int(f)], 1u);
    }
    __syncthreads();
    for (int b = t; b < num_bins; b += kToBlock)
        if (bins[b]) atomicAdd(&counts[b], bins[b]);
}

// Per-device workspace, grown on demand and kept between calls: the views of one timepoint
// allocate once.
struct ThinOutWork : PmWork {
    DBuf<double> pts, ps, dist, part, hvals;
    DBuf<double4> c;
    DBuf<int> pi, nearest, kept, kept_nn, flags, cnt;
    DBuf<unsigned char> keep, hsel;
    DBuf<unsigned int> bins;
    DBuf<int64_t> count;
};

void check_params(const spim_thinout_params* p) {
    SD_CHECK(p, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(p->t_split >= 0, SPIMDECON_ERR_ARG, "thinout: t_split must be >= 0");
    // :220-225 (written so that a NaN threshold fails too)
    SD_CHECK(p->min_distance < p->max_distance, SPIMDECON_ERR_ARG,
             "thinout: min_distance must be smaller than max_distance");
}

// spim_nn_distances (kept == count == nullptr) and spim_thin_out
void thin_out(const double* pts, int64_t n, const double* voxel, const spim_thinout_params* p, double* dist,
              int32_t* nearest, bool compact, int32_t* kept, int64_t cap, int64_t* count) {
    check_params(p);
    SD_CHECK(voxel, SPIMDECON_ERR_ARG, "null argument");
    pm_check_points(pts, n, "thinout");
    SD_CHECK(!compact || (count && cap >= 0 && (cap == 0 || kept)), SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(n == 0 || (dist && nearest), SPIMDECON_ERR_ARG, "null argument");
    if (count) *count = 0;
    with_work<ThinOutWork>(p->device, [&](ThinOutWork& w, hipStream_t s) {
        if (n == 0) return;
        const double* dp = pm_stage_points(pts, n, p->device, w.pts, w.bad, s, "thinout");
        grow(w.c, size_t(n));
        grow(w.flags, 1);
        SD_HIP(hipMemsetAsync(w.flags.p, 0, sizeof(int), s));
        const unsigned gn = unsigned(ceil_div(n, kToBlock));
        hipLaunchKernelGGL(k_to_scale, dim3(gn), dim3(kToBlock), 0, s, dp, int(n), voxel[0], voxel[1], voxel[2],
                           w.c.p, w.flags.p);
        SD_HIP(hipGetLastError());
        // the split of the list: 16,000 points are 63 blocks of rows; aim at 2 blocks of 4 waves per CU
        const int64_t rblocks = ceil_div(n, kToRBlock);
        const PmSplit sp = pm_split(p->t_split, rblocks, n, kToCTile, 2, p->device, "thinout");
        grow(w.ps, size_t(n) * sp.split);
        grow(w.pi, size_t(n) * sp.split);
        hipLaunchKernelGGL(k_to_nn, dim3(unsigned(rblocks), unsigned(sp.split)), dim3(kToRBlock), 0, s, w.c.p, int(n),
                           sp.chunk, w.ps.p, w.pi.p);
        SD_HIP(hipGetLastError());
        grow(w.dist, size_t(n));
        grow(w.nearest, size_t(n));
        grow(w.keep, size_t(n));
        hipLaunchKernelGGL(k_to_merge, dim3(gn), dim3(kToBlock), 0, s, int(n), int(sp.split), w.ps.p, w.pi.p,
                           p->min_distance, p->max_distance, p->keep_range ? 1 : 0, w.dist.p, w.nearest.p, w.keep.p);
        SD_HIP(hipGetLastError());
        const int64_t dcap = std::min<int64_t>(cap, n);
        if (compact) {
            grow(w.count, 1);
            grow(w.kept, size_t(std::max<int64_t>(dcap, 1)));
            grow(w.kept_nn, size_t(std::max<int64_t>(dcap, 1)));
            pm_compact(int(n), w.keep.p, w.nearest.p, w.kept.p, w.kept_nn.p, dcap, w.count.p, s);
            SD_HIP(hipMemcpyAsync(count, w.count.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        }
        int bad = 0;
        SD_HIP(hipMemcpyAsync(&bad, w.flags.p, sizeof(int), hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        if (bad && count) *count = 0;
        SD_CHECK(!bad, SPIMDECON_ERR_ARG, "thinout: non-finite coordinates");
        SD_HIP(hipMemcpyAsync(dist, w.dist.p, size_t(n) * sizeof(double), hipMemcpyDefault, s));
        SD_HIP(hipMemcpyAsync(nearest, w.nearest.p, size_t(n) * sizeof(int), hipMemcpyDefault, s));
        if (compact && *count <= cap && *count)
            SD_HIP(hipMemcpyAsync(kept, w.kept.p, size_t(*count) * sizeof(int), hipMemcpyDefault, s));
        SD_HIP(hipStreamSynchronize(s));
        SD_CHECK(!compact || *count <= cap, SPIMDECON_ERR_ARG,
                 "thinout: " + std::to_string(*count) + " kept detections beyond the capacity " +
                     std::to_string(cap));
    });
}

// the n values of `v` on the device: in place when they already are, else copied into buf
template <typename T>
const T* stage_values(const T* v, int64_t n, int dev, DBuf<T>& buf, hipStream_t s) {
    if (is_device_ptr(v, dev)) return v;
    grow(buf, size_t(n));
    SD_HIP(hipMemcpyAsync(buf.p, v, size_t(n) * sizeof(T), hipMemcpyDefault, s));
    return buf.p;
}

void distance_histogram(const double* dist, int64_t n, const uint8_t* select, int32_t num_bins, int device,
                        double* out_min, double* out_max, int64_t* counts, double* centres) {
    SD_CHECK(num_bins >= 1, SPIMDECON_ERR_ARG, "thinout: num_bins must be >= 1");
    SD_CHECK(num_bins <= kToMaxBins, SPIMDECON_ERR_ARG,
             "thinout: more than " + std::to_string(kToMaxBins) + " bins");
    SD_CHECK(n >= 0 && n <= int64_t(INT32_MAX), SPIMDECON_ERR_ARG, "thinout: more than 2^31 - 1 distances");
    SD_CHECK(n >= 2, SPIMDECON_ERR_ARG, "thinout: a histogram needs at least two points");
    SD_CHECK(dist && out_min && out_max && counts && centres, SPIMDECON_ERR_ARG, "null argument");
    with_work<ThinOutWork>(device, [&](ThinOutWork& w, hipStream_t s) {
        const double* dv = stage_values(dist, n, device, w.hvals, s);
        const unsigned char* ds = select ? stage_values<unsigned char>(select, n, device, w.hsel, s) : nullptr;
        const int blocks = int(std::min<int64_t>(ceil_div(n, kToBlock), kToHistBlocks));
        grow(w.part, 2 * size_t(kToHistBlocks));
        grow(w.cnt, size_t(kToHistBlocks));
        grow(w.flags, 1);
        grow(w.bins, size_t(kToMaxBins));
        SD_HIP(hipMemsetAsync(w.flags.p, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_to_minmax, dim3(unsigned(blocks)), dim3(kToBlock), 0, s, dv, int(n), ds, w.part.p,
                           w.cnt.p, w.flags.p);
        SD_HIP(hipGetLastError());
        std::vector<double> part(2 * size_t(blocks));
        std::vector<int> cnt(static_cast<size_t>(blocks), 0);
        int bad = 0;
        SD_HIP(hipMemcpyAsync(part.data(), w.part.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        SD_HIP(hipMemcpyAsync(cnt.data(), w.cnt.p, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        SD_HIP(hipMemcpyAsync(&bad, w.flags.p, sizeof(int), hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        SD_CHECK(!bad, SPIMDECON_ERR_ARG, "thinout: non-finite distances");
        int64_t selected = 0;
        double vmin = 0, vmax = 0;
        for (int b = 0; b < blocks; ++b) {
            if (!cnt[size_t(b)]) continue;
            vmin = selected ? java_min(vmin, part[2 * size_t(b)]) : part[2 * size_t(b)];
            vmax = selected ? java_max(vmax, part[2 * size_t(b) + 1]) : part[2 * size_t(b) + 1];
            selected += cnt[size_t(b)];
        }
        SD_CHECK(selected > 0, SPIMDECON_ERR_ARG, "thinout: a histogram of an empty selection");
        // avoid the one value that is exactly 100% (:74): (max - min) + 0.000001, each rounded
        const double size = (vmax - vmin) + 0.000001;
        SD_HIP(hipMemsetAsync(w.bins.p, 0, size_t(num_bins) * sizeof(unsigned int), s));
        hipLaunchKernelGGL(k_to_hist, dim3(unsigned(blocks)), dim3(kToBlock), 0, s, dv, int(n), ds, vmin, size,
                           int(num_bins), w.bins.p, w.flags.p);
        SD_HIP(hipGetLastError());
        std::vector<unsigned int> bins(size_t(num_bins), 0u);
        SD_HIP(hipMemcpyAsync(bins.data(), w.bins.p, bins.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        SD_HIP(hipMemcpyAsync(&bad, w.flags.p, sizeof(int), hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        SD_CHECK(!bad, SPIMDECON_ERR_ARG,
                 "thinout: a distance falls beyond the last bin (max - min absorbs the 0.000001)");
        *out_min = vmin;
        *out_max = vmax;
        // :85-87: min + binSize / 2 + binSize * bin, the product and both sums rounded on their own
        // (the pragma at the head of the file)
        const double bin_size = size / double(num_bins);
        const double first = vmin + bin_size / 2;
        for (int b = 0; b < num_bins; ++b) {
            counts[b] = int64_t(bins[size_t(b)]);
            const double offset = bin_size * double(b);
            centres[b] = first + offset;
        }
    });
}

}  // namespace
}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" void spim_thinout_params_default(spim_thinout_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->min_distance = 0.0;   // ThinOut_Detections.defaultThresholdMinValue
    p->max_distance = 5.0;   // .defaultThresholdMaxValue
    p->keep_range = 0;       // .defaultRemoveKeepValue: 0 == remove
    p->t_split = 0;
    p->device = 0;
}

extern "C" void spim_thinout_tiles(int32_t* row_block, int32_t* col_tile) {
    if (row_block) *row_block = kToRBlock;
    if (col_tile) *col_tile = kToCTile;
}

extern "C" int spim_nn_distances(const double* pts, int64_t n, const double voxel[3], const spim_thinout_params* p,
                                 double* dist, int32_t* nearest) {
    return guarded([&] { thin_out(pts, n, voxel, p, dist, nearest, false, nullptr, 0, nullptr); });
}

extern "C" int spim_thin_out(const double* pts, int64_t n, const double voxel[3], const spim_thinout_params* p,
                             double* dist, int32_t* nearest, int32_t* kept, int64_t cap, int64_t* count) {
    return guarded([&] { thin_out(pts, n, voxel, p, dist, nearest, true, kept, cap, count); });
}

extern "C" int spim_distance_histogram(const double* dist, int64_t n, const uint8_t* select_or_null,
                                       int32_t num_bins, int device, double* min, double* max, int64_t* counts,
                                       double* centres) {
    return guarded(
        [&] { distance_histogram(dist, n, select_or_null, num_bins, device, min, max, counts, centres); });
}
