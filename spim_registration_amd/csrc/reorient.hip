// reorient.hip -- "Automatically reorientate and estimate based on sample features": the fusion
// bounding box from the interest points, under the rotation that makes it smallest, on MI355X.
//
// References (under the reference's src/main/java/spim/):
//   process/fusion/boundingbox/AutomaticReorientation.java:277-289   the padded integer box
//   .../AutomaticReorientation.java:306-401    determineOptimalBoundingBox (farthest pair, search)
//   .../AutomaticReorientation.java:413-447    testAxis
//   .../AutomaticReorientation.java:457-477    getRotation
//   .../AutomaticReorientation.java:488-512    determineSizeSimple
//   .../AutomaticReorientation.java:514-573    getAllDetectionsInGlobalCoordinates
//   vecmath/Transform3D.java:1397-1450, :4755-4765    set(AxisAngle4d), transform(Point3d)
//   vecmath/Vector3d.java:127-166                     cross, normalize
//
// Everything is double.  On the device every product, sum and difference is one explicit
// round-to-nearest intrinsic (__dmul_rn / __dadd_rn / __dsub_rn) in the source order of the Java
// code, which never contracts a multiply and an add; the host steps (the vector algebra,
// normalize, getRotation, the matrix of Transform3D.set, the volumes) are plain C++ under the
// build's -ffp-contract=off with std::sqrt / std::acos / std::sin / std::cos.
//   k_ro_world        one thread per used detection: w = M l, row by row ((m0 x + m1 y) + m2 z) + m3;
//                     the corresponding-index gather; flags a bad index and a non-finite result
//   k_ro_far_pair     the upper triangle of the n x n squared distances: a lane owns one row
//                     point, the column points go through LDS in tiles of kRoTile and are read as
//                     broadcasts; grid.x = row tiles, grid.y = partitions of that row's column
//                     tiles (pm_split); diagonal tiles take j > i.  Per lane a running (d, j), then
//                     a wave and a block reduction under the key (larger d, smaller i, smaller j):
//                     one partial per block, no atomics
//   k_ro_far_final    one block: the partials under the same key; then the reference's order of
//                     the pair (by x, except for the start pair (0, 1))
//   k_ro_axis_boxes   grid.y = the matrix (<= 27, kernel arguments), grid.x strides the points:
//                     Transform3D.transform, six Math.min / Math.max values (a NaN spreads,
//                     -0 < +0: order independent, so the tree does not show in the bits)
//   k_ro_axis_final   one block per matrix over the partials
// No kernel waits on another block; every loop is bounded by a count the host passes.
#include <algorithm>
#include <cmath>

#include "pointmatch.hpp"

namespace spimdecon {
namespace {

constexpr int kRoTile = 256;        // row points (lanes) per block = column points per LDS tile
constexpr int kRoBlock = 256;
constexpr int kRoMaxMats = 27;
constexpr int kRoBoxGrid = 64;      // at most that many blocks of points per matrix

struct RoModel {
    double m[12];
};
struct RoMats {
    double m[kRoMaxMats][12];
};

// Java Math.min / Math.max on doubles: a NaN operand is the result, -0 < +0
__device__ __forceinline__ double jmin(double a, double b) {
    double m = b < a ? b : a;               // a when either is NaN
    if (b != b && a == a) m = b;
    if (a == b) m = __longlong_as_double(__double_as_longlong(a) | __double_as_longlong(b));
    return m;
}
__device__ __forceinline__ double jmax(double a, double b) {
    double m = b > a ? b : a;
    if (b != b && a == a) m = b;
    if (a == b) m = __longlong_as_double(__double_as_longlong(a) & __double_as_longlong(b));
    return m;
}

// one row of AffineTransform3D.apply / Transform3D.transform
__device__ __forceinline__ double ro_row(const double* m, double x, double y, double z) {
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z)), m[3]);
}

// ---------------------------------------------------------------- world coordinates
// idx == nullptr: detection t of the list; else detection idx[t], which must lie in [0, n_src).
// flags[0] = 1: an index out of range (nothing is read through it); flags[1] = 1: a non-finite
// world coordinate.
__global__ __launch_bounds__(kRoBlock) void k_ro_world(const double* __restrict__ src, int64_t n_src,
                                                       const int64_t* __restrict__ idx, int n_used, RoModel mdl,
                                                       double* __restrict__ dst, int* __restrict__ flags) {
    const int t = int(blockIdx.x) * kRoBlock + int(threadIdx.x);
    if (t >= n_used) return;
    int64_t k = t;
    if (idx) {
        k = idx[t];
        if (k < 0 || k >= n_src) {
            flags[0] = 1;   // (every writer stores the same value)
            k = 0;
        }
    }
    const double x = src[3 * k], y = src[3 * k + 1], z = src[3 * k + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double w = ro_row(mdl.m + 4 * r, x, y, z);
        if (!(__dsub_rn(w, w) == 0.0)) flags[1] = 1;
        dst[3 * int64_t(t) + r] = w;
    }
}

// ---------------------------------------------------------------- the farthest pair
struct RoBest {
    double d;   // -1: none
    int i, j;
};

// (larger d, smaller i, smaller j): the pair the reference's scan keeps, whatever the launch
__device__ __forceinline__ bool ro_before(const RoBest& a, const RoBest& b) {
    if (a.d != b.d) return a.d > b.d;
    if (a.i != b.i) return a.i < b.i;
    return a.j < b.j;
}

__device__ __forceinline__ RoBest ro_block_best(RoBest b) {
    __shared__ double sd[kRoBlock / 64];
    __shared__ int si[kRoBlock / 64], sj[kRoBlock / 64];
    for (int off = 32; off > 0; off >>= 1) {
        RoBest o;
        o.d = __shfl_xor(b.d, off, 64);
        o.i = __shfl_xor(b.i, off, 64);
        o.j = __shfl_xor(b.j, off, 64);
        if (ro_before(o, b)) b = o;
    }
    if ((threadIdx.x & 63) == 0) {
        sd[threadIdx.x >> 6] = b.d;
        si[threadIdx.x >> 6] = b.i;
        sj[threadIdx.x >> 6] = b.j;
    }
    __syncthreads();
    b = RoBest{sd[0], si[0], sj[0]};
    for (int w = 1; w < kRoBlock / 64; ++w) {
        const RoBest o{sd[w], si[w], sj[w]};
        if (ro_before(o, b)) b = o;
    }
    return b;
}

// squareDistance(a, b): dx = a - b per axis, dx * dx + dy * dy + dz * dz
__device__ __forceinline__ double ro_d2(double ax, double ay, double az, const double* __restrict__ b) {
    const double dx = __dsub_rn(ax, b[0]), dy = __dsub_rn(ay, b[1]), dz = __dsub_rn(az, b[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Block (r, p): the row points of tile r against partition p of the column tiles r .. nt - 1,
// in ascending j.  The lane's maximum is replaced only by a strictly larger distance, so it
// ends at its smallest j.  Partials are [p][r]; an empty partition leaves d = -1 (a squared
// distance is never negative and, the points being finite, never a NaN).
__global__ __launch_bounds__(kRoBlock) void k_ro_far_pair(const double* __restrict__ pts, int n, int nt,
                                                          double* __restrict__ pd, int* __restrict__ pij) {
    __shared__ double tile[kRoTile * 3];
    const int r = int(blockIdx.x);
    const int i = r * kRoTile + int(threadIdx.x);
    const int ic = min(i, n - 1);
    const double ax = pts[3 * int64_t(ic)], ay = pts[3 * int64_t(ic) + 1], az = pts[3 * int64_t(ic) + 2];
    const int per = (nt - r + int(gridDim.y) - 1) / int(gridDim.y);
    const int c0 = int(min(int64_t(r) + int64_t(blockIdx.y) * per, int64_t(nt)));
    const int c1 = int(min(int64_t(c0) + per, int64_t(nt)));
    double best = -1.0;
    int bj = -1;
    for (int c = c0; c < c1; ++c) {
        const int j0 = c * kRoTile;
        const int cnt = min(kRoTile, n - j0);
        __syncthreads();
        for (int e = int(threadIdx.x); e < cnt * 3; e += kRoBlock) tile[e] = pts[3 * int64_t(j0) + e];
        __syncthreads();
        if (c == r) {   // the diagonal tile: j > i only
#pragma unroll 4
            for (int t = 0; t < cnt; ++t) {   // tile[3 t ..]: the same address in every lane, a broadcast
                const double d = ro_d2(ax, ay, az, tile + 3 * t);
                if (j0 + t > i && d > best) {
                    best = d;
                    bj = j0 + t;
                }
            }
        } else {
#pragma unroll 8
            for (int t = 0; t < cnt; ++t) {
                const double d = ro_d2(ax, ay, az, tile + 3 * t);
                if (d > best) {
                    best = d;
                    bj = j0 + t;
                }
            }
        }
    }
    RoBest b{best, i, bj};
    if (i >= n || bj < 0) b = RoBest{-1.0, n, n};
    b = ro_block_best(b);
    if (threadIdx.x == 0) {
        const int64_t o = int64_t(blockIdx.y) * gridDim.x + blockIdx.x;
        pd[o] = b.d;
        pij[2 * o] = b.i;
        pij[2 * o + 1] = b.j;
    }
}

// out_d[0] = maxDist, out_ij = (index of p1, index of p2): AutomaticReorientation.java:329-342
// orders a new maximum by a[0] <= b[0]; the start pair (0, 1) is never reordered.
__global__ __launch_bounds__(kRoBlock) void k_ro_far_final(const double* __restrict__ pts,
                                                           const double* __restrict__ pd,
                                                           const int* __restrict__ pij, int64_t nparts,
                                                           double* __restrict__ out_d, int* __restrict__ out_ij) {
    RoBest b{-1.0, INT32_MAX, INT32_MAX};
    for (int64_t k = threadIdx.x; k < nparts; k += kRoBlock) {
        const RoBest o{pd[k], pij[2 * k], pij[2 * k + 1]};
        if (ro_before(o, b)) b = o;
    }
    b = ro_block_best(b);
    if (threadIdx.x != 0) return;
    int p1 = b.i, p2 = b.j;
    if (b.d < 0.0) {   // no pair at all (fewer than two points: the host refuses that before)
        p1 = p2 = -1;
    } else if (!(p1 == 0 && p2 == 1) && !(pts[3 * int64_t(p1)] <= pts[3 * int64_t(p2)])) {
        p1 = b.j;
        p2 = b.i;
    }
    out_d[0] = b.d;
    out_ij[0] = p1;
    out_ij[1] = p2;
}

// ---------------------------------------------------------------- boxes under M transforms
__device__ __forceinline__ void ro_block_box(double* v) {   // v: min x, y, z, max x, y, z
    __shared__ double sv[kRoBlock / 64][6];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int off = 32; off > 0; off >>= 1) {
            v[a] = jmin(v[a], __shfl_xor(v[a], off, 64));
            v[3 + a] = jmax(v[3 + a], __shfl_xor(v[3 + a], off, 64));
        }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 6; ++a) sv[threadIdx.x >> 6][a] = v[a];
    __syncthreads();
    for (int a = 0; a < 6; ++a) v[a] = sv[0][a];
    for (int w = 1; w < kRoBlock / 64; ++w)
        for (int a = 0; a < 3; ++a) {
            v[a] = jmin(v[a], sv[w][a]);
            v[3 + a] = jmax(v[3 + a], sv[w][3 + a]);
        }
}

// RAW: the coordinates as they are (determineSizeSimple); else under mats.m[blockIdx.y] as
// Transform3D.transform computes them.  part: [matrix][block][6].
template <bool RAW>
__global__ __launch_bounds__(kRoBlock) void k_ro_axis_boxes(const double* __restrict__ pts, int n, RoMats mats,
                                                            double* __restrict__ part) {
    const double* m = mats.m[blockIdx.y];
    double v[6] = {kJavaDoubleMax, kJavaDoubleMax, kJavaDoubleMax, -kJavaDoubleMax, -kJavaDoubleMax, -kJavaDoubleMax};
    for (int64_t i = int64_t(blockIdx.x) * kRoBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kRoBlock) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const double t[3] = {RAW ? x : ro_row(m, x, y, z), RAW ? y : ro_row(m + 4, x, y, z),
                             RAW ? z : ro_row(m + 8, x, y, z)};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[a] = jmin(v[a], t[a]);
            v[3 + a] = jmax(v[3 + a], t[a]);
        }
    }
    ro_block_box(v);
    if (threadIdx.x == 0) {
        double* o = part + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 6;
        for (int a = 0; a < 6; ++a) o[a] = v[a];
    }
}

__global__ __launch_bounds__(kRoBlock) void k_ro_axis_final(const double* __restrict__ part, int nblocks,
                                                            double* __restrict__ out) {
    const double* p = part + int64_t(blockIdx.x) * nblocks * 6;
    double v[6] = {kJavaDoubleMax, kJavaDoubleMax, kJavaDoubleMax, -kJavaDoubleMax, -kJavaDoubleMax, -kJavaDoubleMax};
    for (int k = int(threadIdx.x); k < nblocks; k += kRoBlock)
        for (int a = 0; a < 3; ++a) {
            v[a] = jmin(v[a], p[6 * k + a]);
            v[3 + a] = jmax(v[3 + a], p[6 * k + 3 + a]);
        }
    ro_block_box(v);
    if (threadIdx.x == 0)
        for (int a = 0; a < 6; ++a) out[6 * int64_t(blockIdx.x) + a] = v[a];
}

// ---------------------------------------------------------------- host side
struct RoWork : PmWork {
    DBuf<double> stage, world, pd, part, boxes, far_d;
    DBuf<int> pij, far_ij, flags;
    DBuf<int64_t> idx;
    void release() {
        release_stream();
        release_all(bad, stage, world, pd, part, boxes, far_d, pij, far_ij, flags, idx);
    }
};

// the matchers' rules for a point list, every message led by the caller's name
void ro_check_points(const double* pts, int64_t n, const char* who) {
    SD_CHECK(n >= 0, SPIMDECON_ERR_ARG, std::string(who) + ": negative point count");
    SD_CHECK(pts || n == 0, SPIMDECON_ERR_ARG, std::string(who) + ": null point list with a positive count");
    pm_check_points(pts, n, who);
}

struct FarPair {
    int p1, p2;
    double d2;
};

// dpts: n >= 2 finite points on the device
FarPair far_pair_device(RoWork& w, const double* dpts, int64_t n, int64_t requested_split, int dev, hipStream_t s,
                        const char* who) {
    SD_CHECK(n <= (int64_t(1) << 30), SPIMDECON_ERR_ARG, std::string(who) + ": more than 2^30 points");
    const int64_t nt = ceil_div(n, kRoTile);
    // 160,000 points are 625 row tiles of 625 .. 1 column tiles, the long ones first; aim at 4
    // blocks of 4 waves per CU
    const PmSplit sp = pm_split(requested_split, nt, n, kRoTile, 4, dev, who);
    const int64_t nparts = nt * sp.split;
    grow(w.pd, size_t(nparts));
    grow(w.pij, size_t(2 * nparts));
    grow(w.far_d, 1);
    grow(w.far_ij, 2);
    hipLaunchKernelGGL(k_ro_far_pair, dim3(unsigned(nt), unsigned(sp.split)), dim3(kRoBlock), 0, s, dpts, int(n),
                       int(nt), w.pd.p, w.pij.p);
    hipLaunchKernelGGL(k_ro_far_final, dim3(1), dim3(kRoBlock), 0, s, dpts, w.pd.p, w.pij.p, nparts, w.far_d.p,
                       w.far_ij.p);
    SD_HIP(hipGetLastError());
    FarPair f{};
    int ij[2] = {0, 0};
    SD_HIP(hipMemcpyAsync(&f.d2, w.far_d.p, sizeof(double), hipMemcpyDeviceToHost, s));
    SD_HIP(hipMemcpyAsync(ij, w.far_ij.p, sizeof(ij), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
    f.p1 = ij[0];
    f.p2 = ij[1];
    SD_CHECK(f.p1 >= 0 && f.p1 < n && f.p2 >= 0 && f.p2 < n && f.p1 != f.p2, SPIMDECON_ERR_STATE,
             std::string(who) + ": no farthest pair");
    return f;
}

// out: m x 6 doubles on the host; raw: m == 1, the coordinates as they are
void axis_boxes_device(RoWork& w, const double* dpts, int64_t n, const double* mats, int m, bool raw, double* out,
                       hipStream_t s) {
    RoMats a;
    std::memset(&a, 0, sizeof(a));
    if (!raw) std::memcpy(a.m, mats, size_t(m) * 12 * sizeof(double));
    const int gx = int(std::max<int64_t>(1, std::min<int64_t>(kRoBoxGrid, ceil_div(n, 4 * kRoBlock))));
    grow(w.part, size_t(kRoMaxMats) * kRoBoxGrid * 6);
    grow(w.boxes, size_t(kRoMaxMats) * 6);
    if (raw)
        hipLaunchKernelGGL(k_ro_axis_boxes<true>, dim3(unsigned(gx), unsigned(m)), dim3(kRoBlock), 0, s, dpts, int(n),
                           a, w.part.p);
    else
        hipLaunchKernelGGL(k_ro_axis_boxes<false>, dim3(unsigned(gx), unsigned(m)), dim3(kRoBlock), 0, s, dpts,
                           int(n), a, w.part.p);
    hipLaunchKernelGGL(k_ro_axis_final, dim3(unsigned(m)), dim3(kRoBlock), 0, s, w.part.p, gx, w.boxes.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipMemcpyAsync(out, w.boxes.p, size_t(m) * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
}

// ---- vecmath on the host, operation by operation
struct Vec3 {
    double x, y, z;
};

// Vector3d.normalize: 1.0 / Math.sqrt, then three products (a zero vector becomes NaN)
Vec3 normalize(Vec3 v) {
    const double norm = 1.0 / std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    return {v.x * norm, v.y * norm, v.z * norm};
}

void set_identity(double* t) {
    std::memset(t, 0, 12 * sizeof(double));
    t[0] = t[5] = t[10] = 1.0;
}

// getRotation (:457-477) as the 3 x 4 head of its Transform3D: Vector3d.cross, normalize, the
// identity for a NaN axis (parallel and antiparallel vectors alike), Math.acos of the dot
// product, Transform3D.set(AxisAngle4d) with its almostZero branch
void rotation(Vec3 v0, Vec3 v1, double* t) {
    Vec3 ax;
    ax.x = v0.y * v1.z - v0.z * v1.y;
    ax.y = v1.x * v0.z - v1.z * v0.x;
    ax.z = v0.x * v1.y - v0.y * v1.x;
    ax = normalize(ax);
    if (std::isnan(ax.x)) return set_identity(t);
    const double angle = std::acos(v0.x * v1.x + v0.y * v1.y + v0.z * v1.z);
    double mag = std::sqrt(ax.x * ax.x + ax.y * ax.y + ax.z * ax.z);
    if (mag < 1.0e-5 && mag > -1.0e-5) return set_identity(t);   // almostZero: EPSILON_ABSOLUTE
    mag = 1.0 / mag;
    const double x = ax.x * mag, y = ax.y * mag, z = ax.z * mag;
    const double sinTheta = std::sin(angle), cosTheta = std::cos(angle);
    const double u = 1.0 - cosTheta;
    const double xz = x * z, xy = x * y, yz = y * z;
    t[0] = u * x * x + cosTheta;
    t[1] = u * xy - sinTheta * z;
    t[2] = u * xz + sinTheta * y;
    t[3] = 0.0;
    t[4] = u * xy + sinTheta * z;
    t[5] = u * y * y + cosTheta;
    t[6] = u * yz - sinTheta * x;
    t[7] = 0.0;
    t[8] = u * xz - sinTheta * y;
    t[9] = u * yz + sinTheta * x;
    t[10] = u * z * z + cosTheta;
    t[11] = 0.0;
}

double volume(const double* b) { return (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]); }

// Math.min / Math.max for the host's one use (finite operands or a NaN that must spread)
double host_jmax(double a, double b) {
    if (a != a) return a;
    if (a == 0.0 && b == 0.0 && std::signbit(a)) return b;
    return a >= b ? a : b;
}

// Math.round, then the cast: floor(x + 0.5); beyond the int range is refused here
int64_t round_to_int(double x, const char* who) {
    SD_CHECK(std::isfinite(x) && std::fabs(x) < 2147483000.0, SPIMDECON_ERR_ARG,
             std::string(who) + ": bounding box beyond the int range");
    return int64_t(std::floor(x + 0.5));
}

void far_pair_call(const double* pts, int64_t n, int device, int32_t* i, int32_t* j, double* d2) {
    const char* who = "farthest_pair";
    SD_CHECK(i && j && d2, SPIMDECON_ERR_ARG, "farthest_pair: null argument");
    ro_check_points(pts, n, who);
    SD_CHECK(n >= 2, SPIMDECON_ERR_ARG, "farthest_pair: at least two points are required");
    with_work<RoWork>(device, [&](RoWork& w, hipStream_t s) {
        const double* d = pm_stage_points(pts, n, device, w.world, w.bad, s, who);
        const FarPair f = far_pair_device(w, d, n, 0, device, s, who);
        *i = f.p1;
        *j = f.p2;
        *d2 = f.d2;
    });
}

void axis_boxes_call(const double* pts, int64_t n, const double* mats, int m, bool raw, int device, double* out,
                     const char* who) {
    SD_CHECK(out && (raw || mats), SPIMDECON_ERR_ARG, std::string(who) + ": null argument");
    SD_CHECK(m >= 1 && m <= kRoMaxMats, SPIMDECON_ERR_ARG,
             std::string(who) + ": 1 .. " + std::to_string(kRoMaxMats) + " matrices");
    ro_check_points(pts, n, who);
    SD_CHECK(n >= 1, SPIMDECON_ERR_ARG, std::string(who) + ": at least one point is required");
    with_work<RoWork>(device, [&](RoWork& w, hipStream_t s) {
        const double* d = pm_stage_points(pts, n, device, w.world, w.bad, s, who);
        axis_boxes_device(w, d, n, mats, m, raw, out, s);
    });
}

void reorient_bounding_box(int n_views, const double* const* lists, const int64_t* counts,
                           const int64_t* const* corr, const int64_t* corr_counts, const double* models,
                           const spim_reorient_params* p, spim_reorient_result* res) {
    const char* who = "reorient";
    SD_CHECK(p && res && n_views >= 1 && lists && counts && models, SPIMDECON_ERR_ARG, "reorient: null argument");
    SD_CHECK(!p->use_corresponding || (corr && corr_counts), SPIMDECON_ERR_ARG,
             "reorient: use_corresponding needs the index lists");
    SD_CHECK(std::isfinite(p->percent) && p->percent >= 0.0, SPIMDECON_ERR_ARG,
             "reorient: percent must be finite and >= 0");
    SD_CHECK(p->far_split >= 0, SPIMDECON_ERR_ARG, "reorient: far_split must be >= 0");
    std::memset(res, 0, sizeof(*res));
    res->far_i = res->far_j = -1;
    int64_t n = 0, max_list = 0;
    for (int v = 0; v < n_views; ++v) {
        ro_check_points(lists[v], counts[v], who);
        for (int k = 0; k < 12; ++k)
            SD_CHECK(std::isfinite(models[12 * v + k]), SPIMDECON_ERR_ARG, "reorient: non-finite model");
        int64_t used = counts[v];
        if (p->use_corresponding) {
            used = corr_counts[v];
            SD_CHECK(used >= 0 && (corr[v] || used == 0), SPIMDECON_ERR_ARG,
                     "reorient: null index list with a positive count");
            SD_CHECK(used == 0 || counts[v] > 0, SPIMDECON_ERR_ARG, "reorient: indices into an empty list");
        }
        n += used;
        max_list = std::max(max_list, counts[v]);
        SD_CHECK(n <= int64_t(INT32_MAX), SPIMDECON_ERR_ARG, "reorient: more than 2^31 - 1 points");
    }
    // deliberate deviation: the reference reports "At least one point is required" for none and
    // fails on points.get(1) for one; both are refused here
    SD_CHECK(n >= (p->reorientate ? 2 : 1), SPIMDECON_ERR_ARG,
             p->reorientate ? "reorient: at least two points are required"
                            : "reorient: at least one point is required");
    res->n_points = n;
    const int dev = p->device;
    with_work<RoWork>(dev, [&](RoWork& w, hipStream_t s) {
        grow(w.world, size_t(3 * n));
        grow(w.stage, size_t(3 * std::max<int64_t>(max_list, 1)));
        grow(w.flags, 2);
        SD_HIP(hipMemsetAsync(w.flags.p, 0, 2 * sizeof(int), s));
        int64_t o = 0;
        for (int v = 0; v < n_views; ++v) {   // getAllDetectionsInGlobalCoordinates: the views in order
            const int64_t used = p->use_corresponding ? corr_counts[v] : counts[v];
            if (!used) continue;
            const double* dl = pm_stage_points(lists[v], counts[v], dev, w.stage, w.bad, s, who);
            const int64_t* di = nullptr;
            if (p->use_corresponding) {
                di = corr[v];
                if (!is_device_ptr(di, dev)) {
                    grow(w.idx, size_t(used));
                    SD_HIP(hipMemcpyAsync(w.idx.p, corr[v], size_t(used) * sizeof(int64_t), hipMemcpyDefault, s));
                    di = w.idx.p;
                }
            }
            RoModel mdl;
            std::memcpy(mdl.m, models + 12 * v, sizeof(mdl.m));
            hipLaunchKernelGGL(k_ro_world, dim3(unsigned(ceil_div(used, kRoBlock))), dim3(kRoBlock), 0, s, dl,
                               counts[v], di, int(used), mdl, w.world.p + 3 * o, w.flags.p);
            SD_HIP(hipGetLastError());
            SD_HIP(hipStreamSynchronize(s));   // (the staging buffers are used again by the next view)
            o += used;
        }
        int flags[2] = {0, 0};
        SD_HIP(hipMemcpyAsync(flags, w.flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        SD_CHECK(!flags[0], SPIMDECON_ERR_ARG, "reorient: corresponding index out of range");
        SD_CHECK(!flags[1], SPIMDECON_ERR_ARG, "reorient: non-finite coordinates under the model");
        const double* dw = w.world.p;
        double box[6];
        set_identity(res->transform);
        if (!p->reorientate) {   // determineSizeSimple
            axis_boxes_device(w, dw, n, nullptr, 1, true, box, s);
        } else {                 // determineOptimalBoundingBox
            const FarPair f = far_pair_device(w, dw, n, p->far_split, dev, s, who);
            res->far_i = f.p1;
            res->far_j = f.p2;
            res->far_d2 = f.d2;
            double p1[3], p2[3];
            SD_HIP(hipMemcpyAsync(p1, dw + 3 * int64_t(f.p1), sizeof(p1), hipMemcpyDeviceToHost, s));
            SD_HIP(hipMemcpyAsync(p2, dw + 3 * int64_t(f.p2), sizeof(p2), hipMemcpyDeviceToHost, s));
            SD_HIP(hipStreamSynchronize(s));
            Vec3 sv = normalize({p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]});
            const Vec3 x_axis = {1.0, 0.0, 0.0};
            double mats[kRoMaxMats * 12], boxes[kRoMaxMats * 6];
            rotation(sv, x_axis, mats);
            axis_boxes_device(w, dw, n, mats, 1, false, boxes, s);   // the volume the reference logs first
            res->start_volume = volume(boxes);
            const double steps[8] = {0.4, 0.2, 0.1, 0.05, 0.025, 0.01, 0.005, 0.001};
            double min_volume = kJavaDoubleMax;
            bool have = false;
            for (double step : steps) {
                Vec3 cand[kRoMaxMats];
                int k = 0;
                for (int zi = -1; zi <= 1; ++zi)
                    for (int yi = -1; yi <= 1; ++yi)
                        for (int xi = -1; xi <= 1; ++xi, ++k) {
                            cand[k] = normalize({sv.x + xi * step, sv.y + yi * step, sv.z + zi * step});
                            rotation(cand[k], x_axis, mats + 12 * k);
                        }
                axis_boxes_device(w, dw, n, mats, kRoMaxMats, false, boxes, s);
                Vec3 best_sv = sv;
                for (k = 0; k < kRoMaxMats; ++k) {
                    const double vol = volume(boxes + 6 * k);
                    if (vol < min_volume) {
                        min_volume = vol;
                        std::memcpy(box, boxes + 6 * k, sizeof(box));
                        best_sv = cand[k];
                        have = true;
                    }
                }
                sv = best_sv;
            }
            SD_CHECK(have, SPIMDECON_ERR_ARG, "reorient: no candidate axis gives a volume");
            res->min_volume = min_volume;
            res->axis[0] = sv.x;
            res->axis[1] = sv.y;
            res->axis[2] = sv.z;
            rotation(sv, x_axis, res->transform);
        }
        for (int a = 0; a < 3; ++a) {
            res->min_f[a] = box[a];
            res->max_f[a] = box[3 + a];
        }
    });
    // :277-289
    const double* mn = res->min_f;
    const double* mx = res->max_f;
    const double add_x = (mx[0] - mn[0]) * (p->percent / 100.0) / 2;
    const double add_y = (mx[1] - mn[1]) * (p->percent / 100.0) / 2;
    const double add_z = (mx[2] - mn[2]) * (p->percent / 100.0) / 2;
    const double add = host_jmax(add_x, host_jmax(add_y, add_z));
    for (int a = 0; a < 3; ++a) {
        res->bb_min[a] = round_to_int(mn[a] - add, who);
        res->bb_max[a] = round_to_int(mx[a] + add, who);
        res->bb_dims[a] = res->bb_max[a] - res->bb_min[a] + 1;
    }
}

}  // namespace
}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" void spim_reorient_tile(int32_t* tile) {
    if (tile) *tile = kRoTile;
}

extern "C" int spim_farthest_pair(const double* pts, int64_t n, int device, int32_t* i, int32_t* j, double* d2) {
    return guarded([&] { far_pair_call(pts, n, device, i, j, d2); });
}

extern "C" int spim_axis_boxes(const double* pts, int64_t n, const double* mats, int m, int device, double* out6m) {
    return guarded([&] { axis_boxes_call(pts, n, mats, m, false, device, out6m, "axis_boxes"); });
}

extern "C" int spim_points_min_max(const double* pts, int64_t n, int device, double* out6) {
    return guarded([&] { axis_boxes_call(pts, n, nullptr, 1, true, device, out6, "points_min_max"); });
}

extern "C" void spim_reorient_params_default(spim_reorient_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->use_corresponding = 1;   // AutomaticReorientation.defaultDetections
    p->reorientate = 1;
    p->percent = 10.0;          // .defaultPercent
}

extern "C" int spim_reorient_bounding_box(int n_views, const double* const* lists, const int64_t* counts,
                                          const int64_t* const* corr, const int64_t* corr_counts,
                                          const double* models, const spim_reorient_params* params,
                                          spim_reorient_result* result) {
    return guarded([&] { reorient_bounding_box(n_views, lists, counts, corr, corr_counts, models, params, result); });
}

extern "C" int spim_reorient_release_workspace(int device) {
    return guarded([&] { release_work<RoWork>(device); });
}
