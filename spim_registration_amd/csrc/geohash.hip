// geohash.hip -- "fast 3d geometric hashing (rotation invariant)" of two bead lists on MI355X:
// the candidate stage of the reference's first registration matcher.
//
// References (under the reference's src/main/java/):
//   spim/process/interestpointregistration/geometrichashing/GeometricHashingPairwise.java:45-86   the call, fewer than 4
//   .../geometrichashing/GeometricHasher.java:54-85     two nearest B descriptors, threshold and ratio test
//   .../geometrichashing/GeometricHasher.java:87-116    3 nearest neighbours per point, normalize = false
//   .../geometrichashing/GeometricHashingParameters.java   50 / 10
//   mpicbg/pointdescriptor/AbstractPointDescriptor.java:54-76              neighbour - basis in double
//   mpicbg/pointdescriptor/LocalCoordinateSystemPointDescriptor.java:59-162  the local coordinate system
//   .../LocalCoordinateSystemPointDescriptor.java:37-51, :172-175            descriptorDistance, distanceTo
//   spim/vecmath/Vector3d.java:127, :157, :175, :195                         cross, normalize, dot, length
//   spim/vecmath/Matrix3d.java:1212-1263, :1284-1431, :1451-1509, :2321      invertGeneral, LU, transform
//
// Every double and float operation is one explicit round-to-nearest intrinsic in the source
// order of the Java code (which never contracts a multiply and an add), so the six floats of a
// descriptor and every descriptor distance are bit-exact against a restatement.  Unpinned: the
// reference ranks B descriptors with fiji.util.KDTree (not in its tree); here by
// (float) Math.sqrt(descriptorDistance) ascending, equal floats by lower B index, a NaN distance
// not ranked.
//   k_pm_knn<3>       (pointmatch.hip) per point the 3 nearest others, neighbour - basis in double
//   k_gh_descriptors  one thread per point: x / y / n axes, 3x3 LU inverse, (ax bx by cx cy cz) float
//   k_gh_match        a lane owns one A descriptor in registers; B descriptors go through LDS in
//                     tiles and are read as broadcasts; grid.y splits B (partial two best)
//   k_gh_merge        partials in ascending B order -> two best by (key, index); the two tests
//   k_pm_compact      (pointmatch.hip) the candidates in ascending A order
// The call around them -- argument rules, staging, "not enough detections", the result copies --
// is pm_match_candidates (pointmatch.hpp), shared with rgldm.hip.
// No atomics; every output is written with ordinary stores.
#include <algorithm>
#include <cfloat>

#include "pointmatch.hpp"

namespace spimdecon {
namespace {

constexpr int kGhATile = 256;    // A descriptors (lanes) per block of k_gh_match
constexpr int kGhBTile = 256;    // B descriptors per LDS tile
constexpr int kGhBlock = 256;
constexpr int kGhMinPoints = 4;  // GeometricHashingPairwise.java:58

struct GhVec {
    double x, y, z;
};

// Vector3d.cross (:127-136)
__device__ __forceinline__ GhVec gh_cross(const GhVec& v1, const GhVec& v2) {
    GhVec r;
    r.x = __dsub_rn(__dmul_rn(v1.y, v2.z), __dmul_rn(v1.z, v2.y));
    r.y = __dsub_rn(__dmul_rn(v2.x, v1.z), __dmul_rn(v2.z, v1.x));
    r.z = __dsub_rn(__dmul_rn(v1.x, v2.y), __dmul_rn(v1.y, v2.x));
    return r;
}
__device__ __forceinline__ double gh_len2(const GhVec& v) {
    return __dadd_rn(__dadd_rn(__dmul_rn(v.x, v.x), __dmul_rn(v.y, v.y)), __dmul_rn(v.z, v.z));
}
// Vector3d.normalize() (:157-166)
__device__ __forceinline__ GhVec gh_normalize(const GhVec& v) {
    const double norm = __ddiv_rn(1.0, __dsqrt_rn(gh_len2(v)));
    return GhVec{__dmul_rn(v.x, norm), __dmul_rn(v.y, norm), __dmul_rn(v.z, norm)};
}
// Vector3d.dot (:175-178)
__device__ __forceinline__ double gh_dot(const GhVec& a, const GhVec& b) {
    return __dadd_rn(__dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)), __dmul_rn(a.z, b.z));
}
// Matrix3d.transform(Tuple3d) (:2321-2328)
__device__ __forceinline__ GhVec gh_transform(const double (&m)[9], const GhVec& t) {
    GhVec r;
    r.x = __dadd_rn(__dadd_rn(__dmul_rn(m[0], t.x), __dmul_rn(m[1], t.y)), __dmul_rn(m[2], t.z));
    r.y = __dadd_rn(__dadd_rn(__dmul_rn(m[3], t.x), __dmul_rn(m[4], t.y)), __dmul_rn(m[5], t.z));
    r.z = __dadd_rn(__dadd_rn(__dmul_rn(m[6], t.x), __dmul_rn(m[7], t.y)), __dmul_rn(m[8], t.z));
    return r;
}

// Matrix3d.invertGeneral (:1212-1263): luDecomposition, then luBacksubstitution on the identity.
// false = no inverse: the SingularMatrixException of a false luDecomposition and its
// RuntimeException (no pivot: every candidate NaN), which the caller's catch treats alike.
// Every index is a compile-time constant after unrolling (a dynamic row is a chain of
// selects), so m, res and the scales stay in registers.
__device__ __forceinline__ bool gh_invert(double (&m)[9], double (&res)[9]) {
    double row_scale[3];
    int row_perm[3];
    // implicit scaling per row (:1290-1323)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double big = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double temp = fabs(m[3 * i + j]);
            if (temp > big) big = temp;
        }
        if (big == 0.0) return false;
        row_scale[i] = __ddiv_rn(1.0, big);
    }
    // Crout's method over the columns (:1332-1427)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) {   // upper triangle
            double sum = m[3 * i + j];
#pragma unroll
            for (int k = 0; k < i; ++k) sum = __dsub_rn(sum, __dmul_rn(m[3 * i + k], m[3 * k + j]));
            m[3 * i + j] = sum;
        }
        double big = 0.0;
        int imax = -1;
#pragma unroll
        for (int i = j; i < 3; ++i) {   // lower triangle and the pivot search
            double sum = m[3 * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) sum = __dsub_rn(sum, __dmul_rn(m[3 * i + k], m[3 * k + j]));
            m[3 * i + j] = sum;
            const double temp = __dmul_rn(row_scale[i], fabs(sum));
            if (temp >= big) {
                big = temp;
                imax = i;
            }
        }
        if (imax < 0) return false;
#pragma unroll
        for (int r = j + 1; r < 3; ++r) {   // j != imax: exchange rows imax and j
            if (r == imax) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double temp = m[3 * r + k];
                    m[3 * r + k] = m[3 * j + k];
                    m[3 * j + k] = temp;
                }
                row_scale[r] = row_scale[j];
            }
        }
        row_perm[j] = imax;
        if (m[3 * j + j] == 0.0) return false;
        if (j != 2) {
            const double temp = __ddiv_rn(1.0, m[3 * j + j]);
#pragma unroll
            for (int i = j + 1; i < 3; ++i) m[3 * i + j] = __dmul_rn(m[3 * i + j], temp);
        }
    }
    // luBacksubstitution on the identity, column by column (:1463-1508)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double c[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        int ii = -1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int ip = row_perm[i];   // i <= ip <= 2
            double sum = c[i];
#pragma unroll
            for (int r = i + 1; r < 3; ++r) {
                if (r == ip) {
                    sum = c[r];
                    c[r] = c[i];
                }
            }
            if (ii >= 0) {
#pragma unroll
                for (int j = 0; j < i; ++j)
                    if (j >= ii) sum = __dsub_rn(sum, __dmul_rn(m[3 * i + j], c[j]));
            } else if (sum != 0.0) {
                ii = i;
            }
            c[i] = sum;
        }
        c[2] = __ddiv_rn(c[2], m[8]);
        c[1] = __ddiv_rn(__dsub_rn(c[1], __dmul_rn(m[5], c[2])), m[4]);
        c[0] = __ddiv_rn(__dsub_rn(__dsub_rn(c[0], __dmul_rn(m[1], c[1])), __dmul_rn(m[2], c[2])), m[0]);
        res[k] = c[0];
        res[3 + k] = c[1];
        res[6 + k] = c[2];
    }
    return true;
}

// buildLocalCoordinateSystem (:59-162), normalize = false: rel = the 3 relative vectors of a
// point, nearest first; desc = ax bx by cx cy cz.
__global__ __launch_bounds__(kGhBlock) void k_gh_descriptors(const double* __restrict__ rel, int n,
                                                             float* __restrict__ desc) {
    const int i = int(blockIdx.x) * kGhBlock + int(threadIdx.x);
    if (i >= n) return;
    const double* r = rel + int64_t(i) * 9;
    const GhVec b{r[0], r[1], r[2]}, c{r[3], r[4], r[5]}, d{r[6], r[7], r[8]};
    const GhVec x = gh_normalize(d);
    const float ax = float(__dsqrt_rn(gh_len2(d)));
    GhVec nv = gh_normalize(gh_cross(b, x));
    if (gh_dot(nv, c) < 0) nv = GhVec{-nv.x, -nv.y, -nv.z};
    const GhVec y = gh_normalize(gh_cross(nv, x));
    double m[9] = {x.x, y.x, nv.x, x.y, y.y, nv.y, x.z, y.z, nv.z};
    double inv[9];
    float bx = 0.0f, by = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (gh_invert(m, inv)) {
        const GhVec bl = gh_transform(inv, b), cl = gh_transform(inv, c);
        bx = float(bl.x);
        by = float(bl.y);
        cx = float(cl.x);
        cy = float(cl.y);
        cz = float(cl.z);
    }
    float* o = desc + int64_t(i) * 6;
    o[0] = ax;
    o[1] = bx;
    o[2] = by;
    o[3] = cx;
    o[4] = cy;
    o[5] = cz;
}

// The two best ranked so far: key = (float) Math.sqrt(distance), d the double distance behind
// it, idx < 0 = empty (an empty slot ranks behind everything, also behind an infinite key).
struct GhTop2 {
    float k1, k2;
    double d1, d2;
    int i1, i2;
};
__device__ __forceinline__ void gh_top2_init(GhTop2& t) {
    t.k1 = t.k2 = __builtin_inff();
    t.d1 = t.d2 = __builtin_inf();
    t.i1 = t.i2 = -1;
}
// Entries come in ascending B index, so strict < keeps the lower index in front of an equal key.
__device__ __forceinline__ void gh_top2_insert(GhTop2& t, double s, int j) {
    const bool full = t.i2 >= 0;
    if (!(s < t.d2)) {
        // a full pair: sqrt and the float rounding are monotone, so the key is no smaller than
        // the second's either; not full: only an infinite distance (ranked) or a NaN (not)
        if (full || s != s) return;
    }
    const float key = float(__dsqrt_rn(s));
    if (full && !(key < t.k2)) return;
    if (t.i1 < 0 || key < t.k1) {
        t.k2 = t.k1; t.d2 = t.d1; t.i2 = t.i1;
        t.k1 = key; t.d1 = s; t.i1 = j;
    } else {
        t.k2 = key; t.d2 = s; t.i2 = j;
    }
}

// descriptorDistance (:37-51): float differences and float products, widened and summed in
// double in the order ax bx by cx cy cz (0.0 + p0 == p0: a square is never -0)
__device__ __forceinline__ double gh_distance(const float (&a)[6], const float* __restrict__ b) {
    float p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float df = __fsub_rn(a[k], b[k]);
        p[k] = __fmul_rn(df, df);
    }
    double s = double(p[0]);
#pragma unroll
    for (int k = 1; k < 6; ++k) s = __dadd_rn(s, double(p[k]));
    return s;
}

// One block: kGhATile A descriptors against the B descriptors of partition blockIdx.y.
// Partials are [partition][na].
__global__ __launch_bounds__(kGhATile) void k_gh_match(const float* __restrict__ da, int na,
                                                       const float* __restrict__ db, int nb, int chunk,
                                                       double* __restrict__ pd1, double* __restrict__ pd2,
                                                       int* __restrict__ pi1, int* __restrict__ pi2) {
    __shared__ float sb[kGhBTile * 6];
    const int i = int(blockIdx.x) * kGhATile + int(threadIdx.x);
    const int ic = min(i, na - 1);
    float a[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = da[int64_t(ic) * 6 + k];
    const int b0 = int(min(int64_t(blockIdx.y) * chunk, int64_t(nb)));
    const int b1 = int(min(int64_t(b0) + chunk, int64_t(nb)));
    GhTop2 top;
    gh_top2_init(top);
    for (int j0 = b0; j0 < b1; j0 += kGhBTile) {
        const int cnt = min(kGhBTile, b1 - j0);
        __syncthreads();
        for (int e = int(threadIdx.x); e < cnt * 6; e += kGhATile) sb[e] = db[int64_t(j0) * 6 + e];
        __syncthreads();
        for (int t = 0; t < cnt; ++t)   // sb + t * 6: the same address in every lane, a broadcast
            gh_top2_insert(top, gh_distance(a, sb + t * 6), j0 + t);
    }
    if (i < na) {
        const int64_t o = int64_t(blockIdx.y) * na + i;
        pd1[o] = top.d1;
        pd2[o] = top.d2;
        pi1[o] = top.i1;
        pi2[o] = top.i2;
    }
}

// The partitions in ascending B order through the same insertion; then GeometricHasher.java:67-70.
// Fewer than two ranked: the fill values of spim_rgldm_match, no candidate.
__global__ __launch_bounds__(kGhBlock) void k_gh_merge(int na, int nparts, const double* __restrict__ pd1,
                                                       const double* __restrict__ pd2, const int* __restrict__ pi1,
                                                       const int* __restrict__ pi2, double thr, double ratio,
                                                       double* __restrict__ best_out, double* __restrict__ second_out,
                                                       int* __restrict__ idx_out, unsigned char* __restrict__ flag) {
    const int i = int(blockIdx.x) * kGhBlock + int(threadIdx.x);
    if (i >= na) return;
    GhTop2 top;
    gh_top2_init(top);
    for (int p = 0; p < nparts; ++p) {
        const int64_t o = int64_t(p) * na + i;
        const int i1 = pi1[o], i2 = pi2[o];
        if (i1 >= 0) gh_top2_insert(top, pd1[o], i1);
        if (i2 >= 0) gh_top2_insert(top, pd2[o], i2);
    }
    const bool two = top.i2 >= 0;
    const double best = two ? top.d1 : kJavaDoubleMax, second = two ? top.d2 : kJavaDoubleMax;
    best_out[i] = best;
    second_out[i] = second;
    idx_out[i] = two ? top.i1 : -1;
    flag[i] = (two && best < thr && __dmul_rn(best, ratio) <= second) ? 1 : 0;
}

// Per-device workspace, grown on demand and kept between calls.
struct GhWork : PmCandidateWork {
    DBuf<double> rel, pd1, pd2;
    DBuf<float> desc_a, desc_b;
    DBuf<int> nbr, pi1, pi2;
};

void gh_check_params(const spim_gh_params* p) {
    SD_CHECK(p, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(p->b_split >= 0, SPIMDECON_ERR_ARG, "geometric hashing: b_split must be >= 0");
}

// neighbours (w.nbr, w.rel) and the descriptors of n >= 4 staged points into desc
void gh_describe(const double* dpts, int n, GhWork& w, float* desc, hipStream_t s) {
    grow(w.nbr, size_t(n) * 3);
    grow(w.rel, size_t(n) * 9);
    pm_knn(dpts, n, 3, w.nbr.p, w.rel.p, s);
    hipLaunchKernelGGL(k_gh_descriptors, dim3(unsigned(ceil_div(n, kGhBlock))), dim3(kGhBlock), 0, s, w.rel.p, n,
                       desc);
    SD_HIP(hipGetLastError());
}

void gh_descriptors(const double* pts, int64_t n, const spim_gh_params* p, int32_t* neighbors, float* desc) {
    gh_check_params(p);
    pm_check_points(pts, n, "geometric hashing");
    SD_CHECK(neighbors && desc, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(n >= kGhMinPoints, SPIMDECON_ERR_ARG, "geometric hashing: a descriptor needs 4 points");
    with_work<GhWork>(p->device, [&](GhWork& w, hipStream_t s) {
        const double* d = pm_stage_points(pts, n, p->device, w.pts_a, w.bad, s, "geometric hashing");
        grow(w.desc_a, size_t(n) * 6);
        gh_describe(d, int(n), w, w.desc_a.p, s);
        SD_HIP(hipMemcpyAsync(neighbors, w.nbr.p, size_t(n) * 3 * sizeof(int), hipMemcpyDefault, s));
        SD_HIP(hipMemcpyAsync(desc, w.desc_a.p, size_t(n) * 6 * sizeof(float), hipMemcpyDefault, s));
        SD_HIP(hipStreamSynchronize(s));
    });
}

void gh_match(const double* a, int64_t na, const double* b, int64_t nb, const spim_gh_params* p, int32_t* best_idx,
              double* best, double* second, int32_t* cand_a, int32_t* cand_b, int64_t cap, int64_t* count) {
    gh_check_params(p);
    // fewer than 4 points: GeometricHashingPairwise.java:58-65, "Not enough detections to match": no candidates
    pm_match_candidates<GhWork>(
        "geometric hashing", kGhMinPoints, p->device, a, na, b, nb, best_idx, best, second, cand_a, cand_b, cap,
        count, [&](GhWork& w, const double* da, const double* db, hipStream_t s) {
            grow(w.desc_a, size_t(na) * 6);
            grow(w.desc_b, size_t(nb) * 6);
            gh_describe(da, int(na), w, w.desc_a.p, s);
            gh_describe(db, int(nb), w, w.desc_b.p, s);
            // B split: 16,000 A descriptors are 63 blocks; aim at 2 blocks of 4 waves per CU
            const int64_t ablocks = ceil_div(na, kGhATile);
            const PmSplit sp = pm_split(p->b_split, ablocks, nb, kGhBTile, 2, p->device, "geometric hashing");
            grow(w.pd1, size_t(na) * sp.split);
            grow(w.pd2, size_t(na) * sp.split);
            grow(w.pi1, size_t(na) * sp.split);
            grow(w.pi2, size_t(na) * sp.split);
            hipLaunchKernelGGL(k_gh_match, dim3(unsigned(ablocks), unsigned(sp.split)), dim3(kGhATile), 0, s,
                               w.desc_a.p, int(na), w.desc_b.p, int(nb), sp.chunk, w.pd1.p, w.pd2.p, w.pi1.p, w.pi2.p);
            SD_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_gh_merge, dim3(unsigned(ceil_div(na, kGhBlock))), dim3(kGhBlock), 0, s, int(na),
                               int(sp.split), w.pd1.p, w.pd2.p, w.pi1.p, w.pi2.p, p->difference_threshold,
                               p->ratio_of_distance, w.best.p, w.second.p, w.idx.p, w.flag.p);
            SD_HIP(hipGetLastError());
        });
}

}  // namespace
}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" void spim_gh_params_default(spim_gh_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->ratio_of_distance = 10.0;      // GeometricHashingParameters.ratioOfDistance
    p->difference_threshold = 50.0;   // .differenceThreshold
    p->b_split = 0;
    p->device = 0;
}

extern "C" void spim_gh_tiles(int32_t* a_tile, int32_t* b_tile) {
    if (a_tile) *a_tile = kGhATile;
    if (b_tile) *b_tile = kGhBTile;
}

extern "C" int spim_gh_descriptors(const double* pts, int64_t n, const spim_gh_params* p, int32_t* neighbors,
                                   float* desc) {
    return guarded([&] { gh_descriptors(pts, n, p, neighbors, desc); });
}

extern "C" int spim_gh_match(const double* a, int64_t na, const double* b, int64_t nb, const spim_gh_params* p,
                             int32_t* best_idx, double* best, double* second, int32_t* cand_a, int32_t* cand_b,
                             int64_t cap, int64_t* count) {
    return guarded([&] { gh_match(a, na, b, nb, p, best_idx, best, second, cand_a, cand_b, cap, count); });
}
