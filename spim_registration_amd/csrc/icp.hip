// icp.hip -- "Iterative closest-point (ICP, no invariance)" of two bead lists on MI355X: the
// per-iteration correspondence search of the reference's third pairwise matcher.
//
// References (under the reference's src/main/java/):
//   spim/process/interestpointregistration/icp/IterativeClosestPointPairwise.java:40-122   the loop (host here)
//   .../icp/IterativeClosestPointParameters.java                                         5 / 100
//   mpicbg/icp/ICP.java:91-115                     apply, assign, removeAmbigousMatches, fit
//   mpicbg/icp/ICP.java:208-317                    removeAmbigousMatches, getOccurences
//   mpicbg/icp/SimplePointMatchIdentification.java:32-48   nearest target per reference point, <= threshold
//   spim/process/interestpointregistration/Detection.java:96-115   distanceTo, get
//
// List A is the target (moved by the model), list B the reference.  Every double and float
// operation is one explicit round-to-nearest intrinsic in the source order of the Java code
// (which never contracts a multiply and an add), so the nearest index, the float distance and
// the match list are bit-exact against a restatement.  Unpinned: the reference searches with
// fiji.util.KDTree (not in its tree); among equal float distances the lower target index wins
// here, as in k_pm_knn.
//   k_icp_apply     one thread per target point: w = M l in double, three floats padded to 16 bytes
//   k_icp_assign    a lane owns one reference point; the target floats go through LDS in tiles
//                   and are read as broadcasts; grid.y splits the target (partial nearest)
//   k_icp_merge     partials in ascending target order -> nearest, distance, the threshold;
//                   per-target claim counts over the thresholded matches (integer atomics)
//   k_icp_resolve   a match survives when its target is claimed once; counts the others
//   k_pm_compact    (pointmatch.hip) the survivors in ascending reference order
// No kernel waits on another block; every loop is bounded by a count the host passes.
#include <algorithm>
#include <cfloat>

#include "pointmatch.hpp"

namespace spimdecon {
namespace {

constexpr int kIcpRBlock = 256;    // reference points (lanes) per block of k_icp_assign
constexpr int kIcpTTile = 1024;    // target points per LDS tile (16 KiB of float4)
constexpr int kIcpBlock = 256;

struct IcpModel {
    double m[12];
};

// Point.apply through AffineModel3D / RigidModel3D / TranslationModel3D.applyInPlace: per row
// ((m0 x + m1 y) + m2 z) + m3, every product and sum rounded on its own.  bad[0] = 1 when a
// coordinate is not finite as the float Detection.get returns.
__global__ __launch_bounds__(kIcpBlock) void k_icp_apply(const double* __restrict__ target, int nt, IcpModel mdl,
                                                         float4* __restrict__ tw, int64_t* __restrict__ bad) {
    const int i = int(blockIdx.x) * kIcpBlock + int(threadIdx.x);
    if (i >= nt) return;
    const double x = target[3 * int64_t(i)], y = target[3 * int64_t(i) + 1], z = target[3 * int64_t(i) + 2];
    float f[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double* m = mdl.m + 4 * r;
        const double w =
            __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z)), m[3]);
        f[r] = float(w);
    }
    if (!(f[0] - f[0] == 0.0f) || !(f[1] - f[1] == 0.0f) || !(f[2] - f[2] == 0.0f))
        bad[0] = 1;   // (every writer stores the same value)
    tw[i] = make_float4(f[0], f[1], f[2], 0.0f);
}

// Detection.distanceTo's argument: per-axis float differences o.get(k) - get(k) (o the reference
// point), widened, squared and summed in double
__device__ __forceinline__ double icp_s(float rx, float ry, float rz, const float4& t) {
    const double x = double(__fsub_rn(rx, t.x)), y = double(__fsub_rn(ry, t.y)), z = double(__fsub_rn(rz, t.z));
    return __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z));
}

// One block: kIcpRBlock reference points against the targets of partition blockIdx.y, in
// ascending target index.  The running nearest is replaced only on a strictly smaller float
// distance.  s >= the sum behind the kept distance: the rounded root is no smaller either
// (sqrt and the float rounding are monotone), so the root is taken only for a smaller sum --
// which still may round to the same float, and then the lower index stays.  Partials are
// [partition][nr]; an empty partition leaves index -1.
__global__ __launch_bounds__(kIcpRBlock) void k_icp_assign(const float4* __restrict__ tw, int nt,
                                                           const double* __restrict__ ref, int nr, int chunk,
                                                           float* __restrict__ pd, int* __restrict__ pi) {
    __shared__ float4 tile[kIcpTTile];
    const int i = int(blockIdx.x) * kIcpRBlock + int(threadIdx.x);
    const int ic = min(i, nr - 1);
    const float rx = float(ref[3 * int64_t(ic)]), ry = float(ref[3 * int64_t(ic) + 1]),
                rz = float(ref[3 * int64_t(ic) + 2]);
    const int t0 = int(min(int64_t(blockIdx.y) * chunk, int64_t(nt)));
    const int t1 = int(min(int64_t(t0) + chunk, int64_t(nt)));
    double best_s = __builtin_inf();
    float best_d = FLT_MAX;
    int best_i = -1;
    for (int j0 = t0; j0 < t1; j0 += kIcpTTile) {
        const int cnt = min(kIcpTTile, t1 - j0);
        __syncthreads();
        for (int e = int(threadIdx.x); e < cnt; e += kIcpRBlock) tile[e] = tw[int64_t(j0) + e];
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < cnt; ++t) {   // tile[t]: the same address in every lane, a broadcast
            const double s = icp_s(rx, ry, rz, tile[t]);
            if (best_i >= 0 && !(s < best_s)) continue;
            const float d = float(__dsqrt_rn(s));
            if (best_i >= 0 && !(d < best_d)) continue;
            best_s = s;
            best_d = d;
            best_i = j0 + t;
        }
    }
    if (i < nr) {
        const int64_t o = int64_t(blockIdx.y) * nr + i;
        pd[o] = best_d;
        pi[o] = best_i;
    }
}

// The partitions in ascending target order, again replaced only on a strictly smaller float;
// SimplePointMatchIdentification.java:43: a match when (double) dist <= distanceThreshold.
// claims[t] = the thresholded matches that name target t.
__global__ __launch_bounds__(kIcpBlock) void k_icp_merge(int nr, int nparts, const float* __restrict__ pd,
                                                         const int* __restrict__ pi, double thr,
                                                         int* __restrict__ nearest, float* __restrict__ dist,
                                                         unsigned char* __restrict__ matched,
                                                         int* __restrict__ claims) {
    const int i = int(blockIdx.x) * kIcpBlock + int(threadIdx.x);
    if (i >= nr) return;
    float best_d = FLT_MAX;
    int best_i = -1;
    for (int p = 0; p < nparts; ++p) {
        const int64_t o = int64_t(p) * nr + i;
        const int j = pi[o];
        if (j < 0) continue;
        const float d = pd[o];
        if (best_i >= 0 && !(d < best_d)) continue;
        best_d = d;
        best_i = j;
    }
    nearest[i] = best_i;
    dist[i] = best_d;
    const bool m = best_i >= 0 && double(best_d) <= thr;
    matched[i] = m ? 1 : 0;
    if (m) atomicAdd(&claims[best_i], 1);
}

// ICP.removeAmbigousMatches (:208-249) with every reference point in at most one match: a match
// goes when another match names its target.  stats[1] += the matches removed.
__global__ __launch_bounds__(kIcpBlock) void k_icp_resolve(int nr, const int* __restrict__ nearest,
                                                           const unsigned char* __restrict__ matched,
                                                           const int* __restrict__ claims,
                                                           unsigned char* __restrict__ keep,
                                                           int64_t* __restrict__ stats) {
    const int i = int(blockIdx.x) * kIcpBlock + int(threadIdx.x);
    bool amb = false;
    if (i < nr) {
        const bool m = matched[i] != 0;
        const int c = m ? claims[nearest[i]] : 0;
        keep[i] = (m && c == 1) ? 1 : 0;
        amb = m && c > 1;
    }
    const int n = __syncthreads_count(amb ? 1 : 0);
    if (threadIdx.x == 0 && n) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 1), (unsigned long long)n);
}

__global__ __launch_bounds__(kIcpBlock) void k_icp_fill(int nr, int* __restrict__ nearest, float* __restrict__ dist) {
    const int i = int(blockIdx.x) * kIcpBlock + int(threadIdx.x);
    if (i >= nr) return;
    nearest[i] = -1;
    dist[i] = FLT_MAX;
}

// Per-device workspace, grown on demand and kept between calls:
// the iterations of one pair, and the pairs of one timepoint, allocate once.
struct IcpWork : PmWork {
    DBuf<double> pts_t, pts_r;
    DBuf<float4> tw;
    DBuf<float> pd, dist;
    DBuf<int> pi, nearest, claims, match_t, match_r;
    DBuf<unsigned char> matched, keep;
    DBuf<int64_t> stats;   // the matches, the ambiguous ones, the non-finite flag of k_icp_apply
};

void icp_assign(const double* target, int64_t nt, const double* reference, int64_t nr, const double* model,
                const spim_icp_params* p, int32_t* nearest, float* dist, int32_t* match_t, int32_t* match_r,
                int64_t cap, int64_t* count, int64_t* ambiguous) {
    SD_CHECK(p, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(p->t_split >= 0, SPIMDECON_ERR_ARG, "icp: t_split must be >= 0");
    pm_check_points(target, nt, "icp");
    pm_check_points(reference, nr, "icp");
    SD_CHECK(count && ambiguous && cap >= 0 && (cap == 0 || (match_t && match_r)), SPIMDECON_ERR_ARG,
             "null argument");
    SD_CHECK(nr == 0 || (nearest && dist), SPIMDECON_ERR_ARG, "null argument");
    *count = 0;
    *ambiguous = 0;
    with_work<IcpWork>(p->device, [&](IcpWork& w, hipStream_t s) {
        IcpModel mdl = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
        if (model && is_device_ptr(model, p->device)) {
            SD_HIP(hipMemcpyAsync(mdl.m, model, sizeof(mdl.m), hipMemcpyDeviceToHost, s));
            SD_HIP(hipStreamSynchronize(s));
        } else if (model) {
            std::memcpy(mdl.m, model, sizeof(mdl.m));
        }
        const double* dt = nt ? pm_stage_points(target, nt, p->device, w.pts_t, w.bad, s, "icp") : nullptr;
        const double* dr = nr ? pm_stage_points(reference, nr, p->device, w.pts_r, w.bad, s, "icp") : nullptr;
        if (nr == 0) return;
        grow(w.nearest, size_t(nr));
        grow(w.dist, size_t(nr));
        grow(w.stats, 3);
        SD_HIP(hipMemsetAsync(w.stats.p, 0, 3 * sizeof(int64_t), s));
        const unsigned gr = unsigned(ceil_div(nr, kIcpBlock));
        if (nt == 0) {
            hipLaunchKernelGGL(k_icp_fill, dim3(gr), dim3(kIcpBlock), 0, s, int(nr), w.nearest.p, w.dist.p);
            SD_HIP(hipGetLastError());
        } else {
            grow(w.tw, size_t(nt));
            hipLaunchKernelGGL(k_icp_apply, dim3(unsigned(ceil_div(nt, kIcpBlock))), dim3(kIcpBlock), 0, s, dt, int(nt),
                               mdl, w.tw.p, w.stats.p + 2);
            SD_HIP(hipGetLastError());
            // target split: 16,000 reference points are 63 blocks; aim at 2 blocks of 4 waves per CU
            const int64_t rblocks = ceil_div(nr, kIcpRBlock);
            const PmSplit sp = pm_split(p->t_split, rblocks, nt, kIcpTTile, 2, p->device, "icp");
            grow(w.pd, size_t(nr) * sp.split);
            grow(w.pi, size_t(nr) * sp.split);
            hipLaunchKernelGGL(k_icp_assign, dim3(unsigned(rblocks), unsigned(sp.split)), dim3(kIcpRBlock), 0, s,
                               w.tw.p, int(nt), dr, int(nr), sp.chunk, w.pd.p, w.pi.p);
            SD_HIP(hipGetLastError());
            grow(w.matched, size_t(nr));
            grow(w.keep, size_t(nr));
            grow(w.claims, size_t(nt));
            SD_HIP(hipMemsetAsync(w.claims.p, 0, size_t(nt) * sizeof(int), s));
            hipLaunchKernelGGL(k_icp_merge, dim3(gr), dim3(kIcpBlock), 0, s, int(nr), int(sp.split), w.pd.p, w.pi.p,
                               double(p->max_distance), w.nearest.p, w.dist.p, w.matched.p, w.claims.p);
            SD_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_icp_resolve, dim3(gr), dim3(kIcpBlock), 0, s, int(nr), w.nearest.p, w.matched.p,
                               w.claims.p, w.keep.p, w.stats.p);
            SD_HIP(hipGetLastError());
            const int64_t dcap = std::min<int64_t>(cap, nr);
            grow(w.match_t, size_t(std::max<int64_t>(dcap, 1)));
            grow(w.match_r, size_t(std::max<int64_t>(dcap, 1)));
            pm_compact(int(nr), w.keep.p, w.nearest.p, w.match_r.p, w.match_t.p, dcap, w.stats.p, s);
        }
        int64_t stats[3] = {0, 0, 0};
        SD_HIP(hipMemcpyAsync(stats, w.stats.p, sizeof(stats), hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        SD_CHECK(!stats[2], SPIMDECON_ERR_ARG, "icp: non-finite coordinates under the model");
        SD_HIP(hipMemcpyAsync(nearest, w.nearest.p, size_t(nr) * sizeof(int), hipMemcpyDefault, s));
        SD_HIP(hipMemcpyAsync(dist, w.dist.p, size_t(nr) * sizeof(float), hipMemcpyDefault, s));
        *count = stats[0];
        *ambiguous = stats[1];
        if (*count <= cap && *count) {
            SD_HIP(hipMemcpyAsync(match_t, w.match_t.p, size_t(*count) * sizeof(int), hipMemcpyDefault, s));
            SD_HIP(hipMemcpyAsync(match_r, w.match_r.p, size_t(*count) * sizeof(int), hipMemcpyDefault, s));
        }
        SD_HIP(hipStreamSynchronize(s));
        SD_CHECK(*count <= cap, SPIMDECON_ERR_ARG,
                 "icp: " + std::to_string(*count) + " matches beyond the capacity " + std::to_string(cap));
    });
}

}  // namespace
}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" void spim_icp_params_default(spim_icp_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_distance = 5.0f;     // IterativeClosestPointParameters.maxDistance
    p->max_iterations = 100;    // .maxIterations
    p->t_split = 0;
    p->device = 0;
}

extern "C" void spim_icp_tiles(int32_t* ref_block, int32_t* target_tile) {
    if (ref_block) *ref_block = kIcpRBlock;
    if (target_tile) *target_tile = kIcpTTile;
}

extern "C" int spim_icp_assign(const double* target, int64_t nt, const double* reference, int64_t nr,
                               const double* model, const spim_icp_params* p, int32_t* nearest, float* dist,
                               int32_t* match_t, int32_t* match_r, int64_t cap, int64_t* count,
                               int64_t* ambiguous) {
    return guarded([&] {
        icp_assign(target, nt, reference, nr, model, p, nearest, dist, match_t, match_r, cap, count, ambiguous);
    });
}
