// pointmatch.hpp -- the host scaffold and the point-list stages that the matchers of two bead
// lists share (rgldm.hip, geohash.hip, icp.hip): one copy of the argument rules, the staging,
// the partition rule, the neighbour search and the compaction.  A matcher keeps its own
// workspace (per_device<ItsWork>: its own mutex, stream and buffers), its parameter checks and
// the kernels that are its own.
#pragma once

#include <algorithm>
#include <cfloat>

#include "hostcall.hpp"

namespace spimdecon {

constexpr double kJavaDoubleMax = DBL_MAX;   // Double.MAX_VALUE

// What every matcher's per-device workspace starts with.  Grown on demand and kept between
// calls; one call at a time per matcher and device holds mu.
struct PmWork : WorkBase {
    DBuf<int> bad;   // pm_stage_points' flag
};

// the buffers of pm_match_candidates
struct PmCandidateWork : PmWork {
    DBuf<double> pts_a, pts_b, best, second;
    DBuf<int> idx, cand_a, cand_b;
    DBuf<unsigned char> flag;
    DBuf<int64_t> count;
};

// the argument rules of a point list: not null unless empty, no more points than an int holds
// (SPIMDECON_ERR_ARG, the second message led by <who>)
void pm_check_points(const double* pts, int64_t n, const char* who);

// The (n, 3) points on device `dev` -- in place when they already are, else copied into buf --
// after the finite check (as double and as the float Detection.get returns):
// SPIMDECON_ERR_ARG "<who>: non-finite coordinates".  Drains s.
const double* pm_stage_points(const double* pts, int64_t n, int dev, DBuf<double>& buf, DBuf<int>& bad,
                              hipStream_t s, const char* who);

// The partitions of the n_cols columns (col_tile of them per LDS tile) that grid.y runs over
// beside row_blocks blocks of rows: `requested`, or with requested <= 0 enough to put
// blocks_per_cu blocks on every CU of dev, no more than there are tiles; at most 65535.
// chunk = the columns of one partition.  SPIMDECON_ERR_ARG, led by <who>, when the grid would
// hold 2^31 blocks or more.
struct PmSplit {
    int64_t split;
    int chunk;
};
PmSplit pm_split(int64_t requested, int64_t row_blocks, int64_t n_cols, int col_tile, int blocks_per_cu, int dev,
                 const char* who);

// k_pm_knn<m>: per point its m (1..6) nearest others in ascending Detection.distanceTo
// order, equal floats by lower index -- nbr[n * m] --, neighbour minus basis -- rel[n * m * 3].
void pm_knn(const double* dpts, int n, int m, int* nbr, double* rel, hipStream_t s);

// k_pm_compact: (i, idx[i]) of every flag[i] != 0 in ascending i, at most cap of them written;
// count[0] = how many there are.
void pm_compact(int na, const unsigned char* flag, const int* idx, int* cand_a, int* cand_b, int64_t cap,
                int64_t* count, hipStream_t s);

// k_pm_fill: best = second = Double.MAX_VALUE, idx = -1 over na points ("Not enough detections")
void pm_fill(int na, double* best, double* second, int* idx, hipStream_t s);

// A candidate matcher's call (spim_rgldm_match, spim_gh_match) around what is its own:
// `run(w, da, db, s)` describes the staged lists da (na points) and db (nb), matches them and
// merges into w.best / w.second / w.idx / w.flag (na each, grown here) on s.  It is called when
// both lists hold min_points; with fewer there are the fill values and no candidate.  W is the
// matcher's workspace, a PmCandidateWork; the matcher's own parameter checks come before this.
template <class W, class Run>
void pm_match_candidates(const char* who, int min_points, int dev, const double* a, int64_t na, const double* b,
                         int64_t nb, int32_t* best_idx, double* best, double* second, int32_t* cand_a,
                         int32_t* cand_b, int64_t cap, int64_t* count, Run&& run) {
    pm_check_points(a, na, who);
    pm_check_points(b, nb, who);
    SD_CHECK(count && cap >= 0 && (cap == 0 || (cand_a && cand_b)), SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(na == 0 || (best_idx && best && second), SPIMDECON_ERR_ARG, "null argument");
    *count = 0;
    with_work<W>(dev, [&](W& w, hipStream_t s) {
        const double* da = na ? pm_stage_points(a, na, dev, w.pts_a, w.bad, s, who) : nullptr;
        const double* db = nb ? pm_stage_points(b, nb, dev, w.pts_b, w.bad, s, who) : nullptr;
        if (na == 0) return;
        grow(w.best, size_t(na));
        grow(w.second, size_t(na));
        grow(w.idx, size_t(na));
        if (na < min_points || nb < min_points) {
            pm_fill(int(na), w.best.p, w.second.p, w.idx.p, s);
        } else {
            grow(w.flag, size_t(na));
            run(w, da, db, s);
            grow(w.count, 1);
            const int64_t dcap = std::min<int64_t>(cap, na);
            grow(w.cand_a, size_t(std::max<int64_t>(dcap, 1)));
            grow(w.cand_b, size_t(std::max<int64_t>(dcap, 1)));
            pm_compact(int(na), w.flag.p, w.idx.p, w.cand_a.p, w.cand_b.p, dcap, w.count.p, s);
            SD_HIP(hipMemcpyAsync(count, w.count.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        }
        SD_HIP(hipMemcpyAsync(best_idx, w.idx.p, size_t(na) * sizeof(int), hipMemcpyDefault, s));
        SD_HIP(hipMemcpyAsync(best, w.best.p, size_t(na) * sizeof(double), hipMemcpyDefault, s));
        SD_HIP(hipMemcpyAsync(second, w.second.p, size_t(na) * sizeof(double), hipMemcpyDefault, s));
        SD_HIP(hipStreamSynchronize(s));
        SD_CHECK(*count <= cap, SPIMDECON_ERR_ARG,
                 std::string(who) + ": " + std::to_string(*count) + " candidates beyond the capacity " +
                     std::to_string(cap));
        if (*count) {
            SD_HIP(hipMemcpyAsync(cand_a, w.cand_a.p, size_t(*count) * sizeof(int), hipMemcpyDefault, s));
            SD_HIP(hipMemcpyAsync(cand_b, w.cand_b.p, size_t(*count) * sizeof(int), hipMemcpyDefault, s));
            SD_HIP(hipStreamSynchronize(s));
        }
    });
}

}  // namespace spimdecon
