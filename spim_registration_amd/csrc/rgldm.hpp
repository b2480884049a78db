// rgldm.hpp -- the point-list stages of rgldm.hip that geohash.hip runs too: one copy of the
// kernels, so the neighbour search of both matchers is the same code.
#pragma once

#include "common.hpp"

namespace spimdecon {

// The (n, 3) points on device `dev` -- in place when they already are, else copied into buf --
// after the argument rules (null, n <= 2^31 - 1) and the finite check (as double and as the
// float Detection.get returns): SPIMDECON_ERR_ARG "<who>: non-finite coordinates".  Drains s.
const double* pm_stage_points(const double* pts, int64_t n, int dev, DBuf<double>& buf, DBuf<int>& bad,
                              hipStream_t s, const char* who);

// k_rgldm_knn<m>: per point its m (1..6) nearest others in ascending Detection.distanceTo
// order, equal floats by lower index -- nbr[n * m] --, neighbour minus basis -- rel[n * m * 3].
void pm_knn(const double* dpts, int n, int m, int* nbr, double* rel, hipStream_t s);

// k_rgldm_compact: (i, idx[i]) of every flag[i] != 0 in ascending i, at most cap of them written;
// count[0] = how many there are.
void pm_compact(int na, const unsigned char* flag, const int* idx, int* cand_a, int* cand_b, int64_t cap,
                int64_t* count, hipStream_t s);

}  // namespace spimdecon
