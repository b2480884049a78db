// sepconv.hpp -- the separable convolution passes (sepconv.hip): the convolve_N ABI's engine,
// and the DoG's fallback for Gaussians of 63 / 127 taps.
#pragma once

#include "common.hpp"

namespace spimdecon {

// what a pass reads beyond an axis' ends (CUDASeparableConvolution's outofbounds argument)
enum Oob { OOB_ZERO = 0, OOB_VALUE = 1, OOB_BORDER = 2, OOB_MIRROR = 3 };

// the packed pair of both sigmas' operands (v_pk_mul / v_pk_add per component: bit-exact)
typedef float dg_v2 __attribute__((ext_vector_type(2)));

// index i of an axis of n under `mode`; `outside`: the pass takes the mode's value instead
template <typename I>
__device__ __forceinline__ I ext_index(I i, I n, int mode, bool& outside) {
    outside = false;
    if (i >= 0 && i < n) return i;
    if (mode == OOB_BORDER) return i < 0 ? 0 : n - 1;
    if (mode == OOB_MIRROR) {
        if (n == 1) return 0;
        const I p = 2 * (n - 1);
        I j = i % p;
        if (j < 0) j += p;
        return j >= n ? p - j : j;
    }
    outside = true;
    return 0;
}
__device__ __forceinline__ int ext_index32(int i, int n, int mode, bool& o) { return ext_index(i, n, mode, o); }

// One pass along `axis` (0 = x, 1 = y, 2 = z) of one kernel (in1 == k1 == nullptr) or of two
// of equal length K; `mm`: the device {min, max} the input is normalised by on the fly, or
// nullptr.  dog: out0 = (o1 - o0) * dog_scale instead of both results.
void sep_pass(const Dims3& d, int axis, const float* in0, const float* in1, const float* k0, const float* k1, int K,
              int mode, float value, float* out0, float* out1, bool dog, float dog_scale, const float* mm,
              hipStream_t s);

}  // namespace spimdecon
