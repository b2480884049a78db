// minmax.hpp -- FusionHelper.minMax (:105-138) of a float image in two stages, for the
// content-based weights and the automatic bounding box: a fixed tree (grid-stride partials,
// then one block), so the result does not depend on scheduling.  R is the caller's rule:
// R::mn / R::mx, its Math.min / Math.max (how they treat NaN and +-0 is the caller's).
#pragma once

#include <algorithm>

#include "common.hpp"

namespace spimdecon {

constexpr int kRedBlock = 256, kRedGrid = 1024;
constexpr float kFloatMax = 3.402823466e+38f;

template <class R>
__device__ __forceinline__ void block_minmax(float& mn, float& mx) {
    __shared__ float smn[kRedBlock / 64], smx[kRedBlock / 64];
    for (int off = 32; off > 0; off >>= 1) {
        mn = R::mn(mn, __shfl_xor(mn, off, 64));
        mx = R::mx(mx, __shfl_xor(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    mn = smn[0];
    mx = smx[0];
    for (int w = 1; w < kRedBlock / 64; ++w) {
        mn = R::mn(mn, smn[w]);
        mx = R::mx(mx, smx[w]);
    }
}

template <class R>
__global__ __launch_bounds__(kRedBlock) void k_minmax_partial(const float* __restrict__ c, int64_t n,
                                                              float* __restrict__ part) {
    float mn = kFloatMax, mx = -kFloatMax;
    for (int64_t i = int64_t(blockIdx.x) * kRedBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kRedBlock) {
        const float v = c[i];
        mn = R::mn(mn, v);
        mx = R::mx(mx, v);
    }
    block_minmax<R>(mn, mx);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = mn;
        part[2 * blockIdx.x + 1] = mx;
    }
}

template <class R>
__global__ __launch_bounds__(kRedBlock) void k_minmax_final(const float* __restrict__ part, int nparts,
                                                            float* __restrict__ mm) {
    float mn = kFloatMax, mx = -kFloatMax;
    for (int i = threadIdx.x; i < nparts; i += kRedBlock) {
        mn = R::mn(mn, part[2 * i]);
        mx = R::mx(mx, part[2 * i + 1]);
    }
    block_minmax<R>(mn, mx);
    if (threadIdx.x == 0) {
        mm[0] = mn;
        mm[1] = mx;
    }
}

// the blocks of the first stage over n values
inline int minmax_parts(int64_t n) {
    return int(std::max<int64_t>(1, std::min<int64_t>(kRedGrid, ceil_div(n, kRedBlock))));
}

// {min, max} of c[0 .. n) into mm[0 .. 2) on s; part: 2 * parts floats
template <class R>
void minmax_launch(const float* c, int64_t n, int parts, float* part, float* mm, hipStream_t s) {
    hipLaunchKernelGGL(k_minmax_partial<R>, dim3(unsigned(parts)), dim3(kRedBlock), 0, s, c, n, part);
    hipLaunchKernelGGL(k_minmax_final<R>, dim3(1), dim3(kRedBlock), 0, s, part, parts, mm);
}

}  // namespace spimdecon
