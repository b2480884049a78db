// content_weights.hip -- content-based fusion weights on the GPU.
//
// Restates spim/process/fusion/weights/ContentBased.java:60-98 (approximateEntropy):
//   c = G(sigma1) (*) I;  c = (c - I)^2;  c = G(sigma2) (*) c;  normalizeImage(c)
// per source view, in the view's own voxel grid, float32.  The reference convolves
// through FFTConvolution over extendMirrorSingle with the 3-D kernel
// float(kx[x] * ky[y] * kz[z]) of Util.createGaussianKernel1DDouble factors; here the
// Gaussian is applied as three 1-D passes whose taps are the float casts of the same
// double factors, accumulated in float32.  The separable float product differs from
// the reference's float(kx * ky * kz) tap by rounding only (each 1-D tap carries one
// 2^-24 relative rounding instead of one for the product), which stays inside the
// bound the tests derive from the reference's own float FFT error.
//
// k_gauss_pass: one block = 64 lines x up to 128 outputs along the pass axis.  The
// block stages the lines with their mirror-extended halo in LDS once (every input
// voxel is fetched about once per pass; the halo re-reads of neighbouring tiles are
// L2 hits), then each thread slides a register window along its line: 16 outputs per
// thread, one LDS read per 16 FMAs, taps through scalar loads.  The pass is VALU-bound
// (723 FMA per voxel at sigma 40 against 24 B of traffic).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "fusion.hpp"
#include "hostcall.hpp"
#include "minmax.hpp"
#include "resample.hpp"

namespace spimdecon {
namespace {

constexpr int kCwBlock = 512;                   // 8 waves: one group of outputs each
constexpr int kCwLines = 64;                    // lines per block = lanes of a wave
constexpr int kCwOut = 16;                      // outputs per thread along the axis
constexpr int kCwTile = kCwOut * (kCwBlock / 64);  // 128 outputs per line and block
constexpr int kCwChunk = 16;                    // taps per register-window step
constexpr int kCwMaxTaps = 463;                 // LDS: 64 x ((128 + 464) | 1) floats <= 160 KiB

inline int padded_taps(int k) { return (k + kCwChunk - 1) / kCwChunk * kCwChunk; }
inline int lds_width(int k) { return kCwTile + padded_taps(k); }

// extendMirrorSingle index; interior positions skip the division
__device__ __forceinline__ int mirror_fast(int i, int n) {
    return unsigned(i) < unsigned(n) ? i : mirror1(i, n);
}

// One 16-tap step of the sliding window: w is a 32-entry ring (OFF = where the 16
// values already held start), lp the LDS position of the window's first value.
template <int OFF>
__device__ __forceinline__ void window_step(float (&w)[32], float (&acc)[kCwOut], const float* lp, int ps,
                                            const float* __restrict__ taps) {
#pragma unroll
    for (int j = 0; j < 16; ++j) w[(OFF + 16 + j) & 31] = lp[(16 + j) * ps];
#pragma unroll
    for (int kk = 0; kk < kCwChunk; ++kk) {
        const float t = taps[kk];
#pragma unroll
        for (int j = 0; j < kCwOut; ++j) acc[j] = fmaf(w[(OFF + j + kk) & 31], t, acc[j]);
    }
}

// 1-D convolution with K (odd) taps along one axis of an x-fastest volume over
// extendMirrorSingle.  XAXIS: lines are the ny*nz rows, positions run along x.
// Otherwise lines are 64 consecutive x at one index `o` of the third axis and the
// positions run along y (pstride nx, ostride nx*ny) or z (pstride nx*ny, ostride nx).
// sub != nullptr: the value convolved is (in - sub)^2, formed on load
// (ContentBased.java:86-87: float difference, then float square).
// taps: padded_taps(K) floats, zero beyond K.  LDS: XAXIS [line][pos] with an odd
// pitch, else [pos][line]; both make the window reads (lanes = lines) and the staging
// writes conflict-free.
template <bool XAXIS>
__global__ __launch_bounds__(kCwBlock) void k_gauss_pass(const float* __restrict__ in,
                                                         const float* __restrict__ sub,
                                                         float* __restrict__ out,
                                                         const float* __restrict__ taps, int K, int n,
                                                         int64_t pstride, int64_t ostride, int64_t nlines,
                                                         int nat, int nlt) {
    extern __shared__ __attribute__((aligned(16))) float cw_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const int kpad = (K + kCwChunk - 1) / kCwChunk * kCwChunk;
    const int lw = kCwTile + kpad;           // LDS positions per line
    const int lp = XAXIS ? (lw | 1) : kCwLines;   // pitch between lines (XAXIS) / positions
    const int R = K / 2;
    const int64_t b = blockIdx.x;
    const int at = int(b % nat);
    const int64_t rest = b / nat;
    const int p0 = at * kCwTile;
    const int tile = min(kCwTile, n - p0);
    const int wfill = tile + K - 1;          // positions holding data; zero beyond
    int64_t l0, base;
    if (XAXIS) {
        l0 = rest * kCwLines;
        base = 0;
    } else {
        l0 = (rest % nlt) * kCwLines;
        base = (rest / nlt) * ostride;
    }

    if (XAXIS) {
        for (int l = wave; l < kCwLines; l += kCwBlock / 64) {
            const bool lv = l0 + l < nlines;
            const int64_t row = base + (l0 + l) * int64_t(n);
            for (int p = lane; p < lw; p += 64) {
                float v = 0.0f;
                if (lv && p < wfill) {
                    const int64_t a = row + mirror_fast(p0 - R + p, n);
                    v = in[a];
                    if (sub) {
                        const float d = v - sub[a];
                        v = d * d;
                    }
                }
                cw_lds[l * lp + p] = v;
            }
        }
    } else {
        const bool lv = l0 + lane < nlines;
        const int64_t col = base + l0 + lane;
#pragma unroll 4
        for (int p = wave; p < lw; p += kCwBlock / 64) {
            float v = 0.0f;
            if (lv && p < wfill) {
                const int64_t a = col + int64_t(mirror_fast(p0 - R + p, n)) * pstride;
                v = in[a];
                if (sub) {
                    const float d = v - sub[a];
                    v = d * d;
                }
            }
            cw_lds[p * kCwLines + lane] = v;
        }
    }
    __syncthreads();

    const int q0 = wave * kCwOut;
    const int ps = XAXIS ? 1 : kCwLines;
    float acc[kCwOut];
#pragma unroll
    for (int j = 0; j < kCwOut; ++j) acc[j] = 0.0f;
    if (q0 < tile) {   // wave-uniform: groups beyond a short tile have nothing to store
        const float* lpos = XAXIS ? cw_lds + lane * lp + q0 : cw_lds + q0 * kCwLines + lane;
        float w[32];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = lpos[j * ps];
        int kc = 0;
        for (; kc + 2 * kCwChunk <= kpad; kc += 2 * kCwChunk) {
            window_step<0>(w, acc, lpos + kc * ps, ps, taps + kc);
            window_step<16>(w, acc, lpos + (kc + kCwChunk) * ps, ps, taps + kc + kCwChunk);
        }
        if (kc < kpad) window_step<0>(w, acc, lpos + kc * ps, ps, taps + kc);
    }

    if (XAXIS) {
        // through LDS again so that the rows are written in whole segments
        constexpr int op = kCwTile + 1;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kCwOut; ++j) cw_lds[lane * op + q0 + j] = acc[j];
        __syncthreads();
        for (int l = wave; l < kCwLines; l += kCwBlock / 64) {
            if (l0 + l >= nlines) break;
            const int64_t row = base + (l0 + l) * int64_t(n) + p0;
            for (int p = lane; p < tile; p += 64) out[row + p] = cw_lds[l * op + p];
        }
    } else if (q0 < tile && l0 + lane < nlines) {
        const int64_t col = base + l0 + lane;
#pragma unroll
        for (int j = 0; j < kCwOut; ++j)
            if (q0 + j < tile) out[col + int64_t(p0 + q0 + j) * pstride] = acc[j];
    }
}

// Java Math.min / Math.max on floats: NaN propagates
__device__ __forceinline__ float jmin(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ __forceinline__ float jmax(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

struct ContentMinMax {   // the rule of minmax.hpp's reduction
    static __device__ __forceinline__ float mn(float a, float b) { return jmin(a, b); }
    static __device__ __forceinline__ float mx(float a, float b) { return jmax(a, b); }
};

// FusionHelper.normalizeImage (:176-211): (c - min) / diff in float, skipped when the
// range is NaN, infinite or 0
__global__ __launch_bounds__(kRedBlock) void k_normalise(float* __restrict__ c, int64_t n,
                                                         const float* __restrict__ mm) {
    const float mn = mm[0];
    const float diff = mm[1] - mn;
    if (isnan(diff) || isinf(diff) || diff == 0.0f) return;
    const int64_t i = int64_t(blockIdx.x) * kRedBlock + threadIdx.x;
    if (i < n) c[i] = (c[i] - mn) / diff;
}

// gaussian_kernel(sigma), cast to float and zero-padded for the kernel
std::vector<float> gaussian_taps(double sigma, int* K) {
    const std::vector<double> g = gaussian_kernel(sigma);
    *K = int(g.size());
    std::vector<float> t(size_t(padded_taps(*K)), 0.0f);
    for (size_t i = 0; i < g.size(); ++i) t[i] = float(g[i]);
    return t;
}

void launch_pass(int axis, const float* in, const float* sub, float* out, const float* taps, int K,
                 const int64_t dims[3], hipStream_t s) {
    const int64_t nx = dims[0], ny = dims[1], nz = dims[2];
    const int n = int(dims[axis]);
    const int nat = int(ceil_div(n, kCwTile));
    const int lw = lds_width(K);
    if (axis == 0) {
        const int64_t nlines = ny * nz;
        const int64_t blocks = nat * ceil_div(nlines, kCwLines);
        SD_CHECK(blocks < (int64_t(1) << 31), SPIMDECON_ERR_ARG, "view too large");
        const size_t lds = size_t(kCwLines) * size_t(lw | 1) * 4;
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gauss_pass<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
        hipLaunchKernelGGL(k_gauss_pass<true>, dim3(unsigned(blocks)), dim3(kCwBlock), lds, s, in, sub, out, taps,
                           K, n, int64_t(1), int64_t(0), nlines, nat, 1);
    } else {
        const int64_t pstride = axis == 1 ? nx : nx * ny;
        const int64_t ostride = axis == 1 ? nx * ny : nx;
        const int64_t no = axis == 1 ? nz : ny;
        const int nlt = int(ceil_div(nx, kCwLines));
        const int64_t blocks = int64_t(nat) * nlt * no;
        SD_CHECK(blocks < (int64_t(1) << 31), SPIMDECON_ERR_ARG, "view too large");
        const size_t lds = size_t(kCwLines) * size_t(lw) * 4;
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gauss_pass<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
        hipLaunchKernelGGL(k_gauss_pass<false>, dim3(unsigned(blocks)), dim3(kCwBlock), lds, s, in, sub, out, taps,
                           K, n, pstride, ostride, nx, nat, nlt);
    }
    SD_HIP(hipGetLastError());
}

}  // namespace

void check_content_sigmas(const double* sigma1, const double* sigma2) {
    SD_CHECK(sigma1 && sigma2, SPIMDECON_ERR_ARG, "content-based weights: null sigma");
    for (int d = 0; d < 3; ++d) {
        for (const double sg : {sigma1[d], sigma2[d]}) {
            SD_CHECK(std::isfinite(sg) && sg > 0.0, SPIMDECON_ERR_ARG,
                     "content-based weights: sigma must be finite and > 0");
            SD_CHECK(sg < 1e6 && 2 * int64_t(3 * sg + 0.5) + 1 <= kCwMaxTaps, SPIMDECON_ERR_ARG,
                     "content-based weights: sigma too large (kernel longer than " +
                         std::to_string(kCwMaxTaps) + " taps)");
        }
    }
}

// (fusion.hpp)  Enqueued on s; the taps and the reduction scratch are released after a
// synchronise.
void content_weights_device(const float* img, const int64_t dims[3], const double* sigma1, const double* sigma2,
                            float* out, float* tmp, hipStream_t s) {
    check_content_sigmas(sigma1, sigma2);
    const int64_t n = dims[0] * dims[1] * dims[2];
    int K[6];
    std::vector<float> host;
    size_t off[6];
    for (int i = 0; i < 6; ++i) {
        const std::vector<float> t = gaussian_taps(i < 3 ? sigma1[i] : sigma2[i - 3], &K[i]);
        off[i] = host.size();
        host.insert(host.end(), t.begin(), t.end());
    }
    DBuf<float> taps(host.size());
    SD_HIP(hipMemcpyAsync(taps.p, host.data(), host.size() * 4, hipMemcpyHostToDevice, s));
    // c = G(sigma1) (*) I
    launch_pass(0, img, nullptr, tmp, taps.p + off[0], K[0], dims, s);
    launch_pass(1, tmp, nullptr, out, taps.p + off[1], K[1], dims, s);
    launch_pass(2, out, nullptr, tmp, taps.p + off[2], K[2], dims, s);
    // c = G(sigma2) (*) (c - I)^2, the square formed on the first pass's load
    launch_pass(0, tmp, img, out, taps.p + off[3], K[3], dims, s);
    launch_pass(1, out, nullptr, tmp, taps.p + off[4], K[4], dims, s);
    launch_pass(2, tmp, nullptr, out, taps.p + off[5], K[5], dims, s);
    const int parts = minmax_parts(n);
    DBuf<float> red(size_t(2 * parts + 2));
    float* mm = red.p + 2 * parts;
    SD_CHECK(ceil_div(n, kRedBlock) < (int64_t(1) << 31), SPIMDECON_ERR_ARG, "view too large");
    minmax_launch<ContentMinMax>(out, n, parts, red.p, mm, s);
    hipLaunchKernelGGL(k_normalise, dim3(unsigned(ceil_div(n, kRedBlock))), dim3(kRedBlock), 0, s, out, n, mm);
    SD_HIP(hipGetLastError());
    SD_HIP(hipStreamSynchronize(s));
}

void content_based_weights(const float* img, const int64_t* dims, const double* sigma1, const double* sigma2,
                           float* out, int device) {
    SD_CHECK(img && dims && out, SPIMDECON_ERR_ARG, "content-based weights: null argument");
    check_content_sigmas(sigma1, sigma2);
    const int64_t n = check_volume(dims, "content-based weights: bad dims", "content-based weights: bad dims");
    check_device(device);
    DeviceGuard guard(device);
    ScopedStream st;
    DBuf<float> dimg, dout, tmp{size_t(n)};
    const float* in = stage_in(img, n, device, dimg, st.s);
    ImageDest dst(out, n, device);
    content_weights_device(in, dims, sigma1, sigma2, dst.store(dout), tmp.p, st.s);
    dst.copy_out(st.s);
    if (!dst.out_dev) SD_HIP(hipStreamSynchronize(st.s));
}

}  // namespace spimdecon

using namespace spimdecon;

extern "C" void spim_content_tiles(int32_t sizes[6]) {
    if (!sizes) return;
    const int32_t v[6] = {kCwTile, kCwLines, kCwChunk, kCwMaxTaps, kRedBlock, kRedGrid};
    std::copy(v, v + 6, sizes);
}

extern "C" int spim_content_based_weights(const float* img, const int64_t dims[3], const double sigma1[3],
                                          const double sigma2[3], float* out, int device) {
    return guarded([&] { content_based_weights(img, dims, sigma1, sigma2, out, device); });
}
