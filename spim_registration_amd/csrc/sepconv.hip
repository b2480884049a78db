// sepconv.hip -- separable convolution on MI355X: the SeparableConvolutionCUDALib ABI
// (convolve_7 .. convolve_127; the reference's spim/process/cuda/CUDASeparableConvolution.java:13-21,
// CUDASeparableConvolutionFunctions.java:127-245) and the passes the DoG falls back to for
// Gaussians of 63 / 127 taps.  Accumulation order = tap order in float32 (the oracle's bits).
#include <algorithm>

#include "hostcall.hpp"
#include "sepconv.hpp"

namespace spimdecon {
namespace {

constexpr int kBlock = 256;

// FusionHelper.normalizeImage: (t - min) / (max - min) in float; skipped when
// the range is NaN / inf / 0 (the reference then keeps the raw image).
__device__ __forceinline__ float normalize(float v, const float* mm) {
    if (!mm) return v;
    const float mn = mm[0];
    const float diff = __fsub_rn(mm[1], mn);
    if (isnan(diff) || isinf(diff) || diff == 0.0f) return v;
    return __fdiv_rn(__fsub_rn(v, mn), diff);
}

// One separable pass along `axis` (0 = x, 1 = y, 2 = z) for NK (1 or 2) kernels
// of equal length K; MODE_OUT: 0 = write each result, 1 = write (o1 - o0) * scale.
template <int NK>
__global__ __launch_bounds__(kBlock) void k_sep_pass(Dims3 d, int axis, const float* __restrict__ in0,
                                                      const float* __restrict__ in1,
                                                      const float* __restrict__ k0,
                                                      const float* __restrict__ k1, int K, int mode,
                                                      float value, float* __restrict__ out0,
                                                      float* __restrict__ out1, int dog_out,
                                                      float dog_scale, const float* mm) {
    const int64_t n = d.nx * d.ny * d.nz;
    const int r = K / 2;
    const int64_t len = axis == 0 ? d.nx : (axis == 1 ? d.ny : d.nz);
    const int64_t stride = axis == 0 ? 1 : (axis == 1 ? d.nx : d.nx * d.ny);
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += int64_t(gridDim.x) * kBlock) {
        int64_t pos;
        if (axis == 0) pos = i % d.nx;
        else if (axis == 1) pos = (i / d.nx) % d.ny;
        else pos = i / (d.nx * d.ny);
        const int64_t base = i - pos * stride;
        float a0 = 0.0f, a1 = 0.0f;
        for (int j = 0; j < K; ++j) {
            bool outside;
            const int64_t src = ext_index(pos + j - r, len, mode, outside);
            float v0, v1 = 0.0f;
            if (outside) {
                v0 = mode == OOB_VALUE ? value : 0.0f;
                v1 = v0;
            } else {
                v0 = normalize(in0[base + src * stride], mm);
                if (NK == 2) v1 = in1 ? normalize(in1[base + src * stride], mm) : v0;
            }
            a0 = __fadd_rn(a0, __fmul_rn(v0, k0[j]));
            if (NK == 2) a1 = __fadd_rn(a1, __fmul_rn(v1, k1[j]));
        }
        if (dog_out) {
            out0[i] = __fmul_rn(__fsub_rn(a1, a0), dog_scale);
        } else {
            out0[i] = a0;
            if (NK == 2) out1[i] = a1;
        }
    }
}

// Tiled separable passes (the bench path): 32-bit indices, the line segment of a
// block staged in LDS once (extension and normalisation applied while loading),
// taps from LDS, the same float32 tap order per output as k_sep_pass.  x pass: a
// block = 256 consecutive outputs of one row; y / z passes: 64 x-columns x 64
// positions along the axis (lanes run along x: coalesced, conflict-free).
constexpr int kSepX = 256;
constexpr int kSepRows = 8;  // rows per x-pass block (one 256-thread block per row segment was launch-bound)
constexpr int kSepTX = 64;
constexpr int kSepTY = 4;
constexpr int kSepTL = 64;

template <int NK>
__global__ __launch_bounds__(kSepX) void k_sep_x(Dims3 d, const float* __restrict__ in0,
                                                  const float* __restrict__ in1, const float* __restrict__ k0,
                                                  const float* __restrict__ k1, int K, int mode, float value,
                                                  float* __restrict__ out0, float* __restrict__ out1, int dog_out,
                                                  float dog_scale, const float* mm) {
    // NK == 2: both kernels' operands interleaved (float2), so one packed v_pk_mul /
    // v_pk_add (IEEE round-to-nearest per component, no FMA: bit-exact) serves both
    extern __shared__ __attribute__((aligned(8))) float sm[];
    const int r = K / 2;
    const int W = kSepX + K - 1;
    float* s0 = sm;                 // NK == 1: [W]; NK == 2: float2 [W]
    float* t0 = sm + NK * W;        // NK == 1: [K]; NK == 2: float2 [K]
    float2* s01 = reinterpret_cast<float2*>(sm);
    float2* t01 = reinterpret_cast<float2*>(t0);
    const int nx = int(d.nx);
    const int x0 = int(blockIdx.x) * kSepX;
    const int t = threadIdx.x;
    for (int i = t; i < K; i += kSepX) {
        if (NK == 2) t01[i] = make_float2(k0[i], k1[i]);
        else t0[i] = k0[i];
    }
    const bool same = in1 == nullptr || in1 == in0;
    const int y0 = int(blockIdx.y) * kSepRows;
    const int y1 = min(int(d.ny), y0 + kSepRows);
    for (int y = y0; y < y1; ++y) {
    const uint32_t row = (uint32_t(blockIdx.z) * uint32_t(d.ny) + uint32_t(y)) * uint32_t(nx);
    __syncthreads();  // the previous row's LDS reads are done
    for (int i = t; i < W; i += kSepX) {
        bool outside;
        const int src = ext_index32(x0 - r + i, nx, mode, outside);
        float v0, v1;
        if (outside) {
            v0 = mode == OOB_VALUE ? value : 0.0f;
            v1 = v0;
        } else {
            v0 = normalize(in0[row + src], mm);
            v1 = same ? v0 : normalize(in1[row + src], mm);
        }
        if (NK == 2) s01[i] = make_float2(v0, v1);
        else s0[i] = v0;
    }
    __syncthreads();
    const int x = x0 + t;
    if (x < nx) {
        float a0 = 0.0f, a1 = 0.0f;
        if constexpr (NK == 2) {
            dg_v2 acc = {0.0f, 0.0f};
            for (int j = 0; j < K; ++j) {
                const float2 v = s01[t + j], k = t01[j];
                acc = acc + dg_v2{v.x, v.y} * dg_v2{k.x, k.y};  // tap order kept, no contraction
            }
            a0 = acc.x;
            a1 = acc.y;
        } else {
            for (int j = 0; j < K; ++j) a0 = __fadd_rn(a0, __fmul_rn(s0[t + j], t0[j]));
        }
        if (dog_out) {
            out0[row + x] = __fmul_rn(__fsub_rn(a1, a0), dog_scale);
        } else {
            out0[row + x] = a0;
            if (NK == 2) out1[row + x] = a1;
        }
    }
    }
}

// AX 1 (y) or 2 (z): grid (x tiles, axis tiles, other coordinate)
// KW > 0: the tap count K == KW is known at compile time and a thread computes 16
// consecutive outputs from a register window of 16 + KW - 1 staged values (KW + 15
// LDS reads instead of 16 * KW); same per-output tap order.
template <int NK, int AX, int KW = 0>
__global__ __launch_bounds__(kSepTX * kSepTY) void k_sep_yz(Dims3 d, const float* __restrict__ in0,
                                                            const float* __restrict__ in1,
                                                            const float* __restrict__ k0,
                                                            const float* __restrict__ k1, int K, int mode,
                                                            float value, float* __restrict__ out0,
                                                            float* __restrict__ out1, int dog_out,
                                                            float dog_scale, const float* mm) {
    extern __shared__ __attribute__((aligned(8))) float sm[];
    const int r = K / 2;
    const int H = kSepTL + K - 1;  // staged positions along the axis
    float* s0 = sm;                       // NK == 1: [H][64]; NK == 2: float2 [H][64]
    float* t0 = sm + NK * H * kSepTX;     // NK == 1: [K]; NK == 2: float2 [K]
    float2* s01 = reinterpret_cast<float2*>(sm);
    float2* t01 = reinterpret_cast<float2*>(t0);
    const int nx = int(d.nx), ny = int(d.ny), nz = int(d.nz);
    const int len = AX == 1 ? ny : nz;
    const uint32_t astride = AX == 1 ? uint32_t(nx) : uint32_t(nx) * uint32_t(ny);
    const int tx = threadIdx.x % kSepTX, ty = threadIdx.x / kSepTX;
    const int x = int(blockIdx.x) * kSepTX + tx;
    const int a0p = int(blockIdx.y) * kSepTL;
    const int other = int(blockIdx.z);  // z for the y pass, y for the z pass
    const uint32_t base = AX == 1 ? uint32_t(other) * uint32_t(nx) * uint32_t(ny) + uint32_t(x)
                                  : uint32_t(other) * uint32_t(nx) + uint32_t(x);
    for (int i = threadIdx.x; i < K; i += kSepTX * kSepTY) {
        if (NK == 2) t01[i] = make_float2(k0[i], k1[i]);
        else t0[i] = k0[i];
    }
    const bool xin = x < nx;
    const bool same = in1 == nullptr || in1 == in0;
    for (int i = ty; i < H; i += kSepTY) {
        bool outside;
        const int src = ext_index32(a0p - r + i, len, mode, outside);
        float v0 = 0.0f, v1 = 0.0f;
        if (outside) {
            v0 = mode == OOB_VALUE ? value : 0.0f;
            v1 = v0;
        } else if (xin) {
            v0 = normalize(in0[base + uint32_t(src) * astride], mm);
            v1 = same ? v0 : normalize(in1[base + uint32_t(src) * astride], mm);
        }
        if (NK == 2) s01[i * kSepTX + tx] = make_float2(v0, v1);
        else s0[i * kSepTX + tx] = v0;
    }
    __syncthreads();
    if (!xin) return;
    if constexpr (KW > 0) {
        constexpr int OW = kSepTL / kSepTY;  // 16 consecutive outputs per thread
        constexpr int WN = OW + KW - 1;
        const int ob = ty * OW;
        if constexpr (NK == 2) {
            dg_v2 acc[OW], w[WN];
#pragma unroll
            for (int i = 0; i < WN; ++i) {
                const float2 v = s01[(ob + i) * kSepTX + tx];
                w[i] = dg_v2{v.x, v.y};
            }
#pragma unroll
            for (int o = 0; o < OW; ++o) acc[o] = dg_v2{0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                const float2 kk = t01[j];
                const dg_v2 k = dg_v2{kk.x, kk.y};
#pragma unroll
                for (int o = 0; o < OW; ++o) acc[o] = acc[o] + w[o + j] * k;  // tap order kept
            }
#pragma unroll
            for (int o = 0; o < OW; ++o) {
                const int p = a0p + ob + o;
                if (p < len) {
                    const uint32_t idx = base + uint32_t(p) * astride;
                    if (dog_out) {
                        out0[idx] = __fmul_rn(__fsub_rn(acc[o].y, acc[o].x), dog_scale);
                    } else {
                        out0[idx] = acc[o].x;
                        out1[idx] = acc[o].y;
                    }
                }
            }
        } else {
            float acc[OW], w[WN];
#pragma unroll
            for (int i = 0; i < WN; ++i) w[i] = s0[(ob + i) * kSepTX + tx];
#pragma unroll
            for (int o = 0; o < OW; ++o) acc[o] = 0.0f;
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                const float k = t0[j];
#pragma unroll
                for (int o = 0; o < OW; ++o) acc[o] = __fadd_rn(acc[o], __fmul_rn(w[o + j], k));
            }
#pragma unroll
            for (int o = 0; o < OW; ++o) {
                const int p = a0p + ob + o;
                if (p < len) out0[base + uint32_t(p) * astride] = acc[o];
            }
        }
        return;
    }
    for (int o = ty; o < kSepTL; o += kSepTY) {
        const int p = a0p + o;
        if (p >= len) break;
        float a0 = 0.0f, a1 = 0.0f;
        if constexpr (NK == 2) {
            dg_v2 acc = {0.0f, 0.0f};
            for (int j = 0; j < K; ++j) {
                const float2 v = s01[(o + j) * kSepTX + tx], k = t01[j];
                acc = acc + dg_v2{v.x, v.y} * dg_v2{k.x, k.y};
            }
            a0 = acc.x;
            a1 = acc.y;
        } else {
            for (int j = 0; j < K; ++j) a0 = __fadd_rn(a0, __fmul_rn(s0[(o + j) * kSepTX + tx], t0[j]));
        }
        const uint32_t idx = base + uint32_t(p) * astride;
        if (dog_out) {
            out0[idx] = __fmul_rn(__fsub_rn(a1, a0), dog_scale);
        } else {
            out0[idx] = a0;
            if (NK == 2) out1[idx] = a1;
        }
    }
}

}  // namespace

void sep_pass(const Dims3& d, int axis, const float* in0, const float* in1, const float* k0,
              const float* k1, int K, int mode, float value, float* out0, float* out1, bool dog,
              float dog_scale, const float* mm, hipStream_t s) {
    const int64_t n = d.nx * d.ny * d.nz;
    const bool two = in1 || k1;
    const int nk = two ? 2 : 1;
    // tiled passes: 32-bit indices, grid y/z extents within 65535
    const int64_t tl = axis == 0 ? 1 : ceil_div(axis == 1 ? d.ny : d.nz, int64_t(kSepTL));
    const int64_t oth = axis == 0 ? d.nz : (axis == 1 ? d.nz : d.ny);
    if (n < (int64_t(1) << 31) && (axis == 0 ? d.ny : tl) <= 65535 && oth <= 65535) {
        if (axis == 0) {
            const size_t lds = size_t(nk * (kSepX + K - 1) + nk * K) * sizeof(float);
            const dim3 grid(unsigned(ceil_div(d.nx, int64_t(kSepX))), unsigned(ceil_div(d.ny, int64_t(kSepRows))),
                            unsigned(d.nz));
            if (two)
                hipLaunchKernelGGL(k_sep_x<2>, grid, dim3(kSepX), lds, s, d, in0, in1, k0, k1, K, mode, value,
                                   out0, out1, int(dog), dog_scale, mm);
            else
                hipLaunchKernelGGL(k_sep_x<1>, grid, dim3(kSepX), lds, s, d, in0, in1, k0, k1, K, mode, value,
                                   out0, out1, int(dog), dog_scale, mm);
        } else {
            const size_t lds = size_t(nk * (kSepTL + K - 1) * kSepTX + nk * K) * sizeof(float);
            const dim3 grid(unsigned(ceil_div(d.nx, int64_t(kSepTX))), unsigned(tl), unsigned(oth));
#define SD_SEPYZ1(NKV, AXV, KWV)                                                                          \
            SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sep_yz<NKV, AXV, KWV>),           \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));            \
            hipLaunchKernelGGL((k_sep_yz<NKV, AXV, KWV>), grid, dim3(kSepTX * kSepTY), lds, s, d, in0, in1, k0, \
                               k1, K, mode, value, out0, out1, int(dog), dog_scale, mm);
#define SD_SEPYZ(NKV, AXV)                                    \
            if (K == 7) { SD_SEPYZ1(NKV, AXV, 7) }            \
            else if (K == 15) { SD_SEPYZ1(NKV, AXV, 15) }     \
            else { SD_SEPYZ1(NKV, AXV, 0) }
            if (two && axis == 1) { SD_SEPYZ(2, 1) }
            else if (two) { SD_SEPYZ(2, 2) }
            else if (axis == 1) { SD_SEPYZ(1, 1) }
            else { SD_SEPYZ(1, 2) }
#undef SD_SEPYZ
#undef SD_SEPYZ1
        }
        SD_HIP(hipGetLastError());
        return;
    }
    const dim3 grid(unsigned(std::min<int64_t>(std::max<int64_t>(ceil_div(n, kBlock), 1), 4096)));
    if (in1 || k1)
        hipLaunchKernelGGL(k_sep_pass<2>, grid, dim3(kBlock), 0, s, d, axis, in0, in1, k0,
                           k1, K, mode, value, out0, out1, int(dog), dog_scale, mm);
    else
        hipLaunchKernelGGL(k_sep_pass<1>, grid, dim3(kBlock), 0, s, d, axis, in0, in1, k0,
                           k1, K, mode, value, out0, out1, int(dog), dog_scale, mm);
    SD_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- convolve_N
void separable_convolve(float* image, const float* kx, const float* ky, const float* kz, int w,
                        int h, int dd, bool cx, bool cy, bool cz, int oob, float oobv, int dev, int K) {
    SD_CHECK(image, SPIMDECON_ERR_ARG, "null image");
    SD_CHECK(w >= 1 && h >= 1 && dd >= 1, SPIMDECON_ERR_ARG, "bad dims");
    SD_CHECK(oob >= 0 && oob <= 3, SPIMDECON_ERR_ARG, "bad outofbounds mode");
    SD_CHECK((!cx || kx) && (!cy || ky) && (!cz || kz), SPIMDECON_ERR_ARG, "null kernel");
    check_device(dev);
    DeviceGuard guard(dev);
    ScopedStream st;
    const hipStream_t s = st.s;
    const Dims3 d{w, h, dd};
    const int64_t n = int64_t(w) * h * dd;
    DBuf<float> a(n), b(n), dk(3 * size_t(K));
    SD_HIP(hipMemcpyAsync(a.p, image, n * 4, hipMemcpyHostToDevice, s));
    const float* ks[3] = {kx, ky, kz};
    const bool on[3] = {cx, cy, cz};
    float* cur = a.p;
    float* nxt = b.p;
    for (int ax = 0; ax < 3; ++ax) {
        if (!on[ax]) continue;
        SD_HIP(hipMemcpyAsync(dk.p + ax * K, ks[ax], K * 4, hipMemcpyHostToDevice, s));
        sep_pass(d, ax, cur, nullptr, dk.p + ax * K, nullptr, K, oob, oobv, nxt, nullptr, false, 0.f,
                 nullptr, s);
        std::swap(cur, nxt);
    }
    SD_HIP(hipMemcpyAsync(image, cur, n * 4, hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
}

}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

#define CONVOLVE_N(N)                                                                            \
    extern "C" int32_t convolve_##N(float* image, const float* kernelX, const float* kernelY,  \
                                    const float* kernelZ, int imageW, int imageH, int imageD,   \
                                    int32_t convolveX, int32_t convolveY, int32_t convolveZ,    \
                                    int outofbounds, float outofboundsvalue, int devCUDA) {     \
        const int st = guarded([&] {                                                            \
            separable_convolve(image, kernelX, kernelY, kernelZ, imageW, imageH, imageD,         \
                               convolveX != 0, convolveY != 0, convolveZ != 0, outofbounds,     \
                               outofboundsvalue, devCUDA, N);                                   \
        });                                                                                     \
        return st == SPIMDECON_OK ? 1 : 0;                                                      \
    }

CONVOLVE_N(7)
CONVOLVE_N(15)
CONVOLVE_N(31)
CONVOLVE_N(63)
CONVOLVE_N(127)
