// downsample.hip -- the view downsampling in front of interest point detection on MI355X.
//
// References (under the reference's src/main/java/):
//   spim/process/interestpointdetection/Downsample.java:65-162             simple2x along one axis
//   spim/fiji/plugin/interestpointdetection/DifferenceOf.java:446-535      openAndDownsample: every x level,
//                                                                          then every y level, then every z level
//   spim/fiji/plugin/interestpointdetection/DifferenceOf.java:430-444      downsampleFactor ("Match Z Resolution")
//
// One level along an axis, a line of n voxels to m = n / 2 (double arithmetic in Java's order,
// one rounding to float per level: every level is stored as a float image):
//   out[0]     = (in[0] + in[1] * 0.5) / 1.5
//   out[q]     = (in[2q-1] * 0.5 + in[2q] + in[2q+1] * 0.5) / 2.0          0 < q < m - 1
//   out[m - 1] = (in[2m-2] + in[2m-3] * 0.5) / 1.5
// (* 0.5 and / 2.0 are exact; / 1.5 is the IEEE double division; the build has no contraction.)
// Output q of a level reads inputs 2q-1 .. 2q+1 at most, so a final output p of an L-level chain
// reads inputs 2^L p - (2^L - 1) .. 2^L p + (2^L - 1): the window of a tile of T final outputs
// is 2^(L-l) (T + 1) - 1 wide at level l, whatever the edge formulas select inside it.
//   k_ds_xy  per block one plane's tile of final outputs: the input window (tile + halo) goes to
//            LDS in 16-byte row loads, its rows are reduced level by level (x chain), then its
//            columns (y chain), ping-pong between two LDS buffers; only the final tile is written
//   k_ds_z   every z level at once over the xy-reduced image: per thread a column of kDsZOut
//            final outputs, its window of planes in registers, reduced in place
// Window entries outside the image are never computed and never read by an entry inside it.
// The xy-reduced image between the two kernels is the shared detector workspace's tmp_a
// (spim_dog_release_workspace frees it); no full-size temporary exists.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "detect.hpp"

namespace spimdecon {
namespace {

constexpr int kDsBlock = 256;
constexpr int kDsTileX = 128;   // input columns a tile's final outputs stand for (halo not counted)
constexpr int kDsTileY = 64;    // input rows, when y is downsampled (kDsTileY0 rows otherwise)
constexpr int kDsTileY0 = 32;
constexpr int kDsZOut = 4;      // final z outputs per thread of k_ds_z

struct DsXY {
    int nx, ny, nz;     // the input
    int nxo, nyo;       // the xy-reduced plane
    int lx, ly;         // levels (0..3)
    int ltx;            // log2 of the tile's final outputs in x
    int tyo;            // the tile's final outputs in y
    int s0;             // LDS row stride of level 0 (a multiple of 4)
    int a_floats;       // floats of the first LDS buffer (the second follows it)
    int vec;            // rows are read as float4 (nx % 4 == 0 and a 16-byte aligned image)
    unsigned ntx, nty;  // tiles per plane
};

// one output of simple2x: p points at input 2q - 1 of the line (stride st), m outputs in the line
__device__ __forceinline__ float ds_step(const float* p, int st, int q, int m) {
    if (q == 0) return float((double(p[st]) + double(p[2 * st]) * 0.5) / 1.5);
    if (q == m - 1) return float((double(p[st]) + double(p[0]) * 0.5) / 1.5);
    return float(((double(p[0]) * 0.5 + double(p[st])) + double(p[2 * st]) * 0.5) * 0.5);
}

// the same on values: a, b, c = inputs 2q - 1, 2q, 2q + 1 (a value that does not exist is not used)
__device__ __forceinline__ float ds_step3(float a, float b, float c, bool first, bool last) {
    if (first) return float((double(b) + double(c) * 0.5) / 1.5);
    if (last) return float((double(b) + double(a) * 0.5) / 1.5);
    return float(((double(a) * 0.5 + double(b)) + double(c) * 0.5) * 0.5);
}

// window of level l of an L-level chain over final outputs [p0, p0 + t): first index, length
__device__ __forceinline__ int ds_lo(int p0, int up) { return (p0 << up) - ((1 << up) - 1); }
__device__ __forceinline__ int ds_len(int t, int up) { return ((t + 1) << up) - 1; }

__global__ __launch_bounds__(kDsBlock) void k_ds_xy(const float* __restrict__ in, DsXY g,
                                                    float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float ds_lds[];
    const int tid = int(threadIdx.x);
    const unsigned bid = blockIdx.x;
    const unsigned bq = bid / g.ntx;
    const int tix = int(bid - bq * g.ntx), tiy = int(bq % g.nty), z = int(bq / g.nty);
    const int txo = 1 << g.ltx;
    const int p0x = tix << g.ltx, p0y = tiy * g.tyo;
    const int lox0 = ds_lo(p0x, g.lx), loy0 = ds_lo(p0y, g.ly);
    const int h0 = ds_len(g.tyo, g.ly);
    const int x0a = lox0 & ~3;             // the first loaded column (floor to 4, also below 0)
    float* bufa = ds_lds;
    float* bufb = ds_lds + g.a_floats;
    const float* src = in + int64_t(z) * g.ny * g.nx;

    // level 0: rows loy0 .. loy0 + h0 - 1, columns x0a .. x0a + s0 - 1, where they exist
    if (g.vec) {
        const int s4 = g.s0 >> 2;
        for (int e = tid; e < s4 * h0; e += kDsBlock) {
            const int r = e / s4, k = e - r * s4;
            const int gy = loy0 + r, gx = x0a + 4 * k;
            if (gy < 0 || gy >= g.ny || gx < 0 || gx >= g.nx) continue;
            *reinterpret_cast<float4*>(bufa + r * g.s0 + 4 * k) =
                *reinterpret_cast<const float4*>(src + int64_t(gy) * g.nx + gx);
        }
    } else {
        for (int e = tid; e < g.s0 * h0; e += kDsBlock) {
            const int r = e / g.s0, c = e - r * g.s0;
            const int gy = loy0 + r, gx = x0a + c;
            if (gy < 0 || gy >= g.ny || gx < 0 || gx >= g.nx) continue;
            bufa[e] = src[int64_t(gy) * g.nx + gx];
        }
    }
    __syncthreads();

    float* cur = bufa;
    float* nxt = bufb;
    int cs = g.s0, coff = lox0 - x0a;      // row stride of cur, column of its window's first entry
    // the x chain over every row of the window
    for (int l = 1; l <= g.lx; ++l) {
        const int w = ds_len(txo, g.lx - l), lo = ds_lo(p0x, g.lx - l), m = g.nx >> l;
        for (int e = tid; e < w * h0; e += kDsBlock) {
            const int r = e / w, j = e - r * w;
            const int gy = loy0 + r, q = lo + j;
            if (gy < 0 || gy >= g.ny || q < 0 || q >= m) continue;
            nxt[e] = ds_step(cur + r * cs + coff + 2 * j, 1, q, m);
        }
        __syncthreads();
        float* done = nxt;
        nxt = cur;
        cur = done;
        cs = w;
        coff = 0;
    }
    // the y chain over the tile's columns
    for (int l = 1; l <= g.ly; ++l) {
        const int h = ds_len(g.tyo, g.ly - l), lo = ds_lo(p0y, g.ly - l), m = g.ny >> l;
        for (int e = tid; e < (h << g.ltx); e += kDsBlock) {
            const int r = e >> g.ltx, c = e & (txo - 1);
            const int q = lo + r;
            if (q < 0 || q >= m || p0x + c >= g.nxo) continue;
            nxt[e] = ds_step(cur + 2 * r * cs + coff + c, cs, q, m);
        }
        __syncthreads();
        float* done = nxt;
        nxt = cur;
        cur = done;
        cs = txo;
        coff = 0;
    }
    float* dst = out + int64_t(z) * g.nyo * g.nxo;
    for (int e = tid; e < (g.tyo << g.ltx); e += kDsBlock) {
        const int r = e >> g.ltx, c = e & (txo - 1);
        const int gx = p0x + c, gy = p0y + r;
        if (gx >= g.nxo || gy >= g.nyo) continue;
        dst[int64_t(gy) * g.nxo + gx] = cur[r * cs + coff + c];
    }
}

// L z levels over an image of nz planes of `plane` voxels: nzo = nz >> L planes out
template <int L>
__global__ __launch_bounds__(kDsBlock) void k_ds_z(const float* __restrict__ in, int plane, int nz, int nzo,
                                                   float* __restrict__ out) {
    const int i = int(blockIdx.x) * kDsBlock + int(threadIdx.x);
    if (i >= plane) return;
    const int p0 = int(blockIdx.y) * kDsZOut;
    constexpr int W0 = ((kDsZOut + 1) << L) - 1;
    float v[W0];
    const int lo0 = (p0 << L) - ((1 << L) - 1);
#pragma unroll
    for (int j = 0; j < W0; ++j) {
        const int zz = min(max(lo0 + j, 0), nz - 1);   // (a clamped plane stands in an entry nothing valid reads)
        v[j] = in[int64_t(zz) * plane + i];
    }
#pragma unroll
    for (int l = 1; l <= L; ++l) {
        const int w = ((kDsZOut + 1) << (L - l)) - 1;
        const int lo = (p0 << (L - l)) - ((1 << (L - l)) - 1), m = nz >> l;
#pragma unroll
        for (int j = 0; j < w; ++j) {      // in place: entry j is written after 2j .. 2j + 2 are read
            const int q = lo + j;
            v[j] = ds_step3(v[2 * j], v[2 * j + 1], v[2 * j + 2], q == 0, q == m - 1);
        }
    }
#pragma unroll
    for (int k = 0; k < kDsZOut; ++k)
        if (p0 + k < nzo) out[int64_t(p0 + k) * plane + i] = v[k];
}

int ds_levels(int32_t f) { return f == 1 ? 0 : f == 2 ? 1 : f == 4 ? 2 : f == 8 ? 3 : -1; }

// repeated / 2; every level's input at least 4 long (Downsample.java:115-140 reads in[1] and
// in[2m - 3]: a line of 2 or 3 would leave the image)
void downsample_dims(const int64_t* dims, const int32_t* factor, int64_t* out_dims) {
    SD_CHECK(dims && factor && out_dims, SPIMDECON_ERR_ARG, "null argument");
    for (int a = 0; a < 3; ++a) {
        const int lv = ds_levels(factor[a]);
        SD_CHECK(lv >= 0, SPIMDECON_ERR_ARG, "downsample: a factor must be 1, 2, 4 or 8");
        SD_CHECK(dims[a] >= 1, SPIMDECON_ERR_ARG, "bad dims");
        int64_t n = dims[a];
        for (int l = 0; l < lv; ++l) {
            SD_CHECK(n >= 4, SPIMDECON_ERR_ARG,
                     "downsample: an axis shorter than 4 voxels at one of its levels cannot be halved");
            n /= 2;
        }
        out_dims[a] = n;
    }
}

void launch_xy(const float* in, const int64_t* dims, int lx, int ly, const int64_t* od, float* out,
               hipStream_t s) {
    DsXY g{};
    g.nx = int(dims[0]);
    g.ny = int(dims[1]);
    g.nz = int(dims[2]);
    g.nxo = int(od[0]);
    g.nyo = int(od[1]);
    g.lx = lx;
    g.ly = ly;
    int ltx = 0;
    while ((1 << ltx) < (kDsTileX >> lx)) ++ltx;
    g.ltx = ltx;
    g.tyo = ly ? kDsTileY >> ly : kDsTileY0;
    const int txo = 1 << ltx;
    const int w0 = ((txo + 1) << lx) - 1, h0 = ((g.tyo + 1) << ly) - 1;
    g.s0 = (w0 + 3 + 3) & ~3;   // up to 3 columns in front of the window (float4 alignment)
    g.a_floats = g.s0 * h0;
    // the second buffer holds the level after level 0: x level 1 of every row, else y level 1
    const int b_floats = lx ? (((txo + 1) << (lx - 1)) - 1) * h0 : ly ? txo * (((g.tyo + 1) << (ly - 1)) - 1) : 0;
    g.vec = g.nx % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
    g.ntx = unsigned(ceil_div(g.nxo, txo));
    g.nty = unsigned(ceil_div(g.nyo, g.tyo));
    const int64_t blocks = int64_t(g.ntx) * g.nty * g.nz;
    SD_CHECK(blocks < (int64_t(1) << 31), SPIMDECON_ERR_ARG, "volume too large");
    const size_t lds = size_t(g.a_floats + b_floats) * sizeof(float);
    SD_CHECK(lds <= 64 * 1024, SPIMDECON_ERR_STATE, "downsample tile beyond 64 KB of LDS");
    hipLaunchKernelGGL(k_ds_xy, dim3(unsigned(blocks)), dim3(kDsBlock), lds, s, in, g, out);
    SD_HIP(hipGetLastError());
}

void launch_z(const float* in, int64_t plane, int64_t nz, int lz, int64_t nzo, float* out, hipStream_t s) {
    const dim3 grid(unsigned(ceil_div(plane, int64_t(kDsBlock))), unsigned(ceil_div(nzo, int64_t(kDsZOut))));
    SD_CHECK(grid.y <= 65535, SPIMDECON_ERR_ARG, "volume too large");
    if (lz == 1)
        hipLaunchKernelGGL(k_ds_z<1>, grid, dim3(kDsBlock), 0, s, in, int(plane), int(nz), int(nzo), out);
    else if (lz == 2)
        hipLaunchKernelGGL(k_ds_z<2>, grid, dim3(kDsBlock), 0, s, in, int(plane), int(nz), int(nzo), out);
    else
        hipLaunchKernelGGL(k_ds_z<3>, grid, dim3(kDsBlock), 0, s, in, int(plane), int(nz), int(nzo), out);
    SD_HIP(hipGetLastError());
}

void downsample(const float* img, const int64_t* dims, const int32_t* factor, int device, float* out) {
    SD_CHECK(img && out, SPIMDECON_ERR_ARG, "null argument");
    int64_t od[3];
    downsample_dims(dims, factor, od);
    const int lx = ds_levels(factor[0]), ly = ds_levels(factor[1]), lz = ds_levels(factor[2]);
    const int64_t n = dims[0] * dims[1] * dims[2], no = od[0] * od[1] * od[2];
    SD_CHECK(dims[0] < (int64_t(1) << 30) && dims[1] < (int64_t(1) << 30) && dims[2] < (int64_t(1) << 30) &&
                 n < (int64_t(1) << 40) && dims[0] * dims[1] < (int64_t(1) << 31),
             SPIMDECON_ERR_ARG, "volume too large");
    with_work<DogWork>(device, [&](DogWork& w, hipStream_t s) {
        const float* in = stage_in(img, n, device, w.in, s);
        ImageDest dest(out, no, device);
        float* const dst = dest.store(w.dog);
        const bool xy = lx || ly;
        if (!xy && !lz) {
            SD_HIP(hipMemcpyAsync(dst, in, n * 4, hipMemcpyDeviceToDevice, s));
        } else if (xy && lz) {
            const int64_t mid[3] = {od[0], od[1], dims[2]};
            grow(w.tmp_a, size_t(mid[0] * mid[1] * mid[2]));
            launch_xy(in, dims, lx, ly, mid, w.tmp_a.p, s);
            launch_z(w.tmp_a.p, mid[0] * mid[1], mid[2], lz, od[2], dst, s);
        } else if (xy) {
            launch_xy(in, dims, lx, ly, od, dst, s);
        } else {
            launch_z(in, dims[0] * dims[1], dims[2], lz, od[2], dst, s);
        }
        dest.copy_out(s);
        SD_HIP(hipStreamSynchronize(s));
    });
}

// DifferenceOf.java:430-444 in its own arithmetic (Math.round = floor(x + 0.5))
void downsample_factor_xy(int more, int32_t ds_z, const double* voxel, int32_t* factor) {
    SD_CHECK(voxel && factor, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(ds_levels(ds_z) >= 0, SPIMDECON_ERR_ARG, "downsample: a factor must be 1, 2, 4 or 8");
    for (int a = 0; a < 3; ++a)
        SD_CHECK(std::isfinite(voxel[a]) && voxel[a] > 0.0, SPIMDECON_ERR_ARG,
                 "voxel size must be finite and > 0");
    const double cal_xy = std::min(voxel[0], voxel[1]);
    const double cal_z = voxel[2] * double(ds_z);
    const double log2ratio = std::log(cal_z / cal_xy) / std::log(2.0);
    const double exp2 = std::pow(2.0, more ? std::ceil(log2ratio) : std::floor(log2ratio));
    const double r = std::floor(exp2 + 0.5);
    // below 1 (z finer than xy; the reference would return 0 and scale every coordinate by 0): 1
    SD_CHECK(r <= 8.0, SPIMDECON_ERR_ARG,
             "downsample: matching the z resolution needs an xy factor above 8, beyond the reference's choices");
    *factor = r < 1.0 ? 1 : int32_t(r);
}

}  // namespace
}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" int spim_downsample_dims(const int64_t dims[3], const int32_t factor[3], int64_t out_dims[3]) {
    return guarded([&] { downsample_dims(dims, factor, out_dims); });
}

extern "C" int spim_downsample(const float* img, const int64_t dims[3], const int32_t factor[3], int device,
                               float* out) {
    return guarded([&] { downsample(img, dims, factor, device, out); });
}

extern "C" int spim_downsample_factor_xy(int more, int32_t ds_z, const double voxel[3], int32_t* factor) {
    return guarded([&] { downsample_factor_xy(more, ds_z, voxel, factor); });
}
