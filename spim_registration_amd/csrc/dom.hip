// dom.hip -- "Difference-of-Mean (Integral image based)" bead detection on MI355X.
//
// References (under the reference's src/main/java/):
//   spim/fiji/plugin/interestpointdetection/DifferenceOfMean.java:27-133   defaults (2, 3, 0.02)
//   spim/process/interestpointdetection/ProcessDOM.java:36-117             diameters, min / max, peaks
//   mpicbg/spim/segmentation/IntegralImage3d.java:60-210                   (long)(int) voxel, prefix sums
//   mpicbg/spim/segmentation/DOM.java:29-171                               the two box sums and the value
//
// dom(p) = (float) s2 / d2 - (float) s1 / d1 where s_b is the sum of (int) voxel over the
// box b centred on p (as long) and d_b = (float)(box voxels) * (max - min).  The reference
// reads s_b off a (nx+1)(ny+1)(nz+1) long integral image; integer addition is exact and
// associative (also modulo 2^64), so any order of summation gives the same s_b, and the
// integral image is never built here.  One pass over HBM instead:
//   k_dom        per block a TX x TY tile of columns (plus the box halo) walking a chunk of z:
//                each thread keeps the z box sums of both boxes of its columns as running
//                sums in registers (enter / leave one plane per step), the x then y box sums
//                of those go through two LDS tiles, then the two divisions and the store
//   k_dom_frame  the zero frame (ProcessDOM.java:89-94: every voxel the boxes do not reach)
// All sums are 64-bit (unsigned in the code: wrap-around is then defined).  Everything from
// the stored image on is the shared detection stage (detect.hpp).
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"
#include "detect.hpp"

namespace spimdecon {
namespace {

constexpr int kDomBlock = 256;
constexpr int kDomMaxDiameter = 33;     // per axis; the LDS tiles of k_dom are sized for it
constexpr size_t kDomLdsMax = 64 * 1024;
constexpr size_t kDomLdsCu = 160 * 1024;   // LDS of one gfx950 CU

typedef unsigned long long u64;

struct DomBox {
    int h1[3], h2[3], hm[3];   // half sizes of box 1, box 2, and their maximum, per axis
    int vol1, vol2;            // sx * sy * sz as int (DOM.java:33-34)
};

struct DomTile {
    int lx;       // log2 of the tile's x extent
    int ty;       // its y extent
    int zc;       // output planes per block
};

// Java's (int) of a float: toward zero, NaN -> 0, saturating (IntegralImage3d.java:102,110)
__device__ __forceinline__ int java_int(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT_MAX;
    if (v <= -2147483648.0f) return INT_MIN;
    return int(v);
}
__device__ __forceinline__ u64 widen(int v) { return u64((long long)v); }

// NC: columns (tile + halo) per thread
template <int NC>
__global__ __launch_bounds__(kDomBlock) void k_dom(Dims3 d, const float* __restrict__ in,
                                                   const float* __restrict__ mm, DomBox b, DomTile t,
                                                   float* __restrict__ out) {
    extern __shared__ ulonglong2 dom_lds[];
    const int tid = int(threadIdx.x);
    const int nx = int(d.nx), ny = int(d.ny), nz = int(d.nz);
    const int TX = 1 << t.lx, TY = t.ty;
    const int HX = TX + 2 * b.hm[0], HY = TY + 2 * b.hm[1], ncol = HX * HY;
    ulonglong2* tile1 = dom_lds;          // [HY][HX]: z box sums (box 1, box 2) per column
    ulonglong2* tile2 = dom_lds + ncol;   // [HY][TX]: x then z box sums
    const unsigned ntx = unsigned((nx - 2 * b.hm[0] + TX - 1) >> t.lx);
    const unsigned nty = unsigned((ny - 2 * b.hm[1] + TY - 1) / TY);
    const unsigned bid = blockIdx.x;
    const unsigned q = bid / ntx;
    const int tix = int(bid - q * ntx), tiy = int(q % nty), tiz = int(q / nty);
    const int gx0 = tix << t.lx, gy0 = tiy * TY;             // the halo's first column
    const int za = b.hm[2] + tiz * t.zc, zb = min(za + t.zc, nz - b.hm[2]);   // output planes
    const int64_t plane = int64_t(nx) * ny;

    int off[NC];      // the columns' offsets in a plane (-1: outside the image or the tile)
    u64 a1[NC], a2[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int c = tid + k * kDomBlock;
        const int cy = c / HX, cx = c - cy * HX;
        const int gx = gx0 + cx, gy = gy0 + cy;
        off[k] = c < ncol && gx < nx && gy < ny ? gy * nx + gx : -1;
        a1[k] = a2[k] = 0;
    }
    // the z box sums of the chunk's first plane
    for (int dz = -b.hm[2]; dz <= b.hm[2]; ++dz) {
        const float* pl = in + int64_t(za + dz) * plane;
        const bool in1 = abs(dz) <= b.h1[2], in2 = abs(dz) <= b.h2[2];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (off[k] < 0) continue;
            const u64 v = widen(java_int(pl[off[k]]));
            if (in1) a1[k] += v;
            if (in2) a2[k] += v;
        }
    }
    const float diff = __fsub_rn(mm[1], mm[0]);                // DOM.java:31-37
    const float d1 = __fmul_rn(float(b.vol1), diff), d2 = __fmul_rn(float(b.vol2), diff);

    for (int z = za; z < zb; ++z) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int c = tid + k * kDomBlock;
            if (c < ncol) tile1[c] = make_ulonglong2(a1[k], a2[k]);
        }
        // the planes entering and leaving the two z boxes (used after the tile's passes)
        int e1[NC], l1[NC], e2[NC], l2[NC];
        const bool more = z + 1 < zb;
        if (more) {
            const float* pe1 = in + int64_t(z + 1 + b.h1[2]) * plane;
            const float* pl1 = in + int64_t(z - b.h1[2]) * plane;
            const float* pe2 = in + int64_t(z + 1 + b.h2[2]) * plane;
            const float* pl2 = in + int64_t(z - b.h2[2]) * plane;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const bool ok = off[k] >= 0;
                const int o = ok ? off[k] : 0;
                e1[k] = ok ? java_int(pe1[o]) : 0;
                l1[k] = ok ? java_int(pl1[o]) : 0;
                e2[k] = ok ? java_int(pe2[o]) : 0;
                l2[k] = ok ? java_int(pl2[o]) : 0;
            }
        }
        __syncthreads();
        // x box sums of every row of the tile (halo rows included)
        for (int e = tid; e < (HY << t.lx); e += kDomBlock) {
            const int r = e >> t.lx, x = e & (TX - 1);
            const ulonglong2* row = tile1 + r * HX + x + b.hm[0];
            u64 s1 = 0, s2 = 0;
            for (int j = -b.h1[0]; j <= b.h1[0]; ++j) s1 += row[j].x;
            for (int j = -b.h2[0]; j <= b.h2[0]; ++j) s2 += row[j].y;
            tile2[e] = make_ulonglong2(s1, s2);
        }
        __syncthreads();
        // y box sums, the value, the store
        for (int o = tid; o < (TY << t.lx); o += kDomBlock) {
            const int y = o >> t.lx, x = o & (TX - 1);
            const int gx = gx0 + b.hm[0] + x, gy = gy0 + b.hm[1] + y;
            if (gx >= nx - b.hm[0] || gy >= ny - b.hm[1]) continue;
            const ulonglong2* col = tile2 + ((y + b.hm[1]) << t.lx) + x;
            u64 s1 = 0, s2 = 0;
            for (int j = -b.h1[1]; j <= b.h1[1]; ++j) s1 += col[j * TX].x;
            for (int j = -b.h2[1]; j <= b.h2[1]; ++j) s2 += col[j * TX].y;
            // (float) s2 / d2 - (float) s1 / d1 (DOM.java:155): long -> float to nearest even,
            // IEEE divisions, no contraction
            const float v = __fsub_rn(__fdiv_rn(__ll2float_rn((long long)s2), d2),
                                      __fdiv_rn(__ll2float_rn((long long)s1), d1));
            out[int64_t(z) * plane + int64_t(gy) * nx + gx] = v;
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                a1[k] += widen(e1[k]) - widen(l1[k]);
                a2[k] += widen(e2[k]) - widen(l2[k]);
            }
        }
        // (tile1 is rewritten after the second barrier of this step, tile2 after the first
        // of the next: no third barrier)
    }
}

// FusionHelper.minMax (FusionHelper.java:87-141) as Java computes it: Math.min / Math.max
// from Float.MAX_VALUE / -Float.MAX_VALUE, so one NaN voxel makes both NaN (the DOM image
// is then NaN wherever the boxes fit) -- min, max and "saw a NaN" per block, then one wave.
// Not k_minmax's rule (dog.hip: a NaN is skipped and only raises the finite flag), so the
// two stay separate kernels.
constexpr int kDomMmBlocks = 2048;
constexpr float kFloatMax = 3.402823466e+38f;
__device__ __forceinline__ void dom_mm_wave(float& mn, float& mx, int& nan) {
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        nan |= __shfl_xor(nan, o, 64);
    }
}
__global__ __launch_bounds__(kDomBlock) void k_dom_minmax(const float* __restrict__ in, int64_t n,
                                                          float* __restrict__ partial) {
    __shared__ float smn[kDomBlock / 64], smx[kDomBlock / 64];
    __shared__ int snan[kDomBlock / 64];
    float mn = kFloatMax, mx = -kFloatMax;
    int nan = 0;
    for (int64_t i = int64_t(blockIdx.x) * kDomBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kDomBlock) {
        const float v = in[i];
        nan |= v != v ? 1 : 0;
        mn = fminf(mn, v);   // (fminf / fmaxf drop a NaN: the flag carries it)
        mx = fmaxf(mx, v);
    }
    dom_mm_wave(mn, mx, nan);
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
        snan[threadIdx.x >> 6] = nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kDomBlock / 64; ++w) {
            mn = fminf(mn, smn[w]);
            mx = fmaxf(mx, smx[w]);
            nan |= snan[w];
        }
        partial[3 * blockIdx.x] = mn;
        partial[3 * blockIdx.x + 1] = mx;
        partial[3 * blockIdx.x + 2] = nan ? 1.0f : 0.0f;
    }
}
__global__ __launch_bounds__(64) void k_dom_minmax_final(const float* __restrict__ partial, int nb,
                                                         float* __restrict__ mm) {
    float mn = kFloatMax, mx = -kFloatMax;
    int nan = 0;
    for (int b = int(threadIdx.x); b < nb; b += 64) {
        mn = fminf(mn, partial[3 * b]);
        mx = fmaxf(mx, partial[3 * b + 1]);
        nan |= partial[3 * b + 2] != 0.0f ? 1 : 0;
    }
    dom_mm_wave(mn, mx, nan);
    if (threadIdx.x == 0) {
        mm[0] = nan ? __builtin_nanf("") : mn;
        mm[1] = nan ? __builtin_nanf("") : mx;
    }
}

// zeros outside hm <= p < n - hm; a wave per row of x.  interior = 0: the boxes fit nowhere,
// the whole image is zero.
__global__ __launch_bounds__(kDomBlock) void k_dom_frame(Dims3 d, int hx, int hy, int hz, int interior,
                                                         float* __restrict__ out) {
    const int lane = int(threadIdx.x & 63);
    const int64_t nrows = d.ny * d.nz;
    const int64_t nw = int64_t(gridDim.x) * (kDomBlock / 64);
    const int nx = int(d.nx);
    for (int64_t row = int64_t(blockIdx.x) * (kDomBlock / 64) + (threadIdx.x >> 6); row < nrows; row += nw) {
        const int64_t z = row / d.ny, y = row - z * d.ny;
        float* o = out + row * d.nx;
        if (interior && y >= hy && y < d.ny - hy && z >= hz && z < d.nz - hz) {
            for (int x = lane; x < hx; x += 64) o[x] = 0.0f;
            for (int x = nx - hx + lane; x < nx; x += 64) o[x] = 0.0f;
        } else {
            for (int x = lane; x < nx; x += 64) o[x] = 0.0f;
        }
    }
}

// the tile of k_dom for the half sizes hm: the most outputs per column summed, weighted by
// the blocks a CU holds (LDS-bound; beyond 4 blocks the weight stays)
DomTile dom_tile(const int hm[3], size_t* lds_bytes, int* ncols) {
    DomTile best{};
    double best_score = -1.0;
    for (int lx = 4; lx <= 6; ++lx)
        for (int ty = 1; ty <= 32; ++ty) {
            const int tx = 1 << lx, hx = tx + 2 * hm[0], hy = ty + 2 * hm[1];
            const int64_t ncol = int64_t(hx) * hy;
            const size_t lds = size_t(ncol + int64_t(tx) * hy) * sizeof(ulonglong2);
            if (ncol > 16 * kDomBlock || lds > kDomLdsMax) continue;
            const double score = double(tx * ty) / double(ncol) * double(std::min<size_t>(kDomLdsCu / lds, 4));
            if (score > best_score) {
                best_score = score;
                best = DomTile{lx, ty, 0};
                *lds_bytes = lds;
                *ncols = int(ncol);
            }
        }
    SD_CHECK(best_score > 0.0, SPIMDECON_ERR_STATE, "no DOM tile fits");
    best.zc = std::max(64, 8 * hm[2]);
    return best;
}

double dom_nan() { return std::nan(""); }

// every argument rule that needs no GPU
void dom_check_params(const spim_dom_params* p) {
    SD_CHECK(p, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(p->radius1 >= 1 && p->radius2 >= 1, SPIMDECON_ERR_ARG, "radius1 and radius2 must be >= 1");
    for (int a = 0; a < 3; ++a)
        SD_CHECK(std::isfinite(p->image_sigma[a]) && p->image_sigma[a] > 0.0, SPIMDECON_ERR_ARG,
                 "image_sigma must be finite and > 0");
}

// ProcessDOM.java:71-78 (double arithmetic, Math.round = floor(x + 0.5))
void dom_diameters(const spim_dom_params* p, int32_t s1[3], int32_t s2[3]) {
    dom_check_params(p);
    SD_CHECK(s1 && s2, SPIMDECON_ERR_ARG, "null argument");
    auto diam = [](int radius, double sigma, int least) {
        const double r = std::floor(double(radius) * (0.5 / sigma) + 0.5);
        const int ri = r > 1.0e9 ? 1000000000 : int(r);   // (far beyond any supported box)
        return std::max(least, ri * 2 + 1);
    };
    for (int a = 0; a < 3; ++a) {
        s1[a] = diam(p->radius1, p->image_sigma[a], 3);
        s2[a] = diam(p->radius2, p->image_sigma[a], 5);
    }
}

// the DOM image (the caller's device buffer, else the workspace's) and its candidates
void dom_run(const float* img, const int64_t* dims, const spim_dom_params* p, float* dom_out, hipStream_t s,
             DogWork& w, DogRun& r) {
    const Dims3 d{dims[0], dims[1], dims[2]};
    const int64_t n = d.nx * d.ny * d.nz;
    SD_CHECK(d.nx < (int64_t(1) << 31) && d.ny < (int64_t(1) << 31) && d.nz < (int64_t(1) << 31) &&
                 n < (int64_t(1) << 40),
             SPIMDECON_ERR_ARG, "volume too large");
    SD_CHECK(d.nx * d.ny < (int64_t(1) << 31), SPIMDECON_ERR_ARG,
             "DOM: a plane must hold fewer than 2^31 voxels");
    int32_t s1[3], s2[3];
    dom_diameters(p, s1, s2);
    DomBox b{};
    for (int a = 0; a < 3; ++a) {
        SD_CHECK(s1[a] <= kDomMaxDiameter && s2[a] <= kDomMaxDiameter, SPIMDECON_ERR_ARG,
                 "DOM box diameter beyond the supported maximum of 33 voxels per axis");
        b.h1[a] = s1[a] / 2;
        b.h2[a] = s2[a] / 2;
        b.hm[a] = std::max(b.h1[a], b.h2[a]);
    }
    b.vol1 = s1[0] * s1[1] * s1[2];
    b.vol2 = s2[0] * s2[1] * s2[2];

    const float* in = stage_in(img, n, p->device, w.in, s);
    // ProcessDOM.java:54-66 (the rule of ProcessDOG)
    grow(w.mm, 3 * 4096);   // {min, max, -, -, the per-block partials}
    static_assert(4 + 3 * kDomMmBlocks <= 3 * 4096, "partials beyond the min / max buffer");
    const bool use_given = !(std::isnan(p->min_intensity) || std::isnan(p->max_intensity) ||
                             std::isinf(p->min_intensity) || std::isinf(p->max_intensity) ||
                             p->min_intensity == p->max_intensity);
    if (use_given) {
        const float h2[3] = {float(p->min_intensity), float(p->max_intensity), 1.0f};
        SD_HIP(hipMemcpyAsync(w.mm.p, h2, 12, hipMemcpyHostToDevice, s));
    } else {
        const int nb = int(std::min<int64_t>(ceil_div(n, int64_t(kDomBlock)), kDomMmBlocks));
        hipLaunchKernelGGL(k_dom_minmax, dim3(unsigned(nb)), dim3(kDomBlock), 0, s, in, n, w.mm.p + 4);
        hipLaunchKernelGGL(k_dom_minmax_final, dim3(1), dim3(64), 0, s, w.mm.p + 4, nb, w.mm.p);
        SD_HIP(hipGetLastError());
    }
    ImageDest dst(dom_out, n, p->device);
    float* const domp = dst.store(w.dog);
    // DOM.java:47-53: where the boxes fit; elsewhere (everywhere, when they fit nowhere) zero
    const bool interior = d.nx > 2 * b.hm[0] && d.ny > 2 * b.hm[1] && d.nz > 2 * b.hm[2];
    const unsigned gf = unsigned(std::min<int64_t>(ceil_div(d.ny * d.nz, int64_t(kDomBlock / 64)), 8192));
    hipLaunchKernelGGL(k_dom_frame, dim3(gf), dim3(kDomBlock), 0, s, d, b.hm[0], b.hm[1], b.hm[2], int(interior),
                       domp);
    SD_HIP(hipGetLastError());
    if (interior) {
        size_t lds = 0;
        int ncol = 0;
        const DomTile t = dom_tile(b.hm, &lds, &ncol);
        const int64_t blocks = ceil_div(d.nx - 2 * b.hm[0], int64_t(1) << t.lx) *
                               ceil_div(d.ny - 2 * b.hm[1], int64_t(t.ty)) *
                               ceil_div(d.nz - 2 * b.hm[2], int64_t(t.zc));
        SD_CHECK(blocks < (int64_t(1) << 31), SPIMDECON_ERR_ARG, "volume too large");
#define SD_DOM(NCV)                                                                                       \
        SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dom<NCV>),                            \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));                \
        hipLaunchKernelGGL(k_dom<NCV>, dim3(unsigned(blocks)), dim3(kDomBlock), lds, s, d, in, w.mm.p, b, t, domp);
        if (ncol <= 8 * kDomBlock) { SD_DOM(8) } else { SD_DOM(16) }
#undef SD_DOM
        SD_HIP(hipGetLastError());
    }
    // ProcessDOM.java:104: the threshold as given (no / 10 with quadratic localisation)
    detect_stored(w, d, domp, p->threshold, p->find_min ? 1 : 0, p->find_max ? 1 : 0, p->ij_threads, s, r);
    dst.copy_out(s);
}

}  // namespace

void dom_compute(const float* img, const int64_t* dims, const spim_dom_params* p, float* dom_out, spim_peak* peaks,
                 int64_t max_peaks, int64_t* npeaks) {
    SD_CHECK(npeaks, SPIMDECON_ERR_ARG, "null argument");
    check_detector_args(img, dims, p, [&] { dom_check_params(p); });
    with_work<DogWork>(p->device, [&](DogWork& w, hipStream_t s) {
        DogRun r;
        dom_run(img, dims, p, dom_out, s, w, r);
        peaks_to_host(r, peaks, max_peaks, npeaks, s);
    });
}

// ProcessDOM.compute's result: interest points after Localization (ProcessDOM.java:107-112)
void dom_interest_points(const float* img, const int64_t* dims, const spim_dom_params* p, float* dom_out,
                         spim_interest_point* out, int64_t max_out, int64_t* nout) {
    SD_CHECK(nout, SPIMDECON_ERR_ARG, "null argument");
    check_detector_args(img, dims, p, [&] { dom_check_params(p); });
    with_work<DogWork>(p->device, [&](DogWork& w, hipStream_t s) {
        DogRun r;
        dom_run(img, dims, p, dom_out, s, w, r);
        points_from_peaks(w, r, p->localization, p->threshold, out, max_out, nout, s);
    });
}

}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" void spim_dom_params_default(spim_dom_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->radius1 = 2;
    p->radius2 = 3;
    p->threshold = 0.02f;
    p->localization = 0;
    p->image_sigma[0] = p->image_sigma[1] = p->image_sigma[2] = 0.5;
    p->find_min = 0;
    p->find_max = 1;
    p->min_intensity = dom_nan();
    p->max_intensity = dom_nan();
    p->ij_threads = 8;
    p->device = 0;
}

extern "C" int spim_dom_diameters(const spim_dom_params* p, int32_t s1[3], int32_t s2[3]) {
    return guarded([&] { dom_diameters(p, s1, s2); });
}

extern "C" int spim_dom_compute(const float* img, const int64_t* dims, const spim_dom_params* p, float* dom_out,
                                spim_peak* peaks, int64_t max_peaks, int64_t* npeaks) {
    return guarded([&] { dom_compute(img, dims, p, dom_out, peaks, max_peaks, npeaks); });
}

extern "C" int spim_dom_interest_points(const float* img, const int64_t* dims, const spim_dom_params* p,
                                        float* dom_out, spim_interest_point* out, int64_t max_out,
                                        int64_t* nout) {
    return guarded([&] { dom_interest_points(img, dims, p, dom_out, out, max_out, nout); });
}
