// dog.hip -- the fused Difference-of-Gaussian of the bead detection on MI355X.
//
// References (under the reference's src/main/java/):
//   spim/process/interestpointdetection/ProcessDOG.java:40-178   pipeline, sigmas
//   spim/process/interestpointdetection/DifferenceOfGaussianCUDA.java:116-181  both GPU modes:
//       accurate    = extendMirrorSingle (:153-154)                  -> OOB_MIRROR
//       approximate = EXTEND_BORDER_PIXELS on the plain image (:125-148, blocks of
//                     BlockGeneratorVariableSizeSimple, which do not change a voxel) -> OOB_BORDER
//   spim/process/fusion/FusionHelper.java:176-234                 normalizeImage
//
// One DoG, all HBM-resident (Gaussians of 7 / 15 / 31 taps -- the ProcessDOG sigmas):
//   k_dog_xy     img --(normalise on the fly)--> x then y Gaussians of both sigmas -> G12
//   k_dog_zconv  G12 -> z Gaussians -> dog = (G2 - G1) * 1/(k-1), stored; its candidates: detect.hip
//   k_dog_z      beyond k_dog_zconv's limits: the same DoG and the 26-neighbour test in one
// (63 / 127 taps: the passes of sepconv.hip.)  From the candidates on: detect.hpp.
// Accumulation order = tap order in float32 (matches the oracle bit for bit).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "detect_dev.hpp"
#include "sepconv.hpp"

namespace spimdecon {

namespace {

// ---------------------------------------------------------------- fused DoG (the ProcessDOG path)
// Every output keeps the float32 tap order of k_sep_x / k_sep_yz (packed mul, then
// packed add, no contraction): the DoG image is bit-identical to the separate passes.
// HBM per voxel: 4 B read + 8 B write (xy), 8 B read (+ 4 B DoG write) (z) -- 20-24 B
// against 48 B for the separate passes plus two re-reads of the DoG by the peak passes.
constexpr int kDxyTX = 64;   // xy tile: outputs along x (TY along y: template)
constexpr int kDxySeg = 8;   // x outputs per thread in the x phase (register window)
constexpr int kDzBX = 64;    // z kernel: a box of 64 x BY columns = one wave per row, the
                             // outer ring is the peak test's halo (62 x (BY - 2) tested columns)
// planes loaded ahead of use (3 left the HBM latency exposed; 12 or 16 no better, 16
// costs a wave per SIMD); KW + kDzPD must be a multiple of 4 (the ring slots)
#ifndef SPIMDECON_DZ_PD
#define SPIMDECON_DZ_PD 9
#endif
constexpr int kDzPD = SPIMDECON_DZ_PD;
                             // (a step computes in ~350 cycles; a load takes thousands)
constexpr int kDzChunk = 128; // DoG planes per block (the window adds KW - 1 + 2 loads; 64: 2.46 vs 2.35 ms)
constexpr int kDzMaxLen = 512;   // k_dog_z plane-offset table: chunk + 2 + KW - 1 + PD entries
#ifndef SPIMDECON_DZC_PD
#define SPIMDECON_DZC_PD 9
#endif
#ifndef SPIMDECON_DZC_ILV
#define SPIMDECON_DZC_ILV 0
#endif
constexpr int kDzcPD = SPIMDECON_DZC_PD;   // k_dog_zconv: planes loaded ahead

__device__ __forceinline__ int mirror32(int i, int n) {
    bool o;
    return ext_index32(i, n, OOB_MIRROR, o);
}
// EXTEND_BORDER_PIXELS: the nearest voxel of the axis
__device__ __forceinline__ int clamp32(int i, int n) { return min(max(i, 0), n - 1); }

// LDS writes visible to the block, without the release fence of __syncthreads (which
// would also wait for the planes loaded ahead)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS pitch (floats) of the staged input rows of k_dog_xy: >= iw, a multiple of 4 (16-B
// aligned rows for the b128 window reads) and 4 * odd modulo 64, so that the 16 lanes of a
// ds_read_b128 group -- 16 consecutive rows of one segment, rows mod 16 all distinct --
// start on 16 distinct 4-bank groups (MI355X_MICROARCH.md LDS table): conflict-free
__host__ __device__ constexpr int dxy_in_pitch(int iw) {
    int p = (iw + 3) / 4 * 4;
    while ((p / 4) % 2 == 0) p += 4;
    return p;
}
// row pitch (float2) of the x-phase results: 64 + 2, so the 8 consecutive rows of a
// ds_write_b128 group land on 8 distinct 4-bank groups mod 32
constexpr int kDxySxP = kDxyTX + 2;

// (v - mn) / diff correctly rounded (__fdiv_rn's result) from the reciprocal rd = RN(1/diff):
// q = v * rd, then two Markstein corrections q += (a - q * diff) * rd with exact fma
// residuals -- the second starts from a faithful quotient, so it rounds correctly
// (Markstein's theorem; the Tikhonov step, rl_math.hpp, uses the same scheme in double).
// Outside the range where the residuals are exact (0, tiny, huge or non-finite a) the
// IEEE division itself.  5 VALU instead of the ~10 of the scaled division sequence.
// (caller: |a| in [2^-48, 2^48] or a == +0, and diff in [2^-48, 2^48]: q and the
// residuals stay normal; -0 would come out +0, so it takes the division)
__device__ __forceinline__ float div_rn_rcp_core(float a, float diff, float rd) {
    float q = __fmul_rn(a, rd);
    q = __fmaf_rn(__fmaf_rn(-q, diff, a), rd, q);
    return __fmaf_rn(__fmaf_rn(-q, diff, a), rd, q);
}

// The box of a k_dog_z block.  With `xcd` the dispatch order is remapped so that each
// XCD (blocks go round-robin to the 8 XCDs, each with its own L2) walks a contiguous
// range of boxes with y fastest: the boxes it holds at once are y-neighbours, whose
// overlapping halo rows (2 of every BY) then come from that L2 instead of HBM.
// (k_dog_xy: x fastest, so each XCD's resident tiles share their x and y halo columns.)
struct DzBox { int bx, by, bz; };
template <bool YFAST>
__device__ __forceinline__ DzBox xcd_box(bool xcd) {
    if (!xcd) return {int(blockIdx.x), int(blockIdx.y), int(blockIdx.z)};
    const unsigned gx = gridDim.x, gy = gridDim.y;
    const unsigned n = gx * gy * gridDim.z;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned k = lin & 7u, j = lin >> 3, q = n >> 3, r = n & 7u;
    const unsigned l = k * q + min(k, r) + j;           // XCD k: logical boxes [k q + min(k, r), ...)
    if (YFAST) return {int((l / gy) % gx), int(l % gy), int(l / (gy * gx))};
    return {int(l % gx), int((l / gx) % gy), int(l / (gx * gy))};
}

// Strips: a block walks one 64-column strip of one plane down y in steps of TY output rows.
// Each step stages, normalises and x-convolves only its TY new input rows; the KW - 1 rows
// above them are the previous step's last x results, carried (the y phase's last run holds
// them in registers and writes them to the first LDS rows after a barrier), and a strip
// starts with the KW - 1 rows above its first step.  Tiles of TY rows (round 4) recomputed
// the KW - 1 halo rows of every tile: (TY + KW - 1) / TY = 1.29 times the x phase and the
// normalisation at TY = 48, against (ny + KW - 1) / ny = 1.02 here.  TY = 32: a step's x
// phase is 32 rows x 8 segments = one item per thread (48 rows left two of the four waves
// a second item, and the blocks of a CU run their phases in step, so the SIMDs of those
// waves set the pace: no gain at 48), 4 blocks per CU; 768^3: k_dog_xy 1.63 -> 1.47 ms,
// DoG 3.67 -> 3.52 ms (profiles/r05_dog_strips_ab.txt).
// BORDER (the fused kernels' only two modes): false = mirror-single, true = clamp to the
// edge voxel (EXTEND_BORDER_PIXELS).  It is read only where a step that is not `inside`
// forms a source index.  The carried rows stay valid under clamp: the x results of row
// clamp(y) ARE the x results of that row of the extended image.  (A template parameter: as
// a runtime argument it cost the 15-tap kernel, at its 128-VGPR bound, 4 spilled VGPRs and
// changed the registers of the z kernels -- DESIGN.md 4.2; the mirror instantiations are
// the code they were.)
template <int KW, int TY, bool BUF = true, int JT = 0, bool BORDER = false>
__global__ __launch_bounds__(256, 4) void k_dog_xy(Dims3 d, const float* __restrict__ in, const float2* __restrict__ kx,
                                                const float2* __restrict__ ky, float2* __restrict__ g12,
                                                const float* __restrict__ mm, int xcd, int mm_exact) {
    constexpr bool border = BORDER;
    constexpr int R = KW / 2;
    constexpr int IW = kDxyTX + KW - 1;          // staged input columns
    constexpr int IP = dxy_in_pitch(IW);         // pitch (see dxy_in_pitch)
    constexpr int IH = TY + KW - 1;              // x-result rows of a step's window
    constexpr int NSEG = kDxyTX / kDxySeg;
    constexpr int WX = kDxySeg + KW - 1;
    constexpr int OY = TY / 4;                   // y outputs per thread (4 runs per column)
    constexpr int WY = OY + KW - 1;
    static_assert(TY % 4 == 0 && OY + 2 * R == WY, "4 runs per column");
    __shared__ __attribute__((aligned(16))) float sin_[TY * IP];
    __shared__ __attribute__((aligned(16))) float2 sx[IH * kDxySxP];
    const int nx = int(d.nx), ny = int(d.ny);
    const int gx = (nx + kDxyTX - 1) / kDxyTX, gy = (ny + TY - 1) / TY;
    const int nstrips = gx * int(d.nz);
    const int t = threadIdx.x;
    // FusionHelper.normalizeImage constants (skipped for a NaN / inf / zero range)
    bool norm = false;
    float mn = 0.0f, diff = 1.0f, rd = 1.0f;
    if (mm) {
        mn = mm[0];
        diff = __fsub_rn(mm[1], mn);
        norm = !(isnan(diff) || isinf(diff) || diff == 0.0f);
        rd = __frcp_rn(diff);
        if (!(fabsf(diff) >= 0x1p-48f && fabsf(diff) <= 0x1p48f)) rd = 0.0f;   // (division only)
    }
    // mm_exact: mn / mx are the image's own min / max (k_minmax, not caller-given), so
    // every finite value has mn <= v <= mx and a = v - mn lies in [0, diff]; with
    // |mn| >= 2^-20 a non-zero a is at least the float spacing just below 2^-20 (2^-44), and
    // a = 0 is +0: every a is in the reciprocal path's exact range (NaN stays NaN either
    // way), so the per-value range check is skipped for the whole launch
    const bool allfast = norm && mm_exact != 0 && rd != 0.0f && fabsf(mn) >= 0x1p-20f;
    // Tap trim: the JT leading (and trailing) taps of the x and y kernels are zero for both
    // sigmas (padded to KW; the host instantiates JT).  When k_minmax found every value
    // finite (mm[2] == 0) and the image is normalised by its own range, every staged value
    // lies in [0, 1] and every partial sum is finite and never -0 (it starts at +0; the
    // taps are >= 0), so such a tap's +-0 product leaves the sum's bits unchanged: skipped.
    // (Either extension: a clamped index stages an image value like a mirrored one, so the
    // [0, 1] range and the argument hold for the border mode too -- the trim is kept there.)
    // Otherwise (NaN / inf in the image, a caller-given range) every padded tap is applied,
    // as before (one uniform branch per item between the two unrolled tap loops).
    const bool trim = JT > 0 && mm && norm && mm_exact != 0 && mm[2] == 0.0f;
    // thread t stages column t % IPC (IPC = IP rounded up so three rows fit 256 threads)
    // of rows t / IPC, t / IPC + RPT, ...: the column's mirror index once, the row's per
    // load.  Steps whose staged box lies inside the volume index without the mirror
    // arithmetic.
    constexpr int RPT = 256 / IW;                // rows staged per pass
    constexpr int IPC = 256 / RPT;               // threads per row (>= IW)
    constexpr int NE = (TY + RPT - 1) / RPT;     // rows per thread and step
    const int col = t % IPC, r0 = t / IPC;
    const bool cact = col < IW && r0 < RPT;
    // BUF (image below 4 GiB): buffer loads, the lane's row offset in a VGPR and the
    // pass offset RPT * e * nx in the scalar offset (no per-load address arithmetic; rows
    // past the step load in range or return 0 and are never staged); y mirror indices by
    // one reflection when ny > R (the modulo of mirror32 cost ~15 VALU per staged value
    // on the border strips)
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(in), 0, int(uint32_t(BUF ? uint64_t(d.nx * d.ny * d.nz) * 4u : 0u)), 0x00020000);
    const bool yrefl = ny > R;
    // input rows [ys, ys + NR) of strip s -> v (row r0 + RPT e of the unit; NR = 2R for the
    // rows above a strip, TY for a step)
    auto stage_loads = [&](int s, int ys, auto nrc, float* v) {
        constexpr int NR = decltype(nrc)::value;
        constexpr int NEc = (NR + RPT - 1) / RPT;
        const int x0 = (s % gx) * kDxyTX;
        const uint32_t plane = uint32_t(s / gx) * uint32_t(ny) * uint32_t(nx);
        const bool inside = x0 - R >= 0 && x0 - R + IW <= nx && ys >= 0 && ys + NR <= ny;
        if (inside) {
            const uint32_t base = plane + uint32_t(ys) * uint32_t(nx) + uint32_t(x0 - R + min(col, IW - 1));
            if constexpr (BUF) {
                const uint32_t vo = (base + uint32_t(r0) * uint32_t(nx)) * 4u;
#pragma unroll
                for (int e = 0; e < NEc; ++e)
                    v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                         rin, int(vo), int(uint32_t(RPT * e) * uint32_t(nx) * 4u), 0));
            } else {
#pragma unroll
                for (int e = 0; e < NEc; ++e) v[e] = in[base + uint32_t(min(r0 + RPT * e, NR - 1)) * uint32_t(nx)];
            }
        } else {
            const int xx = x0 - R + min(col, IW - 1);
            const uint32_t gxo = plane + uint32_t(border ? clamp32(xx, nx) : mirror32(xx, nx));
#pragma unroll
            for (int e = 0; e < NEc; ++e) {
                const int yy = ys + min(r0 + RPT * e, NR - 1);
                const int my = border  ? clamp32(yy, ny)
                               : yrefl ? (ny - 1) - abs((ny - 1) - abs(yy))
                                       : mirror32(yy, ny);
                if constexpr (BUF)
                    v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                         rin, int((gxo + uint32_t(my) * uint32_t(nx)) * 4u), 0, 0));
                else
                    v[e] = in[gxo + uint32_t(my) * uint32_t(nx)];
            }
        }
    };
    // normalise the staged values of a step and store them to the LDS rows
    auto norm_store = [&](auto nrc, float* v) {
        constexpr int NR = decltype(nrc)::value;
        constexpr int NEc = (NR + RPT - 1) / RPT;
        if (norm) {
            // one wave-uniform decision for all values: the reciprocal path unless a value
            // of the wave leaves its exact range (then the IEEE division for all)
            bool bad = rd == 0.0f;
#pragma unroll
            for (int e = 0; e < NEc; ++e) {
                v[e] = __fsub_rn(v[e], mn);
                if (!allfast) {
                    const float aa = fabsf(v[e]);
                    bad |= !((aa >= 0x1p-48f && aa <= 0x1p48f) || __float_as_uint(v[e]) == 0u);   // (+0 only)
                }
            }
            if (allfast || !__any(bad)) {
#pragma unroll
                for (int e = 0; e < NEc; ++e) v[e] = div_rn_rcp_core(v[e], diff, rd);
            } else {
#pragma unroll
                for (int e = 0; e < NEc; ++e) v[e] = __fdiv_rn(v[e], diff);
            }
        }
        if (cact) {   // (the previous step's x phase finished at its mid-step barrier)
#pragma unroll
            for (int e = 0; e < NEc; ++e) {
                const int row = r0 + RPT * e;
                if (row >= NR) break;
                sin_[row * IP + col] = v[e];
            }
        }
    };
    // x phase over the step's NR staged rows into sx rows xrow0 + row: lane = staged row,
    // a segment of kDxySeg outputs from a window of WX values (b128 reads through the pitch IP)
    auto x_phase = [&](auto nrc, int xrow0) {
        constexpr int NR = decltype(nrc)::value;
#pragma unroll 1
        for (int it = t; it < NR * NSEG; it += 256) {
            const int row = it % NR, seg = it / NR;
            const float* src = sin_ + row * IP + seg * kDxySeg;
            float w[WX];
#pragma unroll
            for (int i = 0; i < WX; ++i) w[i] = src[i];
            dg_v2 acc[kDxySeg];
#pragma unroll
            for (int o = 0; o < kDxySeg; ++o) acc[o] = dg_v2{0.0f, 0.0f};
            auto taps = [&](auto j0c) {
                constexpr int J0 = decltype(j0c)::value;
#pragma unroll
                for (int j = J0; j < KW - J0; ++j) {
                    const dg_v2 k = dg_v2{kx[j].x, kx[j].y};
#pragma unroll
                    for (int o = 0; o < kDxySeg; ++o) acc[o] = acc[o] + dg_v2{w[o + j], w[o + j]} * k;  // tap order kept
                }
            };
            if (trim) taps(std::integral_constant<int, JT>{});
            else taps(std::integral_constant<int, 0>{});
            float2* dst = sx + (xrow0 + row) * kDxySxP + seg * kDxySeg;
#pragma unroll
            for (int o = 0; o < kDxySeg; ++o) dst[o] = make_float2(acc[o].x, acc[o].y);
        }
    };
    using PREc = std::integral_constant<int, 2 * R>;
    using TYc = std::integral_constant<int, TY>;
    // persistent blocks over the strips; the next step's input values are loaded into
    // registers while this step is transformed
    // xcd: blocks go round-robin to the 8 XCDs (each its own L2); the logical block index
    // makes XCD k's blocks a contiguous range, so the strips one XCD holds at a time are x
    // neighbours whose halo columns its L2 serves (else they come from HBM twice)
    float v[NE];
    int strip = int(blockIdx.x);
    if (xcd) {
        const unsigned b = blockIdx.x, k = b & 7u, j = b >> 3, q = gridDim.x >> 3, r = gridDim.x & 7u;
        strip = int(k * q + min(k, r) + j);
    }
    // units of a strip: step -1 stages and x-convolves the 2R rows above the strip into sx
    // rows 0 .. 2R - 1; step k >= 0 its TY new rows [k TY + R, k TY + TY + R) into sx rows
    // 2R .., then the y phase of output rows [k TY, k TY + TY)
    int step = -1;
    if (strip < nstrips) stage_loads(strip, -R, PREc{}, v);
    const int c = t & (kDxyTX - 1), run = t / kDxyTX;
    while (strip < nstrips) {
        const int x0 = (strip % gx) * kDxyTX;
        const uint32_t plane = uint32_t(strip / gx) * uint32_t(ny) * uint32_t(nx);
        const int y0 = step * TY;
        const bool pre = step < 0;
        if (pre) norm_store(PREc{}, v);
        else norm_store(TYc{}, v);
        // the next unit's values are in flight during this unit's phases
        int nstrip = strip, nstep = step + 1;
        if (nstep == gy) {
            nstrip = strip + int(gridDim.x);
            nstep = -1;
        }
        if (nstrip < nstrips) {
            if (nstep < 0) stage_loads(nstrip, -R, PREc{}, v);
            else stage_loads(nstrip, nstep * TY + R, TYc{}, v);
        }
        __syncthreads();   // (also: the previous step's y phase no longer reads sx)
        if (pre) x_phase(PREc{}, 0);
        else x_phase(TYc{}, 2 * R);
        __syncthreads();
        if (pre) {   // (block-uniform)
            strip = nstrip;
            step = nstep;
            continue;
        }
        // y phase: column c, OY consecutive outputs
        const int x = x0 + c;
        dg_v2 w[WY];
        if (x < nx) {
#pragma unroll
            for (int i = 0; i < WY; ++i) {
                const float2 vv = sx[(run * OY + i) * kDxySxP + c];
                w[i] = dg_v2{vv.x, vv.y};
            }
            dg_v2 acc[OY];
#pragma unroll
            for (int o = 0; o < OY; ++o) acc[o] = dg_v2{0.0f, 0.0f};
            auto taps = [&](auto j0c) {
                constexpr int J0 = decltype(j0c)::value;
#pragma unroll
                for (int j = J0; j < KW - J0; ++j) {
                    const dg_v2 k = dg_v2{ky[j].x, ky[j].y};
#pragma unroll
                    for (int o = 0; o < OY; ++o) acc[o] = acc[o] + w[o + j] * k;
                }
            };
            if (trim) taps(std::integral_constant<int, JT>{});
            else taps(std::integral_constant<int, 0>{});
#pragma unroll
            for (int o = 0; o < OY; ++o) {
                const int y = y0 + run * OY + o;
                if (y < ny) g12[plane + uint32_t(y) * uint32_t(nx) + uint32_t(x)] = make_float2(acc[o].x, acc[o].y);
            }
        }
        // the last run holds the x results of the next step's first 2R rows: to sx rows
        // 0 .. 2R - 1 once every run has read its window (block-uniform branch)
        if (nstep >= 0) {
            __syncthreads();
            if (run == 3 && x < nx) {
#pragma unroll
                for (int i = 0; i < 2 * R; ++i) sx[i * kDxySxP + c] = make_float2(w[OY + i].x, w[OY + i].y);
            }
        }
        strip = nstrip;
        step = nstep;
    }
}

// z Gaussians + DoG + peak test over one column box and one chunk of planes.  Each
// thread keeps its column's window of KW planes (+ kDzPD loaded ahead) of (G1, G2) in
// registers, rotating by unrolling; the DoG planes go through a 4-plane LDS ring.  The
// 26-neighbour test is min / max of the 3x3x3 box (the box includes the centre, so
// "all neighbours >= c" <=> box min >= c); a plane holding a NaN takes the
// reference's comparison loop instead (NaN compares false).
//
// The ring: slot = (plane - qa) & 3, a compile-time constant of the unrolled step (NW is
// a multiple of 4), rows padded by one above and below and one element before and after,
// so the 3x3 neighbourhood is ONE per-thread address plus eight immediate offsets (edge
// lanes read a neighbouring row's element or a pad -- they are never tested).  The
// step's VALU work is the convolution's 2 KW packed ops plus ~20 for the test: the test
// had cost as much VALU as the convolution (r3t cost split).
template <int BY, int BX>
struct DzRing {
    static constexpr int kRow = BX, kSlot = (BY + 2) * BX, kSize = 4 * kSlot + 2;
    // element (slot, row r in [-1, BY], column c in [-1, BX])
    static __device__ __forceinline__ int at(int slot, int r, int c) { return 1 + slot * kSlot + (r + 1) * kRow + c; }
};

// InteractiveIntegral.isSpecialPoint (:443-468) over the ring (centre plane slot sc,
// row ty, column tx): 2 = every neighbour >= c ("MAX"), 1 = every neighbour <= c, 0 =
// neither.  Only for boxes holding a NaN (compares false), out of line.
template <int BY, int BX>
__device__ __noinline__ int dz_special_nan(const float* Dr, int sc, int ty, int tx, float c) {
    bool ge = true, le = true;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dz == 0 && dy == 0 && dx == 0) continue;
                const float v = Dr[DzRing<BY, BX>::at((sc + dz) & 3, ty + dy, tx + dx)];
                ge &= v >= c;
                le &= v <= c;
            }
    return ge ? 2 : (le ? 1 : 0);
}

// BX x BY columns per block (64 x 8: one wave per row; 62 x 6 of them tested).
// ONE: the DoG image is below 2 GiB, one buffer resource covers it (the plane goes in
// the scalar offset); else a resource per plane.  want: bit 0 minima, bit 1 maxima.
// The z taps are symmetric (gaussian_kernel builds them so): taps j and KW - 1 - j are
// the same value and only R + 1 of them are held in SGPRs.
// SL: the source plane of each load from scalar mirror arithmetic (needs nz > KW / 2: one
// reflection) and a buffer resource per plane, so the load's address is the column's
// constant byte offset; else the LDS plane table and a 64-bit address per load.
// BORDER: the plane index is clamped instead (either form; the host keeps the same
// dispatch conditions for both modes, under clamp they are merely conservative).
template <int KW, int BY, int PD, int BX, bool ONE, bool SL, bool BORDER = false>
__global__ __launch_bounds__(BX * BY) void k_dog_z(Dims3 d, const float2* __restrict__ g12,
                                                         const float2* __restrict__ kz, float scale, int zc_len,
                                                         float* __restrict__ dog, float minv, int want,
                                                         const PeakSink* __restrict__ sink, int xcd) {
    constexpr bool border = BORDER;
    constexpr int R = KW / 2;
    constexpr int NW = KW + PD;
    static_assert(NW % 4 == 0, "ring slots are compile-time: the unrolled rotation is whole ring turns");
    using Ring = DzRing<BY, BX>;
    __shared__ float Dr[Ring::kSize];
    __shared__ int nanq[4];
    __shared__ int4 cbuf[BX * BY / 64][kCandBuf];   // one candidate buffer per wave
    int ccount = 0;                       // wave-uniform fill of this wave's buffer
    const int t = threadIdx.x, tx = t & (BX - 1), ty = t / BX;
    const int wv = t >> 6, lane = t & 63;
    const int nx = int(d.nx), ny = int(d.ny), nz = int(d.nz);
    const DzBox bb = xcd_box<true>(xcd != 0);
    const int X0 = bb.bx * (BX - 2), Y0 = bb.by * (BY - 2);
    const int x = X0 + tx, y = Y0 + ty;
    const bool valid = x < nx && y < ny;
    const int z0 = bb.bz * zc_len, z1 = min(nz, z0 + zc_len);
    const int qa = max(z0 - 1, 0), qb = min(z1 + 1, nz);   // DoG planes computed
    const int len = qb - qa + KW - 1;                       // source planes loaded
    const int tlo = max(z0, 1), thi = min(z1, nz - 1);      // centre planes tested
    const uint32_t ntest = uint32_t(max(thi - tlo, 0));
    const uint32_t pstride = uint32_t(nx) * uint32_t(ny);
    const uint32_t col = valid ? uint32_t(y) * uint32_t(nx) + uint32_t(x) : 0u;
    // DoG store ownership: the tile's tested columns, plus the volume's outer ring
    const bool lastx = bb.bx == int(gridDim.x) - 1, lasty = bb.by == int(gridDim.y) - 1;
    const bool own = valid && tx >= (bb.bx == 0 ? 0 : 1) && (lastx || tx < BX - 1) &&
                     ty >= (bb.by == 0 ? 0 : 1) && (lasty || ty < BY - 1);
    const bool inner = valid && tx >= 1 && tx < BX - 1 && ty >= 1 && ty < BY - 1 && x <= nx - 2 &&
                       y <= ny - 2;
    // element offset of the source plane of every window index (mirror-single
    // extension, the tail repeating the last plane), for volumes the scalar path cannot take
    __shared__ uint32_t zoff[SL ? 1 : kDzMaxLen];
    if constexpr (!SL)
        for (int i = t; i < kDzMaxLen; i += BX * BY)
            zoff[i] = uint32_t(border ? clamp32(qa - R + min(i, len - 1), nz)
                                      : mirror32(qa - R + min(i, len - 1), nz)) * pstride;
    if (t < 4) nanq[t] = INT_MIN;   // (no plane)
    __syncthreads();
    // unconditional loads (columns outside the volume read column 0): no branch merge,
    // so they stay in flight PD planes ahead
    const uint32_t plane_bytes = pstride * 8u;
    auto ld = [&](int i) -> float2 {
        if constexpr (SL) {
            const int tz = qa - R + min(i, len - 1);
            // mirror-single, one reflection; or the clamped plane
            const int m = border ? clamp32(tz, nz) : (nz - 1) - abs((nz - 1) - abs(tz));
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float2*>(g12) + size_t(uint32_t(m)) * pstride, 0, int(plane_bytes), 0x00020000);
            return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, int(col * 8u), 0, 0));
        } else {
            return g12[zoff[min(i, kDzMaxLen - 1)] + col];
        }
    };
    // step s: window = source planes s .. s + KW - 1 in slots (s + j) % NW, DoG plane
    // q = qa + s; the step count is padded to whole NW rotations (padded steps test and
    // store nothing), so the unrolled body has no exits
    float2 w[NW];
#pragma unroll
    for (int p = 0; p < NW - 1; ++p) w[p] = ld(p);
    const int nsteps = (qb - qa + NW - 1) / NW * NW;
    float mnA = 0.f, mxA = 0.f, mnB = 0.f, mxB = 0.f, mnC = 0.f, mxC = 0.f, dB = 0.f, dC = 0.f;
    int nanhist = 0;   // bit k: the block's DoG plane q - k holds a NaN
    // DoG stores: one buffer resource over the whole image with the plane in the scalar
    // offset when the image is below 2 GiB (else one resource per plane)
    const uint64_t dog_total = dog ? uint64_t(pstride) * uint64_t(nz) * 4u : 0u;
    const __amdgpu_buffer_rsrc_t rall = __builtin_amdgcn_make_buffer_rsrc(dog, 0, ONE ? int(dog_total) : 0,
                                                                          0x00020000);
    const uint32_t dog_bytes = dog ? pstride * 4u : 0u;
    const bool want_min = (want & 1) != 0, want_max = (want & 2) != 0;
    float* const rbase = Dr + Ring::at(0, ty - 1, tx - 1);   // this thread's neighbourhood corner
    for (int sb = 0; sb < nsteps; sb += NW) {
#pragma unroll
        for (int ph = 0; ph < NW; ++ph) {
            const int st = sb + ph;
            w[(ph + NW - 1) % NW] = ld(st + NW - 1);
            dg_v2 acc = {0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < KW; ++j) {   // tap order kept
                const float2 v = w[(ph + j) % NW];
                const float2 k = kz[j <= R ? j : KW - 1 - j];
                acc = acc + dg_v2{v.x, v.y} * dg_v2{k.x, k.y};
            }
            const float dv = valid ? __fmul_rn(__fsub_rn(acc.y, acc.x), scale) : 0.0f;
            const int q = qa + st;
            {   // the DoG store: a buffer store, dropped (out of range) unless owned
                const bool st_ok = own && uint32_t(q - z0) < uint32_t(z1 - z0);
                const int vo = int(st_ok ? col * 4u : 0x80000000u);
                if constexpr (ONE) {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, dv), rall, vo,
                                                          int(uint32_t(min(q, nz - 1)) * pstride * 4u), 0);
                } else {
                    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
                        dog + (dog ? size_t(min(q, nz - 1)) * pstride : 0), 0, int(dog_bytes), 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, dv), rd, vo, 0, 0);
                }
            }
            const int slot = ph & 3;   // == (q - qa) & 3 (sb is a multiple of NW, so of 4): a constant once unrolled
            float* const P = rbase + slot * Ring::kSlot;
            P[Ring::kRow + 1] = dv;        // (row ty, column tx)
            if (__ballot(dv != dv) != 0ull && tx == 0) nanq[slot] = q;
            lds_barrier();
            const int nq = __builtin_amdgcn_readfirstlane(nanq[slot]);
            nanhist = ((nanhist << 1) | (nq == q ? 1 : 0)) & 7;
            mnA = mnB; mxA = mxB; mnB = mnC; mxB = mxC;
            dB = dC;
            dC = dv;
            {   // 3x3 box of this plane (the centre included), every lane
                const float a0 = P[0], a1 = P[1], a2 = P[2];
                const float b0 = P[Ring::kRow], b2 = P[Ring::kRow + 2];
                const float c0 = P[2 * Ring::kRow], c1 = P[2 * Ring::kRow + 1], c2 = P[2 * Ring::kRow + 2];
                mnC = dz_min3(dz_min3(a0, a1, a2), dz_min3(b0, b2, c0), dz_min3(c1, c2, dv));
                mxC = dz_max3(dz_max3(a0, a1, a2), dz_max3(b0, b2, c0), dz_max3(c1, c2, dv));
            }
            const int zc = q - 1;   // centre plane of the test
            if (uint32_t(zc - tlo) < ntest) {   // zc in [tlo, thi)
                const float c = dB;
                const bool cand = inner && !(fabsf(c) < minv);
                // "this mixup is intended" (InteractiveIntegral.isSpecialPoint): every
                // neighbour >= c is a MAX (sp 2), every neighbour <= c a MIN (sp 1); lane
                // masks, no per-lane branches
                // (the min / max path for every lane, then -- a uniform branch, rare -- the
                // comparison loop when a plane of the box held a NaN: no exec-mask merges)
                const bool ge = dz_min3(mnA, mnB, mnC) >= c;
                const bool le = dz_max3(mxA, mxB, mxC) <= c;
                bool is_max = cand && ge;
                bool is_min = cand && !ge && le;
                if (nanhist != 0) {   // a NaN in the box: the reference's comparison loop
                    const int spn = cand ? dz_special_nan<BY, BX>(Dr, (slot + 3) & 3, ty, tx, c) : 0;
                    is_max = spn == 2;
                    is_min = spn == 1;
                }
                const int sp = is_max ? 2 : 1;
                const bool flag = (is_max && want_max) || (is_min && want_min);
                const unsigned long long bal = __ballot(flag);
                if (bal != 0ull) {
                    const int nb = __popcll(bal);
                    if (ccount + nb > kCandBuf) {
                        cand_flush(sink, cbuf[wv], ccount, nx, pstride);
                        ccount = 0;
                    }
                    if (flag)
                        cbuf[wv][ccount + __popcll(bal & ((1ull << lane) - 1ull))] =
                            make_int4(x, y | (sp << 30), zc, __float_as_int(fabsf(c)));
                    ccount += nb;
                }
            }
        }
    }
    cand_flush(sink, cbuf[wv], ccount, nx, pstride);
}

// The split z stage, part 1: z Gaussians + DoG for every voxel, one thread per (x, y)
// column of a chunk of zc_len planes (a wave = 64 consecutive x of one row), a register
// window of KW planes + PD loaded ahead, rotating by unrolling; the DoG is stored for
// every voxel and the 26-neighbour test runs afterwards over the stored image
// (k_dog_peaks, detect.hip).  Columns are independent: no halo ring (the fused k_dog_z
// convolved its box's ring too, 1.38x the loads and convolutions), no LDS, no barrier.
// Same tap order and DoG expression as k_dog_z: the same bits.
// (plane bytes nx * ny * 8 < 2^31: one buffer resource per source plane; ONE: the DoG
// image below 2 GiB, one resource with the plane in the scalar offset)
template <int KW, int PD, bool ONE, bool ONEG, bool BORDER = false>
__global__ __launch_bounds__(256) void k_dog_zconv(Dims3 d, const float2* __restrict__ g12,
                                                   const float2* __restrict__ kz, float scale, int zc_len,
                                                   float* __restrict__ dog) {
    constexpr bool border = BORDER;
    constexpr int R = KW / 2;
    constexpr int NW = KW + PD;
    const int nx = int(d.nx), ny = int(d.ny), nz = int(d.nz);
    const int lane = int(threadIdx.x & 63);
    const int gxw = (nx + 63) / 64;                                          // waves per row
    const int wid = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * 4 + int(threadIdx.x >> 6));
    const int y = wid / gxw;
    if (y >= ny) return;   // (wave-uniform; no barriers in this kernel)
    const int x = (wid % gxw) * 64 + lane;
    const bool valid = x < nx;
    const int z0 = int(blockIdx.y) * zc_len, z1 = min(nz, z0 + zc_len);
    const int len = z1 - z0 + KW - 1;   // source planes
    const uint32_t pstride = uint32_t(nx) * uint32_t(ny);
    const uint32_t col = uint32_t(y) * uint32_t(nx) + uint32_t(valid ? x : nx - 1);
    // G12 below 4 GiB (every 768^3-class view): one resource, the source plane's byte
    // offset in the scalar offset (a resource per plane held 4 SGPRs per window slot)
    const uint64_t g12_bytes = uint64_t(pstride) * uint64_t(nz) * 8u;
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float2*>(g12), 0, int(uint32_t(g12_bytes < 0xffffffffull ? g12_bytes : 0xffffffffull)), 0x00020000);
    auto ld = [&](int i) -> float2 {
        // mirror-single extension, one reflection (the host takes this kernel for nz > KW / 2),
        // or (border) the clamped plane
        const int tz = z0 - R + min(i, len - 1);
        const int m = border ? clamp32(tz, nz) : (nz - 1) - abs((nz - 1) - abs(tz));
        if constexpr (ONEG)
            return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rg, int(col * 8u),
                                                                                   int(uint32_t(m) * pstride * 8u), 0));
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float2*>(g12) + size_t(uint32_t(m)) * pstride, 0, int(pstride * 8u), 0x00020000);
        return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, int(col * 8u), 0, 0));
    };
    float2 w[NW];
#pragma unroll
    for (int p = 0; p < NW - 1; ++p) w[p] = ld(p);
    const int nsteps = (z1 - z0 + NW - 1) / NW * NW;   // padded to whole rotations (stores dropped)
    const uint64_t dog_total = uint64_t(pstride) * uint64_t(nz) * 4u;
    const __amdgpu_buffer_rsrc_t rall = __builtin_amdgcn_make_buffer_rsrc(dog, 0, ONE ? int(dog_total) : 0, 0x00020000);
    for (int sb = 0; sb < nsteps; sb += NW) {
#pragma unroll
        for (int ph = 0; ph < NW; ++ph) {
            const int st = sb + ph;
            w[(ph + NW - 1) % NW] = ld(st + NW - 1);
            dg_v2 acc = {0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < KW; ++j) {   // tap order kept
                const float2 v = w[(ph + j) % NW];
                const float2 k = kz[j <= R ? j : KW - 1 - j];
                acc = acc + dg_v2{v.x, v.y} * dg_v2{k.x, k.y};
                if (SPIMDECON_DZC_ILV) __builtin_amdgcn_sched_barrier(0);
            }
            const float dv = __fmul_rn(__fsub_rn(acc.y, acc.x), scale);
            const int q = z0 + st;
            const int vo = int(valid && q < z1 ? col * 4u : 0x80000000u);
            if constexpr (ONE) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, dv), rall, vo,
                                                      int(uint32_t(min(q, nz - 1)) * pstride * 4u), 0);
            } else {
                const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
                    dog + size_t(min(q, nz - 1)) * pstride, 0, int(pstride * 4u), 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, dv), rd, vo, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);   // one load per step (hoisting them all held a rotation of VGPRs)
        }
    }
}

// min / max of the view by fminf / fmaxf (a NaN is skipped) plus a flag "some value is NaN or
// infinite".  Not k_dom_minmax's rule (dom.hip: Java's Math.min, which a NaN poisons), so
// the two stay separate kernels.
__global__ __launch_bounds__(kBlock) void k_minmax(const float* __restrict__ in, int64_t n,
                                                    float* __restrict__ partial) {
    __shared__ float smn[kBlock / 64], smx[kBlock / 64];
    __shared__ int sbad[kBlock / 64];
    float mn = INFINITY, mx = -INFINITY;
    float z = 0.0f;   // v * 0 summed: NaN once any value is NaN or infinite (finite: +-0)
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int64_t t0 = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(in) & 15u) == 0) {   // 16-B loads, then the tail
        const float4* in4 = reinterpret_cast<const float4*>(in);
        const int64_t n4 = n / 4;
        for (int64_t i = t0; i < n4; i += stride) {
            const float4 v = in4[i];
            mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
            mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
            z += (v.x * 0.0f + v.y * 0.0f) + (v.z * 0.0f + v.w * 0.0f);
        }
        for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
            mn = fminf(mn, in[i]);
            mx = fmaxf(mx, in[i]);
            z += in[i] * 0.0f;
        }
    } else {
        for (int64_t i = t0; i < n; i += stride) {
            const float v = in[i];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            z += v * 0.0f;
        }
    }
    int bad = isnan(z) ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        bad |= __shfl_xor(bad, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
        sbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            mn = fminf(mn, smn[w]);
            mx = fmaxf(mx, smx[w]);
            bad |= sbad[w];
        }
        partial[2 * blockIdx.x] = mn;
        partial[2 * blockIdx.x + 1] = mx;
        partial[2 * gridDim.x + blockIdx.x] = bad ? 1.0f : 0.0f;
    }
}

// min / max over the per-block partials: one wave, lane-strided then shuffles
// (min and max are order-independent, so the result equals a sequential scan)
// partial[2] = 1 when any value is NaN or infinite, else 0 (k_dog_xy's tap trim)
__global__ __launch_bounds__(64) void k_minmax_final(float* partial, int nb) {
    float mn = INFINITY, mx = -INFINITY, bad = 0.0f;
    for (int b = threadIdx.x; b < nb; b += 64) {
        mn = fminf(mn, partial[2 * b]);
        mx = fmaxf(mx, partial[2 * b + 1]);
        bad = fmaxf(bad, partial[2 * nb + b]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        bad = fmaxf(bad, __shfl_xor(bad, off, 64));
    }
    if (threadIdx.x == 0) {
        partial[0] = mn;
        partial[1] = mx;
        partial[2] = bad;
    }
}

// ---------------------------------------------------------------- host-side kernel math
// LaPlaceFunctions.computeK / computeKWeight / computeSigma / computeSigmaDiff
void dog_sigmas(float sigma, const double image_sigma[3], double s1[3], double s2[3], float* kinv) {
    const float k = float(std::pow(2.0, double(1.0f / 4.0f)));
    *kinv = 1.0f / (k - 1.0f);
    float steps[4];
    steps[0] = sigma;
    for (int i = 1; i <= 3; ++i) steps[i] = steps[i - 1] * k;
    for (int d = 0; d < 3; ++d) {
        const float isg = std::min(float(image_sigma[d]), sigma);
        auto diff = [&](float b) {
            const float dd = b * b - isg * isg;
            return float(std::sqrt(double(dd)));
        };
        s1[d] = diff(steps[0]);
        s2[d] = diff(steps[1]);
    }
}

// CUDASeparableConvolutionFunctions.getCUDAKernels: pad to the smallest supported size
int cuda_kernels(const double sig[3], std::vector<float> out[3]) {
    static const int sizes[5] = {7, 15, 31, 63, 127};
    std::vector<double> k[3];
    size_t longest = 0;
    for (int d = 0; d < 3; ++d) {
        k[d] = gaussian_kernel(sig[d]);
        longest = std::max(longest, k[d].size());
    }
    int size = -1;
    for (int s : sizes)
        if (longest <= size_t(s)) { size = s; break; }
    SD_CHECK(size > 0, SPIMDECON_ERR_ARG, "Gaussian kernel bigger than maximally supported size (127)");
    for (int d = 0; d < 3; ++d) {
        out[d].assign(size, 0.0f);
        const int s = (size - int(k[d].size())) / 2;
        for (size_t i = 0; i < k[d].size(); ++i) out[d][s + i] = float(k[d][i]);
    }
    return size;
}

// Compile-time dispatch of the fused kernels: with_taps(K, f, b...) calls
// f(integral_constant<int, K>, bool_constant<b>...) for the run-time K in {7, 15, 31} and bools.
template <bool... B, typename F>
void with_bools(F&& f) {
    f(std::bool_constant<B>{}...);
}
template <bool... B, typename F, typename... Bools>
void with_bools(F&& f, bool b, Bools... rest) {
    b ? with_bools<B..., true>(f, rest...) : with_bools<B..., false>(f, rest...);
}
template <typename F, typename... Bools>
void with_taps(int K, F&& f, Bools... bools) {
    with_bools([&](auto... c) {
        if (K == 7) f(std::integral_constant<int, 7>{}, c...);
        else if (K == 15) f(std::integral_constant<int, 15>{}, c...);
        else f(std::integral_constant<int, 31>{}, c...);
    }, bools...);
}

}  // namespace

// tuning knobs for A/B runs (tools/dog_bench.py); defaults are the measured best
int dog_env(const char* name, int def) {
    const char* v = std::getenv(name);
    return v && *v ? std::atoi(v) : def;
}

// oob: OOB_MIRROR (the reference's accurate mode) or OOB_BORDER (its approximate mode)
void dog_run(const float* img, const int64_t* dims, const spim_dog_params* p, int oob, float* dog_out, bool need_dog,
             hipStream_t s, DogWork& w, DogRun& r) {
    check_detector_args(img, dims, p, [] {});
    const bool border = oob == OOB_BORDER;   // (dog_oob gives no third mode)
    const Dims3 d{dims[0], dims[1], dims[2]};
    r.d = d;
    const int64_t n = d.nx * d.ny * d.nz;
    SD_CHECK(n < (int64_t(1) << 40), SPIMDECON_ERR_ARG, "volume too large");

    // ProcessDOG.java:61-105; DifferenceOfGaussianNewPeakFinder.getSimplePeaks level: candidates
    // with |v| >= threshold (localization 0) or threshold / 10 (localization 1)
    const float min_peak = p->localization == 0 ? p->threshold : p->threshold / 10.0f;
    double s1[3], s2[3];
    float kinv;
    dog_sigmas(p->sigma, p->image_sigma, s1, s2, &kinv);
    std::vector<float> k1[3], k2[3];
    const int K1 = cuda_kernels(s1, k1);
    const int K2 = cuda_kernels(s2, k2);
    const int K = std::max(K1, K2);
    auto pad_to = [](std::vector<float>& k, int K) {
        if (int(k.size()) == K) return;
        std::vector<float> o(K, 0.0f);
        const int off = (K - int(k.size())) / 2;
        std::copy(k.begin(), k.end(), o.begin() + off);
        k.swap(o);
    };
    std::vector<float> kall;
    for (int a = 0; a < 3; ++a) {
        pad_to(k1[a], K);
        pad_to(k2[a], K);
        kall.insert(kall.end(), k1[a].begin(), k1[a].end());
        kall.insert(kall.end(), k2[a].begin(), k2[a].end());
    }
    // the same taps interleaved per axis, (sigma1[j], sigma2[j]) pairs, for the fused kernels
    // (k_dog_z reads the z taps as a symmetric half)
    for (int j = 0; j < K; ++j)
        SD_CHECK(k1[2][j] == k1[2][K - 1 - j] && k2[2][j] == k2[2][K - 1 - j], SPIMDECON_ERR_STATE,
                 "asymmetric z taps");
    for (int a = 0; a < 3; ++a)
        for (int j = 0; j < K; ++j) {
            kall.push_back(k1[a][j]);
            kall.push_back(k2[a][j]);
        }
    grow(w.taps, kall.size());
    SD_HIP(hipMemcpyAsync(w.taps.p, kall.data(), kall.size() * 4, hipMemcpyHostToDevice, s));
    auto kp = [&](int axis, int which) { return w.taps.p + (2 * axis + which) * K; };
    auto kp2 = [&](int axis) { return reinterpret_cast<const float2*>(w.taps.p + 6 * K + 2 * axis * K); };
    // leading taps zero for both sigmas along an axis (k_dog_xy may skip them, see there)
    auto zero_lead = [&](int a) {
        int t = 0;
        while (t < K / 2 && k1[a][t] == 0.0f && k2[a][t] == 0.0f && k1[a][K - 1 - t] == 0.0f &&
               k2[a][K - 1 - t] == 0.0f)
            ++t;
        return t;
    };
    // (instantiated for 0 and 1 trimmed taps -- 1 at the default sigma 1.8; 2 spilled VGPRs)
    // (SPIMDECON_DOG_TRIM=0: every padded tap always)
    const int jt = dog_env("SPIMDECON_DOG_TRIM", 1) ? std::min(1, std::min(zero_lead(0), zero_lead(1))) : 0;

    const float* in = stage_in(img, n, p->device, w.in, s);
    grow(w.mm, 3 * 4096);
    const bool use_given = !(std::isnan(p->min_intensity) || std::isnan(p->max_intensity) ||
                             std::isinf(p->min_intensity) || std::isinf(p->max_intensity) ||
                             p->min_intensity == p->max_intensity);
    if (use_given) {
        // (mm[2] = 1: values not scanned, k_dog_xy keeps every padded tap)
        const float h2[3] = {float(p->min_intensity), float(p->max_intensity), 1.0f};
        SD_HIP(hipMemcpyAsync(w.mm.p, h2, 12, hipMemcpyHostToDevice, s));
    } else {
        const unsigned nb = grid_of(n);
        hipLaunchKernelGGL(k_minmax, dim3(nb), dim3(kBlock), 0, s, in, n, w.mm.p);
        hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(64), 0, s, w.mm.p, int(nb));
        SD_HIP(hipGetLastError());
    }
    // the DoG image is stored when the caller or the localisation needs it -- and below, when
    // the split z stage or the separate passes do
    ImageDest dst(dog_out, n, p->device);
    if (need_dog) dst.store(w.dog);
    const int T = p->ij_threads;
    const int wmin = p->find_min ? 1 : 0, wmax = p->find_max ? 1 : 0;
    // what the kernels' addressing forms need, each named once
    const bool img_4g = image_below_4gib(n);                 // the image (or the DoG): one buffer resource
    const bool img_2g = uint64_t(n) * 4u < 0x80000000ull;    // ... with the plane in the scalar offset
    const bool g12_4g = uint64_t(n) * 8u < 0xffffffffull;    // G12: one buffer resource
    // scalar plane indices: one mirror reflection (nz > K / 2) and a plane's G12 bytes in 31 bits
    const bool zscalar = d.nz > K / 2 && d.nx * d.ny * 8 < (int64_t(1) << 31);
    const bool fused = (K == 7 || K == 15 || K == 31) && n < (int64_t(1) << 32) && d.ny <= 65535 * 32 &&
                       d.nz <= 65535;
    // (chunk + 2 + KW - 1 source planes must fit k_dog_z's kDzMaxLen plane table)
    const int zc = std::min(kDzMaxLen - 128, kDzChunk);
    constexpr int ty = 32;     // strip steps (48-row tiles: 32 measured slower; strips: 32 beat 48, r05_dog_strips_ab.txt)
    constexpr int xcd = 1;     // XCD-contiguous y-fastest boxes of k_dog_z
    constexpr int xcd_xy = 1;  // XCD-contiguous tile ranges of k_dog_xy
    // k_dog_xy: persistent blocks (4 per CU at 32-row steps: 34.5 KB of LDS each), strips x
    // fastest
    const int64_t xy_strips = ceil_div(d.nx, kDxyTX) * d.nz;
    const dim3 gxy(unsigned(std::min<int64_t>(xy_strips, int64_t(256) * 4)));
    // k_dog_z box: 64 x 8 (512 threads); 64 x 16 and 32 x 16 measured slower (r3i)
    constexpr int bx = kDzBX, bz_y = 8;
    const dim3 gz(unsigned(std::max<int64_t>(1, ceil_div(d.nx - 2, bx - 2))),
                  unsigned(std::max<int64_t>(1, ceil_div(d.ny - 2, bz_y - 2))), unsigned(ceil_div(d.nz, zc)));
    // the split z stage (default): k_dog_zconv stores the DoG of every voxel, then k_dog_peaks
    // tests over the stored image (SPIMDECON_DOG_SPLIT=0: the fused k_dog_z); a candidate
    // overflow reruns the test pass only
    // (k_dog_zconv takes its plane indices the scalar way; k_dog_peaks needs the DoG below 4 GiB)
    const bool split = fused && dog_env("SPIMDECON_DOG_SPLIT", 1) != 0 && zscalar && img_4g;
    const int zc1 = std::max(1, dog_env("SPIMDECON_DOG_ZC_CHUNK", 256));
    if (split) dst.store(w.dog);
    if (fused) {
        grow(w.g12, size_t(n));
        // (k_minmax's own range: the per-value range check is skipped; SPIMDECON_DOG_MM_EXACT=0
        // keeps it -- 1.52-1.62 vs 1.66 ms per 768^3, bit-exact)
        const int mmx = !use_given && dog_env("SPIMDECON_DOG_MM_EXACT", 1) != 0 ? 1 : 0;
        with_taps(K, [&](auto kw, auto buf, auto trim, auto bord) {
            hipLaunchKernelGGL((k_dog_xy<kw(), ty, buf(), trim() ? 1 : 0, bord()>), gxy, dim3(256), 0, s, d, in, kp2(0),
                               kp2(1), w.g12.p, w.mm.p, xcd_xy, mmx);
        }, img_4g, jt == 1, border);
        SD_HIP(hipGetLastError());
        if (split) {
            const int64_t waves = ceil_div(d.nx, int64_t(64)) * d.ny;
            const dim3 gc(unsigned(ceil_div(waves, int64_t(4))), unsigned(ceil_div(d.nz, int64_t(zc1))));
            // (ONE only with ONEG -- a DoG below 2 GiB has its G12 below 4 GiB: three combinations)
            with_taps(K, [&](auto kw, auto one, auto oneg, auto bord) {
                hipLaunchKernelGGL((k_dog_zconv<kw(), kDzcPD, one() && oneg(), oneg(), bord()>), gc, dim3(256), 0, s, d,
                                   w.g12.p, kp2(2), kinv, zc1, dst.p);
            }, img_2g, g12_4g, border);
            SD_HIP(hipGetLastError());
        }
    } else {
        // Gaussians of 63 / 127 taps: the separate passes, then a candidate pass over the DoG
        grow(w.tmp_a, size_t(n));
        grow(w.tmp_b, size_t(n));
        grow(w.tmp_c, size_t(n));
        grow(w.tmp_d, size_t(n));
        dst.store(w.dog);
        sep_pass(d, 0, in, in, kp(0, 0), kp(0, 1), K, oob, 0.f, w.tmp_a.p, w.tmp_b.p, false, 0.f, w.mm.p, s);
        sep_pass(d, 1, w.tmp_a.p, w.tmp_b.p, kp(1, 0), kp(1, 1), K, oob, 0.f, w.tmp_c.p, w.tmp_d.p, false,
                 0.f, nullptr, s);
        sep_pass(d, 2, w.tmp_c.p, w.tmp_d.p, kp(2, 0), kp(2, 1), K, oob, 0.f, dst.p, nullptr, true, kinv,
                 nullptr, s);
    }
    // a candidate overflow reruns the pass with the DoG already stored
    const unsigned total = collect_candidates(w, n, min_peak, wmin, wmax, T, s, [&](const PeakSink& pk, int attempt) {
        if (split) {
            stored_candidates(w, d, dst.p, true, pk, s);
        } else if (fused) {
            float* store = need_dog && attempt == 0 ? dst.p : nullptr;
            grow(w.sink, 1);
            SD_HIP(hipMemcpyAsync(w.sink.p, &pk, sizeof(pk), hipMemcpyHostToDevice, s));   // (synchronised below)
            const int want = wmin | (wmax << 1);
            with_taps(K, [&](auto kw, auto one, auto sl, auto bord) {
                hipLaunchKernelGGL((k_dog_z<kw(), bz_y, kDzPD, bx, one(), sl(), bord()>), gz, dim3(bx * bz_y), 0, s, d,
                                   w.g12.p, kp2(2), kinv, zc, store, min_peak, want, w.sink.p, xcd);
            }, img_2g, zscalar, border);
        } else {
            stored_candidates(w, d, dst.p, false, pk, s);
        }
    });
    r.dog = dst.p;
    sort_candidates(w, total, T, s, r);
    dst.copy_out(s);
}

// SPIM_DOG_EXTEND_* (the C ABI's `extension` argument) -> the kernels' mode
int dog_oob(int32_t extension) {
    SD_CHECK(extension == SPIM_DOG_EXTEND_MIRROR || extension == SPIM_DOG_EXTEND_BORDER, SPIMDECON_ERR_ARG,
             "extension must be SPIM_DOG_EXTEND_MIRROR (0) or SPIM_DOG_EXTEND_BORDER (1)");
    return extension == SPIM_DOG_EXTEND_BORDER ? OOB_BORDER : OOB_MIRROR;
}

void dog_compute(const float* img, const int64_t* dims, const spim_dog_params* p, int32_t extension, float* dog_out,
                 spim_peak* peaks, int64_t max_peaks, int64_t* npeaks) {
    SD_CHECK(npeaks && p, SPIMDECON_ERR_ARG, "null argument");
    const int oob = dog_oob(extension);
    with_work<DogWork>(p->device, [&](DogWork& w, hipStream_t s) {
        DogRun r;
        dog_run(img, dims, p, oob, dog_out, dog_out != nullptr, s, w, r);
        peaks_to_host(r, peaks, max_peaks, npeaks, s);
    });
}

// ProcessDOG.compute's result: interest points after Localization (:150-168).
void dog_interest_points(const float* img, const int64_t* dims, const spim_dog_params* p, int32_t extension,
                         float* dog_out, spim_interest_point* out, int64_t max_out, int64_t* nout) {
    SD_CHECK(nout && p, SPIMDECON_ERR_ARG, "null argument");
    const int oob = dog_oob(extension);
    with_work<DogWork>(p->device, [&](DogWork& w, hipStream_t s) {
        DogRun r;
        dog_run(img, dims, p, oob, dog_out, p->localization == 1 || dog_out != nullptr, s, w, r);
        points_from_peaks(w, r, p->localization, float(p->threshold), out, max_out, nout, s);
    });
}

}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" void spim_dog_params_default(spim_dog_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->sigma = 1.8f;
    p->threshold = 0.008f;
    p->localization = 0;
    p->image_sigma[0] = p->image_sigma[1] = p->image_sigma[2] = 0.5;
    p->find_min = 0;
    p->find_max = 1;
    p->min_intensity = std::nan("");
    p->max_intensity = std::nan("");
    p->ij_threads = 8;
    p->device = 0;
}

extern "C" int spim_dog_interest_points(const float* img, const int64_t* dims, const spim_dog_params* p,
                                        float* dog_out, spim_interest_point* out, int64_t max_out,
                                        int64_t* nout) {
    return spim_dog_interest_points_ext(img, dims, p, SPIM_DOG_EXTEND_MIRROR, dog_out, out, max_out, nout);
}

extern "C" int spim_dog_interest_points_ext(const float* img, const int64_t* dims, const spim_dog_params* p,
                                            int32_t extension, float* dog_out, spim_interest_point* out,
                                            int64_t max_out, int64_t* nout) {
    return guarded([&] { dog_interest_points(img, dims, p, extension, dog_out, out, max_out, nout); });
}

extern "C" int spim_dog_compute(const float* img, const int64_t* dims, const spim_dog_params* p,
                                float* dog_out, spim_peak* peaks, int64_t max_peaks,
                                int64_t* npeaks) {
    return spim_dog_compute_ext(img, dims, p, SPIM_DOG_EXTEND_MIRROR, dog_out, peaks, max_peaks, npeaks);
}

extern "C" int spim_dog_compute_ext(const float* img, const int64_t* dims, const spim_dog_params* p,
                                    int32_t extension, float* dog_out, spim_peak* peaks, int64_t max_peaks,
                                    int64_t* npeaks) {
    return guarded([&] { dog_compute(img, dims, p, extension, dog_out, peaks, max_peaks, npeaks); });
}
