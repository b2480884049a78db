// fftconv_xt.inc -- x (row) pass as tiles of 8 or 16 packed row pairs (two-factor lengths).
// Included by fftconv.hip inside namespace spimdecon::{anonymous}, after fftconv_x.inc.
//
// PMC showed the per-wave x passes VALU-bound: one 540-point transform per wave
// leaves 37-63 % of the lanes idle in every DFT phase (k_xrows two-factor) or pays
// integer division per Stockham butterfly.  Here a block of 512 threads owns 16
// row pairs at once, exactly like the column passes own 16 columns:
//   load    TR threads per pair (32, or 64 for factors > 32): 16-B buffer loads of both half-spectrum rows,
//           Hermitian extension written to Z[c][x] (LDS pitch L+1, odd)
//   inverse thread (c, r): N1-point DFT over Z[c][N2*n1 + r], twiddle, in place;
//           then N2-point DFTs over Z[c][r*N2 + n2] -> Z[c][r + N1*k2]
//   RL step TR threads per pair, 4 voxels per lane per step (quotient | update)
//   forward same two phases
//   store   unpack to the two half spectra, 16-B buffer stores; a row that must not
//           be written gets an out-of-range offset and the range check drops it.
// LDS = NP * (L + 2) float2 + twiddles (xt_lds); 4 waves per SIMD at L = 540.

// LDS pitch (float2) of a row pair in the tile: even, so rows stay 16-B aligned for
// the b128 load / RL / store steps.  L + 2 keeps the DFT phases' b64 stores (16-lane
// groups, banks mod 32) conflict-free: c*P*2 mod 32 is distinct for the 8 row pairs c
// of a lane group.  Measured (PMC SQ_LDS_BANK_CONFLICT, 540): P = 540 -- better for the
// b64 reads alone -- raised the conflict cycles 4x (1.2e7 -> 5.1e7 quotient, 4.2e7 ->
// 7.8e7 update); tools/lds_bank_model.py models both access kinds.
// A pitch of 2 mod 4 for every length: L + 4 at 1050 (the only table length with L + 2
// = 0 mod 4), whose DFT phases' b64 writes are 2-way conflicted at 1052 (tools/
// lds_bank_model.py: -20 % LDS cycles).  Measured on C3 (1050-point tiles, same box):
// quotient 1.914 -> 1.796 ms, update 2.986 -> 2.925 ms (profiles/r04_pitch_1050.txt).
// SD_XT_PITCH4=0 restores L + 2 (A/B builds).
#ifndef SD_XT_VB_TIK64
#define SD_XT_VB_TIK64 2
#endif
#ifndef SD_XT_VB_TIK32
#define SD_XT_VB_TIK32 2
#endif
// x tiles in descending row order: the y-inverse pass before them writes its planes in
// ascending z, so the rows it wrote last -- still in the 256-MB Infinity Cache -- are read
// first (ascending, they came last, after the tile's own traffic had evicted them); the x
// pass in turn leaves the low planes hot for the ascending forward y pass.  540: quotient
// 0.393 -> 0.378 ms, update 0.504-0.527 -> 0.499-0.506 ms, headline +1.1..1.7 %, default mode
// +0.5..0.8 %; C3 (1050) neutral (profiles/r06_xtile_rev_ab.txt).  SD_XT_REV=0: ascending.
#ifndef SD_XT_REV
#define SD_XT_REV 1
#endif
#ifndef SD_XT_VB_WAVE
#define SD_XT_VB_WAVE 0
#endif
#ifndef SD_XT_PITCH4
#define SD_XT_PITCH4 1
#endif
#ifndef SD_XT_AMAP
#define SD_XT_AMAP 1
#endif
// Lane map of the DFT phases (xt_fft): AM low lane bits carry r, the next log2(NP) carry
// the row pair c, the rest r again (AM = 0: c = t % NP, r = t / NP; a wave still covers
// the same 8 values of r).  tools/lds_xtile_model.py --remap: with AM = 2 a b64 read's
// 32-lane group spans 4 r x 8 c and a b64 write's 16-lane group 4 r x 4 c, which the
// pitch makes conflict-free in both directions at 1050 (pitch L + 2; modeled conflict
// cycles per wave 178 -> 49).  Measured (profiles/r04_xtile_amap_ab.txt, same box):
// 1050 quotient 1.749 -> 1.734 ms, update 2.501 -> 2.480 ms; 540 (pitch L + 8, modeled
// 188 -> 50) within noise; 800 (L + 4, 462 -> 362) slower (quotient 1.377 -> 1.424 ms).
// So AM = 2 at 1050 only.  SD_XT_AMAP=0 restores AM = 0 there (A/B builds).
// The 4-pair update tiles (xt_np) kept AM = 0 at first: 1.5e8 bank-conflict cycles per 1050
// launch against 1.7e7 for 8 pairs (profiles/r05_pmc_1050_np4.md); the model's best maps
// for 4 pairs are AM = 3 at pitch L + 14 (1050: 572 -> 49 cycles per wave) and AM = 3 at
// pitch L + 8 (800: 1438 -> 746).
__host__ __device__ constexpr int xt_amap(int L, int NP) {
    return !SD_XT_AMAP ? 0 : NP == 8 && L == 1050 ? 2 : NP == 4 && (L == 1050 || L == 800) ? 3 : 0;
}
__host__ __device__ constexpr int xt_pitch(int L, int NP) {
    return xt_amap(L, NP) == 2 ? L + 2
         : xt_amap(L, NP) == 3 ? L + (L == 1050 ? 14 : 8)
         : L + 2 + (SD_XT_PITCH4 && (L + 2) % 4 == 0 ? 2 : 0);
}

// LDS bytes of a block: NP row pairs, plus the L-entry twiddle table unless the
// phase-A twiddles are read from global memory (L1/L2 resident, 6.4 KB at L = 800).
// The table stays in LDS unless leaving it out fits one more block per CU: L = 800
// tiles take 57.7 KB with it (2 blocks, 2 waves per SIMD) and 51.3 KB without (3).
__host__ __device__ constexpr size_t xt_lds(int L, int NP, bool twg) {
    return size_t((twg ? 0 : L + 2) + NP * xt_pitch(L, NP)) * 8u;
}
__host__ __device__ constexpr bool xt_twg(int L, int NP) {
    return 163840 / xt_lds(L, NP, true) > 163840 / xt_lds(L, NP, false);
}
// Diagnostic build only (-DSD_XT_STAMPS=1, tools/build_variant.sh): per-phase s_memtime
// stamps of one tile in 64, summed per MODE into g_xt_stamp (a buffer nothing else reads)
// and printed by launch_xtile; never quote that build's run time, only its shares.
#ifndef SD_XT_STAMPS
#define SD_XT_STAMPS 0
#endif
#if SD_XT_STAMPS
__device__ unsigned long long g_xt_stamp[3][8];
#define XT_STAMP(i)                                                                              \
    do {                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        unsigned long long t_;                                                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        xts[i] = t_;                                                                             \
    } while (0)
#else
#define XT_STAMP(i) do {} while (0)
#endif

// wave tiles: one wave per block owning 64 / TR row pairs (1 at TR = 64, 2 at TR = 32), so
// no block barrier couples waves and each CU's resident waves sit at different phases
// (the loads and stores of some under the transforms of others).  SD_XT_WAVE: bit mask of
// the lengths that use them (1: 2100, 2: 1050, 4: 800, 8: 540).  Measured (same box, C5
// rank slab, padded 2100 x 1050 x 280 fp16, profiles/r06_xtile_wave_ab.txt): quotient
// 2.35 -> 1.95 ms, update 3.11 -> 2.84 ms, C5 rank 8,015 -> 8,494 Mvox/s against the
// persistent 8-pair tiles (one 151-KB block per CU, 2 waves per SIMD: every HBM phase of a
// tile serialised behind its block barriers); at 1050 (C3) slower, quotient 1.67 -> 1.83 ms
// (two 8-wave blocks per CU already overlap each other there)
#ifndef SD_XT_WAVE
#define SD_XT_WAVE 1
#endif
#ifndef SD_XT_WAVE_W
#define SD_XT_WAVE_W 2   // launch bound of the wave tiles: waves per SIMD
#endif
// fp16 quotient wave tiles: the image rows are loaded with the spectra, before the inverse
// transform (170 VGPRs, 8 waves per CU where the LDS allows 9): C5 quotient 1.95 -> 1.77 ms
#ifndef SD_XT_WAVE_QPF
#define SD_XT_WAVE_QPF 1
#endif
__host__ __device__ constexpr bool xt_wave(int L) {
    return (L == 2100 && (SD_XT_WAVE & 1)) || (L == 1050 && (SD_XT_WAVE & 2)) || (L == 800 && (SD_XT_WAVE & 4)) ||
           (L == 540 && (SD_XT_WAVE & 8));
}

// Block barrier for LDS data only: __syncthreads() also waits for every outstanding
// global load (its release fence), which would drain the voxel loads the quotient
// tile issues before its inverse transform.
__device__ __forceinline__ void xt_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// component-wise select (a select of whole float4 values became a private-memory
// copy indexed by the condition)
__device__ __forceinline__ float4 sel4(int c, float4 a, float4 b) {
    return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// twiddle table read through a buffer resource (the xt_twg tiles)
struct XtTwGlobal {
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ float2 operator[](int i) const {
        return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r, i * 8, 0, 0));
    }
};

// NP row pairs per block (NP*TR threads): 8 (measured best against 4 and 16 at 540), but 4
// for the update tiles at 1050 and 800 -- four blocks of 4 waves per CU instead of two of 8
// (1050: update 2.455 -> 2.365 ms, C3 +0.6 %; 800: 1.91 -> 1.89 ms), not for their
// quotients (1050: 1.68 -> 1.90 ms) nor at 2100 (C5 rank -9 %): profiles/r05_xtile_np4_ab.txt
__host__ __device__ constexpr int xt_np(int mode, int L) {
    return xt_wave(L) ? (L == 1050 || L == 2100 ? 1 : 2)   // one wave: 64 / TR pairs (TR = SD_2F_TR)
         : mode == XM_UPDATE && (L == 1050 || L == 800) ? 4 : 8;
}
constexpr int kXtVB = 4;  // voxel float4 per lane per batch in the update step (rows longer than 5)

// Lane map of the DFT phases (see xt_amap): row pair c and residue r of thread t.
template <int L, int NP>
__device__ __forceinline__ void xt_cr(int t, int& c, int& r) {
    int tt = t;
    asm volatile("" : "+v"(tt));  // keep the per-thread LDS addresses inside the caller's loop
    constexpr int AM = xt_amap(L, NP);   // (NP a power of two when AM > 0)
    constexpr int LNP = NP == 8 ? 3 : NP == 4 ? 2 : 0;
    static_assert(AM == 0 || (1 << LNP) == NP, "lane map for 4 or 8 row pairs");
    c = AM ? (tt >> AM) & (NP - 1) : tt % NP;
    r = AM ? (tt & ((1 << AM) - 1)) | ((tt >> (AM + LNP)) << AM) : tt / NP;
}

// Phase A of an L = N1*N2 transform over the NP rows Z[c][.] (pitch P), in place:
// thread (c, r < N2) takes the residue class x = N2*n1 + r, an N1-point register DFT,
// twiddle W_L^(r*k1) (conjugate when INV), back to Z[c][k1*N2 + r].  Barrier after.
template <int N1, int N2, bool INV, int NP, typename TW>
__device__ __forceinline__ void xt_phaseA(float2* Z, TW tw, int P, int t) {
    int c, r;
    xt_cr<N1 * N2, NP>(t, c, r);
    float2* row = Z + c * P;
    if (r < N2) {  // read and written by this thread only
        float2 v[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) v[n1] = row[N2 * n1 + r];
        fft_reg<N1, INV>(v);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k1 = 0; k1 < N1; ++k1) {
            float2 w = tw[r * k1];
            if (INV) w.y = -w.y;
            row[k1 * N2 + r] = k1 == 0 ? v[0] : cmul(v[k1], w);
        }
    }
    xt_barrier();
}

// Phase B: thread (c, r < N1) takes the contiguous Z[c][r*N2 + n2], an N2-point DFT,
// and writes X[r + N1*k2] (natural order).  Barriers between the reads and the writes
// and after the writes.
template <int N1, int N2, bool INV, int NP>
__device__ __forceinline__ void xt_phaseB(float2* Z, int P, int t) {
    int c, r;
    xt_cr<N1 * N2, NP>(t, c, r);
    float2* row = Z + c * P;
    float2 u[N2];
    if (r < N1) {
#pragma unroll
        for (int n2 = 0; n2 < N2; ++n2) u[n2] = row[r * N2 + n2];
    }
    xt_barrier();  // every phase-B read is done before any phase-B write
    if (r < N1) {
        fft_reg<N2, INV>(u);
#pragma unroll
        for (int k2 = 0; k2 < N2; ++k2) row[r + N1 * k2] = u[k2];
    }
    xt_barrier();
}

// N1-point DFTs (phase A) then N2-point DFTs (phase B) of the NP rows Z[c][.]
// (pitch P) in place; natural order in and out.  Block-wide barriers inside.
template <int N1, int N2, bool INV, int NP, typename TW>
__device__ __forceinline__ void xt_fft(float2* Z, TW tw, int P, int t) {
    xt_phaseA<N1, N2, INV, NP>(Z, tw, P, t);
    xt_phaseB<N1, N2, INV, NP>(Z, P, t);
}

// 4 voxels of an f32 / f16 volume as loaded (f16: kept packed until used -- half the
// registers of a prefetch held across a transform)
template <int S>
using vraw4 = typename std::conditional<S == 0, float4, uint2>::type;
template <int S>
__device__ __forceinline__ vraw4<S> bloadraw4(__amdgpu_buffer_rsrc_t r, uint32_t vox) {
    if constexpr (S == 0) return bload4(r, vox * 4u);
    else return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(r, int(vox * 2u), 0, 0));
}
template <int S>
__device__ __forceinline__ float4 cvt4(const vraw4<S>& u) {
    if constexpr (S == 0) {
        return u;
    } else {
        const float2 lo = __half22float2(__builtin_bit_cast(__half2, u.x));
        const float2 hi = __half22float2(__builtin_bit_cast(__half2, u.y));
        return make_float4(lo.x, lo.y, hi.x, hi.y);
    }
}


// One tile of NP row pairs per block.  (Round 5's persistent 2100 tiles -- the resident
// blocks striding over the tiles with the next tile's spectra prefetched into registers, and
// a two-slot voxel pipeline -- were replaced by the wave tiles (xt_wave) in round 6 and
// removed: profiles/r06_xtile_wave_ab.txt.)
template <int MODE, int S, int N1, int N2, bool TIK, int NP, int TR>
__global__ __launch_bounds__(NP * TR, (NP * TR == 64 && N1 * N2 > 1204) ? SD_XT_WAVE_W : N1 * N2 > 1204 ? 2 : 4)
void k_xtile(XArgs a) {
    static_assert(N1 <= TR && N2 <= TR, "factor exceeds the threads per row pair");
    constexpr int kXtThreads = NP * TR;
    static_assert(MODE == XM_QUOT || MODE == XM_UPDATE || MODE == XM_PSI, "quotient / update / psi rows only");
    constexpr int L = N1 * N2;
    // even pitch: rows 16-B aligned for the b128 accesses of the load / RL / store
    // steps; a phase-A access (16 lanes = 16 rows c, same r) still hits distinct banks
    static_assert(L % 2 == 0, "even lengths only");
    constexpr int P = xt_pitch(L, NP);
    constexpr int cHx = L / 2 + 1;
    constexpr int cHp2 = (cHx + 15) / 16 * 8;     // float4 (2 complex) per padded spectrum row
    constexpr int KS = (cHp2 + TR - 1) / TR;      // float4 per lane per spectrum row
    constexpr int KV = (L / 4 + TR - 1) / TR;     // float4 per lane per voxel row (nx <= L)
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    constexpr bool TWG = xt_twg(L, NP);
    float2* tw = smem;                       // [L] (unless TWG)
    float2* Z = TWG ? smem : smem + L + 2;   // [NP][P]  (16-B aligned rows)
    const XtTwGlobal twg{brsrc(a.fx.tw, uint32_t(L) * 8u)};
    const SlabGeom& g = a.g;
    constexpr int Hx = cHx;
    constexpr int Hp = cHp2 * 2;
    constexpr int Hp2 = cHp2;
    const int nx = int(g.nx);
    const int nx4 = nx / 4;
    const int ny = int(g.ny);
    const int My = int(g.My);
    const int cx = g.cx;
    const int t0 = threadIdx.x;
#if SD_XT_STAMPS
    unsigned long long xt_entry;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(xt_entry)::"memory");
#endif
    if constexpr (!TWG)
        for (int i = t0; i < L; i += kXtThreads) tw[i] = a.fx.tw[i];
    const int nrows = int(g.My * g.Mz);
    const int nlin = a.pn0 + a.pn1;  // launch-linear pair indices, mapped by x_pair
    const int ntiles = (nlin + NP - 1) / NP;
    const __amdgpu_buffer_rsrc_t rcin = brsrc(a.Cin, a.spec_bytes);
    const __amdgpu_buffer_rsrc_t rcout = brsrc(a.Cout, a.Cout ? a.spec_bytes : 0u);
    const __amdgpu_buffer_rsrc_t rpsi = brsrc(a.psi_in, a.nvox * 4u);
    const __amdgpu_buffer_rsrc_t rpo = brsrc(a.psi_out, a.nvox * 4u);
    const __amdgpu_buffer_rsrc_t rimg = brsrc(MODE == XM_QUOT ? a.img : a.w, a.nvox * (S == 0 ? 4u : 2u));
    double ssum = 0.0;
    float smax = -1.0f;
    const double inv_lambda = TIK ? 1.0 / a.lambda : 0.0;  // (next_value_t)
    __syncthreads();
#if SD_XT_STAMPS
    unsigned long long xts[8] = {0, 0, 0, 0, 0, 0, xt_entry, 0};
    bool xt_first = true;
#endif
    // the half-spectrum rows a tile T needs (previous convolution's result), 16-B loads
    // into xa / xb; a tile past the last reads zeros (out-of-range offsets)
    auto spec_issue = [&](int T, float4 (&xa)[KS], float4 (&xb)[KS]) {
        int tq = t0;
        asm volatile("" : "+v"(tq));
        const int c = tq / TR;
        const int hl = tq % TR;
        const int pr = T < ntiles ? x_pair(a, T * NP + c) : -1;
        const int r0 = pr >= 0 ? 2 * pr : nrows, r1 = r0 + 1;
        const bool v0 = r0 < nrows, v1 = r1 < nrows;
        int q0, q1;  // padded rows holding the needed convolution results
        if constexpr (MODE == XM_QUOT) {
            q0 = v0 && a.row_one[r0] >= 0 ? r0 : -1;
            q1 = v1 && a.row_one[r1] >= 0 ? r1 : -1;
        } else {
            const int sm0 = v0 ? a.row_mirror[r0] : -1, sm1 = v1 ? a.row_mirror[r1] : -1;
            q0 = sm0 >= 0 ? (sm0 / ny) * My + sm0 % ny : -1;
            q1 = sm1 >= 0 ? (sm1 / ny) * My + sm1 % ny : -1;
        }
        const uint32_t o0 = q0 >= 0 ? uint32_t(q0) * uint32_t(Hp) * 8u : kOOB;
        const uint32_t o1 = q1 >= 0 ? uint32_t(q1) * uint32_t(Hp) * 8u : kOOB;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const uint32_t jo = uint32_t(min(hl + TR * i, Hp2 - 1)) * 16u;
            xa[i] = bload4(rcin, o0 + jo);
            xb[i] = bload4(rcin, o1 + jo);
        }
    };
    for (int tile_ = blockIdx.x; tile_ < ntiles; tile_ += gridDim.x) {   // (one iteration: see the end)
        const int tile = SD_XT_REV ? ntiles - 1 - tile_ : tile_;
        XT_STAMP(0);
        // The row pair of this thread in the load / RL / store steps and its row-map
        // entries, re-derived in each step behind an opaque asm (cheap, cached
        // loads) instead of being held across the transforms.
#define SD_XT_ROWS                                                                   \
    int tt_ = t0;                                                                    \
    asm volatile("" : "+v"(tt_));                                                    \
    const int c = tt_ / TR;                                                          \
    const int hl = tt_ % TR;                                                         \
    float2* zr = Z + c * P;                                                          \
    /* b128 slot order of the RL step: lanes l, l^4 and l^8 take the two 16-B halves */ \
    /* of their 32-B voxel quad in opposite order -- conflict-free 16-lane b128 reads */ \
    /* and 8-lane b128 writes (MI355X_MICROARCH.md LDS groups) */                      \
    const int sw = ((hl >> 2) ^ (hl >> 3)) & 1;                                      \
    const int pr_ = x_pair(a, tile * NP + c);                                        \
    const int r0 = pr_ >= 0 ? 2 * pr_ : nrows, r1 = r0 + 1;                          \
    const bool v0 = r0 < nrows, v1 = r1 < nrows;                                     \
    const int sm0 = v0 ? a.row_mirror[r0] : -1, sm1 = v1 ? a.row_mirror[r1] : -1;   \
    const int so0 = v0 ? a.row_one[r0] : -1, so1 = v1 ? a.row_one[r1] : -1;         \
    (void)so0; (void)so1; (void)sm0; (void)sm1; (void)sw;
        // quotient: the image rows are loaded with the spectra, before the inverse
        // transform, so they arrive while it computes
        // (rows of up to 5 float4 per lane: longer ones would spill under 128 VGPRs; up to 7
        // at L = 800 under occupancy-aware launch bounds measured slower,
        // profiles/r04_xtile_qpf7_ab.txt; under round 5's persistent 2100 tiles equal or slower,
        // r05_xtile_variants_ab.txt.  At 1050 (64 threads per pair) it measured slower while the
        // tile spilled SGPRs, and 1.74 -> 1.68 ms once the tile-loop removal had removed the
        // spills, C3 +0.5 %: r05_xtile_c3_ab.txt)
        constexpr bool QPF = MODE == XM_QUOT && (KV <= 5 || (SD_XT_WAVE_QPF && NP * TR == 64 && S == 1 && KV <= 9));
        vraw4<S> ia[MODE == XM_QUOT ? KV : 1], ib[MODE == XM_QUOT ? KV : 1];
        // (the update tile gained nothing from loading its psi rows early: 0.526 vs 0.514 ms at
        // 540; the fp16 2100 wave tiles: 240 VGPRs, update 2.84 -> 2.98 ms, r06_xtile_wave_ab.txt)
        if constexpr (MODE != XM_PSI) {  // XM_PSI starts from psi itself: no spectra, no inverse
        // ---- load: previous convolution's half spectra -> Hermitian-extended row pair
        {
            SD_XT_ROWS
            float4 sa[KS], sb[KS];  // all loads in flight before the first use
            spec_issue(tile, sa, sb);
            if constexpr (QPF) {
                const uint32_t b0 = so0 >= 0 ? uint32_t(so0) * uint32_t(nx) : kOOBV;
                const uint32_t b1 = so1 >= 0 ? uint32_t(so1) * uint32_t(nx) : kOOBV;
#pragma unroll
                for (int i = 0; i < KV; ++i) {
                    const uint32_t jo = uint32_t(min(hl + TR * i, nx4 - 1)) * 4u;
                    ia[i] = bloadraw4<S>(rimg, b0 + jo);
                    ib[i] = bloadraw4<S>(rimg, b1 + jo);
                }
            }
#pragma unroll
            for (int i = 0; i < KS; ++i) {
                const int j = hl + TR * i;
                if (j >= Hp2) break;
                const float4 s0 = sa[i], s1 = sb[i];
                float2 zo[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = 2 * j + h;
                    float2 xa = h ? make_float2(s0.z, s0.w) : make_float2(s0.x, s0.y);
                    float2 xb = h ? make_float2(s1.z, s1.w) : make_float2(s1.x, s1.y);
                    if (k == 0 || 2 * k == L) {
                        xa.y = 0.f;
                        xb.y = 0.f;
                    }
                    zo[h] = make_float2(xa.x - xb.y, xa.y + xb.x);
                    if (k < Hx && k > 0 && 2 * k < L) zr[L - k] = make_float2(xa.x + xb.y, xb.x - xa.y);
                }
                // k = 2j, 2j + 1 in one b128 write; a pair straddling Hx writes k = 2j only
                // (slot Hx = L/2 + 1 holds the mirror of k = L/2 - 1)
                if (2 * j + 1 < Hx) *reinterpret_cast<float4*>(zr + 2 * j) = make_float4(zo[0].x, zo[0].y, zo[1].x, zo[1].y);
                else if (2 * j < Hx) zr[2 * j] = zo[0];
            }
        }
        xt_barrier();
        XT_STAMP(1);
        if constexpr (TWG) xt_fft<N1, N2, true, NP>(Z, twg, P, t0);
        else xt_fft<N1, N2, true, NP>(Z, (const float2*)tw, P, t0);
        XT_STAMP(2);
        }
        // ---- RL step on the real row pair zr[x] = (row r0, row r1)
        {
        SD_XT_ROWS
        if constexpr (MODE == XM_PSI) {
            // x spectra of the mirror-extended psi (once per mvd_run; the update tiles
            // produce them afterwards): psi rows of the mirror map, then the extension
            const uint32_t b0 = sm0 >= 0 ? uint32_t(sm0) * uint32_t(nx) : kOOBV;
            const uint32_t b1 = sm1 >= 0 ? uint32_t(sm1) * uint32_t(nx) : kOOBV;
            float4 pa[KV], pb[KV];
#pragma unroll
            for (int i = 0; i < KV; ++i) {
                const uint32_t jo = uint32_t(min(hl + TR * i, nx4 - 1)) * 4u;
                pa[i] = bload4(rpsi, (b0 + jo) * 4u);
                pb[i] = bload4(rpsi, (b1 + jo) * 4u);
            }
#pragma unroll
            for (int i = 0; i < KV; ++i) {
                const int j = hl + TR * i;
                if (j >= nx4) break;
                float4* zq = reinterpret_cast<float4*>(zr + 4 * j);
                const float4 p0 = pa[i], p1 = pb[i];
                const float4 o01 = make_float4(p0.x, p1.x, p0.y, p1.y), o23 = make_float4(p0.z, p1.z, p0.w, p1.w);
                zq[sw] = sel4(sw, o23, o01);
                zq[sw ^ 1] = sel4(sw, o01, o23);
            }
            xt_barrier();
            for (int qx = nx + hl; qx < L; qx += TR) {
                const int sx = qx < nx + cx ? qx : qx - L;
                zr[qx] = zr[mirror_idx(sx, nx)];
            }
        } else if constexpr (MODE == XM_QUOT) {
            const float one0 = sm0 != -1 ? 1.0f : 0.0f;  // constant-1 extension (0: exchanged halo)
            const float one1 = v1 && sm1 != -1 ? 1.0f : 0.0f;
            if constexpr (!QPF) {
                const uint32_t b0 = so0 >= 0 ? uint32_t(so0) * uint32_t(nx) : kOOBV;
                const uint32_t b1 = so1 >= 0 ? uint32_t(so1) * uint32_t(nx) : kOOBV;
#pragma unroll
                for (int i = 0; i < KV; ++i) {
                    const uint32_t jo = uint32_t(min(hl + TR * i, nx4 - 1)) * 4u;
                    ia[i] = bloadraw4<S>(rimg, b0 + jo);
                    ib[i] = bloadraw4<S>(rimg, b1 + jo);
                }
            }
#pragma unroll
            for (int i = 0; i < KV; ++i) {
                const int j = hl + TR * i;
                if (j >= nx4) break;
                const float4 i0 = cvt4<S>(ia[i]), i1 = cvt4<S>(ib[i]);
                float4* zq = reinterpret_cast<float4*>(zr + 4 * j);  // 4 voxels = 2 b128
                const float4 za = zq[sw], zb = zq[sw ^ 1];
                const float4 z01 = sel4(sw, zb, za), z23 = sel4(sw, za, zb);
                float qa[4], qb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 bz = e == 0 ? make_float2(z01.x, z01.y) : e == 1 ? make_float2(z01.z, z01.w)
                                    : e == 2 ? make_float2(z23.x, z23.y) : make_float2(z23.z, z23.w);
                    const float a0 = f4c(i0, e), a1 = f4c(i1, e);
                    qa[e] = (so0 >= 0 && a0 > 0.0f) ? __fdiv_rn(a0, bz.x) : one0;
                    qb[e] = (so1 >= 0 && a1 > 0.0f) ? __fdiv_rn(a1, bz.y) : one1;
                }
                const float4 o01 = make_float4(qa[0], qb[0], qa[1], qb[1]), o23 = make_float4(qa[2], qb[2], qa[3], qb[3]);
                zq[sw] = sel4(sw, o23, o01);
                zq[sw ^ 1] = sel4(sw, o01, o23);
            }
            for (int qx = nx + hl; qx < L; qx += TR) zr[qx] = make_float2(one0, one1);
        } else {
            const uint32_t b0 = sm0 >= 0 ? uint32_t(sm0) * uint32_t(nx) : kOOBV;
            const uint32_t b1 = sm1 >= 0 ? uint32_t(sm1) * uint32_t(nx) : kOOBV;
            // psi_out is written by the interior rows only (the one writer of each voxel)
            const uint32_t w0o = so0 >= 0 ? b0 * 4u : kOOB, w1o = so1 >= 0 ? b1 * 4u : kOOB;
            // voxel rows in batches of VB float4 per lane: all KV (<= 5) at once (540: 0.51 vs
            // 0.52 ms in batches of 4), else batches of kXtVB (L = 800 would spill)
            // The Tikhonov update holds its double-precision step beside the voxel batch; at
            // TR = 64 (L = 1050) the batch of 4 float4 per row spilled VGPRs under the 128
            // of two blocks per CU: batches of 2 measured update 2.93 -> 2.53 ms, C3 on one
            // GPU 8,648 -> 9,011 Mvox/s (profiles/r04_xtile_1050_ab.txt).  SD_XT_VB_TIK64 /
            // SD_XT_VB_TIK32 set the Tikhonov batch per TR (0: the default rule; A/B builds)
            // (TR = 32: batches of 2 for rows of up to 5 float4 per lane -- 540: default-mode
            // update 0.59 -> 0.572 ms, headline unchanged; at 800 the 4-float4 batches stay,
            // 2 measured 2.06 -> 2.12 ms: profiles/r04_xtile_tik_ab.txt)
            // one float4 of voxels of both rows: next(), blend, stats, psi' to HBM and the LDS row
            auto upd4 = [&](int j, const float4& p0, const float4& p1, const float4& w0, const float4& w1) {
                const uint32_t jo = uint32_t(j) * 4u;
                float o0[4], o1[4];
                float4* zq = reinterpret_cast<float4*>(zr + 4 * j);  // 4 voxels = 2 b128
                const float4 za = zq[sw], zb = zq[sw ^ 1];
                const float4 z01 = sel4(sw, zb, za), z23 = sel4(sw, za, zb);
                // branch-free (row validity is uniform per pair anyway): conditional code
                // here made the compiler split the b128 reads into b32 reads inside branches
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 iz = e == 0 ? make_float2(z01.x, z01.y) : e == 1 ? make_float2(z01.z, z01.w)
                                    : e == 2 ? make_float2(z23.x, z23.y) : make_float2(z23.z, z23.w);
                    const float l0 = f4c(p0, e), l1 = f4c(p1, e);
                    const float n0 = next_value_t<TIK>(l0, iz.x, f4c(w0, e), a.lambda, inv_lambda);
                    const float n1 = next_value_t<TIK>(l1, iz.y, f4c(w1, e), a.lambda, inv_lambda);
                    o0[e] = sm0 >= 0 ? n0 : 0.f;
                    o1[e] = sm1 >= 0 ? n1 : 0.f;
                    // |change| of interior voxels, each promoted to double before the sum
                    // (MVDeconvolution.java:591-626 adds float changes into a double)
                    const float c0 = so0 >= 0 ? fabsf(__fsub_rn(n0, l0)) : 0.f;
                    const float c1 = so1 >= 0 ? fabsf(__fsub_rn(n1, l1)) : 0.f;
                    ssum += (double)c0;
                    ssum += (double)c1;
                    smax = fmaxf(smax, fmaxf(c0, c1));
                }
                const float4 o01 = make_float4(o0[0], o1[0], o0[1], o1[1]), o23 = make_float4(o0[2], o1[2], o0[3], o1[3]);
                zq[sw] = sel4(sw, o23, o01);
                zq[sw ^ 1] = sel4(sw, o01, o23);
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned,
                                       make_float4(o0[0], o0[1], o0[2], o0[3])),
                    rpo, int(w0o + jo * 4u), 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned,
                                       make_float4(o1[0], o1[1], o1[2], o1[3])),
                    rpo, int(w1o + jo * 4u), 0, 0);
            };
            {
            constexpr int VBT = TR == 64 ? SD_XT_VB_TIK64 : (KV <= 5 ? SD_XT_VB_TIK32 : 0);
            constexpr int VB0 = (TIK && VBT > 0) ? (VBT < KV ? VBT : KV) : (KV <= 5 ? KV : kXtVB);
            // the fp16 2100 wave tiles take the whole row (9 float4 per lane) in one batch: one
            // round trip per tile instead of five, 156 VGPRs, still 3 waves per SIMD (C5 update
            // 2.84-2.90 -> 2.50-2.53 ms, batches of 5: 2.75-2.78 ms; r06_xtile_wave_ab.txt);
            // fp32 would need 188 (SD_XT_VB_WAVE > 0: that batch for both, A/B builds)
            constexpr bool WAVE = NP * TR == 64 && N1 * N2 > 1204;
            constexpr int VBW = SD_XT_VB_WAVE > 0 ? SD_XT_VB_WAVE : (S == 1 ? KV : 0);
            constexpr int VB = (WAVE && VBW > 0) ? (VBW < KV ? VBW : KV) : VB0;
            int hb = hl;
            for (int i0 = 0; i0 < KV; i0 += VB) {
            asm volatile("" : "+v"(hb));  // next batch's loads after this batch's stores
            float4 pa[VB], pb[VB];
            vraw4<S> wa[VB], wb[VB];   // (f16 weights packed until used)
#pragma unroll
            for (int i = 0; i < VB; ++i) {
                const uint32_t jo = uint32_t(min(hb + TR * (i0 + i), nx4 - 1)) * 4u;
                pa[i] = bload4(rpsi, (b0 + jo) * 4u);
                pb[i] = bload4(rpsi, (b1 + jo) * 4u);
                wa[i] = bloadraw4<S>(rimg, b0 + jo);
                wb[i] = bloadraw4<S>(rimg, b1 + jo);
            }
#pragma unroll
            for (int i = 0; i < VB; ++i) {
                const int j = hb + TR * (i0 + i);
                if (j < nx4) upd4(j, pa[i], pb[i], cvt4<S>(wa[i]), cvt4<S>(wb[i]));
            }
            }
            }
            xt_barrier();
            for (int qx = nx + hl; qx < L; qx += TR) {
                const int sx = qx < nx + cx ? qx : qx - L;
                zr[qx] = zr[mirror_idx(sx, nx)];
            }
        }
        }
        xt_barrier();
        XT_STAMP(3);
        if (!(MODE == XM_UPDATE && a.Cout == nullptr)) {   // (the last update: no spectra)
        if constexpr (TWG) xt_fft<N1, N2, false, NP>(Z, twg, P, t0);
        else xt_fft<N1, N2, false, NP>(Z, (const float2*)tw, P, t0);
        XT_STAMP(4);
        // ---- store: unpack the two half spectra (16-B stores; skipped rows go out of range)
        {
            SD_XT_ROWS
            const uint32_t o0 = v0 && sm0 != -1 ? uint32_t(r0) * uint32_t(Hp) * 8u : kOOB;
            const uint32_t o1 = v1 && sm1 != -1 ? uint32_t(r1) * uint32_t(Hp) * 8u : kOOB;
#pragma unroll
            for (int i = 0; i < KS; ++i) {
                const int j = hl + TR * i;
                if (j >= Hp2) break;
                float o[2][4];
                const float4 zkk = *reinterpret_cast<const float4*>(zr + 2 * j);  // k = 2j, 2j + 1
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = 2 * j + h;
                    float2 xa = make_float2(0.f, 0.f), xb = make_float2(0.f, 0.f);
                    if (k < Hx) {
                        const float2 zk = h ? make_float2(zkk.z, zkk.w) : make_float2(zkk.x, zkk.y);
                        const float2 zm = zr[k == 0 ? 0 : L - k];
                        xa = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
                        xb = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
                    }
                    o[0][2 * h] = xa.x;
                    o[0][2 * h + 1] = xa.y;
                    o[1][2 * h] = xb.x;
                    o[1][2 * h + 1] = xb.y;
                }
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned,
                                       make_float4(o[0][0], o[0][1], o[0][2], o[0][3])),
                    rcout, int(o0 + uint32_t(j) * 16u), 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned,
                                       make_float4(o[1][0], o[1][1], o[1][2], o[1][3])),
                    rcout, int(o1 + uint32_t(j) * 16u), 0, 0);
            }
        }
        xt_barrier();  // Z is rewritten by the next tile
#if SD_XT_STAMPS
        XT_STAMP(5);
        if (t0 == 0 && (tile & 63) == 0 && MODE >= 0 && MODE < 3) {
            for (int i = 0; i < 5; ++i) atomicAdd(&g_xt_stamp[MODE][i], xts[i + 1] - xts[i]);
            if (xt_first) atomicAdd(&g_xt_stamp[MODE][5], xts[0] - xts[6]);   // prologue (first tile)
            atomicAdd(&g_xt_stamp[MODE][7], 1ull);
        }
        xt_first = false;
#endif
        }
        // one tile per block: without a loop the compiler keeps no DFT constants live across
        // tiles (hoisted out of the loop, the 1050 tiles' 30- and 35-point constants overflowed
        // the SGPRs into VGPR lanes: 48-101 SGPR spills)
        break;
    }
#undef SD_XT_ROWS
    if constexpr (MODE == XM_UPDATE) {
        __shared__ double sh_sum[kXtThreads / 64];
        __shared__ float sh_max[kXtThreads / 64];
        for (int off = 32; off > 0; off >>= 1) {
            ssum += __shfl_xor(ssum, off, 64);
            smax = fmaxf(smax, __shfl_xor(smax, off, 64));
        }
        if ((t0 & 63) == 0) {
            sh_sum[t0 >> 6] = ssum;
            sh_max[t0 >> 6] = smax;
        }
        __syncthreads();
        if (t0 == 0) {
            for (int i = 1; i < kXtThreads / 64; ++i) {
                ssum += sh_sum[i];
                smax = fmaxf(smax, sh_max[i]);
            }
            a.partials[2 * (a.pofs + blockIdx.x)] = ssum;
            a.partials[2 * (a.pofs + blockIdx.x) + 1] = (double)smax;
        }
    }
}
