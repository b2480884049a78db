// fftconv_zd.inc -- z pass as a DIRECT circular convolution with the compact kernel.
// Included by fftconv.hip inside namespace spimdecon::{anonymous}, after fftconv_x.inc.
//
// After the x and y transforms, the convolution left to do along z is, for every
// (kx, ky) column, the circular convolution of the column with the kernel's xy
// partial spectrum, which is non-zero on the 2*kc+1 planes qz in [-kc, kc] only
// (the compact kernel, engine_kernel_compact):
//     out[z] = Mz * sum_{q=-kc..kc} Kc[q + kc] * C[(z - q) mod Mz]
// (Kc carries the engine's 1/(Mx My Mz) scale; the z FFT pair it replaces would
// have contributed the factor Mz).  That is exactly what the fused FFT z pass
// (k_col2f MODE 5) computes, but with 2*(2kc+1) packed FMAs per output instead of
// two length-Mz FFTs plus the kernel's own z transform.  Cheaper for kernels up to
// 25 planes (kc <= 8: 0.26-0.27, kc 12: 0.298 vs 0.30-0.31 ms at 540^3); larger
// kernels keep the FFT z pass (engine_zdirect_ok).
// Only the nz interior planes are written: the halo planes of the result are never
// read (the x passes read interior rows only).
// Thread (c, r) keeps element c's 2*KC+1 taps in registers and computes OPT consecutive
// outputs, streaming the OPT + 2*KC window inputs from LDS (input-stationary: each input
// updates every output it contributes to).  Taps beyond the runtime kc are zero (KC = the
// instantiated bound).

constexpr int kZdThreads = 512;

// ---------------------------------------------------------------- LDS-DMA, double-buffered
// The column tiles are streamed into LDS by global_load_lds_dwordx4 (no VGPR staging):
// while a block computes one item from one buffer, the next item's planes are already
// in flight into the other (a register-staged pass serialised its load and compute
// phases inside a block and sat at 4.3 TB/s, latency-bound).  One DMA wave-instruction
// writes 1 KiB = 4 plane slots of 32 complex.  The DMA and the waits are inline asm: the
// compiler neither sees the loads (no vmcnt(0) before every ds_read) nor the waits
// (counted: the stores issued after an item's DMA may stay in flight).
__device__ __forceinline__ void zd_glds16(const void* gsrc, uint32_t lds_byte) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte) : "memory");
}

// s_waitcnt vmcnt(n) for a runtime n (0 when n is past the 6-bit field)
__device__ __forceinline__ void zd_wait_vmcnt(int n) {
    switch (n) {
#define SD_VMC(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); return;
        SD_VMC(1) SD_VMC(2) SD_VMC(3) SD_VMC(4) SD_VMC(5) SD_VMC(6) SD_VMC(7) SD_VMC(8) SD_VMC(9)
        SD_VMC(10) SD_VMC(11) SD_VMC(12) SD_VMC(13) SD_VMC(14) SD_VMC(15) SD_VMC(16) SD_VMC(17)
        SD_VMC(18) SD_VMC(19) SD_VMC(20) SD_VMC(21) SD_VMC(22) SD_VMC(23) SD_VMC(24) SD_VMC(25)
        SD_VMC(26) SD_VMC(27) SD_VMC(28) SD_VMC(29) SD_VMC(30) SD_VMC(31) SD_VMC(32) SD_VMC(33)
        SD_VMC(34) SD_VMC(35) SD_VMC(36) SD_VMC(37) SD_VMC(38) SD_VMC(39) SD_VMC(40) SD_VMC(41)
        SD_VMC(42) SD_VMC(43) SD_VMC(44) SD_VMC(45) SD_VMC(46) SD_VMC(47) SD_VMC(48) SD_VMC(49)
        SD_VMC(50) SD_VMC(51) SD_VMC(52) SD_VMC(53) SD_VMC(54) SD_VMC(55) SD_VMC(56) SD_VMC(57)
        SD_VMC(58) SD_VMC(59) SD_VMC(60) SD_VMC(61) SD_VMC(62) SD_VMC(63)
#undef SD_VMC
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); return;
    }
}

// ------------------------------------------------ LDS-DMA over z chunks, carried in the block
// A tile is TX consecutive complex elements of the flattened (y, kx) plane (the z
// convolution is per element; the compact kernel has the same layout), split into
// chunks of H <= TR * OPT output planes that ONE block processes in order, so only
// H + 2 KC planes per buffer need the LDS (two buffers for any Mz, 32-column tiles =
// 256-B plane segments at every length; whole-column tiles needed 8 columns at 800^3).  In place and race-free: chunk c + 1's first
// 2 KC window planes include chunk c's last KC outputs, so they are not re-read from
// HBM but copied, with the taps, from chunk c's buffer (which holds them unmodified)
// before chunk c computes; everything chunk c + 1 loads lies past chunk c's outputs,
// and no other block touches the tile.
// Slot s of a chunk at zc holds plane (zc - KC + s) mod Mz; a half-wave reads one 256-B
// slot.  Threads whose outputs lie past H read slots nobody loaded (dropped at the store).
__host__ __device__ constexpr int zdc_spp(int TX) { return 1024 / (TX * 8); }
__host__ __device__ constexpr int zdc_slots(int KC, int OPT, int TX) {
    // window reads of the last thread row: (TR - 1) OPT + OPT + 2 KC
    return ((kZdThreads / TX) * OPT + 2 * KC + zdc_spp(TX) - 1) / zdc_spp(TX) * zdc_spp(TX);
}
__host__ __device__ constexpr int zdc_tap_slots(int KC, int TX) {
    return (2 * KC + 1 + zdc_spp(TX) - 1) / zdc_spp(TX) * zdc_spp(TX);
}
__host__ __device__ constexpr int zdc_lds(int KC, int OPT, int TX) {
    return 2 * (zdc_slots(KC, OPT, TX) + zdc_tap_slots(KC, TX)) * TX * 8;
}

// Two buffers: item i + 1's DMA is issued when item i starts.
// KD = KC - kc known at compile time (1: a 31-plane kernel in the 33-slot layout of KC 16,
// C4's 31^3 PSFs): the KD outermost taps on each side are zero and skipped (the window
// starts KD slots later and is 2 KD shorter), 2 KD / (2 KC + 1) of the FMAs.  KD = 0: the
// runtime kc masks the taps as before.
template <int KC, int OPT, int KD = 0>
__global__ __launch_bounds__(kZdThreads) void k_zdmc(SlabGeom g, int64_t nflat, float2* C, const float2* Kc, int kc,
                                                     int H, uint32_t bytes, float kscale, int zmir) {
    constexpr int TX = 32, NB = 2, NT = kZdThreads;
    constexpr int NQ = 2 * KC + 1;
    constexpr int W = OPT + 2 * KC - 2 * KD;   // window inputs per thread (from slot zb + KD)
    constexpr int TR = NT / TX;
    constexpr int SPP = zdc_spp(TX);
    constexpr int LPS = TX / 2;                 // lanes per slot (16 B each)
    constexpr int NSP = zdc_slots(KC, OPT, TX);
    constexpr int NKP = zdc_tap_slots(KC, TX);
    constexpr int bufslots = NSP + NKP;
    constexpr int HEAD = 2 * KC;                // carried window slots (a whole number of pieces)
    static_assert(HEAD % SPP == 0, "the carried head must be whole DMA pieces");
    static_assert(zdc_lds(KC, OPT, TX) <= 160 * 1024, "the buffers must fit the LDS");
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    const int Mz = int(g.Mz);
    const int nz = int(g.nz);
    const uint32_t lds0 = (uint32_t)(size_t)((__attribute__((address_space(3))) char*)smem);
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t / 64);
    const int ntc = int((nflat + TX - 1) / TX);  // tiles (nflat % 16 == 0)
    const int nch = (nz + H - 1) / H;            // chunks per tile
    const int nitems = ntc * nch;                // this block: items blockIdx.x * nch + ..., grid-strided by tile
    const uint64_t es = uint64_t(nflat) * 8u;    // bytes between z planes (C and Kc alike)
    // item i of this block = (tile, chunk): tile = blockIdx.x + (i / nch) * gridDim.x
    auto item_tile = [&](int i) { return int(blockIdx.x) + (i / nch) * int(gridDim.x); };
    // DMA of item i -> buffer b (continuation chunks skip the carried head and the taps)
    auto issue = [&](int i, int b) {
        const int tile = item_tile(i);
        const int ch = i % nch;
        const int lane = t & 63;
        const int64_t f0 = int64_t(tile) * TX;
        int col = (lane % LPS) * 2;
        // past the last column (nflat % 16 == 0): re-read a column of the tile (dropped at the store)
        if (f0 + col >= nflat) col %= int(nflat - f0);
        const char* cb = reinterpret_cast<const char*>(C + f0 + col);
        const char* kb = reinterpret_cast<const char*>(Kc + f0 + col);
        const uint32_t bl = lds0 + uint32_t(b * bufslots) * uint32_t(TX * 8);
        const int zc = ch * H;
        const int hh = min(H, nz - zc);
        const int p0 = ch == 0 ? 0 : HEAD / SPP;                 // first column piece
        const int p1 = (hh + 2 * KC + SPP - 1) / SPP;            // column pieces end
        const int ncp = p1 - p0;
        const int npieces = ncp + (ch == 0 ? NKP / SPP : 0);
        // staggered plane order per block: in lock step all blocks would read the same few
        // planes (a few HBM channels) at a time
        const int stag = int((uint32_t(blockIdx.x) * 2654435761u) % uint32_t(npieces));
        for (int jj = wave; jj < npieces; jj += NT / 64) {
            const int jc = jj + stag < npieces ? jj + stag : jj + stag - npieces;
            const int j = jc < ncp ? p0 + jc : NSP / SPP + (jc - ncp);
            const int s = SPP * j + lane / LPS;
            const char* src;
            if (s < NSP) {   // slot s = plane (zc - KC + s) mod Mz
                int z = zc - KC + s;
                z += z < 0 ? Mz : 0;
                z %= Mz;
                // zmir (Mz = nz + 2 kc, no neighbours): an extension plane is not in memory;
                // the plane it mirrors, in [0, nz), holds the same spectra
                if (zmir && z >= nz) z = z < nz + kc ? 2 * (nz - 1) - z : Mz - z;
                src = cb + uint64_t(z) * es;
            } else {         // tap slot: kernel plane (s - NSP) - KC + kc, clamped (zeroed at use)
                const int q = min(max(s - NSP - KC + kc, 0), 2 * kc);
                src = kb + uint64_t(q) * es;
            }
            zd_glds16(src, __builtin_amdgcn_readfirstlane(bl + uint32_t(j) * 1024u));
        }
    };
    int nmine = 0;  // items of this block
    if (int(blockIdx.x) < ntc) nmine = ((ntc - 1 - int(blockIdx.x)) / int(gridDim.x) + 1) * nch;
    if (nmine > 0) issue(0, 0);
    (void)nitems;
    for (int i = 0; i < nmine; ++i) {
        const int b = i % NB;
        // item i's DMA landed; what this wave issued after it may still fly: the OPT
        // stores of the item computed before
        zd_wait_vmcnt(i == 0 ? 0 : OPT);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and the head carried into it
        __builtin_amdgcn_s_barrier();          // ... in every wave; item i - 1's buffer is no longer read
        float2* Y = smem + b * bufslots * TX;
        const float2* Kt = Y + NSP * TX;
        if (i + 1 < nmine) {
            const int ch = i % nch;
            if (ch + 1 < nch) {                // continuation: carry the window head and the taps
                float2* Yn = smem + ((i + 1) % NB) * bufslots * TX;
                const int hh = min(H, nz - ch * H);
                for (int e = t; e < HEAD * TX; e += NT) Yn[e] = Y[hh * TX + e];
                for (int e = t; e < NKP * TX; e += NT) Yn[NSP * TX + e] = Kt[e];
            }
        }
        if (i + NB - 1 < nmine) issue(i + NB - 1, (i + NB - 1) % NB);
        int tt = t;
        asm volatile("" : "+v"(tt));
        const int c = tt % TX;
        const int r = tt / TX;
        sd_v2 K[NQ];  // column c's taps scaled by Mz; zero beyond the runtime kc
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) K[qi] = v2_(Kt[qi * TX + c]);
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            const float m = (qi - KC >= -kc && qi - KC <= kc) ? kscale : 0.0f;
            K[qi] = K[qi] * sd_v2{m, m};
        }
        const int64_t f0 = int64_t(item_tile(i)) * TX;
        const int zc = (i % nch) * H;
        const int zend = min(nz, zc + H);
        const __amdgpu_buffer_rsrc_t rc = brsrc(C + f0, bytes);
        const bool cok = f0 + c < nflat;
        const int zb = r * OPT;
        sd_v2 acc[OPT];
#pragma unroll
        for (int o = 0; o < OPT; ++o) acc[o] = sd_v2{0.0f, 0.0f};
        // input i = slot zb + i = plane zc + zb - KC + i (mod Mz); groups of ZG window
        // inputs, the next group's LDS reads issued before this group's FMAs
        const float2* win = Y + (zb + KD) * TX + c;
        constexpr int ZG = 8;
        constexpr int NG = (W + ZG - 1) / ZG;
        sd_v2 X[2][ZG];
#pragma unroll
        for (int ii = 0; ii < ZG; ++ii)
            if (ii < W) X[0][ii] = v2_(win[ii * TX]);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            if (gi + 1 < NG) {
#pragma unroll
                for (int ii = 0; ii < ZG; ++ii)
                    if ((gi + 1) * ZG + ii < W) X[(gi + 1) & 1][ii] = v2_(win[((gi + 1) * ZG + ii) * TX]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ii = 0; ii < ZG; ++ii) {
                const int iw = gi * ZG + ii;
                if (iw >= W) break;
                const sd_v2 Xi = X[gi & 1][ii];
#pragma unroll
                for (int o = 0; o < OPT; ++o) {
                    const int qi = o + 2 * KC - (iw + KD);
                    if (qi >= KD && qi < NQ - KD) {
                        acc[o] = __builtin_elementwise_fma(K[qi].xx, Xi, acc[o]);
                        acc[o] = __builtin_elementwise_fma(sd_v2{-K[qi].y, K[qi].y}, Xi.yx, acc[o]);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int o = 0; o < OPT; ++o) {
            const int z = zc + zb + o;
            bstore2(rc, int(cok && z < zend ? uint32_t(c * 8) + uint32_t(z) * uint32_t(es) : kOOB), 0, f2_(acc[o]));
        }
    }
}
