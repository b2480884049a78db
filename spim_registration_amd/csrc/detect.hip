// detect.hip -- the shared side of the detectors (detect.hpp): the per-device workspace, the
// staging of a view, and the detection stage over a stored device image: the 26-neighbour
// test (k_dog_peaks; k_peaks_append beyond its 4 GiB) appends candidates as (key, record), a
// device radix sort on the key (x % T) << 40 | flat restores the reference's order
// (dog_sort.hip), k_localize / k_to_points / point_select turn them into interest points.
// References (under the reference's src/main/java/):
//   mpicbg/spim/segmentation/InteractiveIntegral.java:360-468     findPeaks / isSpecialPoint
//   spim/process/interestpointdetection/DifferenceOfGaussianNewPeakFinder.java:54-136
#include <algorithm>
#include <cstddef>

#include "detect_dev.hpp"

namespace spimdecon {
namespace {

// one wave-wide append; every lane of the wave must call it
__device__ __forceinline__ void sink_append(const PeakSink& pk, bool flag, int x, int y, int z, uint64_t flat,
                                            float c, int sp) {
    const unsigned long long bal = __ballot(flag);
    if (bal == 0ull) return;
    const int lane = int(threadIdx.x & 63);
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(pk.count, unsigned(__popcll(bal)));
    base = unsigned(__shfl(int(base), 0, 64));
    const unsigned pos = base + unsigned(__popcll(bal & ((1ull << lane) - 1ull)));
    if (flag && pos < pk.cap) {
        pk.keys[pos] = (uint64_t(x % pk.T) << 40) | flat;
        pk.vals[pos] = pos;
        PeakOut o;
        o.x = x;
        o.y = y;
        o.z = z;
        o.intensity = fabsf(c);
        o.is_min = sp == 1;
        o.is_max = sp == 2;
        pk.recs[pos] = o;
    }
}

// The split z stage, part 2: the 26-neighbour test over the stored DoG image.  A wave =
// 64 consecutive x (lanes 1..62 tested, lanes 0 and 63 their halo) x DPY rows per lane,
// walking a chunk of zc_len centre planes: per plane each lane loads its column's DPY + 2
// rows (PD planes ahead), the x neighbours come from DPP lane shifts, the y neighbours
// from the lane's own rows, and the 3x3 min / max of the last two planes stay in
// registers -- no LDS ring, no barrier (the ring test of k_dog_z over the same image: 1.19
// vs 0.42 ms per 768^3).  A centre plane next to a plane holding a NaN
// (any loaded value of the wave) takes the reference's comparison loop over the image
// for the wave (NaN compares false; min3 / max3 would drop it).
constexpr int kDpkX = 62;   // columns tested per wave (lanes 1 .. 62)
constexpr int kDpkY = 4;    // rows per lane
constexpr int kDpkZ = 64;   // centre planes per chunk
constexpr int kDpkPD = 2;   // planes loaded ahead
__device__ __forceinline__ float dpp_from_left(float v) {    // lane i <- lane i - 1 (wave_shr:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_from_right(float v) {   // lane i <- lane i + 1 (wave_shl:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

template <int DPY, int PD>
__global__ __launch_bounds__(256) void k_dog_peaks(Dims3 d, const float* __restrict__ dog, int zc_len, float minv,
                                                   int want, const PeakSink* __restrict__ sink, int xcd) {
    constexpr int NR = DPY + 2;    // rows loaded per plane
    constexpr int NW = PD + 1;     // planes in the load ring
    __shared__ int4 cbuf[4][kCandBuf];
    const int lane = int(threadIdx.x & 63), wv = int(threadIdx.x >> 6);
    const int nx = int(d.nx), ny = int(d.ny), nz = int(d.nz);
    const int nsx = (nx - 2 + kDpkX - 1) / kDpkX, nyb = (ny - 2 + DPY - 1) / DPY;
    const int nzc = (nz - 2 + zc_len - 1) / zc_len;
    // xcd: blocks go round-robin to the 8 XCDs; the logical block index gives each XCD a
    // contiguous range, so the y-neighbour waves sharing a halo row run on one L2
    int lb = int(blockIdx.x);
    if (xcd) {
        const unsigned b = blockIdx.x, k = b & 7u, j = b >> 3, q = gridDim.x >> 3, r = gridDim.x & 7u;
        lb = int(k * q + min(k, r) + j);
    }
    const int wid = __builtin_amdgcn_readfirstlane(lb * 4 + wv);
    if (wid >= nsx * nyb * nzc) return;   // (wave-uniform; no block barriers below)
    const int sx = wid % nsx, yb = (wid / nsx) % nyb, zb = wid / (nsx * nyb);
    const int x = sx * kDpkX + lane;                       // lane 0: the halo column x0 - 1
    const bool xt = lane >= 1 && lane <= kDpkX && x <= nx - 2;
    const int xl = min(x, nx - 1);
    const int ybase = yb * DPY;                         // row r of the lane: y = ybase + r (r = 0: halo)
    const int tlo = 1 + zb * zc_len, thi = min(nz - 1, tlo + zc_len);   // centre planes tested
    const int qa = tlo - 1, qb = thi + 1;               // planes loaded
    const uint32_t pstride = uint32_t(nx) * uint32_t(ny);
    const uint64_t total = uint64_t(pstride) * uint64_t(nz) * 4u;
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(dog), 0, int(uint32_t(total < 0xffffffffull ? total : 0xffffffffull)), 0x00020000);
    const uint32_t xoff = uint32_t(xl) * 4u;   // the only per-lane offset: rows and planes are scalar
    auto ldp = [&](int i, float* v) {   // plane qa + i (the tail repeating the last plane)
        const uint32_t po = uint32_t(qa + min(i, qb - qa - 1)) * pstride * 4u;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t so = po + uint32_t(min(ybase + r, ny - 1)) * uint32_t(nx) * 4u;
            v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, int(xoff), int(so), 0));
        }
    };
    float ring[NW][NR];
#pragma unroll
    for (int p = 0; p < NW - 1; ++p) ldp(p, ring[p]);
    float mnA[DPY], mxA[DPY], mnB[DPY], mxB[DPY], cB[DPY];
#pragma unroll
    for (int r = 0; r < DPY; ++r) mnA[r] = mxA[r] = mnB[r] = mxB[r] = cB[r] = 0.0f;
    int nanhist = 0;   // bit k: plane q - k held a NaN (any loaded value of the wave)
    int ccount = 0;
    const bool want_min = (want & 1) != 0, want_max = (want & 2) != 0;
    const int nsteps = (qb - qa + NW - 1) / NW * NW;
    for (int sb = 0; sb < nsteps; sb += NW) {
#pragma unroll
        for (int ph = 0; ph < NW; ++ph) {
            const int st = sb + ph;
            ldp(st + NW - 1, ring[(ph + NW - 1) % NW]);
            const float* v = ring[ph % NW];   // plane q = qa + st
            const int q = qa + st;
            bool hasnan = false;
            float xmn[NR], xmx[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                hasnan |= v[r] != v[r];
                const float l = dpp_from_left(v[r]), rr = dpp_from_right(v[r]);
                xmn[r] = dz_min3(l, v[r], rr);
                xmx[r] = dz_max3(l, v[r], rr);
            }
            nanhist = ((nanhist << 1) | (__ballot(hasnan) != 0ull ? 1 : 0)) & 7;
            float mnC[DPY], mxC[DPY];
#pragma unroll
            for (int r = 0; r < DPY; ++r) {
                mnC[r] = dz_min3(xmn[r], xmn[r + 1], xmn[r + 2]);
                mxC[r] = dz_max3(xmx[r], xmx[r + 1], xmx[r + 2]);
            }
            const int zc = q - 1;   // centre plane of the test
            if (q < qb && zc >= tlo) {
                // per row: bit r of fl = candidate, of mx = a MAX ("this mixup is intended",
                // InteractiveIntegral.isSpecialPoint: every neighbour >= c is a MAX)
                unsigned fl = 0u, mxb = 0u;
#pragma unroll
                for (int r = 0; r < DPY; ++r) {
                    const float c = cB[r];
                    const bool cand = xt && ybase + 1 + r <= ny - 2 && !(fabsf(c) < minv);
                    const bool ge = dz_min3(mnA[r], mnB[r], mnC[r]) >= c;
                    const bool le = dz_max3(mxA[r], mxB[r], mxC[r]) <= c;
                    const bool is_max = cand && ge, is_min = cand && !ge && le;
                    fl |= unsigned((is_max && want_max) || (is_min && want_min)) << r;
                    mxb |= unsigned(is_max) << r;
                }
                if (nanhist != 0) {   // a NaN next to this plane: the comparison loop (rare)
                    fl = 0u;
                    mxb = 0u;
#pragma unroll 1
                    for (int r = 0; r < DPY; ++r) {
                        const int y = ybase + 1 + r;
                        const float c = dog[size_t(zc) * pstride + size_t(min(y, ny - 1)) * size_t(nx) + size_t(xl)];
                        const bool cand = xt && y <= ny - 2 && !(fabsf(c) < minv);
                        bool ge = true, le = true;
                        if (cand) {
#pragma unroll 1
                            for (int k = 0; k < 27; ++k) {
                                if (k == 13) continue;   // (the centre)
                                const float u = dog[size_t(zc + k / 9 - 1) * pstride + size_t(y + (k / 3) % 3 - 1) * size_t(nx) +
                                                    size_t(x + k % 3 - 1)];
                                ge &= u >= c;
                                le &= u <= c;
                            }
                        }
                        const int spn = !cand ? 0 : ge ? 2 : le ? 1 : 0;
                        fl |= unsigned((spn == 2 && want_max) || (spn == 1 && want_min)) << r;
                        mxb |= unsigned(spn == 2) << r;
                    }
                }
                if (__ballot(fl != 0u) != 0ull) {   // (rare: a few candidates per million voxels)
#pragma unroll
                    for (int r = 0; r < DPY; ++r) {
                        const bool flag = ((fl >> r) & 1u) != 0u;
                        const unsigned long long bal = __ballot(flag);
                        if (bal == 0ull) continue;
                        const int nb = __popcll(bal);
                        if (ccount + nb > kCandBuf) {
                            cand_flush(sink, cbuf[wv], ccount, nx, pstride);
                            ccount = 0;
                        }
                        const int sp = ((mxb >> r) & 1u) ? 2 : 1;
                        if (flag)
                            cbuf[wv][ccount + __popcll(bal & ((1ull << lane) - 1ull))] =
                                make_int4(x, (ybase + 1 + r) | (sp << 30), zc, __float_as_int(fabsf(cB[r])));
                        ccount += nb;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < DPY; ++r) {
                mnA[r] = mnB[r]; mxA[r] = mxB[r];
                mnB[r] = mnC[r]; mxB[r] = mxC[r];
                cB[r] = v[r + 1];
            }
        }
    }
    cand_flush(sink, cbuf[wv], ccount, nx, pstride);
}

// InteractiveIntegral.isSpecialPoint: 0 invalid, 1 MIN, 2 MAX
__device__ __forceinline__ int special_point(const float* __restrict__ dog, Dims3 d, int64_t i,
                                             int64_t x, int64_t y, int64_t z, float minv, float& val) {
    if (x < 1 || y < 1 || z < 1 || x > d.nx - 2 || y > d.ny - 2 || z > d.nz - 2) return 0;
    const float c = dog[i];
    val = c;
    if (fabsf(c) < minv) return 0;
    bool is_min = true, is_max = true;
    const int64_t sy = d.nx, sz = d.nx * d.ny;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dz == 0 && dy == 0 && dx == 0) continue;
                const float v = dog[i + dz * sz + dy * sy + dx];
                is_min &= (v >= c);
                is_max &= (v <= c);
            }
    // "this mixup is intended": all neighbours >= centre => MAX (bright bead)
    if (is_min) return 2;
    if (is_max) return 1;
    return 0;
}

// (x, y, z) of flat index i: 32-bit divisions when the volume allows (a 64-bit
// division is a ~100-instruction software routine on the GPU)
__device__ __forceinline__ void flat_coords(int64_t i, const Dims3& d, int64_t& x, int64_t& y, int64_t& z) {
    if (d.nx * d.ny * d.nz < (int64_t(1) << 32)) {
        const uint32_t ii = uint32_t(i), nx = uint32_t(d.nx), ny = uint32_t(d.ny);
        const uint32_t q = ii / nx;
        x = ii - q * nx;
        z = q / ny;
        y = q - uint32_t(z) * ny;
    } else {
        x = i % d.nx;
        y = (i / d.nx) % d.ny;
        z = i / (d.nx * d.ny);
    }
}

// candidates of a DoG volume already in HBM (the fallback for Gaussians of 63 / 127 taps)
__global__ __launch_bounds__(kBlock) void k_peaks_append(const float* __restrict__ dog, Dims3 d, PeakSink pk) {
    const int64_t n = d.nx * d.ny * d.nz;
    for (int64_t i0 = int64_t(blockIdx.x) * kBlock; i0 < n; i0 += int64_t(gridDim.x) * kBlock) {
        const int64_t i = i0 + threadIdx.x;
        int sp = 0;
        float v = 0.0f;
        int64_t x = 0, y = 0, z = 0;
        if (i < n) {
            flat_coords(i, d, x, y, z);
            sp = special_point(dog, d, i, x, y, z, pk.minv, v);
        }
        const bool flag = (sp == 2 && pk.want_max) || (sp == 1 && pk.want_min);
        sink_append(pk, flag, int(x), int(y), int(z), uint64_t(i), v, sp);
    }
}

__global__ void k_gather_peaks(const PeakOut* __restrict__ recs, const uint32_t* __restrict__ order, int64_t n,
                               PeakOut* __restrict__ out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = recs[order[i]];
}

}  // namespace

// ---------------------------------------------------------------- quadratic localization
// IPD/Localization.java:47-88 (imglib1 SubpixelLocalization, maxNumMoves 10,
// allowMaximaTolerance); finite differences and 3x3 inverse as in the reference's
// own fit, mpicbg/spim/registration/bead/laplace/LaPlaceFunctions.java:30-170,243-466.
// One thread per peak; all fit arithmetic in double, -ffp-contract=off.  (LocOut: detect.hpp)
constexpr int kLocMaxMoves = 10;
constexpr double kLocTolerance = 0.01;

__global__ void k_localize(const float* __restrict__ dog, Dims3 d, const PeakOut* __restrict__ pk,
                           int64_t np, LocOut* __restrict__ out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const PeakOut q = pk[i];
    int p[3] = {q.x, q.y, q.z};
    const int64_t dim[3] = {d.nx, d.ny, d.nz};
    auto v = [&](int dx, int dy, int dz) -> float {
        return dog[(int64_t(p[2] + dz) * d.ny + (p[1] + dy)) * d.nx + (p[0] + dx)];
    };
    double X[3] = {0, 0, 0}, g[3] = {0, 0, 0};
    bool stable = false, valid = true;
    int moves = 0;
    for (;;) {
        ++moves;
        const float temp = 2.0f * v(0, 0, 0);
        double H[9];
        H[0] = double(v(1, 0, 0) - temp) + double(v(-1, 0, 0));
        H[4] = double(v(0, 1, 0) - temp) + double(v(0, -1, 0));
        H[8] = double(v(0, 0, 1) - temp) + double(v(0, 0, -1));
        auto cross = [](float a, float b, float c, float e) {
            return double(((a - b) / 2.0f - (c - e) / 2.0f) / 2.0f);
        };
        H[5] = H[7] = cross(v(0, 1, 1), v(0, -1, 1), v(0, 1, -1), v(0, -1, -1));
        H[2] = H[6] = cross(v(1, 0, 1), v(-1, 0, 1), v(1, 0, -1), v(-1, 0, -1));
        H[1] = H[3] = cross(v(1, 1, 0), v(-1, 1, 0), v(1, -1, 0), v(-1, -1, 0));
        g[0] = (double(v(1, 0, 0)) - double(v(-1, 0, 0))) / 2.0;
        g[1] = (double(v(0, 1, 0)) - double(v(0, -1, 0))) / 2.0;
        g[2] = (double(v(0, 0, 1)) - double(v(0, 0, -1))) / 2.0;
        const double det = H[0] * H[4] * H[8] + H[3] * H[7] * H[2] + H[6] * H[1] * H[5] -
                            H[2] * H[4] * H[6] - H[5] * H[7] * H[0] - H[8] * H[1] * H[3];
        if (det == 0.0) {
            valid = false;
            break;
        }
        const double A[9] = {(H[4] * H[8] - H[5] * H[7]) / det, (H[2] * H[7] - H[1] * H[8]) / det,
                             (H[1] * H[5] - H[2] * H[4]) / det, (H[5] * H[6] - H[3] * H[8]) / det,
                             (H[0] * H[8] - H[2] * H[6]) / det, (H[2] * H[3] - H[0] * H[5]) / det,
                             (H[3] * H[7] - H[4] * H[6]) / det, (H[1] * H[6] - H[0] * H[7]) / det,
                             (H[0] * H[4] - H[1] * H[3]) / det};
        for (int r = 0; r < 3; ++r) X[r] = -(A[3 * r] * g[0] + A[3 * r + 1] * g[1] + A[3 * r + 2] * g[2]);
        stable = true;
        const double thr = 0.5 + moves * kLocTolerance;
        for (int a = 0; a < 3; ++a)
            if (fabs(X[a]) > thr) {
                p[a] += X[a] > 0 ? 1 : -1;
                stable = false;
            }
        if (!stable)
            for (int a = 0; a < 3; ++a)
                if (p[a] <= 0 || p[a] >= dim[a] - 1) valid = false;
        if (!valid || stable || moves > kLocMaxMoves) break;
    }
    LocOut o;
    if (valid && stable) {
        const double fit = (X[0] * g[0] + X[1] * g[1] + X[2] * g[2]) / 2.0;
        for (int a = 0; a < 3; ++a) o.pos[a] = float(p[a]) + float(X[a]);
        o.value = v(0, 0, 0) + float(fit);
    } else {  // no stable fit: the peak stays as detected
        o.pos[0] = float(q.x);
        o.pos[1] = float(q.y);
        o.pos[2] = float(q.z);
        o.value = q.intensity;
    }
    out[i] = o;
}

// ---------------------------------------------------------------- the shared detection stage
void stored_candidates(DogWork& w, const Dims3& d, const float* dogp, bool peaks_kernel, const PeakSink& pk,
                       hipStream_t s) {
    if (peaks_kernel) {
        grow(w.sink, 1);
        SD_HIP(hipMemcpyAsync(w.sink.p, &pk, sizeof(pk), hipMemcpyHostToDevice, s));   // (synchronised by the caller)
        const int want = pk.want_min | (pk.want_max << 1);
        if (d.nx >= 3 && d.ny >= 3 && d.nz >= 3) {   // (else no voxel has 26 neighbours)
            constexpr int zcp = kDpkZ;
            const int64_t nwave = ceil_div(d.nx - 2, int64_t(kDpkX)) * ceil_div(d.ny - 2, int64_t(kDpkY)) *
                                  ceil_div(d.nz - 2, int64_t(zcp));
            const dim3 gp(unsigned(ceil_div(nwave, int64_t(4))));
            hipLaunchKernelGGL((k_dog_peaks<kDpkY, kDpkPD>), gp, dim3(256), 0, s, d, dogp, zcp, pk.minv, want, w.sink.p, 1);
        }
    } else {
        hipLaunchKernelGGL(k_peaks_append, dim3(grid_of(d.nx * d.ny * d.nz)), dim3(kBlock), 0, s, dogp, d, pk);
    }
}

void sort_candidates(DogWork& w, unsigned total, int T, hipStream_t s, DogRun& r) {
    r.np = total;
    if (total > 0) {
        grow(w.keys_sorted, total);
        grow(w.vals_sorted, total);
        grow(w.peaks, total);
        int end_bit = 40;   // the key's bits: flat below 2^40, then those of x % T
        while ((uint64_t(T - 1) >> (end_bit - 40)) != 0) ++end_bit;
        const size_t tb = peak_sort_temp_bytes(total, end_bit);
        grow(w.sort_tmp, std::max<size_t>(tb, 1));
        peak_sort(w.sort_tmp.p, tb, w.keys.p, w.keys_sorted.p, w.vals.p, w.vals_sorted.p, total, end_bit, s);
        hipLaunchKernelGGL(k_gather_peaks, dim3(unsigned(ceil_div(total, 256))), dim3(256), 0, s, w.recs.p,
                           w.vals_sorted.p, int64_t(total), w.peaks.p);
        SD_HIP(hipGetLastError());
        r.dpeaks = w.peaks.p;
    }
}

void detect_stored(DogWork& w, const Dims3& d, const float* img, float min_peak, int want_min, int want_max, int T,
                   hipStream_t s, DogRun& r, int route) {
    // (k_dog_peaks' one buffer resource; the route is checked by the caller)
    const bool pkk = route == SPIM_DETECT_ROUTE_APPEND ? false : image_below_4gib(d.nx * d.ny * d.nz);
    const unsigned total = collect_candidates(w, d.nx * d.ny * d.nz, min_peak, want_min, want_max, T, s,
                                              [&](const PeakSink& pk, int) { stored_candidates(w, d, img, pkk, pk, s); });
    r.d = d;
    r.dog = img;
    sort_candidates(w, total, T, s, r);
}

void peaks_to_host(const DogRun& r, spim_peak* peaks, int64_t max_peaks, int64_t* npeaks, hipStream_t s) {
    static_assert(sizeof(spim_peak) == sizeof(PeakOut) && offsetof(spim_peak, is_max) == offsetof(PeakOut, is_max),
                  "PeakOut is spim_peak's layout");
    *npeaks = r.np;
    const int64_t m = peaks ? std::min(r.np, max_peaks) : 0;
    if (m > 0) SD_HIP(hipMemcpyAsync(peaks, r.dpeaks, m * sizeof(PeakOut), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
}

// candidates -> interest points on the device: Localization.noLocalization (:19-45)
// copies them; with quadratic localisation (:47-88) the caller keeps those whose fitted
// |value| > threshold (flag), in candidate order
template <bool LOC>
__global__ void k_to_points(const PeakOut* __restrict__ pk, const LocOut* __restrict__ loc, int64_t np, float thr,
                            spim_interest_point* __restrict__ ips, unsigned char* __restrict__ flags) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= np) return;
    spim_interest_point ip{};
    if constexpr (LOC) {
        const LocOut l = loc[i];
        for (int a = 0; a < 3; ++a) ip.pos[a] = l.pos[a];
        ip.intensity = l.value;
        flags[i] = fabsf(l.value) > thr ? 1 : 0;   // float against float (Localization.java:74)
    } else {
        ip.pos[0] = pk[i].x;
        ip.pos[1] = pk[i].y;
        ip.pos[2] = pk[i].z;
        ip.intensity = pk[i].intensity;
    }
    ip.is_max = pk[i].is_max;
    ips[i] = ip;
}

// The candidates (threshold / 10 with the DoG's quadratic localisation: millions on a
// noisy 768^3 view) stay on the device; only the interest points are copied out.
void points_from_peaks(DogWork& w, const DogRun& r, int localization, float keep_thr, spim_interest_point* out,
                       int64_t max_out, int64_t* nout, hipStream_t s) {
    const int64_t np = r.np;
    int64_t n = 0;
    const spim_interest_point* res = nullptr;
    if (np > 0) {
        grow(w.ips, size_t(np));
        const unsigned grid = unsigned(ceil_div(np, int64_t(256)));
        if (localization == 0) {
            hipLaunchKernelGGL(k_to_points<false>, dim3(grid), dim3(256), 0, s, r.dpeaks, nullptr, np, 0.0f,
                               w.ips.p, nullptr);
            SD_HIP(hipGetLastError());
            res = w.ips.p;
            n = np;
        } else {
            grow(w.loc, size_t(np));
            grow(w.flags, size_t(np));
            grow(w.ips_sel, size_t(np));
            grow(w.nsel, 1);
            hipLaunchKernelGGL(k_localize, dim3(grid), dim3(256), 0, s, r.dog, r.d, r.dpeaks, np, w.loc.p);
            SD_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_to_points<true>, dim3(grid), dim3(256), 0, s, r.dpeaks, w.loc.p, np, keep_thr,
                               w.ips.p, w.flags.p);
            SD_HIP(hipGetLastError());
            const size_t tb = point_select_temp_bytes(np);
            grow(w.sel_tmp, std::max<size_t>(tb, 1));
            point_select(w.sel_tmp.p, tb, w.ips.p, w.flags.p, w.ips_sel.p, w.nsel.p, np, s);
            int hn = 0;
            SD_HIP(hipMemcpyAsync(&hn, w.nsel.p, sizeof(int), hipMemcpyDeviceToHost, s));
            SD_HIP(hipStreamSynchronize(s));
            res = w.ips_sel.p;
            n = hn;
        }
    }
    const int64_t m = out ? std::min<int64_t>(max_out, n) : 0;
    if (m > 0) SD_HIP(hipMemcpyAsync(out, res, size_t(m) * sizeof(spim_interest_point), hipMemcpyDefault, s));
    SD_HIP(hipStreamSynchronize(s));
    *nout = n;
}

// ---------------------------------------------------------------- the stage on a caller's image
namespace {

struct DetectArgs {   // (what check_detector_args reads of a detector's parameters)
    int localization, ij_threads;
};

// the caller's image staged (or read in place) and its candidates, for both entries
void detect_run(const float* img, const int64_t* dims, float min_peak, int find_min, int find_max, int T, int route,
                int device, hipStream_t s, DogWork& w, DogRun& r) {
    const Dims3 d{dims[0], dims[1], dims[2]};
    const float* in = stage_in(img, d.nx * d.ny * d.nz, device, w.in, s);
    detect_stored(w, d, in, min_peak, find_min ? 1 : 0, find_max ? 1 : 0, T, s, r, route);
}

void detect_check(const float* img, const int64_t* dims, const DetectArgs& a, int route) {
    check_detector_args(img, dims, &a, [&] {
        SD_CHECK(dims[0] < (int64_t(1) << 31) && dims[1] < (int64_t(1) << 31) && dims[2] < (int64_t(1) << 31) &&
                     dims[0] * dims[1] < (int64_t(1) << 31) && dims[0] * dims[1] * dims[2] < (int64_t(1) << 40),
                 SPIMDECON_ERR_ARG, "volume too large");
        SD_CHECK(route == SPIM_DETECT_ROUTE_AUTO || route == SPIM_DETECT_ROUTE_WAVE || route == SPIM_DETECT_ROUTE_APPEND,
                 SPIMDECON_ERR_ARG, "route must be SPIM_DETECT_ROUTE_AUTO (0), _WAVE (1) or _APPEND (2)");
        SD_CHECK(route != SPIM_DETECT_ROUTE_WAVE || image_below_4gib(dims[0] * dims[1] * dims[2]), SPIMDECON_ERR_ARG,
                 "SPIM_DETECT_ROUTE_WAVE needs an image below 4 GiB");
    });
}

}  // namespace

void detect_peaks(const float* img, const int64_t* dims, float min_peak, int find_min, int find_max, int T, int route,
                  int device, spim_peak* peaks, int64_t max_peaks, int64_t* npeaks) {
    SD_CHECK(npeaks, SPIMDECON_ERR_ARG, "null argument");
    detect_check(img, dims, DetectArgs{0, T}, route);
    with_work<DogWork>(device, [&](DogWork& w, hipStream_t s) {
        DogRun r;
        detect_run(img, dims, min_peak, find_min, find_max, T, route, device, s, w, r);
        peaks_to_host(r, peaks, max_peaks, npeaks, s);
    });
}

void detect_interest_points(const float* img, const int64_t* dims, float min_peak, int find_min, int find_max, int T,
                            int route, int device, int localization, float keep_thr, spim_interest_point* out,
                            int64_t max_out, int64_t* nout) {
    SD_CHECK(nout, SPIMDECON_ERR_ARG, "null argument");
    detect_check(img, dims, DetectArgs{localization, T}, route);
    with_work<DogWork>(device, [&](DogWork& w, hipStream_t s) {
        DogRun r;
        detect_run(img, dims, min_peak, find_min, find_max, T, route, device, s, w, r);
        points_from_peaks(w, r, localization, keep_thr, out, max_out, nout, s);
    });
}

void dog_release_workspace(int dev) {
    with_work<DogWork>(dev, [](DogWork& w) {
        SD_HIP(hipDeviceSynchronize());
        w.release();
    });
}

}  // namespace spimdecon

extern "C" int spim_dog_release_workspace(int device) {
    return spimdecon::guarded([&] { spimdecon::dog_release_workspace(device); });
}

extern "C" int spim_detect_peaks(const float* img, const int64_t* dims, float min_peak, int32_t find_min,
                                 int32_t find_max, int32_t ij_threads, int32_t route, int32_t device,
                                 spim_peak* peaks, int64_t max_peaks, int64_t* npeaks) {
    return spimdecon::guarded([&] {
        spimdecon::detect_peaks(img, dims, min_peak, find_min, find_max, ij_threads, route, device, peaks, max_peaks,
                                npeaks);
    });
}

extern "C" int spim_detect_interest_points(const float* img, const int64_t* dims, float min_peak, int32_t find_min,
                                           int32_t find_max, int32_t ij_threads, int32_t route, int32_t device,
                                           int32_t localization, float keep_threshold, spim_interest_point* out,
                                           int64_t max_out, int64_t* nout) {
    return spimdecon::guarded([&] {
        spimdecon::detect_interest_points(img, dims, min_peak, find_min, find_max, ij_threads, route, device,
                                          localization, keep_threshold, out, max_out, nout);
    });
}

extern "C" void spim_detect_tiles(int32_t sizes[5]) {
    using namespace spimdecon;
    if (!sizes) return;
    sizes[0] = kDpkX;
    sizes[1] = kDpkY;
    sizes[2] = kDpkZ;
    sizes[3] = kCandBuf;
    sizes[4] = int32_t(kCandCapFloor);
}
