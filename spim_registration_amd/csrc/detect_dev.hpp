// detect_dev.hpp -- the device-inline pieces the candidate kernels share: k_dog_z (dog.hip)
// and k_dog_peaks (detect.hip) collect their candidates per wave and flush them to the sink
// the same way, and both test with min3 / max3.
#pragma once

#include "detect.hpp"

namespace spimdecon {

// Per-wave candidate buffer of k_dog_z and k_dog_peaks: entries {x, y | sp << 30, z, bits(|c|)} collect in
// LDS and go to the sink 64 at a time (one global atomic per flush instead of one per
// wave-step with a candidate; its returned value is the only vmcnt(0) in the loop)
constexpr int kCandBuf = 64;
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (the sink is read through a pointer: its fields are loaded here, at a flush, instead of
// holding 10 SGPRs for the whole z loop)
// (global-address-space stores and atomic: flat ones count in both vmcnt and lgkmcnt,
// and a flat operation pending at a join made every later load wait in k_dog_z's
// loop a vmcnt(0) -- the plane prefetch drained three times per unrolled rotation)
template <typename T>
__device__ __forceinline__ __attribute__((address_space(1))) T* gbl(T* p) {
    return (__attribute__((address_space(1))) T*)p;
}
__device__ __forceinline__ void cand_flush(const PeakSink* __restrict__ sink, const int4* buf, int n, int nx,
                                           uint32_t pstride) {
    if (n == 0) return;
    wave_lds_sync();
    const PeakSink pk = *sink;
    const int lane = int(threadIdx.x & 63);
    unsigned base = 0;
    if (lane == 0)
        base = __hip_atomic_fetch_add(gbl(pk.count), unsigned(n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = unsigned(__shfl(int(base), 0, 64));
    if (lane < n) {
        const int4 e = buf[lane];
        const unsigned pos = base + unsigned(lane);
        if (pos < pk.cap) {
            const int x = e.x, y = e.y & 0x3fffffff, sp = int(unsigned(e.y) >> 30), z = e.z;
            *gbl(pk.keys + pos) = (uint64_t(x % pk.T) << 40) | (uint64_t(z) * pstride + uint64_t(y) * uint32_t(nx) + x);
            *gbl(pk.vals + pos) = pos;
            // the PeakOut record {x, y, z, intensity, is_min, is_max} as three 8-B stores
            typedef int v2i __attribute__((ext_vector_type(2)));
            v2i* r = reinterpret_cast<v2i*>(pk.recs + pos);
            *gbl(r) = v2i{x, y};
            *gbl(r + 1) = v2i{z, e.w};
            *gbl(r + 2) = v2i{sp == 1 ? 1 : 0, sp == 2 ? 1 : 0};
        }
    }
    wave_lds_sync();   // the buffer is rewritten after the flush
}

// min / max of three, one instruction (NaN-free inputs: planes holding a NaN take the
// kernels' comparison loops; minnum / maxnum would add canonicalising maxes of the LDS values)
__device__ __forceinline__ float dz_min3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float dz_max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

}  // namespace spimdecon
