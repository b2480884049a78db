// hostcall.hpp -- the host scaffold every call shares: the stream of one call, the head of a
// per-device workspace and the call around it, the staging of a volume in and out, the
// volume-dims rule and the imglib1 Gaussian.
#pragma once

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.hpp"

namespace spimdecon {

// the non-blocking stream of one call
struct ScopedStream {
    hipStream_t s = nullptr;
    ScopedStream() { SD_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~ScopedStream() { (void)hipStreamDestroy(s); }
    ScopedStream(const ScopedStream&) = delete;
    ScopedStream& operator=(const ScopedStream&) = delete;
};

// What every per-device workspace starts with.  One call at a time per workspace and device
// holds mu; the stream is created once (a stream per call cost ~1 ms of host time per 768^3
// DoG call: r3l trace, 1.17 ms before the first copy).
struct WorkBase {
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipStream_t get_stream() {
        if (!stream) SD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return stream;
    }
    void release_stream() {
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};

template <class... B>
void release_all(B&... b) {
    (b.release(), ...);
}

// One call on `device`: body(w, s) with the device's W and its stream, held under its mutex
// (body(w) where the call needs no stream of W's)
template <class W, typename Body>
void with_work(int device, Body&& body) {
    check_device(device);
    DeviceGuard guard(device);
    W& w = per_device<W>(device);
    std::lock_guard<std::mutex> lk(w.mu);
    if constexpr (std::is_invocable_v<Body, W&>)
        body(w);
    else
        body(w, w.get_stream());
}

// frees the device's W where there is one
template <class W>
void release_work(int device) {
    SD_CHECK(device >= 0, SPIMDECON_ERR_ARG, "bad device");
    PerDevice<W> all = per_device_all<W>();
    auto it = all.by_dev.find(device);
    if (it == all.by_dev.end() || !it->second) return;
    DeviceGuard guard(device);
    std::lock_guard<std::mutex> lk(it->second->mu);
    it->second->release();
}

// the image of n voxels on the device: read in place when it already lives in the device's
// HBM, else one upload into buf (from the host or another device)
inline const float* stage_in(const float* img, int64_t n, int device, DBuf<float>& buf, hipStream_t s) {
    if (is_device_ptr(img, device)) return img;
    grow(buf, size_t(n));
    SD_HIP(hipMemcpyAsync(buf.p, img, size_t(n) * 4, hipMemcpyDefault, s));
    return buf.p;
}

// Where a call's image of n voxels goes: the caller's buffer when that is memory of the
// device, else a buffer of the call's, copied out to the caller's (if any) at the end.
struct ImageDest {
    float* out;            // the caller's buffer, or nullptr
    bool out_dev;          // ... is device memory
    int64_t n;
    float* p = nullptr;    // where the kernels write; nullptr: the image is not stored
    ImageDest(float* out, int64_t n, int device) : out(out), out_dev(out && is_device_ptr(out, device)), n(n) {}
    float* store(DBuf<float>& buf) {
        if (!p && !out_dev) grow(buf, size_t(n));
        if (!p) p = out_dev ? out : buf.p;
        return p;
    }
    void copy_out(hipStream_t s) const {
        if (out && !out_dev) SD_HIP(hipMemcpyAsync(out, p, n * 4, hipMemcpyDefault, s));
    }
};

// The extents of a volume: each >= 1 (else `bad`) and below 2^30 (else `large`), both
// SPIMDECON_ERR_ARG; returns the voxels (modulo 2^64: a caller with a limit on the plane or
// the volume checks the plane first)
inline int64_t check_volume(const int64_t* dims, const char* bad, const char* large) {
    SD_CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, SPIMDECON_ERR_ARG, bad);
    constexpr int64_t lim = int64_t(1) << 30;
    SD_CHECK(dims[0] < lim && dims[1] < lim && dims[2] < lim, SPIMDECON_ERR_ARG, large);
    return int64_t(uint64_t(dims[0]) * uint64_t(dims[1]) * uint64_t(dims[2]));
}

// imglib1 Util.createGaussianKernel1DDouble(sigma, true)
inline std::vector<double> gaussian_kernel(double sigma) {
    std::vector<double> g;
    if (sigma <= 0) {
        g.assign(3, 0.0);
        g[1] = 1.0;
    } else {
        const int size = std::max(3, 2 * int(3 * sigma + 0.5) + 1);
        const double two_sq = 2 * sigma * sigma;
        g.assign(size, 0.0);
        const int c = size / 2;
        for (int x = c; x >= 0; --x) {
            const double val = std::exp(-(double(x) * x) / two_sq);
            g[c - x] = val;
            g[c + x] = val;
        }
    }
    double sum = 0;
    for (double v : g) sum += v;
    for (double& v : g) v /= sum;
    return g;
}

}  // namespace spimdecon
