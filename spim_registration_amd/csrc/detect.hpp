// detect.hpp -- what the detectors (dog.hip, dom.hip) and the downsampler (downsample.hip)
// share (detect.hip): the per-device workspace with its mutex and stream, the scaffold of a
// call, and the detection stage -- everything that starts from a stored device image: the
// candidate pass (InteractiveIntegral.findPeaks), the x % T order, the fit and the selection.
#pragma once

#include <algorithm>

#include "hostcall.hpp"

namespace spimdecon {

constexpr int kBlock = 256;
inline unsigned grid_of(int64_t n, int64_t cap = 4096) {
    int64_t b = ceil_div(n, kBlock);
    return unsigned(b < 1 ? 1 : (b > cap ? cap : b));
}

// a float image of n voxels lies below 4 GiB: one buffer resource with 32-bit offsets covers
// it (k_dog_peaks and the buffer loads of k_dog_xy address it so)
inline bool image_below_4gib(int64_t n) { return uint64_t(n) * 4u < 0xffffffffull; }

struct PeakOut {   // (cand_flush writes it as three int pairs)
    int32_t x, y, z;
    float intensity;
    int32_t is_min, is_max;
};

// candidate sink: unordered append of (key, record); count may exceed cap (the host reruns)
struct PeakSink {
    float minv;
    int want_min, want_max, T;
    uint64_t* keys;
    uint32_t* vals;
    PeakOut* recs;
    unsigned* count;
    unsigned cap;
};

struct LocOut {
    float pos[3];
    float value;
};

// Per-device DoG workspace, grown on demand and kept between calls (a 768^3 view needs
// ~3.6 GB of G12 plus the candidate lists; hipMalloc / hipFree of that per call cost
// more than the DoG itself).  One call at a time per device holds its mutex;
// spim_dog_release_workspace frees it.  (The DOM detector and the downsampler stage their
// input in `in` and write their image to `dog`: they add no buffer of their own.)
struct DogWork : WorkBase {
    DBuf<float> in, dog, taps, mm, tmp_a, tmp_b, tmp_c, tmp_d;
    DBuf<float2> g12;
    DBuf<uint64_t> keys, keys_sorted;
    DBuf<uint32_t> vals, vals_sorted;
    DBuf<PeakOut> recs, peaks;
    DBuf<unsigned> count;
    DBuf<unsigned char> sort_tmp;
    DBuf<LocOut> loc;                      // localisation results
    DBuf<spim_interest_point> ips, ips_sel;  // interest points before / after the threshold
    DBuf<unsigned char> flags, sel_tmp;
    DBuf<int> nsel;
    DBuf<PeakSink> sink;                   // the candidate kernels' sink, read at their flushes
    void release() {
        release_stream();
        release_all(in, dog, taps, mm, tmp_a, tmp_b, tmp_c, tmp_d, g12, keys, keys_sorted, vals, vals_sorted, recs,
                    peaks, count, sort_tmp, loc, ips, ips_sel, flags, sel_tmp, nsel, sink);
    }
};

// The argument rules DoG and DoM share; `own()` runs the detector's own between the view's
// and the localisation's.
template <typename Params, typename Own>
void check_detector_args(const float* img, const int64_t* dims, const Params* p, Own&& own) {
    SD_CHECK(img && dims && p, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, SPIMDECON_ERR_ARG, "bad dims");
    own();
    SD_CHECK(p->localization == 0 || p->localization == 1, SPIMDECON_ERR_ARG,
             "localization must be 0 (none) or 1 (quadratic); the Gaussian fit is not implemented in "
             "the reference either (Localization.java:90-96)");
    SD_CHECK(p->ij_threads >= 1 && p->ij_threads < (1 << 20), SPIMDECON_ERR_ARG, "ij_threads must be >= 1");
}

// ---------------------------------------------------------------- the detection stage
// the detector's image (on the device) and the reference-ordered candidate list (on the device)
struct DogRun {
    Dims3 d{};
    const float* dog = nullptr;   // nullptr when neither localisation nor the image was asked for
    int64_t np = 0;
    const PeakOut* dpeaks = nullptr;
};

// the least capacity of the candidate lists (collect_candidates)
constexpr int64_t kCandCapFloor = int64_t(1) << 16;

// The candidate pass of a detector: `launch(pk, attempt)` enqueues the kernel(s) that append
// to the sink pk; a count beyond the capacity reruns it once with room for every candidate.
template <typename Launch>
unsigned collect_candidates(DogWork& w, int64_t n, float min_peak, int wmin, int wmax, int T, hipStream_t s,
                            Launch&& launch) {
    grow(w.count, 1);
    unsigned cap = unsigned(std::min<int64_t>(std::max<int64_t>(kCandCapFloor, n / 256), int64_t(1) << 30));
    cap = std::max<unsigned>(cap, unsigned(std::min<size_t>(w.recs.n, size_t(1) << 30)));
    unsigned total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        grow(w.keys, cap);
        grow(w.vals, cap);
        grow(w.recs, cap);
        SD_HIP(hipMemsetAsync(w.count.p, 0, sizeof(unsigned), s));
        const PeakSink pk{min_peak, wmin, wmax, T, w.keys.p, w.vals.p, w.recs.p, w.count.p, cap};
        launch(pk, attempt);
        SD_HIP(hipGetLastError());
        SD_HIP(hipMemcpyAsync(&total, w.count.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        if (total <= cap) break;
        cap = total;          // rerun with room for every candidate (the image is already stored)
    }
    return total;
}

// candidates of a stored image: k_dog_peaks, or k_peaks_append where its limits are not met
void stored_candidates(DogWork& w, const Dims3& d, const float* dogp, bool peaks_kernel, const PeakSink& pk,
                       hipStream_t s);

// reference order: ascending (x % T) << 40 | flat, into r.np / r.dpeaks
void sort_candidates(DogWork& w, unsigned total, int T, hipStream_t s, DogRun& r);

// InteractiveIntegral.findPeaks over a stored device image: the extrema with
// |v| >= min_peak of the wanted kinds, in the reference's order, into r.np / r.dpeaks
// (the workspace's memory).  Synchronises the stream.  route: SPIM_DETECT_ROUTE_* (AUTO:
// k_dog_peaks where the image lies below 4 GiB, else k_peaks_append).
void detect_stored(DogWork& w, const Dims3& d, const float* img, float min_peak, int want_min, int want_max, int T,
                   hipStream_t s, DogRun& r, int route = SPIM_DETECT_ROUTE_AUTO);

// the first min(r.np, max_peaks) candidates to the host; *npeaks = r.np
void peaks_to_host(const DogRun& r, spim_peak* peaks, int64_t max_peaks, int64_t* npeaks, hipStream_t s);

// Localization.noLocalization (0) or computeQuadraticLocalization (1: the fit over r.dog,
// kept when |fitted value| > keep_thr) of the candidates; out may be host or device memory
void points_from_peaks(DogWork& w, const DogRun& r, int localization, float keep_thr, spim_interest_point* out,
                       int64_t max_out, int64_t* nout, hipStream_t s);

// ---------------------------------------------------------------- dog_sort.hip
size_t peak_sort_temp_bytes(int64_t n, int end_bit);
void peak_sort(void* tmp, size_t tmp_bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin,
               uint32_t* vout, int64_t n, int end_bit, hipStream_t s);
size_t point_select_temp_bytes(int64_t n);
void point_select(void* tmp, size_t tmp_bytes, const spim_interest_point* in, const unsigned char* flags,
                  spim_interest_point* out, int* nsel, int64_t n, hipStream_t s);

}  // namespace spimdecon
