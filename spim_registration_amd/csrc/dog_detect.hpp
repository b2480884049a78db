// dog_detect.hpp -- the detection stage shared by the bead detectors (dog.hip, dom.hip):
// everything that starts from a stored device image.  The candidate pass
// (InteractiveIntegral.findPeaks), the reference's x % T order, the quadratic fit and the
// selection live in dog.hip; the per-device workspace, its mutex and its stream are one for
// both detectors.
#pragma once

#include "common.hpp"

namespace spimdecon {

struct Dims3 {
    int64_t nx, ny, nz;
};

struct PeakOut {   // (k_dog_z's cand_flush writes it as three int pairs)
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
// spim_dog_release_workspace frees it.  (The DOM detector stages its input in `in` and
// writes its image to `dog`: it adds no buffer of its own.)
struct DogWork {
    std::mutex mu;
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
    DBuf<PeakSink> sink;                   // k_dog_z's sink, read at its flushes
    // the calls' stream, created once (a stream per call cost ~1 ms of host time per
    // 768^3 call: r3l trace, 1.17 ms before the first copy)
    hipStream_t stream = nullptr;
    hipStream_t get_stream() {
        if (!stream) SD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return stream;
    }
    void release() {
        if (stream) {
            (void)hipStreamDestroy(stream);
            stream = nullptr;
        }
        for (DBuf<float>* b : {&in, &dog, &taps, &mm, &tmp_a, &tmp_b, &tmp_c, &tmp_d}) b->release();
        g12.release();
        keys.release(); keys_sorted.release(); vals.release(); vals_sorted.release();
        recs.release(); peaks.release(); count.release(); sort_tmp.release();
        loc.release(); ips.release(); ips_sel.release(); flags.release(); sel_tmp.release(); nsel.release();
        sink.release();
    }
};

DogWork& dog_work(int dev);

struct StreamHolder {   // the workspace's stream (held under its mutex)
    hipStream_t s = nullptr;
    explicit StreamHolder(DogWork& w) : s(w.get_stream()) {}
};

// the detector's image (on the device) and the reference-ordered candidate list (on the device)
struct DogRun {
    Dims3 d{};
    const float* dog = nullptr;   // nullptr when neither localisation nor the image was asked for
    int64_t np = 0;
    const PeakOut* dpeaks = nullptr;
};

// InteractiveIntegral.findPeaks over a stored device image: the extrema with
// |v| >= min_peak of the wanted kinds, in the reference's order, into r.np / r.dpeaks
// (the workspace's memory).  Synchronises the stream.
void detect_stored(DogWork& w, const Dims3& d, const float* img, float min_peak, int want_min, int want_max, int T,
                   hipStream_t s, DogRun& r);

// the first min(r.np, max_peaks) candidates to the host; *npeaks = r.np
void peaks_to_host(const DogRun& r, spim_peak* peaks, int64_t max_peaks, int64_t* npeaks, hipStream_t s);

// Localization.noLocalization (0) or computeQuadraticLocalization (1: the fit over r.dog,
// kept when |fitted value| > keep_thr) of the candidates; out may be host or device memory
void points_from_peaks(DogWork& w, const DogRun& r, int localization, float keep_thr, spim_interest_point* out,
                       int64_t max_out, int64_t* nout, hipStream_t s);

}  // namespace spimdecon
