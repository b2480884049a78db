// autobbox.hip -- "Estimate automatically (experimental)": the fusion bounding box from the data, on MI355X.
//
// References (under the reference's src/main/java/spim/process/fusion/):
//   boundingbox/AutomaticBoundingBox.java:36-131          the maximal box of all views, rounded
//   boundingbox/BoundingBoxGUI.java:340-399               getDimensions, computeMaxBoundingBoxDimensions
//   boundingbox/automatic/MinFilterThreshold.java:76-308  run, computeBoundingBox, computeLazyMinFilter
//   FusionHelper.java:87-138                              minMax
//
// The maximal box is fused at the dialog's downsampling (nearest neighbour, no blending: the
// existing fusion kernel, into device memory), then
//   min / max      Math.min / Math.max from +-Float.MAX_VALUE   k_minmax_partial, k_minmax_final
//   threshold      double(float(max - min)) * (background / 100.0) + double(min)            (host)
//   minimum filter x, then y, then z; window 2r + 1 over a zero extension; Math.min
//                  from Float.MAX_VALUE                                  k_minfilter<axis>
//   box            of the voxels with double(v) > threshold             folded into the z pass
// Math.min is exact and associative (for one NaN payload), so the order of evaluation inside
// a window does not show in the bits; every axis still ends in min(Float.MAX_VALUE, .) as the
// reference's loop does (a window of +Inf gives Float.MAX_VALUE).
//
// k_minfilter: one wave per block; the wave owns 64 lines and a tile of outputs along the
// pass axis.  It stages the tile with its halo of r on both sides (zeros outside the image) in
// LDS, then every lane walks its own line: window minima by doubling, in place and ascending,
//   m_1 = in,  m_2k[i] = min(m_k[i], m_k[i + k]),  out[i] = min(m_p[i], m_p[i + w - p]),
// p the largest power of two <= w (the two windows overlap: min is idempotent).  Element i is
// written after i and i + k are read and nothing below i is read again, so no second buffer and
// no barrier between the levels.  LDS is [position][line]: lanes = lines are conflict-free;
// along x the global rows are read and written with lanes = positions, through a pitch of 65.
// The z pass tests its outputs against the threshold where it holds them and stores the
// filtered image only when the caller wants it: the segmentation path ends in six integers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fusion.hpp"
#include "hostcall.hpp"
#include "minmax.hpp"

namespace spimdecon {
namespace {

constexpr int kMfLines = 64;            // lines per block = lanes of its one wave
constexpr int kMfTileSmall = 64;        // outputs per line and block, r <= kMfSmallRadius
constexpr int kMfTileLarge = 128;       // ... above it (the halo of 2r is shared by more outputs)
constexpr int kMfSmallRadius = 16;
constexpr int kMfMaxRadius = SPIM_MIN_FILTER_MAX_RADIUS;

static_assert((kMfTileLarge + 2 * kMfMaxRadius) * (kMfLines + 1) * 4 <= 160 * 1024, "LDS of one block");

// Java Math.min / Math.max on floats: a NaN operand is the result (the first one), -0 < +0
__device__ __forceinline__ float jmin(float a, float b) {
    float m = b < a ? b : a;               // a when either is NaN
    if (b != b && a == a) m = b;
    if (a == b) m = __uint_as_float(__float_as_uint(a) | __float_as_uint(b));   // equal: the same bits, or +-0
    return m;
}
__device__ __forceinline__ float jmax(float a, float b) {
    float m = b > a ? b : a;
    if (b != b && a == a) m = b;
    if (a == b) m = __uint_as_float(__float_as_uint(a) & __float_as_uint(b));
    return m;
}

struct BoxMinMax {   // the rule of minmax.hpp's reduction
    static __device__ __forceinline__ float mn(float a, float b) { return jmin(a, b); }
    static __device__ __forceinline__ float mx(float a, float b) { return jmax(a, b); }
};

// ---------------------------------------------------------------- the box of voxels above a threshold
// box: min x, y, z (start: the dims), max x, y, z (start: 0).  A lane's box, reduced over its
// wave; lane 0 then extends the global one.  The plain read may be stale, which only costs an
// atomic that changes nothing: the box only ever grows, and min / max do not care about order.
struct LaneBox {
    int lo[3], hi[3];
};

__device__ __forceinline__ void box_commit(LaneBox b, int* __restrict__ box) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int off = 32; off > 0; off >>= 1) {
            b.lo[a] = min(b.lo[a], __shfl_xor(b.lo[a], off, 64));
            b.hi[a] = max(b.hi[a], __shfl_xor(b.hi[a], off, 64));
        }
    if ((threadIdx.x & 63) != 0) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (b.lo[a] < __hip_atomic_load(box + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(box + a, b.lo[a]);
        if (b.hi[a] > __hip_atomic_load(box + 3 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(box + 3 + a, b.hi[a]);
    }
}

__global__ __launch_bounds__(kRedBlock) void k_threshold_box(const float* __restrict__ img, int nx, int ny, int nz,
                                                             double thr, int* __restrict__ box) {
    LaneBox b{{nx, ny, nz}, {0, 0, 0}};
    const int64_t n = int64_t(nx) * ny * nz;
    for (int64_t i = int64_t(blockIdx.x) * kRedBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kRedBlock) {
        if (!(double(img[i]) > thr)) continue;
        const int64_t q = i / nx;
        const int p[3] = {int(i - q * nx), int(q % ny), int(q / ny)};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = min(b.lo[a], p[a]);
            b.hi[a] = max(b.hi[a], p[a]);
        }
    }
    box_commit(b, box);
}

// ---------------------------------------------------------------- the minimum filter
struct MfGeom {
    int nx, ny, nz;
    int r;          // 1 .. kMfMaxRadius
    int tile;       // outputs per line and block
    int nat;        // tiles along the pass axis
    int nlt;        // groups of 64 lines (AXIS 0: of the ny * nz rows; else: of the nx columns)
};

// AXIS 0: lines are rows (consecutive in memory), positions run along x.
// AXIS 1 / 2: lines are 64 consecutive x at one index o of the third axis, positions run along
// y (stride nx; o = z) or z (stride nx * ny; o = y).
// out may be nullptr (AXIS 2 with BOX: only the box is wanted); in == out is not allowed.
template <int AXIS, bool BOX>
__global__ __launch_bounds__(kMfLines) void k_minfilter(const float* __restrict__ in, float* __restrict__ out,
                                                        MfGeom g, double thr, int* __restrict__ box) {
    extern __shared__ __attribute__((aligned(16))) float mf_lds[];
    constexpr int LP = AXIS == 0 ? kMfLines + 1 : kMfLines;   // floats between two positions
    const int lane = int(threadIdx.x);
    const int n = AXIS == 0 ? g.nx : AXIS == 1 ? g.ny : g.nz;
    const unsigned bid = blockIdx.x;
    const int at = int(bid % unsigned(g.nat));
    const unsigned rest = bid / unsigned(g.nat);
    const int p0 = at * g.tile;
    const int tile = min(g.tile, n - p0);
    const int P = tile + 2 * g.r;           // staged positions: p0 - r .. p0 + tile + r - 1
    const int64_t plane = int64_t(g.nx) * g.ny;

    // where the block's lines start and what separates two positions
    int64_t base = 0, pstride = 1;
    int nlines = 0;                          // lines of this block that exist
    if (AXIS == 0) {
        const int64_t rows = int64_t(g.ny) * g.nz, l0 = int64_t(rest) * kMfLines;
        base = l0 * g.nx;
        nlines = rows - l0 < kMfLines ? int(rows - l0) : kMfLines;
    } else {
        const int lt = int(rest % unsigned(g.nlt)), o = int(rest / unsigned(g.nlt));
        const int x0 = lt * kMfLines;
        nlines = min(kMfLines, g.nx - x0);
        pstride = AXIS == 1 ? g.nx : plane;
        base = x0 + int64_t(o) * (AXIS == 1 ? plane : int64_t(g.nx));
    }

    if (AXIS == 0) {
#pragma unroll 4
        for (int l = 0; l < kMfLines; ++l) {
            const float* row = in + base + int64_t(l) * g.nx;
            for (int p = lane; p < P; p += 64) {
                const int gx = p0 - g.r + p;
                mf_lds[p * LP + l] = (l < nlines && gx >= 0 && gx < n) ? row[gx] : 0.0f;
            }
        }
    } else {
        const float* col = in + base + lane;
#pragma unroll 8
        for (int p = 0; p < P; ++p) {
            const int gp = p0 - g.r + p;
            mf_lds[p * LP + lane] = (lane < nlines && gp >= 0 && gp < n) ? col[int64_t(gp) * pstride] : 0.0f;
        }
    }
    __syncthreads();

    // every lane its own line, in place and ascending
    float* line = mf_lds + lane;
    const int w = 2 * g.r + 1;
    int k = 1;
    for (; 2 * k <= w; k *= 2) {
        const int cnt = P - 2 * k + 1;       // m_2k[i] exists for i + 2k - 1 < P
        int i = 0;
        for (; i + 4 <= cnt; i += 4) {
            float a[4], b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = line[(i + j) * LP];
                b[j] = line[(i + j + k) * LP];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) line[(i + j) * LP] = jmin(a[j], b[j]);
        }
        for (; i < cnt; ++i) line[i * LP] = jmin(line[i * LP], line[(i + k) * LP]);
    }
    const int sh = w - k;                    // k = p; 1 <= sh < k
    LaneBox lb{{g.nx, g.ny, g.nz}, {0, 0, 0}};
    for (int i = 0; i < tile; ++i) {
        const float v = jmin(kFloatMax, jmin(line[i * LP], line[(i + sh) * LP]));
        if (AXIS == 0) {
            line[i * LP] = v;                // (i + sh > i: not read again)
        } else if (lane < nlines) {
            if (out) out[base + lane + int64_t(p0 + i) * pstride] = v;
            if (BOX && double(v) > thr) {
                lb.lo[AXIS] = min(lb.lo[AXIS], p0 + i);
                lb.hi[AXIS] = max(lb.hi[AXIS], p0 + i);
            }
        }
    }
    if (AXIS == 0) {
        __syncthreads();
        for (int l = 0; l < nlines; ++l) {
            float* row = out + base + int64_t(l) * g.nx + p0;
            for (int p = lane; p < tile; p += 64) row[p] = mf_lds[p * LP + l];
        }
    } else if (BOX) {
        if (lb.lo[AXIS] <= lb.hi[AXIS]) {    // the lane found a voxel: its x and the block's o
            const int lt = int(rest % unsigned(g.nlt)), o = int(rest / unsigned(g.nlt));
            const int x = lt * kMfLines + lane;
            constexpr int OA = AXIS == 1 ? 2 : 1;
            lb.lo[0] = lb.hi[0] = x;
            lb.lo[OA] = lb.hi[OA] = o;
        }
        box_commit(lb, box);
    }
}

// ---------------------------------------------------------------- host side
struct BoxWork : WorkBase {
    DBuf<float> t1, t2, fused, red;
    DBuf<int> box;
    void release() {
        release_stream();
        release_all(t1, t2, fused, red, box);
    }
};

int64_t check_image(const float* img, const int64_t* dims) {
    SD_CHECK(img && dims, SPIMDECON_ERR_ARG, "null argument");
    const int64_t n = check_volume(dims, "bad dims", "volume too large");
    SD_CHECK(dims[0] * dims[1] < (int64_t(1) << 31) && n < (int64_t(1) << 40), SPIMDECON_ERR_ARG,
             "volume too large");
    return n;
}

void check_radius(int radius) {
    SD_CHECK(radius >= 1, SPIMDECON_ERR_ARG, "minimum filter: radius must be >= 1");
    SD_CHECK(radius <= kMfMaxRadius, SPIMDECON_ERR_ARG,
             "minimum filter: radius above " + std::to_string(kMfMaxRadius) + " is not supported");
}

void check_background(double background) {
    SD_CHECK(std::isfinite(background) && background > 0.0 && background < 100.0, SPIMDECON_ERR_ARG,
             "background must lie inside (0, 100) percent");
}

void minmax_device(BoxWork& w, const float* dimg, int64_t n, float* mn, float* mx, hipStream_t s) {
    grow(w.red, size_t(2 * kRedGrid + 2));
    float* mm = w.red.p + 2 * kRedGrid;
    minmax_launch<BoxMinMax>(dimg, n, minmax_parts(n), w.red.p, mm, s);
    SD_HIP(hipGetLastError());
    float h[2];
    SD_HIP(hipMemcpyAsync(h, mm, sizeof(h), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
    *mn = h[0];
    *mx = h[1];
}

// MinFilterThreshold.run (:90): float difference, the rest in double
double threshold_of(float mn, float mx, double background) {
    const float range = mx - mn;
    return double(range) * (background / 100.0) + double(mn);
}

void box_reset(BoxWork& w, const int64_t* dims, hipStream_t s) {
    grow(w.box, 8);
    const int h[6] = {int(dims[0]), int(dims[1]), int(dims[2]), 0, 0, 0};
    SD_HIP(hipMemcpyAsync(w.box.p, h, sizeof(h), hipMemcpyHostToDevice, s));
    SD_HIP(hipStreamSynchronize(s));   // (h is on the stack)
}

// computeBoundingBox's integers; found = some voxel was above the threshold
void box_fetch(BoxWork& w, int64_t* bmin, int64_t* bmax, int32_t* found, hipStream_t s) {
    int h[6];
    SD_HIP(hipMemcpyAsync(h, w.box.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) {
        bmin[a] = h[a];
        bmax[a] = h[3 + a];
    }
    *found = h[0] <= h[3] ? 1 : 0;
}

template <int AXIS, bool BOX>
void launch_filter(const float* in, float* out, const int64_t* dims, int r, double thr, int* box, hipStream_t s) {
    MfGeom g{};
    g.nx = int(dims[0]);
    g.ny = int(dims[1]);
    g.nz = int(dims[2]);
    g.r = r;
    g.tile = r <= kMfSmallRadius ? kMfTileSmall : kMfTileLarge;
    g.nat = int(ceil_div(dims[AXIS], g.tile));
    int64_t blocks;
    if (AXIS == 0) {
        g.nlt = int(ceil_div(dims[1] * dims[2], kMfLines));
        blocks = int64_t(g.nat) * g.nlt;
    } else {
        g.nlt = int(ceil_div(dims[0], kMfLines));
        blocks = int64_t(g.nat) * g.nlt * dims[AXIS == 1 ? 2 : 1];
    }
    SD_CHECK(blocks < (int64_t(1) << 31), SPIMDECON_ERR_ARG, "volume too large");
    constexpr int LP = AXIS == 0 ? kMfLines + 1 : kMfLines;
    const size_t lds = size_t(g.tile + 2 * r) * LP * sizeof(float);
    auto kern = &k_minfilter<AXIS, BOX>;
    SD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(lds)));
    hipLaunchKernelGGL(kern, dim3(unsigned(blocks)), dim3(kMfLines), lds, s, in, out, g, thr, box);
    SD_HIP(hipGetLastError());
}

// x: in -> t1, y: t1 -> t2, z: t2 -> dst (may be nullptr with want_box); in may be t2, dst may be
// t1 or in
void filter_device(BoxWork& w, const float* in, const int64_t* dims, int r, float* dst, bool want_box, double thr,
                   hipStream_t s) {
    const size_t n = size_t(dims[0] * dims[1] * dims[2]);
    grow(w.t1, n);
    grow(w.t2, n);
    launch_filter<0, false>(in, w.t1.p, dims, r, 0.0, nullptr, s);
    launch_filter<1, false>(w.t1.p, w.t2.p, dims, r, 0.0, nullptr, s);
    if (want_box)
        launch_filter<2, true>(w.t2.p, dst, dims, r, thr, w.box.p, s);
    else
        launch_filter<2, false>(w.t2.p, dst, dims, r, 0.0, nullptr, s);
}

void min_max(const float* img, const int64_t* dims, int device, float* mn, float* mx) {
    SD_CHECK(mn && mx, SPIMDECON_ERR_ARG, "null argument");
    const int64_t n = check_image(img, dims);
    with_work<BoxWork>(device, [&](BoxWork& w, hipStream_t s) {
        minmax_device(w, stage_in(img, n, device, w.t2, s), n, mn, mx, s);
    });
}

void min_filter(const float* img, const int64_t* dims, int radius, int device, float* out) {
    SD_CHECK(out, SPIMDECON_ERR_ARG, "null argument");
    const int64_t n = check_image(img, dims);
    check_radius(radius);
    with_work<BoxWork>(device, [&](BoxWork& w, hipStream_t s) {
        const float* in = stage_in(img, n, device, w.t2, s);
        ImageDest dst(out, n, device);
        filter_device(w, in, dims, radius, dst.store(w.t1), false, 0.0, s);
        dst.copy_out(s);
        SD_HIP(hipStreamSynchronize(s));
    });
}

void threshold_bounds(const float* img, const int64_t* dims, double threshold, int device, int64_t* bmin,
                      int64_t* bmax, int32_t* found) {
    SD_CHECK(bmin && bmax && found, SPIMDECON_ERR_ARG, "null argument");
    const int64_t n = check_image(img, dims);
    SD_CHECK(!std::isnan(threshold), SPIMDECON_ERR_ARG, "threshold is NaN");
    with_work<BoxWork>(device, [&](BoxWork& w, hipStream_t s) {
        const float* in = stage_in(img, n, device, w.t2, s);
        box_reset(w, dims, s);
        const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(2048, ceil_div(n, kRedBlock))));
        hipLaunchKernelGGL(k_threshold_box, dim3(grid), dim3(kRedBlock), 0, s, in, int(dims[0]), int(dims[1]),
                           int(dims[2]), threshold, w.box.p);
        SD_HIP(hipGetLastError());
        box_fetch(w, bmin, bmax, found, s);
    });
}

// min / max -> threshold -> filter -> box over a device image, under the workspace's lock
void segment_device(BoxWork& w, const float* dimg, const int64_t* dims, double background, int radius,
                    float* filtered, int device, spim_segment_result* res, hipStream_t s) {
    const int64_t n = dims[0] * dims[1] * dims[2];
    std::memset(res, 0, sizeof(*res));
    minmax_device(w, dimg, n, &res->min, &res->max, s);
    res->threshold = threshold_of(res->min, res->max, background);
    box_reset(w, dims, s);
    // a host `filtered` is written through t1 (free once the y pass has read it)
    ImageDest dst(filtered, n, device);
    filter_device(w, dimg, dims, radius, filtered ? dst.store(w.t1) : nullptr, true, res->threshold, s);
    dst.copy_out(s);
    box_fetch(w, res->bounds_min, res->bounds_max, &res->found, s);
}

void segment_bounds(const float* img, const int64_t* dims, double background, int radius, int device,
                    float* filtered, spim_segment_result* res) {
    SD_CHECK(res, SPIMDECON_ERR_ARG, "null argument");
    const int64_t n = check_image(img, dims);
    check_radius(radius);
    check_background(background);
    with_work<BoxWork>(device, [&](BoxWork& w, hipStream_t s) {
        const float* in = stage_in(img, n, device, w.t2, s);
        segment_device(w, in, dims, background, radius, filtered, device, res, s);
    });
}

// Math.round: floor(x + 0.5), as a Java int
int64_t java_round(double x) { return int64_t(std::floor(x + 0.5)); }

// computeMaxBoundingBoxDimensions + AutomaticBoundingBox.java:55-60 + getDimensions
void max_bounding_box(int nviews, const int64_t* dims, const double* models, int downsampling, int64_t* bb_min,
                      int64_t* bb_max, int64_t* bb_dims, int64_t* fused_dims) {
    SD_CHECK(nviews >= 1 && dims && models && bb_min && bb_max && bb_dims, SPIMDECON_ERR_ARG, "null argument");
    SD_CHECK(downsampling >= 1, SPIMDECON_ERR_ARG, "downsampling must be >= 1");
    double lo[3] = {1.7976931348623157e308, 1.7976931348623157e308, 1.7976931348623157e308};
    double hi[3] = {-lo[0], -lo[0], -lo[0]};
    for (int v = 0; v < nviews; ++v) {
        const int64_t* d = dims + 3 * v;
        const double* m = models + 12 * v;
        SD_CHECK(d[0] >= 1 && d[1] >= 1 && d[2] >= 1, SPIMDECON_ERR_ARG, "bad dims");
        for (int i = 0; i < 12; ++i) SD_CHECK(std::isfinite(m[i]), SPIMDECON_ERR_ARG, "non-finite model");
        for (int c = 0; c < 8; ++c) {       // estimateBounds: the 8 corners of [0, dim - 1]
            const double p[3] = {(c & 1) ? double(d[0] - 1) : 0.0, (c & 2) ? double(d[1] - 1) : 0.0,
                                 (c & 4) ? double(d[2] - 1) : 0.0};
            for (int a = 0; a < 3; ++a) {
                const double t = m[4 * a] * p[0] + m[4 * a + 1] * p[1] + m[4 * a + 2] * p[2] + m[4 * a + 3];
                lo[a] = std::min(lo[a], t);
                hi[a] = std::max(hi[a], t);
            }
        }
    }
    for (int a = 0; a < 3; ++a) {
        SD_CHECK(std::fabs(lo[a]) < 2147483000.0 && std::fabs(hi[a]) < 2147483000.0, SPIMDECON_ERR_ARG,
                 "bounding box beyond the int range");
        bb_min[a] = java_round(lo[a]);
        bb_max[a] = java_round(hi[a]);
        bb_dims[a] = bb_max[a] - bb_min[a] + 1;
        if (fused_dims) fused_dims[a] = bb_dims[a] / downsampling;
    }
}

void auto_bounding_box(int nviews, const spim_view_source* views, const spim_autobbox_params* p,
                       spim_autobbox_result* res) {
    SD_CHECK(nviews >= 1 && views && p && res, SPIMDECON_ERR_ARG, "null argument");
    check_background(p->background);
    SD_CHECK(p->downsampling >= 1, SPIMDECON_ERR_ARG, "downsampling must be >= 1");
    SD_CHECK(p->discarded_object_size >= 0, SPIMDECON_ERR_ARG, "discarded_object_size must be >= 0");
    std::memset(res, 0, sizeof(*res));
    std::vector<int64_t> dims(size_t(3 * nviews));
    std::vector<double> models(size_t(12 * nviews));
    for (int v = 0; v < nviews; ++v) {
        SD_CHECK(views[v].img, SPIMDECON_ERR_ARG, "null view");
        std::memcpy(&dims[size_t(3 * v)], views[v].dims, 3 * sizeof(int64_t));
        std::memcpy(&models[size_t(12 * v)], views[v].model, 12 * sizeof(double));
    }
    max_bounding_box(nviews, dims.data(), models.data(), p->downsampling, res->max_min, res->max_max, res->max_dims,
                     res->fused_dims);
    res->radius_min = p->discarded_object_size / 2;                       // MinFilterThreshold.java:68
    res->eff_radius = std::max(res->radius_min / p->downsampling, 1);     // :89
    check_radius(res->eff_radius);
    SD_CHECK(res->fused_dims[0] >= 1 && res->fused_dims[1] >= 1 && res->fused_dims[2] >= 1, SPIMDECON_ERR_ARG,
             "downsampling leaves no voxel of the maximal bounding box");
    const int64_t n = check_image(views[0].img, res->fused_dims);
    with_work<BoxWork>(p->device, [&](BoxWork& w, hipStream_t s) {
        grow(w.fused, size_t(n));
        spim_fusion_params fp;
        spim_fusion_params_default(&fp);
        for (int a = 0; a < 3; ++a) {
            fp.bb_min[a] = res->max_min[a];
            fp.bb_dims[a] = res->fused_dims[a];
        }
        fp.downsampling = float(p->downsampling);
        fp.interpolation = 0;     // NearestNeighborInterpolatorFactory
        fp.use_blending = 0;      // ProcessParalell(..., false, false)
        fp.device = p->device;
        fp.src_on_device = p->src_on_device;
        fp.out_on_device = 1;
        fuse_weighted_average(nviews, views, &fp, nullptr, nullptr, nullptr, nullptr, w.fused.p);   // (drains its stream)
        segment_device(w, w.fused.p, res->fused_dims, p->background, res->eff_radius, nullptr, p->device, &res->seg,
                       s);
    });
    res->found = res->seg.found;
    for (int a = 0; a < 3; ++a) {     // :112-125; no clamping to the maximal box
        res->bb_min[a] = res->seg.bounds_min[a] * p->downsampling + res->max_min[a] - 3 * int64_t(res->radius_min);
        res->bb_max[a] = res->seg.bounds_max[a] * p->downsampling + res->max_min[a] + 3 * int64_t(res->radius_min);
        res->bb_dims[a] = res->bb_max[a] - res->bb_min[a] + 1;
    }
}

}  // namespace
}  // namespace spimdecon

// ---------------------------------------------------------------- extern "C"
using namespace spimdecon;

extern "C" int spim_max_bounding_box(int nviews, const int64_t* dims, const double* models, int downsampling,
                                     int64_t bb_min[3], int64_t bb_max[3], int64_t bb_dims[3],
                                     int64_t fused_dims[3]) {
    return guarded([&] { max_bounding_box(nviews, dims, models, downsampling, bb_min, bb_max, bb_dims, fused_dims); });
}

extern "C" int spim_min_max(const float* img, const int64_t dims[3], int device, float* min, float* max) {
    return guarded([&] { min_max(img, dims, device, min, max); });
}

extern "C" int spim_min_filter(const float* img, const int64_t dims[3], int radius, int device, float* out) {
    return guarded([&] { min_filter(img, dims, radius, device, out); });
}

extern "C" void spim_min_filter_tiles(int32_t sizes[6]) {
    if (!sizes) return;
    const int32_t v[6] = {kMfLines, kMfTileSmall, kMfTileLarge, kMfSmallRadius, kRedBlock, kRedGrid};
    std::copy(v, v + 6, sizes);
}

extern "C" int spim_threshold_bounds(const float* img, const int64_t dims[3], double threshold, int device,
                                     int64_t bounds_min[3], int64_t bounds_max[3], int32_t* found) {
    return guarded([&] { threshold_bounds(img, dims, threshold, device, bounds_min, bounds_max, found); });
}

extern "C" int spim_segment_bounds(const float* img, const int64_t dims[3], double background, int radius, int device,
                                   float* filtered, spim_segment_result* res) {
    return guarded([&] { segment_bounds(img, dims, background, radius, device, filtered, res); });
}

extern "C" void spim_autobbox_params_default(spim_autobbox_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->background = 5.0;              // AutomaticBoundingBox.defaultBackgroundIntensity
    p->discarded_object_size = 25;    // defaultDiscardedObjectSize
    p->downsampling = 4;              // defaultDownsamplingAutomatic
}

extern "C" int spim_auto_bounding_box(int nviews, const spim_view_source* views, const spim_autobbox_params* p,
                                      spim_autobbox_result* res) {
    return guarded([&] { auto_bounding_box(nviews, views, p, res); });
}

extern "C" int spim_bbox_release_workspace(int device) {
    return guarded([&] { release_work<BoxWork>(device); });
}
