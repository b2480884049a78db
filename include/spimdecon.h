/*
 * spimdecon.h -- C-ABI of libspimdecon.so, the MI355X-native drop-in for the
 * multiview Richardson-Lucy deconvolution + DoG bead-detection hot path of
 * PreibischLab/SPIM_Registration.
 *
 * Reference interfaces replaced (paths under /root/reference/src/main/java/):
 *   - spim/process/cuda/CUDAFourierConvolution.java:4-10      (FourierConvolutionCUDALib, JNA)
 *   - spim/process/cuda/CUDAStandardFunctions.java:15-23      (device query, JNA)
 *   - spim/process/cuda/CUDASeparableConvolution.java:13-21   (SeparableConvolutionCUDALib, JNA)
 *   - spim/process/fusion/deconvolution/MVDeconvolution.java:73-444 (RL loop; new session API)
 *   - spim/process/fusion/deconvolution/MVDeconFFT.java:162-303     (kernel preparation)
 *   - spim/process/interestpointdetection/ProcessDOG.java:40-178    (DoG pass)
 *
 * Conventions
 *   - Plain C types only; every pointer is caller-owned and only read/written
 *     during the call.  Volumes are x-fastest float32 (ImgLib2 ArrayImg order).
 *   - JNA type mapping: Java boolean -> int32_t, Java long -> int64_t,
 *     float[]/int[] -> pointers (JNA copies arrays in and back out).
 *   - Status codes: 0 = OK, negative = error; the message of the last error of
 *     the calling thread is returned by spimdecon_last_error().
 *   - No CPU fallback: a negative/invalid device id or a missing GPU is an
 *     error (status SPIMDECON_ERR_DEVICE), never a silent CPU path.
 */
#ifndef SPIMDECON_H
#define SPIMDECON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPIMDECON_OK               0
#define SPIMDECON_ERR_ARG         -1
#define SPIMDECON_ERR_DEVICE      -2
#define SPIMDECON_ERR_HIP         -3
#define SPIMDECON_ERR_FFT         -4
#define SPIMDECON_ERR_COMM        -5
#define SPIMDECON_ERR_STATE       -6
#define SPIMDECON_ERR_OOM         -7
#define SPIMDECON_ERR_IO          -8   /* file cannot be opened (Java: IOException) */

/* last error message of the calling thread ("" if none) */
const char* spimdecon_last_error(void);
/* library version string, e.g. "spimdecon 0.1.0 gfx950 rocfft 1.0.36" */
const char* spimdecon_version(void);

/* ======================================================================
 * 1. Legacy FourierConvolutionCUDALib ABI
 *    spim/process/cuda/CUDAFourierConvolution.java:9-10; called from
 *    spim/process/fusion/deconvolution/MVDeconFFTThreads.java:65-68,88-91.
 * ====================================================================== */

/* In-place circular 3D convolution of one block with a kernel whose centre
 * kernelDim/2 is moved to the origin (the block already carries the K-1 halo).
 * imDim / kernelDim are REVERSED: {nz, ny, nx} (MVDeconFFTThreads.java:136-144).
 * Thread-safe: one Java thread per device calls this concurrently
 * (MVDeconFFT.java:424-446); per-device plan and stream caches.
 * Java declares `void`; the int status is ignored by such a binding. */
int convolution3DfftCUDAInPlace(float* im, const int* imDim,
                                const float* kernel, const int* kernelDim,
                                int devCUDA);

/* Out-of-place variant (declared at CUDAFourierConvolution.java:9, never
 * called by the reference).  Returns a buffer owned by the library that must
 * be released with spimdecon_free(); NULL on error. */
float* convolution3DfftCUDA(const float* im, const int* imDim,
                            const float* kernel, const int* kernelDim,
                            int devCUDA);
void spimdecon_free(void* p);

/* ======================================================================
 * 2. Device query ABI -- spim/process/cuda/CUDAStandardFunctions.java:15-23,
 *    consumer spim/process/cuda/CUDATools.java:35-192.
 * ====================================================================== */
int     getNumDevicesCUDA(void);                       /* -1 = driver error, 0 = none */
void    getNameDeviceCUDA(int devCUDA, char* name);    /* name: >= 256 bytes */
int64_t getMemDeviceCUDA(int devCUDA);
int64_t getFreeMemDeviceCUDA(int devCUDA);
/* gfx950 is reported as "compute capability" 9.5 (major 9, minor 5) */
int     getCUDAcomputeCapabilityMajorVersion(int devCUDA);
int     getCUDAcomputeCapabilityMinorVersion(int devCUDA);

/* ======================================================================
 * 3. SeparableConvolutionCUDALib ABI -- spim/process/cuda/CUDASeparableConvolution.java:13-17;
 *    caller spim/process/cuda/CUDASeparableConvolutionFunctions.java:176-196.
 *    In-place separable convolution of a w*h*d x-fastest image with centred
 *    kernels of length N (7/15/31/63/127).  Dims NOT reversed.
 *    outofbounds: 0 = zero, 1 = value (outofboundsvalue), 2 = extend border
 *    pixel; 3 = mirror-single (extension used by this library's DoG pass).
 *    Returns 1 (Java true) on success, 0 on failure.
 * ====================================================================== */
int32_t convolve_7  (float* image, const float* kernelX, const float* kernelY, const float* kernelZ,
                     int imageW, int imageH, int imageD, int32_t convolveX, int32_t convolveY,
                     int32_t convolveZ, int outofbounds, float outofboundsvalue, int devCUDA);
int32_t convolve_15 (float* image, const float* kernelX, const float* kernelY, const float* kernelZ,
                     int imageW, int imageH, int imageD, int32_t convolveX, int32_t convolveY,
                     int32_t convolveZ, int outofbounds, float outofboundsvalue, int devCUDA);
int32_t convolve_31 (float* image, const float* kernelX, const float* kernelY, const float* kernelZ,
                     int imageW, int imageH, int imageD, int32_t convolveX, int32_t convolveY,
                     int32_t convolveZ, int outofbounds, float outofboundsvalue, int devCUDA);
int32_t convolve_63 (float* image, const float* kernelX, const float* kernelY, const float* kernelZ,
                     int imageW, int imageH, int imageD, int32_t convolveX, int32_t convolveY,
                     int32_t convolveZ, int outofbounds, float outofboundsvalue, int devCUDA);
int32_t convolve_127(float* image, const float* kernelX, const float* kernelY, const float* kernelZ,
                     int imageW, int imageH, int imageD, int32_t convolveX, int32_t convolveY,
                     int32_t convolveZ, int outofbounds, float outofboundsvalue, int devCUDA);

/* CPU variant declared by the same interface (CUDASeparableConvolution.java:21) and
 * never called by the reference.  There is no CPU path here: returns
 * SPIMDECON_ERR_DEVICE and leaves the image unchanged (a `void` JNA binding ignores
 * the status; spimdecon_last_error() holds the message). */
int     convolutionCPU(float* image, const float* kernelX, const float* kernelY, const float* kernelZ,
                       int kernelRX, int kernelRY, int kernelRZ, int imageW, int imageH, int imageD,
                       int outofbounds, float outofboundsvalue);

/* ======================================================================
 * 4. Kernel preparation -- spim/process/fusion/deconvolution/MVDeconFFT.java:162-303
 *    (MVDeconInput.init order, AdjustInput.normImg quirk with ij_threads).
 * ====================================================================== */
#define MVD_PSF_OPTIMIZATION_II     0   /* MVDeconFFT.PSFTYPE ordinals, MVDeconFFT.java:28 */
#define MVD_PSF_OPTIMIZATION_I      1
#define MVD_PSF_EFFICIENT_BAYESIAN  2
#define MVD_PSF_INDEPENDENT         3

/* kdims: 3*nviews ints, per view {kx, ky, kz} (odd).  k1_out[v] receives the
 * normalised kernel1, k2_out[v] kernel2 (both kx*ky*kz floats).  Runs on GPU
 * devCUDA. */
int mvd_prepare_kernels(int nviews, const float* const* k1_in, const int* kdims,
                        int psftype, int ij_threads,
                        float* const* k1_out, float* const* k2_out, int devCUDA);

/* out[i] = MVDeconvolution.computeNextValue(last[i], integral[i], weight[i])
 * (MVDeconvolution.java:671-703; lambda > 0: the Tikhonov branch :681-690) for
 * n voxels, DEVICE pointers on the current device -- the exact per-voxel rule the
 * session's update step applies, exposed so callers and tests can check it bit for
 * bit against the reference rule.  Synchronous. */
int spimdecon_next_value(const float* last, const float* integral, const float* weight, int64_t n,
                         double lambda, float* out);

/* ======================================================================
 * 5. GPU-resident RL session (replaces MVDeconvolution.runIteration's
 *    per-view convolve1 -> quotient -> convolve2 -> update loop,
 *    MVDeconvolution.java:333-444, and the init/mask of :95-187).
 * ====================================================================== */
typedef struct mvd_session mvd_session;

typedef struct mvd_params {
    int64_t dims[3];        /* {nx, ny, nz} of THIS rank's z-range of psi          */
    int64_t nz_global;      /* global nz (== dims[2] for a single rank)            */
    int64_t z_offset;       /* first global z plane owned by this rank             */
    int     device;         /* HIP device id (>= 0)                                */
    int     local_slabs;    /* z-slabs held by this process (>= 1); >1 = virtual shards */
    int     nranks;         /* processes in the RCCL communicator (1: none unless comm_id) */
    int     rank;
    const char* comm_id;    /* 128-byte RCCL unique id (required when nranks > 1;
                               with nranks == 1 a non-NULL id still makes a one-rank
                               communicator: collectives and watchdog through RCCL) */
    int     storage_fp16;   /* 1: img/weights stored as fp16 (config-5 mode)       */
    int     fft_pad_policy; /* padded FFT length per axis (>= n + K - 1):            *
                             * 0 = auto (two-factor fast-path length when within    *
                             *     25% of the smallest 2,3,5,7-smooth length),      *
                             * 1 = fast-path table only, 2 = smallest smooth length */
    int     halo[3];        /* max kernel half size {cx,cy,cz}; 0 = derive from views */
    int     ij_threads;     /* pinned reference thread count for the normImg quirk  */
    int     fft_backend;    /* 0 = fused spectral engine (default), 1 = rocFFT       */
    int     slab_axis;      /* axis the volume is split along (local slabs, devices,  *
                             * ranks): 0 = z (default), 1 = y, -1 = the longer of y  *
                             * and z when the volume is split (one rank; else z).    *
                             * With y, dims is this rank's                           *
                             * y-range of every z plane and nz_global / z_offset     *
                             * give the global ny / first y row; the session keeps   *
                             * its slabs in (x, z, y) order internally (one row      *
                             * transposition at upload / download)                   */
    int     reserved[6];
} mvd_params;

/* fills *p with defaults (local_slabs=1, nranks=1, ij_threads=8, ...) */
void mvd_params_default(mvd_params* p);

/* 128-byte RCCL unique id for rank 0 to broadcast (torch.distributed / MPI) */
int mvd_comm_unique_id(char* out128);

/* global [z0, z1) of part `idx` of `nparts` over nz planes (balanced split) */
int mvd_slab_range(int64_t nz, int nparts, int idx, int64_t* z0, int64_t* z1);

/* The halo transfers of one slab (nz interior planes, Mz padded planes, cz halo planes,
 * plane_elems floats per padded plane), as float offsets into its spectrum buffer:
 * out5 = {send_lo, recv_lo, send_hi, recv_hi, count}.  To / from the lower neighbour:
 * send [0, cz), receive into [Mz - cz, Mz); to / from the upper one: send [nz - cz, nz),
 * receive into [nz, nz + cz).  The one helper behind the local slab copies, the device-
 * group peer pulls and the RCCL send / recv (MVDeconFFT.java:424-446 runs the blocks of
 * one volume on several devices; here neighbouring slabs trade halo planes). */
int mvd_halo_plan(int64_t nz, int64_t Mz, int cz, int64_t plane_elems, int64_t* out5);

int  mvd_create(const mvd_params* params, mvd_session** out);
/* One session over several GPUs of this process -- the reference's
 * MVDeconFFT(img, weight, kernel, factory, int[] deviceList, ...) driven from one
 * JVM (MVDeconFFT.java:58-64,91-100,424-446).  params.dims is the whole
 * (this rank's) volume; it is split into ndev * params.local_slabs z-slabs, slabs
 * [i*local_slabs, (i+1)*local_slabs) on devs[i] (params.device is ignored).  One
 * mvd_run drives all devices (one host thread each); halo planes move between
 * neighbouring devices as peer copies over xGMI.  Device ids may repeat (several
 * groups on one GPU: the same code path, e.g. for testing).  Needs the engine
 * backend and nranks == 1. */
int  mvd_create_devices(const int* devs, int ndev, const mvd_params* params, mvd_session** out);
void mvd_destroy(mvd_session* h);
/* devices of the session and the device holding slab s (slabs: ndev * local_slabs) */
int  mvd_num_devices(mvd_session* h, int* ndev);
int  mvd_slab_device(mvd_session* h, int slab, int* dev);
/* slabs of the session: ndev * local_slabs, where local_slabs may exceed
 * params.local_slabs -- the engine splits a device's share further until every
 * slab buffer (psi, views, spectra) stays below 4 GiB, the range of its 32-bit
 * buffer offsets (env SPIMDECON_AUTO_SLABS=0 disables; the slabs are exact, like
 * the reference's precise blocks, BlockGeneratorFixedSizePrecise.java:25-101) */
int  mvd_num_slabs(mvd_session* h, int* nslabs);
/* voxels {nx, ny, nz} of slab s in the session's internal order (a y-split session
 * keeps (x, z, y-slab) rows: nz is then the slab's y extent) */
int  mvd_slab_extent(mvd_session* h, int slab, int64_t* out3);
/* halo exchange counters since mvd_create: bytes and copies moved between slabs
 * (local copies, peer pulls between device groups, RCCL sends); either may be NULL */
int  mvd_exchange_stats(mvd_session* h, int64_t* bytes, int64_t* copies);

/* Adds one view (MVDeconInput.add order).  img/weight: this rank's z-range,
 * dims = params.dims; kernel1: raw (un-normalised) PSF of kdims {kx,ky,kz}.
 * Views are only staged here; mvd_init() builds kernels and uploads. */
int mvd_add_view(mvd_session* h, const float* img, const float* weight,
                 const float* kernel1, const int* kdims);
/* Same, but img/weight are device pointers on params.device (copied). */
int mvd_add_view_device(mvd_session* h, const float* d_img, const float* d_weight,
                        const float* kernel1, const int* kdims);

/* MVDeconInput.init(type): normalises kernel1 and builds kernel2 for all
 * views (MVDeconFFT.java:162-303) then computes the kernel spectra. */
int mvd_init(mvd_session* h, int psftype);
/* Alternative to mvd_init: kernels already prepared by the caller
 * (MVDeconFFT.getKernel1/2, MVDeconFFT.java:352-353). */
int mvd_set_kernels(mvd_session* h, int view, const float* k1, const float* k2);
/* read back prepared kernels (kx*ky*kz floats each) */
int mvd_get_kernels(mvd_session* h, int view, float* k1, float* k2);

/* psi initialisation (MVDeconvolution.java:95-127).  psi == NULL: first-iteration
 * average fusion (FirstIteration.java, NaN -> 0.5); else the given image with
 * the checkNumbers clamp (<= 0 -> minValue). *avg_out may be NULL. */
int mvd_init_psi(mvd_session* h, const float* psi_or_null, double* avg_out);

/* runs `iters` RL iterations (sequential per-view updates).  lambda > 0:
 * Tikhonov.  stats (may be NULL): iters*nviews*2 doubles {sumChange, maxChange}
 * reduced over all slabs and ranks. */
int mvd_run(mvd_session* h, int iters, double lambda, double* stats);

/* final mask: psi = 0 where no view has data (MVDeconvolution.java:180-187) */
int mvd_apply_mask(mvd_session* h);

/* copy this rank's psi to out (dims of params); out may be a host or a device
 * pointer (unified addressing: a device-resident result skips the host) */
int mvd_get_psi(mvd_session* h, float* out);
/* device pointer of local slab s's psi (valid until mvd_destroy); x-fastest
 * [z][y][x] of the slab, or [y][z][x] when the session splits along y */
float* mvd_psi_device(mvd_session* h, int slab);

/* padded FFT dims {Mx, My, Mz} of local slab s (info/bench) */
int mvd_fft_dims(mvd_session* h, int slab, int64_t* out3);
/* z-planes of each stored kernel spectrum (info/bench): 2*cz+1 when the engine
 * keeps compact kernels (the z pass builds their z transform), else Mz */
int mvd_kernel_planes(mvd_session* h, int slab, int* planes);
/* z pass of the engine (info/bench): 0 = fused FFT z pass with full kernel
 * spectra, 1 = fused FFT z pass with compact kernels, 3 = direct circular
 * convolution with the compact kernel over z chunks carried inside a block (only
 * the nz interior planes written; 2 and 4 named passes removed in round 5);
 * -1 for the rocFFT backend */
int mvd_zpass_mode(mvd_session* h, int slab, int* mode);
/* x pass of the last update launch of slab s (info/tests): 2 = two-factor row-pair
 * tiles, 1 = per-wave rows, 0 = Stockham rows, -1 = no run yet, -2 = rocFFT backend */
int mvd_xpass_mode(mvd_session* h, int slab, int* mode);
/* HIP stream the session launches on (hipStream_t as void*) */
void* mvd_stream(mvd_session* h);
/* per-kernel timing: when enabled, mvd_run records HIP events around every
 * kernel class; mvd_timing fills out16[0..7] with the accumulated ms and
 * out16[8..15] with the launch count of each class:
 *   engine backend: [0] x update pass, [1] x quotient pass, [2] y passes,
 *                   [3] z convolve passes, [4] psi forward x pass,
 *                   [5] halo exchange, [6] stats reduce
 *   rocFFT backend: [0] update + pad, [1] quotient + pad, [2] R2C,
 *                   [3] spectral multiply, [4] C2R, [5] halo exchange,
 *                   [6] stats reduce */
int mvd_enable_timing(mvd_session* h, int on);
int mvd_timing(mvd_session* h, double* out16);

/* ======================================================================
 * 6. DoG bead detection -- spim/process/interestpointdetection/ProcessDOG.java:40-178
 * ====================================================================== */
typedef struct spim_dog_params {
    float   sigma;           /* default 1.8 (DifferenceOfGaussian.java:36)          */
    float   threshold;       /* default 0.008 (DifferenceOfGaussian.java:37)        */
    int     localization;    /* 0 = none (threshold), 1 = quadratic (threshold/10)  */
    double  image_sigma[3];  /* default 0.5 each; min(imageSigma, sigma) applied    */
    int32_t find_min;
    int32_t find_max;
    double  min_intensity;   /* NaN -> image min/max                                */
    double  max_intensity;
    int     ij_threads;      /* peak ordering: lists by x % T (InteractiveIntegral.java:394) */
    int     device;
} spim_dog_params;

typedef struct spim_peak {
    int32_t x, y, z;
    float   intensity;       /* |dog| */
    int32_t is_min, is_max;
} spim_peak;

/* InterestPoint(Value) of spim.fiji.spimdata.interestpoints (id = index) */
typedef struct spim_interest_point {
    double  pos[3];          /* x, y, z (sub-pixel with localization 1)             */
    float   intensity;       /* |dog| (localization 0) or the fitted value (1)       */
    int32_t is_max;
} spim_interest_point;

void spim_dog_params_default(spim_dog_params* p);

/* img: dims {nx, ny, nz} x-fastest (not modified).  dog_out (optional, may be
 * NULL) receives the DoG image.  img and dog_out may be host or device (HIP)
 * pointers: a view already resident in HBM is not staged through the host.  peaks: capacity max_peaks, *npeaks = total
 * found (may exceed max_peaks: then only max_peaks were written).  These are
 * the DoG extrema with |v| >= threshold (localization 0) or threshold / 10
 * (localization 1), i.e. DifferenceOfGaussianNewPeakFinder.getSimplePeaks. */
int spim_dog_compute(const float* img, const int64_t* dims, const spim_dog_params* p,
                     float* dog_out, spim_peak* peaks, int64_t max_peaks, int64_t* npeaks);

/* ProcessDOG.compute's result (ProcessDOG.java:150-168): the peaks above
 * after Localization -- localization 0: Localization.noLocalization
 * (Localization.java:19-45); 1: quadratic sub-pixel fit, kept when
 * |fitted value| > threshold (Localization.java:47-88).  Same capacity rule
 * as spim_dog_compute. */
int spim_dog_interest_points(const float* img, const int64_t* dims, const spim_dog_params* p,
                             float* dog_out, spim_interest_point* out, int64_t max_out,
                             int64_t* nout);

/* The same two calls with the reference's choice of GPU mode (DifferenceOfGaussian.java:44,
 * 338-340), i.e. how the Gaussians see beyond the image: `extension` is one of the two
 * values below, anything else returns SPIMDECON_ERR_ARG.  Contract otherwise as above (host
 * or device pointers, the capacity rule, the workspace); the calls without _ext are these
 * with SPIM_DOG_EXTEND_MIRROR.  (spim_dog_params keeps its size: callers pass it by pointer.) */
#define SPIM_DOG_EXTEND_MIRROR 0   /* accurate: extendMirrorSingle (DifferenceOfGaussianCUDA.java:153-154) */
#define SPIM_DOG_EXTEND_BORDER 1   /* approximate: EXTEND_BORDER_PIXELS (:125-148)                          */
int spim_dog_compute_ext(const float* img, const int64_t* dims, const spim_dog_params* p, int32_t extension,
                         float* dog_out, spim_peak* peaks, int64_t max_peaks, int64_t* npeaks);
int spim_dog_interest_points_ext(const float* img, const int64_t* dims, const spim_dog_params* p, int32_t extension,
                                 float* dog_out, spim_interest_point* out, int64_t max_out, int64_t* nout);

/* The DoG calls above keep a per-device workspace between calls (the
 * intermediate Gaussians, candidate lists; ~12 B per voxel of the largest view seen)
 * instead of allocating per call; this frees it.  No reference counterpart (the
 * reference's CUDA library allocates per call, CUDASeparableConvolution.java:13-21). */
int spim_dog_release_workspace(int device);

/* Interest-point list files (InterestPointList.java:66-100 save, :178-220 load):
 * <base_dir>/<file>.ip.txt (base_dir may be NULL or ""; missing parent directories
 * are created), header "id\tx\ty\tz", one line per point with the doubles printed
 * as Java's Double.toString.  ids (may be NULL: id = index, as ProcessDOG assigns
 * them) are written / read beside pos.  Load: *nout = points in the file; at most
 * max_out are stored (intensity / is_max are 0: the file holds positions only). */
int spim_save_interest_points(const char* base_dir, const char* file, const spim_interest_point* pts,
                              const int32_t* ids, int64_t n);
int spim_load_interest_points(const char* base_dir, const char* file, spim_interest_point* out,
                              int32_t* ids, int64_t max_out, int64_t* nout);
/* Java Double.toString of d into out (cap bytes incl. the terminator), in the form of
 * the selected Java version (also used by spim_save_interest_points): 8 (default; Fiji
 * runs Java 8: sun.misc.FloatingDecimal, e.g. 2.0E23 -> "1.9999999999999998E23") or 19
 * (JDK 19+: the shortest decimal that round-trips, "2.0E23").  Process-wide. */
int spim_set_java_version(int jdk);
int spim_java_double_to_string(double d, char* out, int cap);

/* ======================================================================
 * 6b. Difference-of-Mean bead detection ("Difference-of-Mean (Integral image based)") --
 *     spim/process/interestpointdetection/ProcessDOM.java:36-117,
 *     mpicbg/spim/segmentation/DOM.java:29-171, IntegralImage3d.java:60-210:
 *     dom = (float) s2 / d2 - (float) s1 / d1, s_b the sum of (int) voxel over box b
 *     (as long), d_b = (float)(box voxels) * (max - min); zero where the boxes do not
 *     fit.  The image is not normalised.  Bit-exact against the reference's arithmetic.
 * ====================================================================== */
typedef struct spim_dom_params {
    int     radius1;         /* default 2 (DifferenceOfMean.java:29)                 */
    int     radius2;         /* default 3 (:30); radius1 > radius2 is legal          */
    float   threshold;       /* default 0.02 (:31); used as given with either localization */
    int     localization;    /* 0 = none, 1 = quadratic (kept when |fit| > threshold) */
    double  image_sigma[3];  /* default 0.5 each: diameter = max(3 | 5, round(radius * 0.5 / sigma) * 2 + 1) */
    int32_t find_min;
    int32_t find_max;
    double  min_intensity;   /* NaN -> image min/max                                */
    double  max_intensity;
    int     ij_threads;      /* peak ordering, as spim_dog_params                   */
    int     device;
} spim_dom_params;

void spim_dom_params_default(spim_dom_params* p);

/* The box diameters per axis (ProcessDOM.java:71-78): s1 from radius1 (at least 3), s2
 * from radius2 (at least 5).  Host only: needs no GPU. */
int spim_dom_diameters(const spim_dom_params* p, int32_t s1[3], int32_t s2[3]);

/* As spim_dog_compute / spim_dog_interest_points (host or device pointers, optional
 * image out, the capacity rule, the workspace of spim_dog_release_workspace) with the
 * DOM image in place of the DoG image.  Diameters up to 33 voxels per axis; beyond, and
 * for any bad argument (null, dims < 1, radius < 1, image_sigma <= 0 or not finite,
 * ij_threads < 1, localization other than 0 / 1), SPIMDECON_ERR_ARG before any GPU work.
 * A volume the boxes do not fit into gives an all-zero image and no peaks (status OK). */
int spim_dom_compute(const float* img, const int64_t* dims, const spim_dom_params* p,
                     float* dom_out, spim_peak* peaks, int64_t max_peaks, int64_t* npeaks);
int spim_dom_interest_points(const float* img, const int64_t* dims, const spim_dom_params* p,
                             float* dom_out, spim_interest_point* out, int64_t max_out,
                             int64_t* nout);

/* ======================================================================
 * 6b''. The detection stage on a caller's image -- everything spim_dog_* and spim_dom_* run
 *     once their image is stored: InteractiveIntegral.findPeaks (InteractiveIntegral.java:
 *     360-468) over img, the x % ij_threads order, and Localization (Localization.java:19-88).
 *     img: dims {nx, ny, nz} x-fastest, host or device memory, not modified.  A voxel is a
 *     candidate unless |v| < min_peak (InteractiveIntegral.java:409): a NaN min_peak skips
 *     nothing, a NaN voxel is never an extremum.  Capacity rule and workspace as spim_dog_*.
 *     Argument rules as spim_dom_* (null, dims < 1, ij_threads < 1, localization other than
 *     0 / 1, an unknown route: SPIMDECON_ERR_ARG before any GPU work).
 * ====================================================================== */
#define SPIM_DETECT_ROUTE_AUTO   0   /* the library's choice, as spim_dog_* / spim_dom_* take it        */
#define SPIM_DETECT_ROUTE_WAVE   1   /* the wave-per-62-columns kernel; SPIMDECON_ERR_ARG from 4 GiB on */
#define SPIM_DETECT_ROUTE_APPEND 2   /* the thread-per-voxel kernel (images of 4 GiB and more)          */
/* The extrema of the wanted kinds, in the reference's order. */
int spim_detect_peaks(const float* img, const int64_t* dims, float min_peak, int32_t find_min,
                      int32_t find_max, int32_t ij_threads, int32_t route, int32_t device,
                      spim_peak* peaks, int64_t max_peaks, int64_t* npeaks);
/* ... after Localization: 0 copies them; 1 fits, and keeps those with |fitted value| >
 * keep_threshold (float against float), in candidate order.  out: host or device memory. */
int spim_detect_interest_points(const float* img, const int64_t* dims, float min_peak, int32_t find_min,
                                int32_t find_max, int32_t ij_threads, int32_t route, int32_t device,
                                int32_t localization, float keep_threshold, spim_interest_point* out,
                                int64_t max_out, int64_t* nout);
/* The stage's tile sizes, from the constants in the code (for tests that aim at its seams):
 * columns tested per wave, rows per lane, centre planes per chunk, entries of a wave's
 * candidate buffer, the least capacity of the candidate lists.  Host only: needs no GPU. */
void spim_detect_tiles(int32_t sizes[5]);

/* ======================================================================
 * 6b'. Downsampling in front of the detectors ("Downsample_XY" / "Downsample_Z") --
 *     spim/process/interestpointdetection/Downsample.java:65-162 (simple2x along one axis),
 *     spim/fiji/plugin/interestpointdetection/DifferenceOf.java:446-535 (openAndDownsample:
 *     every x level, then y, then z; each level stored as float), :430-444 (downsampleFactor).
 *     A line of n voxels becomes n / 2: out[0] = (in[0] + in[1] * 0.5) / 1.5,
 *     out[q] = (in[2q-1] * 0.5 + in[2q] + in[2q+1] * 0.5) / 2.0, out[m-1] = (in[2m-2] +
 *     in[2m-3] * 0.5) / 1.5, in double, rounded to float once per level.  Output voxel p is
 *     centred on input voxel factor * p: detections scale back by the factor alone
 *     (correctForDownsampling, :402-428).  Bit-exact against the reference's arithmetic.
 * ====================================================================== */
/* out_dims[a] = dims[a] halved (integer division) once per level of factor[a]; dims and
 * factor in x, y, z order.  SPIMDECON_ERR_ARG for a factor outside {1, 2, 4, 8} or a level
 * whose input is shorter than 4 on a downsampled axis (the reference reads out of bounds
 * there).  Host only: needs no GPU. */
int spim_downsample_dims(const int64_t dims[3], const int32_t factor[3], int64_t out_dims[3]);

/* The downsampled view into out (sized by spim_downsample_dims).  Host or device pointers
 * (as spim_dom_*); img is not modified; factor (1, 1, 1) copies.  The x and y chains of a
 * plane are one kernel, the z chain a second one over the xy-reduced image, which lives in
 * the workspace of spim_dog_release_workspace. */
int spim_downsample(const float* img, const int64_t dims[3], const int32_t factor[3], int device,
                    float* out);

/* The xy factor of "Match Z Resolution (less downsampling)" (more = 0: 2^floor) and
 * "(more downsampling)" (more != 0: 2^ceil) of log2(voxel[2] * ds_z / min(voxel[0], voxel[1])),
 * rounded as the reference does.  Deliberate deviation: a result below 1 (a z step finer than
 * xy; the reference returns 0 and scales every coordinate by 0) is 1.  A result above 8 (the
 * reference's fixed choices end there) and a bad argument are SPIMDECON_ERR_ARG.  Host only. */
int spim_downsample_factor_xy(int more, int32_t ds_z, const double voxel[3], int32_t* factor);

/* ======================================================================
 * 6c. Descriptor-based pairwise registration, candidate stage: "redundant geometric local
 *     descriptor matching" (translation invariant) --
 *     spim/process/interestpointregistration/geometricdescriptor/RGLDMMatcher.java:44-123,
 *     RGLDMPairwise.java:34-77, mpicbg/pointdescriptor/{AbstractPointDescriptor,
 *     SimplePointDescriptor}.java, matcher/SubsetMatcher.java, similarity/SquareDistance.java.
 *     Points are (n, 3) doubles (x, y, z), already mapped by the views' current models;
 *     host or device pointers (as spim_dom_*).  Bit-exact against the reference's
 *     arithmetic; the order of equal float distances in the neighbour search is this
 *     library's (lower index first: the reference's kd-tree is not in its tree).
 * ====================================================================== */
typedef struct spim_rgldm_params {
    int32_t num_neighbors;        /* 3   RGLDMParameters.numNeighbors          */
    int32_t redundancy;           /* 1   RGLDMParameters.redundancy            */
    float   ratio_of_distance;    /* 3   (float in the reference, widened to double at use) */
    float   difference_threshold; /* 50                                        */
    int32_t b_split;              /* 0 = auto; >0 forces that many partitions of B (tests) */
    int32_t device;
} spim_rgldm_params;

void spim_rgldm_params_default(spim_rgldm_params* p);

/* The matching kernel's tile sizes: A descriptors per block, B descriptors per LDS tile
 * (the sizes at which its code takes another path).  Host only: needs no GPU. */
void spim_rgldm_tiles(int32_t* a_tile, int32_t* b_tile);

/* Per point its num_neighbors + redundancy nearest other points in ascending
 * Detection.distanceTo (float) order -- neighbors[n * (nn+re)] -- and neighbour minus basis
 * in double -- rel[n * (nn+re) * 3].  1 <= num_neighbors, 0 <= redundancy, nn + re <= 6;
 * n >= nn + re + 1; coordinates finite (also as float); n <= 2^31 - 1: else
 * SPIMDECON_ERR_ARG. */
int spim_rgldm_descriptors(const double* pts, int64_t n, const spim_rgldm_params* p,
                           int32_t* neighbors, double* rel);

/* For every A descriptor over all B descriptors: best = the smallest descriptor distance
 * (min over SubsetMatcher's pairings of the summed square distances / 3.0), best_idx the
 * lowest B index attaining it, second = the second smallest of the multiset (from
 * Double.MAX_VALUE down, best_idx -1 when nothing is below it).  Candidate i -> best_idx[i]
 * is emitted in ascending A order when best < (double) difference_threshold &&
 * best * (double) ratio_of_distance < second.  *count = the number of candidates; more
 * than cap is SPIMDECON_ERR_ARG with *count still the needed size (best_idx / best /
 * second are written all the same).  na or nb < nn + re + 1: no candidates, status OK
 * ("Not enough detections to match").  The result does not depend on b_split. */
int spim_rgldm_match(const double* a, int64_t na, const double* b, int64_t nb,
                     const spim_rgldm_params* p, int32_t* best_idx, double* best, double* second,
                     int32_t* cand_a, int32_t* cand_b, int64_t cap, int64_t* count);

/* ======================================================================
 * 6d. Pairwise registration, candidate stage: "fast 3d geometric hashing (rotation
 *     invariant)" -- spim/process/interestpointregistration/geometrichashing/
 *     GeometricHashingPairwise.java:45-86, GeometricHasher.java:54-116, mpicbg/pointdescriptor/
 *     LocalCoordinateSystemPointDescriptor.java:37-175, spim/vecmath/{Vector3d,Matrix3d}.java.
 *     Every point is described in the local coordinate system of its 3 nearest neighbours
 *     (normalize = false: six floats ax bx by cx cy cz), so the view models need not be
 *     rotationally right.  Points as in 6c.  Bit-exact against the reference's arithmetic;
 *     the ranking of B descriptors is this library's (the reference's kd-tree is not in its
 *     tree): by (float) Math.sqrt(descriptorDistance) ascending, equal floats by lower B
 *     index, a NaN distance not ranked.
 * ====================================================================== */
typedef struct spim_gh_params {
    double  ratio_of_distance;    /* 10  GeometricHashingParameters.ratioOfDistance     */
    double  difference_threshold; /* 50  GeometricHashingParameters.differenceThreshold */
    int32_t b_split;              /* 0 = auto; >0 forces that many partitions of B (tests) */
    int32_t device;
} spim_gh_params;

void spim_gh_params_default(spim_gh_params* p);

/* The matching kernel's tile sizes: A descriptors per block, B descriptors per LDS tile.
 * Host only: needs no GPU. */
void spim_gh_tiles(int32_t* a_tile, int32_t* b_tile);

/* Per point its 3 nearest other points in ascending Detection.distanceTo (float) order, equal
 * floats by lower index -- neighbors[n * 3] -- and its descriptor -- desc[n * 6]: ax bx by cx
 * cy cz (a matrix without inverse leaves bx .. cz at 0, as the reference's catch).  n >= 4;
 * coordinates finite (also as float); n <= 2^31 - 1: else SPIMDECON_ERR_ARG. */
int spim_gh_descriptors(const double* pts, int64_t n, const spim_gh_params* p,
                        int32_t* neighbors, float* desc);

/* For every A descriptor the two first ranked B descriptors: best_idx the first, best and
 * second their descriptorDistance (float differences and products, a double sum); with fewer
 * than two ranked, Double.MAX_VALUE / Double.MAX_VALUE / -1 and no candidate.  Candidate
 * i -> best_idx[i] is emitted in ascending A order when best < difference_threshold &&
 * best * ratio_of_distance <= second.  *count, cap and the written outputs as
 * spim_rgldm_match.  na or nb < 4: no candidates, status OK ("Not enough detections to
 * match").  The result does not depend on b_split. */
int spim_gh_match(const double* a, int64_t na, const double* b, int64_t nb,
                  const spim_gh_params* p, int32_t* best_idx, double* best, double* second,
                  int32_t* cand_a, int32_t* cand_b, int64_t cap, int64_t* count);

/* ======================================================================
 * 6e. Pairwise registration, "Iterative closest-point (ICP, no invariance)": one iteration's
 *     correspondence search -- mpicbg/icp/ICP.java:91-115 (apply, assign), :208-317
 *     (removeAmbigousMatches), SimplePointMatchIdentification.java:32-48,
 *     spim/process/interestpointregistration/Detection.java:96-115 (distanceTo, get).  The
 *     target list is moved by the current model (absolute, target coordinates -> reference
 *     frame), the reference list never; the loop and the model fits of
 *     IterativeClosestPointPairwise.java:40-122 stay with the caller.  Points as in 6c.
 *     Bit-exact against the reference's arithmetic; among equal float distances the lower
 *     target index is the nearest (the reference's kd-tree is not in its tree).
 * ====================================================================== */
typedef struct spim_icp_params {
    float   max_distance;    /* 5   (float in the reference, widened to double at use) */
    int32_t max_iterations;  /* 100 (the caller's loop; spim_icp_assign does not read it) */
    int32_t t_split;         /* 0 = auto; >0 forces that many partitions of the target (tests) */
    int32_t device;
} spim_icp_params;

void spim_icp_params_default(spim_icp_params* p);

/* The assignment kernel's tile sizes: reference points per block, target points per LDS tile.
 * Host only: needs no GPU. */
void spim_icp_tiles(int32_t* ref_block, int32_t* target_tile);

/* One ICP iteration up to the fit.  Every target point becomes w = model * l in double, each
 * row ((m0 x + m1 y) + m2 z) + m3 with every product and sum rounded on its own (model: 12
 * doubles, row-major 3x4, host or device; NULL = the identity).  For every reference point
 * nearest[r] = the target with the smallest Detection.distanceTo (float coordinates, float
 * differences, a double sum, (float) Math.sqrt; lowest index among equal floats) and dist[r]
 * that float; nt == 0: -1 and FLT_MAX.  (nearest[r], r) is a match when (double) dist[r] <=
 * (double) max_distance; matches whose target another match names too are removed
 * (*ambiguous = how many) and the others written in ascending r: match_t[k], match_r[k].
 * *count = their number; more than cap is SPIMDECON_ERR_ARG with *count still the needed size
 * (nearest / dist are written all the same).  nt == 0 or nr == 0: no matches, status OK.
 * Coordinates not finite (as double or as float, before or after the model) or a list longer
 * than 2^31 - 1: SPIMDECON_ERR_ARG.  The result does not depend on t_split. */
int spim_icp_assign(const double* target, int64_t nt, const double* reference, int64_t nr,
                    const double* model, const spim_icp_params* p, int32_t* nearest, float* dist,
                    int32_t* match_t, int32_t* match_r, int64_t cap, int64_t* count,
                    int64_t* ambiguous);

/* ======================================================================
 * 6f. "Thin out detections" -- spim/fiji/plugin/ThinOut_Detections.java:73-166 (thinOut),
 *     :238-299 (plotHistogram), spim/fiji/plugin/thinout/Histogram.java:56-90 (getMinMax,
 *     binData).  Per detection of one view the distance to its nearest other detection in
 *     calibrated units (l[d] * voxel[d]), in double; the detections whose distance lies in
 *     [min_distance, max_distance] are removed, or they alone are kept.  Bit-exact against the
 *     reference's arithmetic: s = ((dx dx) + (dy dy)) + (dz dz), every product and sum rounded
 *     on its own, Math.sqrt of the smallest s.  Unpinned: imglib2's kd-tree is not in the
 *     reference's tree; among equal s the lower index is the nearest here.  A list of one
 *     point has no other point: distance +inf, nearest -1 (kept by remove-range, dropped by
 *     keep-range).
 * ====================================================================== */
typedef struct spim_thinout_params {
    double  min_distance;    /* 0   (ThinOut_Detections.java:38)                              */
    double  max_distance;    /* 5   (:39)                                                     */
    int32_t keep_range;      /* 0 = remove the range (:42), 1 = keep only the range            */
    int32_t t_split;         /* 0 = auto; >0 forces that many partitions of the list (tests)   */
    int32_t device;
} spim_thinout_params;

void spim_thinout_params_default(spim_thinout_params* p);

/* The self-join kernel's tile sizes: points per block, points per LDS tile.  Host only: needs
 * no GPU. */
void spim_thinout_tiles(int32_t* row_block, int32_t* col_tile);

/* dist[i] = the distance of point i of pts (n x 3 doubles, x y z; host or device memory) to its
 * nearest other point after scaling by voxel (3 doubles, host), nearest[i] = that point's index
 * (the self pair is left out by index: an exact duplicate is a neighbour at distance 0).  dist
 * and nearest: n entries, host or device memory.  n == 0: status OK, nothing written.
 * min_distance >= max_distance (or a NaN), a negative t_split, coordinates that are not finite
 * (as double or float, before or after the scaling) or more than 2^31 - 1 points:
 * SPIMDECON_ERR_ARG.  The result does not depend on t_split. */
int spim_nn_distances(const double* pts, int64_t n, const double voxel[3], const spim_thinout_params* p,
                      double* dist, int32_t* nearest);

/* spim_nn_distances, and kept[0 .. *count) = the indices, ascending, of the points the range
 * rule keeps (:141): keep_range d >= min && d <= max, else d < min || d > max.  Entry k is the
 * detection with the new id k.  *count beyond cap: SPIMDECON_ERR_ARG, *count says how many
 * there are (dist / nearest are written all the same).  n == 0: *count = 0, nothing else is
 * touched. */
int spim_thin_out(const double* pts, int64_t n, const double voxel[3], const spim_thinout_params* p,
                  double* dist, int32_t* nearest, int32_t* kept, int64_t cap, int64_t* count);

/* Histogram.getMinMax and binData over the n distances (host or device memory) whose
 * select_or_null[i] != 0 (null: all of them): *min, *max, counts[num_bins] of
 * bin = (int) floor(((v - min) / size) * num_bins) with size = (max - min) + 0.000001, and the
 * bin centres[num_bins] = min + binSize / 2 + binSize * bin, binSize = size / num_bins.
 * SPIMDECON_ERR_ARG: num_bins < 1 or > 4096, n < 2, an empty selection, a selected distance
 * that is not finite, a distance that falls into bin num_bins (Java's
 * ArrayIndexOutOfBoundsException, when max - min absorbs the 0.000001). */
int spim_distance_histogram(const double* dist, int64_t n, const uint8_t* select_or_null, int32_t num_bins,
                            int device, double* min, double* max, int64_t* counts, double* centres);

/* ======================================================================
 * 7. Deconvolution input preparation --
 *    spim/process/fusion/deconvolution/ProcessForDeconvolution.java:159-384:
 *    each view resampled into the fused bounding box through the inverse of
 *    its affine model (TransformInput(AndWeights)), cosine blending weights,
 *    WeightNormalizer, OSEM adjustment.
 * ====================================================================== */
#define SPIM_WEIGHTS_NONE         0   /* WeightType.NO_WEIGHTS                          */
#define SPIM_WEIGHTS_PRECOMPUTED  1   /* WeightType.PRECOMPUTED_WEIGHTS                 */
#define SPIM_WEIGHTS_VIRTUAL      2   /* WeightType.VIRTUAL_WEIGHTS (the default)       */

typedef struct spim_view_source {
    const float* img;        /* source stack, x-fastest {nx, ny, nz}                     */
    int64_t      dims[3];
    double       model[12];  /* row-major 3x4 affine, source -> world (ViewRegistration)  */
} spim_view_source;

typedef struct spim_input_params {
    int64_t bb_min[3];           /* bounding box of the fused volume (world voxels)       */
    int64_t bb_dims[3];
    float   blending_border[3];  /* default -8 (EfficientBayesianBased.java:76)          */
    float   blending_range[3];   /* default 12 (EfficientBayesianBased.java:75)           */
    int     weight_type;         /* SPIM_WEIGHTS_*                                         */
    int     osem_index;          /* 0: osem_speedup, 1: min, 2: average overlapping views  */
    double  osem_speedup;
    int     ij_threads;          /* portions of the overlap statistics (2T)               */
    int     device;
    int     src_on_device;       /* 1: views[].img are device pointers                    */
    int     out_on_device;       /* 1: img_out / weight_out are device pointers           */
    int     reserved[8];
} spim_input_params;

void spim_input_params_default(spim_input_params* p);

/* img_out[v], weight_out[v]: bb_dims voxels each (x-fastest).  osem_used,
 * min_overlap, avg_overlap (may be NULL) report the OSEM factor applied and
 * WeightNormalizer's overlap statistics (-1 / NaN for SPIM_WEIGHTS_NONE). */
int spim_prepare_inputs(int nviews, const spim_view_source* views, const spim_input_params* p,
                        float* const* img_out, float* const* weight_out, double* osem_used,
                        int* min_overlap, double* avg_overlap);

/* ======================================================================
 * 8. Weighted-average fusion --
 *    spim/process/fusion/weightedavg/ProcessParalellPortion(Weight).java:
 *    per fused voxel the (blending-weighted) mean of the views covering it.
 *    Content-based weights (spim/process/fusion/weights/ContentBased.java:60-98):
 *    per view, in its own voxel grid, normalised G(sigma2) * (G(sigma1) * I - I)^2
 *    over extendMirrorSingle; sampled n-linearly over extendZero at fusion time
 *    and multiplied into the blending weight (ProcessParalellPortionWeights.java).
 * ====================================================================== */
typedef struct spim_fusion_params {
    int64_t bb_min[3];      /* bounding box (world voxels)                               */
    int64_t bb_dims[3];     /* fused image dims (after downsampling)                    */
    float   downsampling;   /* 1 = none; s = position * downsampling + bb_min            */
    int     interpolation;  /* 0 nearest neighbour, 1 n-linear (Fusion.defaultInterpolation) */
    int     use_blending;   /* Fusion.defaultUseBlending (content-based: the _content call) */
    int     device;
    int     src_on_device;
    int     out_on_device;
    int     reserved[8];
} spim_fusion_params;

void spim_fusion_params_default(spim_fusion_params* p);

/* blending_borders / blending_ranges: 3 floats per view (may be NULL without
 * blending); out: bb_dims voxels, x-fastest float32. */
int spim_fuse_weighted_average(int nviews, const spim_view_source* views, const spim_fusion_params* p,
                               const float* blending_borders, const float* blending_ranges, float* out);

/* ContentBased.approximateEntropy: out has dims voxels; img / out host or device pointers.
 * sigma: (x, y, z), finite and > 0, at most 463 taps (2 * (int)(3 sigma + 0.5) + 1) per axis. */
int spim_content_based_weights(const float* img, const int64_t dims[3], const double sigma1[3],
                               const double sigma2[3], float* out, int device);

/* The tiling of the content-weight kernels, for tests that straddle it: outputs per line and
 * block along the pass axis, lines per block, taps per register-window step (the taps are
 * zero-padded to a multiple), the tap limit, and the threads per block and the blocks of the
 * min / max reduction.  Needs no GPU. */
void spim_content_tiles(int32_t sizes[6]);

/* spim_fuse_weighted_average with the content weight of every view (sigma1 / sigma2: nviews x 3)
 * multiplied into its blending weight (p->use_blending 1) or used alone (0) */
int spim_fuse_weighted_average_content(int nviews, const spim_view_source* views,
                                       const spim_fusion_params* p, const float* blending_borders,
                                       const float* blending_ranges, const double* sigma1,
                                       const double* sigma2, float* out);

/* ======================================================================
 * 8b. The bounding box estimated from the data ("Estimate automatically (experimental)") --
 *     spim/process/fusion/boundingbox/AutomaticBoundingBox.java:36-131,
 *     automatic/MinFilterThreshold.java:76-308, BoundingBoxGUI.java:340-399,
 *     FusionHelper.minMax: the maximal box of all views is fused at `downsampling` (nearest
 *     neighbour, no blending, ProcessParalell's double accumulation: section 8), a threshold is
 *     put at `background` percent of the fused image's range, a separable minimum filter
 *     (x, y, z; window 2r + 1 over a zero extension) erodes beads and debris, and the box of
 *     what stays above the threshold is scaled back and padded by 3 * (size / 2).
 *     Math.min / Math.max semantics throughout (a NaN spreads, -0 < +0): every image result
 *     is bit-exact against the reference's arithmetic.  Images are x-fastest float32, dims
 *     (x, y, z); img / out / filtered may be host or device pointers (as spim_dom_*).
 * ====================================================================== */
#define SPIM_MIN_FILTER_MAX_RADIUS 64   /* the dialog's sliders need up to 50 */

/* The maximal box: per view the 8 corners of [0, dim - 1] through its row-major 3x4 model
 * (dims: nviews x 3, models: nviews x 12), min / max over the views, Math.round;
 * bb_dims = bb_max - bb_min + 1; fused_dims (may be NULL) = bb_dims / downsampling (integer
 * division, BoundingBoxGUI.getDimensions).  SPIMDECON_ERR_ARG for a non-finite model,
 * dims < 1 or downsampling < 1.  Host only: needs no GPU. */
int spim_max_bounding_box(int nviews, const int64_t* dims, const double* models, int downsampling,
                          int64_t bb_min[3], int64_t bb_max[3], int64_t bb_dims[3], int64_t fused_dims[3]);

/* FusionHelper.minMax: Math.min / Math.max from +-Float.MAX_VALUE over every voxel. */
int spim_min_max(const float* img, const int64_t dims[3], int device, float* min, float* max);

/* MinFilterThreshold.computeLazyMinFilter with one radius for the three axes; out == img is
 * allowed.  radius: 1 .. SPIM_MIN_FILTER_MAX_RADIUS, anything else is SPIMDECON_ERR_ARG.  Two
 * volumes of scratch live in the workspace of spim_bbox_release_workspace. */
int spim_min_filter(const float* img, const int64_t dims[3], int radius, int device, float* out);

/* The tiling of the minimum filter and of the min / max reduction, for tests that straddle it:
 * lines per block, outputs per line and block along the pass axis for a small radius, the
 * same for a large one, the largest small radius, and the threads per block and the blocks of
 * the min / max reduction.  Needs no GPU. */
void spim_min_filter_tiles(int32_t sizes[6]);

/* MinFilterThreshold.computeBoundingBox: per axis the smallest and largest index of the voxels
 * with (double)v > threshold.  With no such voxel the reference's integers come back
 * (bounds_min = dims, bounds_max = 0) and *found = 0. */
int spim_threshold_bounds(const float* img, const int64_t dims[3], double threshold, int device,
                          int64_t bounds_min[3], int64_t bounds_max[3], int32_t* found);

typedef struct spim_segment_result {
    float   min, max;        /* of the image (before the filter)                            */
    double  threshold;       /* (double)(max - min) * (background / 100.0) + (double)min     */
    int64_t bounds_min[3];   /* as spim_threshold_bounds, of the filtered image             */
    int64_t bounds_max[3];
    int32_t found;
    int32_t reserved[3];
} spim_segment_result;

/* min / max -> threshold -> minimum filter -> box in one call.  filtered (may be NULL)
 * receives the filtered image (the reference's "Display image used for segmentation");
 * without it the z pass of the filter only feeds the box and nothing image-sized is written
 * beyond the two scratch volumes.  background: inside (0, 100), in percent. */
int spim_segment_bounds(const float* img, const int64_t dims[3], double background, int radius, int device,
                        float* filtered, spim_segment_result* res);

typedef struct spim_autobbox_params {
    double background;             /* percent of the range; default 5                        */
    int    discarded_object_size;  /* default 25; radiusMin = size / 2                        */
    int    downsampling;           /* default 4; the filter runs at max(radiusMin / ds, 1)    */
    int    device;
    int    src_on_device;          /* 1: views[].img are device pointers                      */
    int    reserved[8];
} spim_autobbox_params;

void spim_autobbox_params_default(spim_autobbox_params* p);

typedef struct spim_autobbox_result {
    int64_t bb_min[3];       /* the estimate, world voxels: bounds * ds + max_min -+ 3 radiusMin */
    int64_t bb_max[3];       /* (not clamped to the maximal box, as the reference)           */
    int64_t bb_dims[3];      /* bb_max - bb_min + 1                                           */
    int32_t found;           /* 0: nothing above the threshold; bb_* then hold the reference's */
    int32_t radius_min;      /*    inverted box and must not be used                          */
    int32_t eff_radius;
    int32_t reserved;
    int64_t max_min[3];      /* the maximal box                                               */
    int64_t max_max[3];
    int64_t max_dims[3];
    int64_t fused_dims[3];   /* max_dims / downsampling                                       */
    spim_segment_result seg; /* of the fused image                                            */
} spim_autobbox_result;

/* AutomaticBoundingBox.queryParameters + MinFilterThreshold.run over nviews views: the
 * maximal box, its fusion into device memory (spim_fuse_weighted_average, interpolation 0,
 * no blending), spim_segment_bounds on it.  An effective radius above
 * SPIM_MIN_FILTER_MAX_RADIUS and a downsampling that leaves no voxel are SPIMDECON_ERR_ARG.
 * Not restated: "Load input images sequentially" (ProcessSequential accumulates in float). */
int spim_auto_bounding_box(int nviews, const spim_view_source* views, const spim_autobbox_params* p,
                           spim_autobbox_result* res);

/* frees device `device`'s scratch of this section (the next call allocates it again) */
int spim_bbox_release_workspace(int device);

/* ======================================================================
 * 8b. The bounding box from the interest points, "Automatically reorientate and estimate based
 *     on sample features" -- spim/process/fusion/boundingbox/AutomaticReorientation.java:277-573
 *     with the vendored vecmath (Transform3D.java:1397-1450, :4755-4765, Vector3d.java:127-166).
 *     All arithmetic is double in the reference's order, no multiply and add contracted; every
 *     result is bit-exact against that arithmetic with the host's libm for sqrt, acos, sin and
 *     cos (the payload of a NaN is not pinned).  Point lists are (n, 3) doubles (x, y, z), host
 *     or device memory; non-finite coordinates (as double or as float), a null list with a
 *     positive count and more than 2^31 - 1 points are SPIMDECON_ERR_ARG, the message led by the
 *     call's name.
 * ====================================================================== */

/* the farthest-pair kernel's tile: row points per block = column points per LDS tile.  Host
 * only: needs no GPU. */
void spim_reorient_tile(int32_t* tile);

/* determineOptimalBoundingBox :316-343 over all n (n - 1) / 2 pairs: *d2 = the largest squared
 * distance (dx * dx + dy * dy + dz * dz of a - b), (*i, *j) = the indices of the reference's p1
 * and p2: the first pair in (i, j) scan order among those at that distance, ordered so that
 * p1.x <= p2.x -- except when it is the start pair (0, 1), which the reference never reorders.
 * n < 2 is SPIMDECON_ERR_ARG (the reference fails on points.get(1)). */
int spim_farthest_pair(const double* pts, int64_t n, int device, int32_t* i, int32_t* j, double* d2);

/* testAxis :429-442 under m (1 .. 27) given transforms at once: mats holds m row-major 3x4
 * doubles (host memory); every point goes through Transform3D.transform, per row
 * ((m0 x + m1 y) + m2 z) + m3, and out6m[6 k ..] = min x, y, z, max x, y, z under matrix k by
 * Math.min / Math.max from +-Double.MAX_VALUE (a NaN spreads: a matrix of NaNs gives NaNs for
 * that matrix only; -0 < +0).  n >= 1. */
int spim_axis_boxes(const double* pts, int64_t n, const double* mats, int m, int device, double* out6m);

/* determineSizeSimple :488-512: min x, y, z, max x, y, z of the coordinates as they are (no
 * transform: a -0 stays -0).  n >= 1. */
int spim_points_min_max(const double* pts, int64_t n, int device, double* out6);

typedef struct spim_reorient_params {
    int32_t use_corresponding;  /* 1 (the dialog's default): only detections corr[v][k] of list v  */
    int32_t reorientate;        /* 1: the minimal-volume rotation; 0: the dialog's fourth choice,  */
                                /*    the identity and determineSizeSimple                         */
    double  percent;            /* "Additional size [%]" of the largest padding; default 10        */
    int32_t device;
    int32_t far_split;          /* 0 = auto; >0 forces the partitions of the column tiles (tests)  */
    int32_t reserved[8];
} spim_reorient_params;

void spim_reorient_params_default(spim_reorient_params* p);

typedef struct spim_reorient_result {
    double  transform[12];   /* row-major 3x4, to preconcatenate to every view's model            */
    double  min_f[3];        /* the box of the world points under transform, before the padding   */
    double  max_f[3];
    int64_t bb_min[3];       /* (int) Math.round(min_f - add); add = the largest over the axes of */
    int64_t bb_max[3];       /* (max_f - min_f) * (percent / 100.0) / 2; Math.round(max_f + add)  */
    int64_t bb_dims[3];      /* bb_max - bb_min + 1                                               */
    int64_t n_points;        /* world points used                                                 */
    int32_t far_i, far_j;    /* as spim_farthest_pair, indices into the concatenated world points */
    double  far_d2;          /* (-1, -1, 0 with reorientate 0)                                    */
    double  start_volume;    /* testAxis of the farthest pair's direction (the reference logs it) */
    double  min_volume;      /* of min_f / max_f: the smallest over the 8 x 27 candidates         */
    double  axis[3];         /* the search vector the transform maps onto the x axis              */
} spim_reorient_result;

/* getAllDetectionsInGlobalCoordinates, then determineOptimalBoundingBox (or determineSizeSimple)
 * and :277-289.  lists[v] (counts[v] points, view pixels) goes through models[12 v ..] (row-major
 * 3x4, host memory) row by row ((m0 x + m1 y) + m2 z) + m3; the views are concatenated in order.
 * With use_corresponding only the detections corr[v][0 .. corr_counts[v]) of list v are taken, in
 * that order (int64 indices, host or device memory; one out of range is SPIMDECON_ERR_ARG);
 * without it corr and corr_counts may be NULL.  The search: from the farthest pair's direction,
 * the steps 0.4 .. 0.001, per step the 27 candidates in zi, yi, xi order about the step's
 * start vector in one spim_axis_boxes launch, a candidate taken on a strictly smaller volume.
 * Deviation: fewer than two world points (one with reorientate 0) are SPIMDECON_ERR_ARG -- the
 * reference stops at none and fails on points.get(1) at one.  A box beyond the int range and
 * world coordinates that are not finite are SPIMDECON_ERR_ARG. */
int spim_reorient_bounding_box(int n_views, const double* const* lists, const int64_t* counts,
                               const int64_t* const* corr, const int64_t* corr_counts,
                               const double* models, const spim_reorient_params* params,
                               spim_reorient_result* result);

/* frees device `device`'s scratch of this section (the next call allocates it again) */
int spim_reorient_release_workspace(int device);

/* ======================================================================
 * 9. PSF extraction / transformation --
 *    spim/process/fusion/deconvolution/ExtractPSF.java.  All buffers are
 *    x-fastest float32 in host memory unless stated; dims are (x, y, z).
 * ====================================================================== */

/* transformPSF (:309-346): odd size of the transformed PSF and the offset that
 * keeps model(dim / 2) at its centre voxel (offset may be NULL). */
int spim_psf_transformed_size(const int64_t psf_size[3], const double model[12], int64_t out_size[3],
                              double offset[3]);

/* transformPSF + transform (:309-346, :424-460): n-linear over a zero-extended
 * PSF at inverse(model)(i + offset); out holds spim_psf_transformed_size voxels.
 * Also the path of loadAndTransformPSFs (:520-575) for PSFs read from files. */
int spim_transform_psf(const float* psf, const int64_t psf_size[3], const double model[12], float* out,
                       int device);

/* extractNextImg (:260-279): extractPSFLocal (:383-422; the sum over beads of
 * the n-linear samples of the periodic-extended view at i - size/2 + bead,
 * locations = nlocations x (x, y, z) local pixel coordinates), normalize
 * (:281-299) into psf_original (psf_size voxels), then -- when psf_transformed
 * is not NULL -- transformPSF with the view model.  img may be a device
 * pointer (img_on_device = 1), e.g. the source stack of spim_prepare_inputs. */
int spim_extract_psf(const float* img, const int64_t dims[3], int img_on_device, const double* locations,
                     int64_t nlocations, const int64_t psf_size[3], const double model[12], float* psf_original,
                     float* psf_transformed, int device);

/* spim_extract_psf for nviews views at once (ExtractPSF.extract over the views of a
 * timepoint): dims, models are nviews x 3 / x 12 (models may be NULL when
 * psf_transformed is NULL; entries of psf_transformed may be NULL); psf_original
 * and psf_transformed entries may be host or device pointers.  The views run
 * concurrently on their own streams: one view's bead sum is psf_size serial float
 * chains (bead order, as the reference), too few to fill the GPU alone.  Results are
 * identical to nviews spim_extract_psf calls. */
int spim_extract_psfs(int nviews, const float* const* imgs, const int64_t* dims, int img_on_device,
                      const double* const* locations, const int64_t* nlocations, const int64_t psf_size[3],
                      const double* models, float* const* psf_original, float* const* psf_transformed,
                      int device);

/* spim_extract_psf(s) keep one view's device buffers and stream per view between
 * calls (a whole view when img is a host pointer, the bead samples, the PSFs); this
 * frees them on `device` (-1: every device), e.g. before an RL session is created on
 * the same GPU.  No reference counterpart (ExtractPSF allocates per call). */
int spim_psf_release_workspace(int device);

/* computeAverageTransformedPSF (:164-208): the PSFs (psf_dims = npsfs x 3)
 * point-mirrored about their centres and summed into the max size, written
 * to avg_dims.  avg == NULL: only the dims are returned. */
int spim_average_transformed_psf(int npsfs, const float* const* psfs, const int64_t* psf_dims, float* avg,
                                 int64_t avg_dims[3], int device);

/* computeMaxProjection (:110-162): max along min_dim (0 x, 1 y, 2 z; < 0 = the
 * first smallest dimension, returned in used_dim).  out == NULL: dims only. */
int spim_max_projection(const float* img, const int64_t dims[3], int min_dim, float* out, int64_t out_dims[2],
                        int* used_dim, int device);

/* ======================================================================
 * 10. Legacy simultaneous-update multiview RL (opt-in) --
 *     mpicbg/spim/postprocessing/deconvolution/LucyRichardsonMultiViewDeconvolution.java
 *     :24-358 (lucyRichardsonMultiView; LucyRichardsonFFT.java:7-38 holds one view).
 *     Every view's correction is computed from the same psi (not MVDeconvolution's
 *     sequential rule, section 5), so the views shard over ranks -- view v on rank
 *     v % nranks, as the reference hands view v to thread v % numThreads (:127-128) --
 *     and the per-voxel merge of the corrections is one RCCL all-reduce of a double
 *     per voxel each iteration (a product when multiplicative, else a sum).  Every
 *     rank holds the whole psi; all ranks return the same psi and statistics.
 *     The convolutions extend their input by mirroring (extendMirrorSingle): the
 *     reference's imglib1 FourierConvolution is absent and its extension not restated.
 * ====================================================================== */
typedef struct lrsim_session lrsim_session;

/* dims {nx, ny, nz} of the whole volume; nranks > 1 needs the 128-byte comm_id of
 * mvd_comm_unique_id (a non-NULL id with nranks == 1 makes a one-rank communicator) */
int  lrsim_create(const int64_t* dims, int device, int nranks, int rank, const char* comm_id,
                  lrsim_session** out);
/* One process, several GPUs (the reference's threads, LRMV:118-178): view v goes to
 * devs[v % ndev] (ids may repeat); each device holds a psi replica and its views' partial,
 * merged on devs[0] over xGMI each iteration (a sum or a product, in device order), and
 * the new psi copied back.  No RCCL. */
int  lrsim_create_devices(const int64_t* dims, const int* devs, int ndev, lrsim_session** out);
void lrsim_destroy(lrsim_session* h);
/* Adds view number <views so far> (the data list order of the reference).  Every rank
 * adds every view; kdims (odd {kx, ky, kz}) is always required, img / weight / kernel
 * (raw PSF; normImage'd at init) only for the views this rank owns -- NULL otherwise.
 * img / weight: dims voxels, host or device pointers.  Weights are required: the
 * reference's normAllImages reads one per view (:401). */
int  lrsim_add_view(lrsim_session* h, const float* img, const float* weight, const float* kernel,
                    const int* kdims);
int  lrsim_owns_view(lrsim_session* h, int view, int* owned);
/* device holding view `view` on this rank (-1: another rank's view) */
int  lrsim_view_device(lrsim_session* h, int view, int* device);
/* normImage of every kernel (:45-58, exact sum as BigDecimal), psi = (float) the
 * average intensity where two or more views overlap (normAllImages :360-457) */
int  lrsim_init(lrsim_session* h, double* avg_out);
/* iters iterations (the reference's do-while runs max(1, maxIterations)); stats (may be
 * NULL): iters x {sumChange, maxChange} (:309-330).  lambda > 0: Tikhonov (:290-301). */
int  lrsim_run(lrsim_session* h, int iters, int multiplicative, double lambda, double* stats);
/* psi (dims voxels) into a host or device buffer */
int  lrsim_get_psi(lrsim_session* h, float* out);
/* padded FFT lengths {Mx, My, Mz} (info) */
int  lrsim_fft_dims(lrsim_session* h, int64_t* out3);
/* The per-voxel rule of lrsim_run alone (:254-330; tests): psi_out = rule(psi_in, value,
 * num), Tikhonov for lambda > 0, the NaN / minValue clamp; stats2 (host) receives
 * {sumChange, maxChange}.  psi_in, value, num, psi_out: n >= 1 voxels in device memory of
 * the current device (psi_out may be psi_in).  Same kernel, launch geometry and reduction
 * as an iteration of lrsim_run. */
int  lrsim_update_rule(const float* psi_in, const double* value, const double* num, int64_t n,
                       int multiplicative, double lambda, float* psi_out, double* stats2);

#ifdef __cplusplus
}
#endif
#endif /* SPIMDECON_H */
