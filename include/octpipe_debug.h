/*
 * octpipe_debug.h -- test and measurement hooks of liboctpipe.so.  NOT part of the drop-in boundary (octpipe.h): nothing here has
 * a counterpart in the reference's kernels.h, and a host application never needs it.  The parity tests use these entry points
 * to look at single stages (cu:109-211 unpack, the spectrum behind cu:1514-1515), to hold two implementations of a stage
 * against each other, and to pin which implementation a configuration runs on.
 */
#ifndef OCTPIPE_DEBUG_H
#define OCTPIPE_DEBUG_H

#include "octpipe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* complex spectrum after IDFT (before mean subtraction) of the first `lines` A-scans of d_raw */
int octpipe_debug_spectrum(octpipe_t* h, const void* d_raw, int lines, float* hostComplexOut);
/* raw unpack (+ bitshift, + rolling average when enabled) of the first `count` samples of d_raw as
 * float32: the stage of cu:109-211 in isolation, for the bit-exactness test */
int octpipe_debug_unpack(octpipe_t* h, const void* d_raw, size_t count, float* hostOut);
/* route uint16 input through the float32 "prepared" path as well (normally only uint8/uint32 input
 * and the Lanczos variant take it); lets a test prove fused-unpack == standalone unpack bit-for-bit */
int octpipe_debug_force_prepared(octpipe_t* h, int enable);
/* Route selection for tests and A/B measurements: where two independent implementations of a stage exist, these flags keep
 * a configuration on the slower / more general one so that the tests can hold one against the other.  Flags of an existing
 * handle take effect with the next buffer; the FFT-backend flags ("creation" below) are read when a handle is created and are
 * passed to octpipe_debug_create.  No environment variable is read anywhere in the library, and no per-thread state either. */
enum {
	OCTPIPE_ROUTE_NO_REAL_INPUT = 1,   /* dispersion compensation off: keep the general kernel instead of the two-A-scans-per-transform kernels */
	OCTPIPE_ROUTE_NO_FUSED_BG   = 2,   /* post-process background removal always as the post pass (cu:1567), never inside the image store */
	OCTPIPE_ROUTE_FULL_DISPLAY  = 4,   /* display frames re-extracted from the whole volume for every buffer (cu:1571-1578 literally) */
	OCTPIPE_ROUTE_NO_TEAM       = 8,   /* samplesPerLine = 4096 / 1664: keep the one-wave-per-A-scan kernel instead of the team kernel (8192: the library route) */
	OCTPIPE_ROUTE_NO_LIBFFT     = 16,  /* creation: Bluestein on the in-register FFT instead of hipFFT for lengths without a fused kernel (<= 2047) */
	OCTPIPE_ROUTE_FORCE_LIBFFT  = 32,  /* creation: every length through unpack -> gather -> hipFFT -> epilogue (the reference's pass structure) */
	OCTPIPE_ROUTE_NO_MIXED      = 64,  /* creation: samplesPerLine = 1664 without the mixed-radix kernel */
	OCTPIPE_ROUTE_NO_MIXEDN     = 128, /* lengths with a generic mixed-radix plan (1000, 1536, 2000 ...): keep the library route / Bluestein */
	OCTPIPE_ROUTE_NO_MIXEDN_STATIC = 512, /* keep the run-time-plan kernel (mixedn_kernel.h) where a kernel compiled for the length exists (mixedn_static.h) */
	OCTPIPE_ROUTE_MIXEDN_STATIC_OLD_LAYOUT = 2048, /* creation: the run-time compiled kernel with its first plan order and exchange layout (largest radix first, always padded) */
	OCTPIPE_ROUTE_TINY_GRID = 1024,    /* the run-time compiled kernel, the general fused kernel and the real-input kernels (real2_kernel.h, real2n_kernel.h) on TWO persistent workgroups: every wave loops over many A-scans even of a small test buffer */
	OCTPIPE_ROUTE_MIXEDN_SIMPLE_RADICES = 256, /* the generic plan from prime and power-of-two radices only (no 6, 10, 12, 14, 15, 20 butterflies) */
	OCTPIPE_ROUTE_TEAM1664_ALWAYS = 16384, /* samplesPerLine = 1664: the two-wave team kernel for every resampling mode it has (by default linear / no resampling run on the one-wave kernel, faster there); A/Bs and the parity of the in-store correction, which always runs on the team kernel */
	OCTPIPE_ROUTE_NO_FUSED_SINUS = 8192, /* sinusoidal scan correction always as the post pass (cu:1551-1554 as one gather pass), never inside a transform kernel's image store (MODE_SINUS of the general, team, N = 1664 and run-time compiled kernels) */
	OCTPIPE_ROUTE_ONE_LANE = 32768, /* every buffer on the compute stream itself, never on the second compute lane (csrc/lanes.h): the steady state as it was before the lanes, for same-build A/Bs and the bit-for-bit parity of the two */
	OCTPIPE_ROUTE_FUSED_DISPLAY = 4096 /* display frames (one frame per view) written by the general fused kernel's image store (MODE_DISP) instead of by oct_display_frames_kernel.
	                                      Opt-in: bit-identical frames, one launch per buffer instead of two, but not faster -- the store side costs the kernel what the extraction kernel
	                                      cost (profiles/r5b..r5f_*_ab.txt) */
};
int octpipe_debug_set_route(octpipe_t* h, unsigned flags);
/* octpipe_create_with_format with OCTPIPE_ROUTE_* flags from the start (the creation-time ones select the FFT backend) */
int octpipe_debug_create(octpipe_t** out, int device, const OctPipeAcquisitionParams* acq, const OctPipeParams* params,
                         void* h_buffer1, void* h_buffer2, int sampleFormat, unsigned routeFlags);
/* what the device holds in the raw slot of the last octpipe_process[_async] call (slot < 0) or in slot 0 / 1: `bytes` bytes from
 * its start, copied on the handle's compute stream behind everything enqueued there.  Lets the group stress harness tell a
 * wrong host-to-device copy from a wrong kernel result. */
int octpipe_debug_read_raw_slot(octpipe_t* h, int slot, void* dst, size_t bytes);
/* persistent-grid size (workgroups) of the last launch of the general fused kernel: each kernel variant has its own
 * occupancy-derived grid, whatever was launched before it in the process */
int octpipe_debug_last_grid(const octpipe_t* h, int* blocks);
/* which implementation the image launch of the last processed buffer took (tests pin the routing with it: a silent fall-back
 * to a slower but equally correct path would otherwise go unnoticed) */
enum {
	OCTPIPE_PATH_PREPARED_ROWS = 1,   /* a row kernel / unpack kernel wrote float32 rows in front of the transform kernel */
	OCTPIPE_PATH_FUSED_BG      = 2,   /* post-process background removal inside the image store */
	OCTPIPE_PATH_TEAM          = 4,   /* one A-scan (or pair) per team of waves: team_kernel.h, team_real2_kernel.h, team1664_kernel.h */
	OCTPIPE_PATH_REAL_INPUT    = 8,   /* two A-scans per complex transform */
	OCTPIPE_PATH_LIBRARY_FFT   = 16,  /* gather -> hipFFT -> epilogue */
	OCTPIPE_PATH_ROLL_IN_KERNEL = 32, /* rolling average inside the transform kernel */
	OCTPIPE_PATH_MIXED_RADIX   = 64,  /* mixed1664.h / mixed1664_real2.h, mixedn_kernel.h */
	OCTPIPE_PATH_BLUESTEIN     = 128,
	OCTPIPE_PATH_STATIC_PLAN   = 256, /* with MIXED_RADIX: the kernel compiled for this length (mixedn_static.h) instead of the run-time plan */
	OCTPIPE_PATH_FUSED_DISPLAY = 512, /* the display frames (one frame per view) written by the image store of the fused kernel */
	OCTPIPE_PATH_FUSED_SINUS   = 1024 /* sinusoidal scan correction inside the image store of the transform kernel (general, team, N = 1664 or run-time compiled; no scratch slot, no post pass) */
};
int octpipe_debug_last_path(const octpipe_t* h, unsigned* path);
/* The compute lanes (csrc/lanes.h): *overlapped = buffers that went out on the lane of their slot with no join in front of them,
 * *joins = how often the compute stream had to be ordered behind work on the second lane (another entry point, or a buffer that is
 * not eligible, arriving while the second lane held work).  A run in which the lanes never engaged shows overlapped == 0. */
int octpipe_debug_lane_stats(const octpipe_t* h, uint64_t* overlapped, uint64_t* joins);
/* The eligibility rule WITHOUT a device (csrc/lanes.h lane_blockers, the function every buffer goes through): what a handle is and
 * holds, as plain facts, next to the parameter snapshot.  *blockers = one bit per condition that keeps the next buffer off the lanes
 * (LaneBlocker of lanes.h, bit order as listed there; 0 = the buffer goes out on the lane of its slot), *allBlockers (may be NULL) = the
 * mask of every condition the rule knows.  planKind / planPrepared / planError: the image route of the buffer as octpipe_debug_route
 * reports it (kind; preparedRollW >= 0; its return code != 0).  lastDisplaySignature: octpipe_debug_display_signature of the settings
 * the frames were last extracted with in full (0: never). */
typedef struct OctPipeLaneFacts {
	uint32_t buffersPerVolume, routeFlags;
	int32_t deviceInput;               /* octpipe_process_device (1) or the ring / H2D path (0) */
	int32_t lutDirty;
	int32_t fpnDetermined, meanLinePinned;
	int32_t floatStreamingRegistered, streamingRegistered, callbacksRegistered;
	int32_t streamExposed, groupMember;
	int32_t planKind, planPrepared, planError;
	uint64_t lastDisplaySignature;
} OctPipeLaneFacts;
int octpipe_debug_lane_blockers(const OctPipeLaneFacts* facts, const OctPipeParams* params, unsigned* blockers, unsigned* allBlockers);
int octpipe_debug_display_signature(const OctPipeParams* params, uint64_t* signature);
/* The same decision WITHOUT a device (csrc/route.h: derive_route_facts + choose_route, the pure functions octpipe_debug_create and
 * every image launch go through): the OCTPIPE_PATH_* bits, the kernel family (route.h RouteKind), the sample container the transform
 * kernel reads (0 uint8, 1 uint16, 3 prepared float32 rows, 4 / 5 packed 12 bit, 6 int16) and the rolling-average window handed to the
 * prepare kernel in front (-1: no prepare kernel) that a buffer with these acquisition parameters, settings, sample format and route
 * flags runs on.  assumeFftLibrary / assumeRtc: libhipfft.so / hiprtc taken to be usable in the process.  spectrum = 1: the launch of
 * the mean-line estimate instead of the image launch.  tests/test_route.py holds the routing table against it in the CPU suite. */
int octpipe_debug_route(const OctPipeAcquisitionParams* acq, const OctPipeParams* params, int sampleFormat, unsigned routeFlags, int assumeFftLibrary, int assumeRtc,
                        int spectrum, unsigned* path, int* kind, int* intype, int* preparedRollW);

/* The work list of the sinusoidal scan correction inside the fused kernel's store (csrc/sinus_plan.h) for `ascansPerBscan`, without a
 * device: *entries = rows of a B-scan the store needs (0: no plan for this B-scan width, the correction stays the post pass); when
 * `out` is not NULL and holds at least 4 x capacityEntries words, the entries {row | firstOutput << 16, frac0, frac1, 0}. */
int octpipe_debug_sinus_plan(unsigned ascansPerBscan, unsigned* entries, uint32_t* out, size_t capacityEntries);
/* MODE_SINUS: blocks of the work list per wave (0 = the library's default); takes effect with the next buffer */
int octpipe_debug_set_sinus_blocks_per_wave(octpipe_t* h, unsigned blocksPerWave);

/* Lengths without a dedicated kernel run a kernel compiled for them at run time (hiprtc; csrc/mixedn_rtc.hip).  Status: whether
 * the handle's length does (h may be NULL), its plan (five radices, 0 = unused), how many instances the process has compiled, the
 * seconds that took, and why the last attempt failed / why this handle keeps another route (empty: no failure). */
int octpipe_debug_rtc_status(const octpipe_t* h, int* usesIt, int* radices5, int* compiledInProcess, double* compileSeconds, char* message, size_t messageBytes);
/* The variants a handle can reach next are compiled on a background thread (octpipe_create / octpipe_set_params): returns OCTPIPE_OK
 * once none is queued or running, an error after timeoutSeconds. */
int octpipe_debug_rtc_wait_idle(double timeoutSeconds);
/* how many instances this process took from the directory of octpipe_set_kernel_cache_dir instead of compiling them */
int octpipe_debug_rtc_disk_hits(int* hits);
/* Further compiler options for the instances compiled from now on (process-wide, blank-separated, NULL = none): the numeric knobs
 * of csrc/mixedn_static.h, e.g. "-DOCT_MXS_LUT_AHEAD=4 -DOCT_MXS_TAP_AHEAD=2".  Instances are cached per option string. */
int octpipe_debug_rtc_set_options(const char* extraOptions);
/* The build check of that path without a device: plan samplesPerLine and compile the instance (intype 1 = uint16 rows, 3 = prepared
 * float32 rows; rs 0 none / 1 linear / 2 cubic; mode 2 spectrum, 4 log, 8 background removal in the store) for `arch` ("gfx950"). */
int octpipe_debug_rtc_compile(unsigned samplesPerLine, int intype, int rs, int mode, const char* arch, size_t* codeBytes, int* waves, int* radices5, double* seconds);

/* Dispersion estimation (octpipe.h): the per-(candidate, A-scan) metric matrix behind octpipe_dispersion_scores, K x M floats
 * [candidate][A-scan] (NULL: not wanted), the K scores (NULL: not wanted) and the summed device time of the sweep kernel's launches
 * in ms (NULL: not timed) */
int octpipe_debug_dispersion_metrics(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m, const float* d2, const float* d3,
                                     unsigned candidates, float* metrics, float* scores, double* sweepKernelMs);
/* the device-built phasor table of a candidate list: theta (K x N floats, NULL: not wanted) and e^{i theta} (K x N complex) */
int octpipe_debug_dispersion_phasors(octpipe_t* h, float d0, float d1, const float* d2, const float* d3, unsigned candidates, float* theta,
                                     float* phasorsComplex);
/* Phase extraction (octpipe.h): octpipe_phase_accumulate, plus the device time in ms between events around the call's work on the
 * stream (device raw: the accumulate kernel alone; host raw: the staged copies as well) */
int octpipe_debug_phase_accumulate(octpipe_t* h, const void* raw, int rawIsDevice, uint32_t firstAscan, uint32_t ascanCount, double* kernelMs);
/* Image statistics (octpipe.h): the two calls, plus the device time in ms between events around the call's work on the stream (device
 * source: the kernels alone; host source: the staged copies as well) */
int octpipe_debug_processed_statistics(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange,
                                       float lo, float hi, uint64_t* histogram, OctPipeImageStatistics* out, double* kernelMs);
int octpipe_debug_raw_statistics(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange,
                                 int64_t lo, uint32_t binWidth, uint64_t* histogram, OctPipeImageStatistics* out, double* kernelMs);
/* Peak analysis (octpipe.h): octpipe_peak_analysis, plus the device time in ms between events around the call's work on the stream
 * (device source: the kernels alone; host source: the staged copies as well) */
int octpipe_debug_peak_analysis(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipePeakSettings* s,
                                OctPipePeak* peaks, float* averaged, double* kernelMs);
/* Volume rendering (octpipe.h): octpipe_render_volume, then a wait for the kernel and its device time in ms between events around
 * the launch (the staging copy of host voxels is outside them) */
int octpipe_debug_render_volume(octpipe_t* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dims[3], const OctPipeRenderSettings* s,
                                void** d_image, size_t* bytes, double* kernelMs);
/* octpipe_render_oct_depth, then a wait and the device times in ms of its two kernels, each between events of its own: the surface
 * pre-pass and the ray cast (either pointer may be NULL) */
int octpipe_debug_render_oct_depth(octpipe_t* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dims[3], const OctPipeRenderSettings* s,
                                   void** d_image, size_t* bytes, double* prepassMs, double* raycastMs);
/* Surface views (octpipe.h): the four calls, then a wait for their work and its device time in ms between events around it on the
 * stream (device source: the kernels alone; host source or host surface: the staged copies as well; the copy of a host result is
 * outside them, except for the slices of a flattened volume).  octpipe_debug_flatten takes the form of the kernel's loads besides:
 * 0 = the one octpipe_flatten uses, 1 = dword loads, 2 = aligned 16-byte loads with a cross-lane shift (anything else:
 * OCTPIPE_ERR_INVALID_ARGUMENT naming `loads`); every form writes the same bits. */
int octpipe_debug_surface_detect(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                 const OctPipeSurfaceDetectSettings* s, int32_t* surface, int surfaceIsDevice, double* kernelMs);
int octpipe_debug_surface_smooth(octpipe_t* h, const int32_t* surface, int surfaceIsDevice, uint32_t rows, uint32_t cols, uint32_t radius,
                                 int32_t* out, int outIsDevice, double* kernelMs);
int octpipe_debug_surface_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface,
                                 int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* s, float* out, int outIsDevice, double* kernelMs);
int octpipe_debug_flatten(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface,
                          int surfaceIsDevice, const OctPipeFlattenSettings* s, float* out, int outIsDevice, unsigned loads, double* kernelMs);
/* Boundary tracing (octpipe.h): the call, then a wait for its work and its device time in ms between events around it on the stream
 * (device source and guide: the kernel alone; host source or host guide: the staged copies as well; the copies of host results are
 * outside them).  `form` is the kernel: 0 = the one octpipe_trace_boundary picks (one wave per B-scan where H <= 64, else one workgroup;
 * the choices in LDS where they fit, else in scratch), 1 = wave, choices in LDS, 2 = wave, choices in scratch, 3 = workgroup, choices in
 * LDS, 4 = workgroup, choices in scratch.  1 and 2 need H <= 64; 1 needs ascanCount * ((H + 1) / 2) <= 32 768, 3 needs it <= 147 328.  A
 * code that does not apply, or any other: OCTPIPE_ERR_INVALID_ARGUMENT naming `form`.  Every form writes the same bits. */
int octpipe_debug_trace_boundary(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* guide,
                                 int guideIsDevice, const OctPipeBoundaryTraceSettings* s, int32_t* surface, float* pathCost,
                                 int surfaceIsDevice, unsigned form, double* kernelMs);
/* Angiography (octpipe.h): the two calls, then a wait for their work and its device time in ms between events around it on the stream
 * (device source: the kernels alone; host source or host surface: the staged copies as well; the copy of a host image is outside them,
 * the slices of a host contrast volume are inside).  octpipe_debug_angiogram_enface takes the form of the kernel besides: 0 = the one
 * octpipe_angiogram_enface uses for the thickness, 1 = one wave per A-scan, 2 = teams of 16 lanes, four A-scans per wave (thickness <= 64
 * only); anything else: OCTPIPE_ERR_INVALID_ARGUMENT naming `form`.  Every form writes the same bits. */
int octpipe_debug_angiogram(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                            float* out, float* mean, int outIsDevice, double* kernelMs);
int octpipe_debug_angiogram_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                   const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out,
                                   int outIsDevice, unsigned form, double* kernelMs);
/* Repeat registration (octpipe.h): the three calls, then a wait for their work and its device time in ms between events around it on the
 * stream (device source and device shifts: the kernels alone; host source, host shifts or host surface: the staged copies as well; the
 * copies of host shifts, costs and images back are outside them, the slices of a host contrast volume are inside).
 * octpipe_debug_angiogram_enface_registered takes `form` as octpipe_debug_angiogram_enface does. */
int octpipe_debug_repeat_shifts(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                const OctPipeRepeatShiftSettings* s, int32_t* shifts, int shiftsIsDevice, double* costs, double* kernelMs);
int octpipe_debug_angiogram_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                       const OctPipeAngioSettings* s, float* out, float* mean, int outIsDevice, const int32_t* shifts,
                                       int shiftsIsDevice, const OctPipeAngioRegistration* registration, double* kernelMs);
int octpipe_debug_angiogram_enface_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                              const OctPipeAngioSettings* s, const int32_t* surface, int surfaceIsDevice,
                                              const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice, const int32_t* shifts,
                                              int shiftsIsDevice, const OctPipeAngioRegistration* registration, unsigned form,
                                              double* kernelMs);
/* Attenuation (octpipe.h): the two calls, then a wait for their work and its device time in ms between events around it on the stream
 * (device source, gain and surface: the kernel alone; host ones: the staged copies as well; the copy of a host image is outside them, the
 * slices of a host coefficient volume are inside).
 * octpipe_debug_attenuation_sums writes the float64 sums `below` of every bin (octpipe.h "attenuation", sum below a bin) instead of mu32:
 * float64 [bscanCount][ascanCount][sampleCount] in host or device memory, otherwise the arguments and checks of octpipe_attenuation.  It
 * is there because the order of the summation shows in the float32 output only at rounding boundaries, and in these sums in most bins. */
int octpipe_debug_attenuation(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                              const OctPipeAttenuationSettings* s, const float* depthGain, int gainIsDevice, float* out, int outIsDevice,
                              double* kernelMs);
int octpipe_debug_attenuation_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                     const OctPipeAttenuationSettings* s, const float* depthGain, int gainIsDevice, const int32_t* surface,
                                     int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice,
                                     double* kernelMs);
int octpipe_debug_attenuation_sums(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                   const OctPipeAttenuationSettings* s, const float* depthGain, int gainIsDevice, double* out, int outIsDevice);

#ifdef __cplusplus
}
#endif
#endif /* OCTPIPE_DEBUG_H */
