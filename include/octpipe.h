/*
 * octpipe.h -- C ABI of the MI355X-native OCT processing pipeline (liboctpipe.so).
 *
 * This is the drop-in boundary for ONE path of spectralcode/OCTproZ: the per-A-scan GPU
 * processing chain that the reference implements in
 *     octproz_project/octproz/src/cuda_code.cu           ("cu:")
 * and exposes through the `extern "C"` block of
 *     octproz_project/octproz/src/kernels.h:63-84        ("kernels.h:")
 * to its single caller octproz_project/octproz/src/processing.cpp ("processing.cpp:").
 *
 * The reference passes a Qt-bearing C++ object (OctAlgorithmParameters*, QString members) across
 * that boundary and keeps all state in module globals (cu:39-105), so it is not a C ABI.  Here the
 * same entry points take a POD mirror of the fields the pipeline actually reads and a handle.
 * Every function below names the reference interface it replaces; INTEGRATION.md shows the
 * ~80-line adapter that re-exports the 15 legacy names on top of these for the Qt host.
 *
 * Conventions: plain pointers and sizes only; every call returns an int status (OCTPIPE_OK = 0)
 * instead of the reference's printf / exit(EXIT_FAILURE) (helper_cuda.h:583-590);
 * octpipe_last_error() gives the text.  Not re-entrant per handle (the reference is not either:
 * all entry points are called from the single processing thread, processing.cpp:136-229).
 */
#ifndef OCTPIPE_H
#define OCTPIPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCTPIPE_ABI_VERSION 2

enum {
	OCTPIPE_OK = 0,
	OCTPIPE_ERR_INVALID_ARGUMENT = 1,
	OCTPIPE_ERR_NOT_INITIALIZED = 2,   /* reference: "Cuda: Device buffers are not initialized!" cu:1391-1394 */
	OCTPIPE_ERR_OUT_OF_MEMORY = 3,     /* reference: initializeCuda returns false, cu:975-1015 */
	OCTPIPE_ERR_DEVICE = 4,            /* any HIP runtime error (reference: checkCudaErrors -> exit) */
	OCTPIPE_ERR_UNSUPPORTED = 5,       /* e.g. samplesPerLine outside 8..65536 (dedicated kernels: 256..8192 and 1664; every other even 2-3-5-7-11-13-smooth
	                                      length up to 8192: a kernel compiled for it at run time; the rest through hipFFT, loaded at run time, or Bluestein up to 2047) */
	OCTPIPE_ERR_NO_DEVICE = 6,         /* no HIP device: the product path never falls back to a CPU */
	OCTPIPE_ERR_IN_CALLBACK = 7        /* a device-touching entry point was called from inside a data / event callback (see below) */
};

/* OctAlgorithmParameters::INTERPOLATION, octalgorithmparameters.h:55-59 */
enum { OCTPIPE_INTERP_LINEAR = 0, OCTPIPE_INTERP_CUBIC = 1, OCTPIPE_INTERP_LANCZOS = 2 };
/* WindowFunction::WindowType, windowfunction.h:41-48 */
enum { OCTPIPE_WINDOW_HANNING = 0, OCTPIPE_WINDOW_GAUSS = 1, OCTPIPE_WINDOW_SINE = 2,
       OCTPIPE_WINDOW_LANCZOS = 3, OCTPIPE_WINDOW_RECTANGULAR = 4, OCTPIPE_WINDOW_FLATTOP = 5 };
/* OctAlgorithmParameters::DISPLAY_FUNCTION, octalgorithmparameters.h:166-169 */
enum { OCTPIPE_DISPLAY_AVERAGING = 0, OCTPIPE_DISPLAY_MIP = 1 };

/* AcquisitionParams, octproz_devkit/src/acquisitionparameter.h:31-37 (same field order). */
typedef struct OctPipeAcquisitionParams {
	uint32_t samplesPerLine;    /* N: raw samples per A-scan */
	uint32_t ascansPerBscan;    /* A */
	uint32_t bscansPerBuffer;   /* B */
	uint32_t buffersPerVolume;
	uint32_t bitDepth;          /* bytes per sample = ceil(bitDepth/8), cu:1077 */
} OctPipeAcquisitionParams;

/* POD mirror of the OctAlgorithmParameters fields read by octCudaPipeline (cu:1389-1605);
 * defaults = octalgorithmparameters.cpp:36-112 (octpipe_default_params).  Flags are int32
 * (0/1).  The three "one-shot" flags are consumed (cleared) inside octpipe_process exactly where
 * the reference clears them, the caller's struct is never written. */
typedef struct OctPipeParams {
	int32_t bitshift;                                  /* cu:1409 */
	int32_t bscanFlip;                                 /* cu:1546 */
	int32_t signalLogScaling;                          /* cu:1538 */
	int32_t sinusoidalScanCorrection;                  /* cu:1551 */
	float   signalGrayscaleMin;
	float   signalGrayscaleMax;
	float   signalMultiplicator;
	float   signalAddend;
	int32_t backgroundRemoval;                         /* rolling-average DC removal, cu:1423 */
	int32_t rollingAverageWindowSize;
	int32_t resampling;                                /* cu:1448-1511 */
	int32_t resamplingInterpolation;                   /* OCTPIPE_INTERP_* */
	int32_t dispersionCompensation;
	int32_t windowing;
	int32_t fixedPatternNoiseRemoval;                  /* cu:1518 */
	int32_t continuousFixedPatternNoiseDetermination;
	int32_t redetermineFixedPatternNoise;              /* one-shot, cu:1524 */
	uint32_t bscansForNoiseDetermination;
	int32_t postProcessBackgroundRemoval;              /* cu:1557 */
	int32_t postProcessBackgroundRecordingRequested;   /* one-shot, cu:1561 */
	float   postProcessBackgroundWeight;
	float   postProcessBackgroundOffset;
	/* result delivery (cu:1595-1604) */
	int32_t streamToHost;                              /* quantised u8/u16/u32 D2H + callback */
	uint32_t streamingBuffersToSkip;
	int32_t streamFloatToHost;                         /* recParams.saveAs32bitFloat leg, cu:1596 */
	/* display-frame extraction (cu:1571-1582); plain device buffers instead of GL interop */
	int32_t bscanViewEnabled;
	int32_t enFaceViewEnabled;
	uint32_t frameNr;
	uint32_t functionFramesBscan;
	int32_t displayFunctionBscan;
	uint32_t frameNrEnFaceView;
	uint32_t functionFramesEnFaceView;
	int32_t displayFunctionEnFaceView;
	int32_t volumeViewEnabled;                         /* 8-bit volume down-conversion, cu:1579-1582 (ABI v2) */
} OctPipeParams;

typedef struct octpipe octpipe_t; /* all state the reference keeps in cu:39-105 */

/* Gpu2HostNotifier callbacks (gpu2hostnotifier.h:47-52, .cpp:45-53,75-86): the 7 arguments of
 * newGpuDataAvailable / newGpuFloatDataAvailable, plus a user pointer.  Fired from the HIP
 * runtime's callback thread (hipLaunchHostFunc), like cudaLaunchHostFunc cu:1369,1385. */
typedef void (*octpipe_data_callback)(void* buffer, unsigned bitDepth, unsigned samplesPerLine,
                                      unsigned linesPerFrame, unsigned framesPerBuffer,
                                      unsigned buffersPerVolume, unsigned currentBufferNr, void* user);
typedef void (*octpipe_event_callback)(void* user); /* backgroundRecorded, gpu2hostnotifier.cpp:57 */
/* Callbacks run inside hipLaunchHostFunc on the pipeline's result stream (the background callback on the compute stream):
 * while a data callback runs, the next device-to-host copy waits, the kernels of the following buffers do not.  They MUST NOT call any octpipe_* function that
 * touches the device (everything except octpipe_last_error, octpipe_get_acquisition_params and
 * octpipe_get_postprocess_background_host) -- HIP calls are not allowed there and a stream wait would deadlock.  The library
 * enforces it: on a thread that is inside one of its callbacks those entry points (octpipe_destroy and octpipe_group_destroy
 * included) return OCTPIPE_ERR_IN_CALLBACK without touching anything -- a host whose garbage collector finalises a pipeline
 * object on the callback thread gets an error code, not a hang.  octpipe_callback_active() tells a binding which case it is in. */
int octpipe_callback_active(void);

/* ------------------------------------------------------------------ library */
int         octpipe_abi_version(void);
const char* octpipe_last_error(void);             /* thread-local text of the last failure */
int         octpipe_device_count(int* count);     /* OCTPIPE_ERR_NO_DEVICE when none */
void        octpipe_default_params(OctPipeParams* p); /* octalgorithmparameters.cpp:36-112 */
/* sizeof(OctPipeParams) / sizeof(OctPipeAcquisitionParams) as this library was built: lets a foreign-language binding check
 * its own struct mirror before the first call */
void        octpipe_struct_sizes(size_t* paramsBytes, size_t* acquisitionParamsBytes);

/* ------------------------------------------------------------------ host curve generators
 * (OctAlgorithmParameters::update*Curve + Polynomial + WindowFunction; bit-exact contract) */
int octpipe_polynomial_curve(const float* coeffs, unsigned order, unsigned size, float* out);            /* polynomial.cpp:108-145 */
int octpipe_resample_curve(float c0, float c1, float c2, float c3, unsigned size, float* out);            /* octalgorithmparameters.cpp:141-168 */
int octpipe_custom_resample_curve(const float* curve, unsigned curveLength, unsigned size, float* out);   /* :153-159,167 + resizeCurve :263 */
int octpipe_dispersion_curve(float d0, float d1, float d2, float d3, unsigned size, float* out);          /* :206-222 */
int octpipe_window_curve(int windowType, float center, float fillFactor, unsigned size, float* out);      /* :234-249, windowfunction.cpp */

/* ------------------------------------------------------------------ lifecycle */
/* initializeCuda(h_buffer1, h_buffer2, params), kernels.h:63 / cu:1067-1162.  h_buffer1/2 are the
 * two acquisition ring slots (may be NULL for device-resident use); they are pinned
 * (hipHostRegister) here and unpinned in octpipe_destroy, ownership stays with the caller. */
int octpipe_create(octpipe_t** out, int device, const OctPipeAcquisitionParams* acq,
                   const OctPipeParams* params, void* h_buffer1, void* h_buffer2);

/* Sample formats beyond "the bit depth decides" (SURVEY 8 row N4).  The reference declares them
 * (src/octalgorithmparameters.h:61-77, enum DATA_TYPE, member :88) but never reads the field, so there
 * is no parity target: the decode is specified here (the test suite restates it independently).
 *   AUTO           uint8 / uint16 / uint32 by bitDepth -- the reference's behaviour (cu:107-149)
 *   UINT12_PACKED  two samples in three bytes, little endian (GenICam Mono12p):
 *                  b0 = s0[7:0], b1 = s0[11:8] | s1[3:0] << 4, b2 = s1[11:4]; buffer = 1.5 B/sample
 *   INT12_PACKED   same packing, samples are 12-bit two's complement
 *   INT8 / INT16 / INT32   two's complement in 1 / 2 / 4 bytes (INT10, INT12 travel as INT16)
 * The sample becomes the float of its integer value (exact; INT32 rounds to nearest even);
 * `bitshift` is an arithmetic >> 4 on the integer.  Everything downstream is unchanged. */
#define OCTPIPE_FORMAT_AUTO 0
#define OCTPIPE_FORMAT_UINT12_PACKED 1
#define OCTPIPE_FORMAT_INT12_PACKED 2
#define OCTPIPE_FORMAT_INT8 3
#define OCTPIPE_FORMAT_INT16 4
#define OCTPIPE_FORMAT_INT32 5
/* octpipe_create with an explicit sample format (fixed for the life of the handle: it sets the size
 * of the ring slots that are pinned here) */
int octpipe_create_with_format(octpipe_t** out, int device, const OctPipeAcquisitionParams* acq,
                               const OctPipeParams* params, void* h_buffer1, void* h_buffer2, int sampleFormat);
/* bytes of one raw acquisition buffer in the handle's sample format */
int octpipe_raw_buffer_bytes(const octpipe_t* h, size_t* bytes);
/* cleanupCuda + releaseBuffers + destroyStreamsAndEvents, kernels.h:65-67 / cu:1164-1212 */
int octpipe_destroy(octpipe_t* h);
/* The three HIP streams of a destroyed handle are kept (at most 4 sets per device) and handed to the next handle created on
 * that device, so that a host which opens and closes pipelines repeatedly does not churn the runtime's hardware queues.  This
 * call destroys every idle set now -- e.g. before the host application resets the device.  Sets the runtime no longer
 * recognises (hipStreamQuery fails) are never handed out. */
int octpipe_release_idle_streams(void);
/* The variants of the run-time compiled kernels a handle can reach next are compiled on ONE background thread of the library.  This
 * call stops it: what is still queued is dropped, the compilation under way is waited for (up to ~2 s), nothing is prefetched afterwards
 * (a launch that needs a variant compiles it itself).  The library does the same from an atexit handler; a host should call it BEFORE it
 * leaves main() (the Python layer does, from its own atexit hook): compiler libraries construct function-local statics during their first
 * compilation, i.e. AFTER the library's handler was registered -- at process exit those are destroyed first, under a compilation that is
 * still running.  Idempotent, callable from any thread but a callback. */
int octpipe_shutdown(void);
/* A-scan lengths without a dedicated kernel get a kernel compiled FOR the length at run time (0.5-1.2 s per variant, once per
 * process and device).  By default nothing is written to disk.  With a directory set here the compiled code
 * objects are also kept there -- one file per (kernel sources, options, architecture, plan, variant), written atomically,
 * a few tens of KiB each -- and the next process loads them instead of compiling.  NULL or "" switches the directory off
 * again.  Process-wide; the directory must exist.  (No reference counterpart: cufftPlan1d keeps its plans in memory.) */
int octpipe_set_kernel_cache_dir(const char* directory);
/* parameter snapshot taken per call in the reference (params-> reads in cu:1409-1604) */
int octpipe_set_params(octpipe_t* h, const OctPipeParams* params);
int octpipe_get_acquisition_params(const octpipe_t* h, OctPipeAcquisitionParams* out);

/* cuda_updateResampleCurve cu:969, cuda_updateDispersionCurve cu:636 (+ fillDispersivePhase
 * cu:624, call cu:1439), cuda_updateWindowCurve cu:641, cuda_updatePostProcessBackground cu:646,
 * cuda_copyPostProcessBackgroundToHost cu:652.  Device LUTs are zero until first update (cu:1082-1085). */
int octpipe_update_resample_curve(octpipe_t* h, const float* curve, int size);
int octpipe_update_dispersion_curve(octpipe_t* h, const float* curve, int size);
int octpipe_update_window_curve(octpipe_t* h, const float* curve, int size);
int octpipe_update_postprocess_background(octpipe_t* h, const float* background, int size);
int octpipe_copy_postprocess_background_to_host(octpipe_t* h, float* background, int size);
/* The host shadow of the recorded background.  The pipeline copies the device line into it in-stream BEFORE the
 * onBackgroundRecorded callback fires (the reference copies into params->postProcessBackground in-stream and the callback
 * only signals, cu:652-656), so this accessor makes no HIP call and is the one to use from inside that callback. */
int octpipe_get_postprocess_background_host(const octpipe_t* h, float* background, int size);

/* Calibration blob for multi-GPU: everything a second GPU needs to produce the same output
 * (curves, phasor LUT, mean A-line, post-process background, FPN state).  The host side moves it
 * between ranks (RCCL broadcast); there is no reference counterpart (single GPU, README.md:27). */
size_t octpipe_calibration_size(const octpipe_t* h);
int    octpipe_export_calibration(octpipe_t* h, void* blob, size_t size);
int    octpipe_import_calibration(octpipe_t* h, const void* blob, size_t size);

/* ------------------------------------------------------------------ processing */
/* octCudaPipeline(h_inputSignal), kernels.h:64 / cu:1389-1605.  Returns once the H2D copy of the
 * raw buffer has completed (the reference's event wait cu:1418-1419), so the caller may hand the
 * ring slot back (processing.cpp:191); the rest of the chain is merely enqueued. */
int octpipe_process(octpipe_t* h, const void* h_inputSignal);
/* The two halves of octpipe_process: enqueue everything (H2D on the copy stream + the chain) without blocking, and wait
 * until the H2D copy of the last enqueued buffer has completed.  A caller that drives several handles (one per GPU,
 * octpipe_group_process) enqueues on all of them before it waits on any. */
int octpipe_process_async(octpipe_t* h, const void* h_inputSignal);
int octpipe_wait_input(octpipe_t* h);
/* Same chain with the raw buffer already resident in HBM (d_raw: device pointer, S*bytesPerSample
 * bytes).  No reference counterpart: it is what the roofline measurement times.  A plain pointer carries no stream ordering:
 * the buffer must be COMPLETE when this is called (or have been written on the stream octpipe_get_stream returns) -- the
 * handle's streams are hipStreamNonBlocking and do not wait for the NULL stream or for another library's streams. */
int octpipe_process_device(octpipe_t* h, const void* d_raw);
int octpipe_synchronize(octpipe_t* h);

/* Device pointer to the processed volume (d_processedBuffer, cu:1118: float32
 * [buffersPerVolume][B][A][N/2]) and the index of the slot the last call wrote (cu:1535).
 * With buffersPerVolume == 1 and float streaming active the pipeline alternates between TWO such buffers, so that the
 * device-to-host copy of buffer k (result stream) overlaps the kernels of buffer k+1 without a race on the volume (the
 * reference lets them race, cu:1396); the pointer returned here is the buffer written last. */
int octpipe_get_processed_device(octpipe_t* h, void** d_processed, size_t* bytes, unsigned* bufferNumberInVolume);
int octpipe_copy_processed_to_host(octpipe_t* h, float* dst, size_t count, size_t offset);
/* the HIP stream the kernels of this handle are enqueued on (as void*), and a way to replace it.  Two more streams belong to
 * the handle: the copy stream (H2D of the raw buffer) and the result stream (quantiser, both D2H copies and the data
 * callbacks, ordered against the compute stream by events: cu:1357-1386 on the rotating streams of cu:1396).
 * Internally a handle may run consecutive octpipe_process_device buffers on a second compute lane as well (csrc/lanes.h).  That is
 * not observable through this interface: every other entry point first orders the compute stream behind the lane, so "enqueued on the
 * compute stream behind what is already there" holds as written, and a handle whose stream has been asked for or replaced here keeps
 * everything on that one stream from then on. */
int octpipe_get_stream(octpipe_t* h, void** stream);
int octpipe_set_stream(octpipe_t* h, void* stream);

/* calibration hooks (no reference counterpart; the multi-GPU group and the tests pin the ill-conditioned FPN stage with them).
 * Test-only entry points (stage outputs, route selection, which kernel ran) live in octpipe_debug.h, not here. */
int octpipe_get_mean_line(octpipe_t* h, float* meanLineComplex /* 2*N floats */);
int octpipe_set_mean_line(octpipe_t* h, const float* meanLineComplex /* 2*N floats */, int pin);
/* run only getMinimumVarianceMean (cu:523-565) on a caller-supplied complex buffer [height][width] */
int octpipe_min_variance_mean(octpipe_t* h, const float* d_or_h_complex, int isDevice, int width, int height, float* meanOutComplex);
/* ------------------------------------------------------------------ result delivery
 * cuda_registerStreamingBuffers / cuda_unregisterStreamingBuffers (kernels.h:69-70, cu:659-675)
 * and the float variants (kernels.h:71-72, cu:677-695): two host buffers, filled alternately
 * starting with the second (cu:1360-1361), each completion announced through the callback. */
int octpipe_register_streaming_buffers(octpipe_t* h, void* h_buf1, void* h_buf2, size_t bytesPerBuffer);
int octpipe_unregister_streaming_buffers(octpipe_t* h);
int octpipe_register_float_streaming_buffers(octpipe_t* h, void* h_buf1, void* h_buf2, size_t bytesPerBuffer);
int octpipe_unregister_float_streaming_buffers(octpipe_t* h);
int octpipe_set_callbacks(octpipe_t* h, octpipe_data_callback onStreamingData,
                          octpipe_data_callback onFloatStreamingData,
                          octpipe_event_callback onBackgroundRecorded, void* user);

/* ------------------------------------------------------------------ display frames
 * changeDisplayedBscanFrame / changeDisplayedEnFaceFrame (kernels.h:81-82, cu:1223-1265) write
 * into plain device buffers owned by the handle (A*N/2 resp. A*B*buffersPerVolume floats);
 * cuda_registerGlBuffer{Bscan,EnFaceView,VolumeView} (kernels.h:73-75) have no meaning on a
 * headless MI355X node and always report failure. */
int octpipe_change_displayed_bscan_frame(octpipe_t* h, unsigned frameNr, unsigned displayFunctionFrames, int displayFunction);
int octpipe_change_displayed_enface_frame(octpipe_t* h, unsigned frameNr, unsigned displayFunctionFrames, int displayFunction);
int octpipe_get_display_buffers(octpipe_t* h, void** d_bscanFrame, size_t* bscanCount, void** d_enFaceFrame, size_t* enFaceCount);
/* updateVolumeDisplayBuffer / updateDisplayedVolume (cu:914-941, cu:1310-1355) into a plain device buffer instead of a GL
 * 3-D texture: uint8 voxels [N/2][B*buffersPerVolume][A] (x = A-scan fastest, then B-scan in the volume, then depth with
 * depth reversed, exactly the texel the reference writes: surf3Dwrite(v, y = A-scan, x = B-scan, z = N/2-1-depth)),
 * voxel = (unsigned char)(value * 255.0) for values in [0, 1]; values outside are clamped to 0 / 255 (undefined cast in the
 * reference).  Written for every buffer while params.volumeViewEnabled is set; the buffer is allocated on first use. */
int octpipe_get_volume_view_buffer(octpipe_t* h, void** d_voxels, size_t* bytes);
int octpipe_register_gl_buffer_bscan(unsigned buf);       /* always OCTPIPE_ERR_UNSUPPORTED */
int octpipe_register_gl_buffer_enface_view(unsigned buf); /* always OCTPIPE_ERR_UNSUPPORTED */
int octpipe_register_gl_buffer_volume_view(unsigned buf); /* always OCTPIPE_ERR_UNSUPPORTED */

/* ------------------------------------------------------------------ multi-GPU group (no reference counterpart: the
 * reference is single-GPU, README.md:27).  One host process, one acquisition buffer per call, n GPUs: the buffer's B-scans are
 * cut into contiguous even-sized slabs (the buffer-local flip rule cu:795 keeps its parity), member i processes slab i on
 * devices[i], no sample data crosses GPUs.  Member 0 determines calibration data (fixed-pattern-noise mean line cu:1518-1525,
 * recorded background cu:1557-1561) on the buffer's first B-scans; the blob reaches the other members through ONE
 * ncclBroadcast (RCCL over xGMI, bound with dlopen at group creation) when all devices are distinct, through plain copies
 * when members share a device.  Result: identical, bit for bit, to one handle processing the whole buffer, for every setting
 * that works per A-scan (not: sinusoidal correction, Lanczos taps, bscansForNoiseDetermination beyond slab 0).
 * The call shape mirrors the single-handle API so that Processing::slot_start (processing.cpp:176-218) only swaps the handle. */
typedef struct octpipe_group octpipe_group_t;
int octpipe_group_create(octpipe_group_t** out, const int* devices, int n, const OctPipeAcquisitionParams* acqWholeBuffer,
                         const OctPipeParams* params, void* h_buffer1, void* h_buffer2);          /* initializeCuda */
/* The same with options.  octpipe_group_create == flags 0: the caller's thread submits to every member, and NO change to the
 * caller's memory policy.
 *   OCTPIPE_GROUP_PLACE_RING_SLABS  move the pages of every member's slab of the two ring slots to the NUMA node of that member's
 *                                   GPU before pinning them (mbind MPOL_PREFERRED | MPOL_MF_MOVE on the caller's buffers, best
 *                                   effort; octpipe_group_info reports how many slabs could be placed).  A side effect on memory
 *                                   the caller owns, hence opt-in.
 *   OCTPIPE_GROUP_SUBMIT_THREADS    one submitting host thread per member (see octpipe_group_set_submit_threads)
 *   OCTPIPE_GROUP_NO_SUBMIT_THREADS the default spelled out: the caller's thread submits to every member
 * On failure *out is NULL and everything the call had allocated (member handles, communicators, staging buffers, pinning of
 * the ring slots) has been released again; octpipe_group_last_error() names the step and the member that failed. */
enum { OCTPIPE_GROUP_PLACE_RING_SLABS = 1, OCTPIPE_GROUP_NO_SUBMIT_THREADS = 2, OCTPIPE_GROUP_SUBMIT_THREADS = 4 };
int octpipe_group_create_ex(octpipe_group_t** out, const int* devices, int n, const OctPipeAcquisitionParams* acqWholeBuffer,
                            const OctPipeParams* params, void* h_buffer1, void* h_buffer2, unsigned flags);
int octpipe_group_destroy(octpipe_group_t* g);                                                     /* cleanupCuda */
int octpipe_group_size(const octpipe_group_t* g);
octpipe_t* octpipe_group_member(octpipe_group_t* g, int i);   /* NULL for a member without B-scans */
int octpipe_group_slab(const octpipe_group_t* g, int i, unsigned* firstBscan, unsigned* bscanCount);
/* One submitting host thread per member (persistent, asleep between buffers), so that the n enqueue sequences of a call run
 * side by side instead of one after the other: ~0.1 ms of host work per member and buffer, which at 8 members is more than a
 * 32 MiB slab copy takes over a member's own PCIe link.  OPT-IN (OCTPIPE_GROUP_SUBMIT_THREADS or this call): the default is the
 * caller's thread.  A caller-owned host buffer that is NOT one of the two
 * registered ring slots (h_buffer1 / h_buffer2 of the creation call, pinned there) is submitted member after member by the
 * caller's thread instead: the threads only ever start DMA transfers out of pinned memory, never concurrent on-the-fly pinning
 * or staging of pageable memory (octpipe_group_serial_submit_count counts such calls).
 * octpipe_group_info reports the thread count (0 = the caller's thread submits) and how many member slabs of the ring slots
 * were moved to the NUMA node of their GPU (only with OCTPIPE_GROUP_PLACE_RING_SLABS; 0 on single-node hosts or where the
 * container forbids mbind). */
int octpipe_group_set_submit_threads(octpipe_group_t* g, int enable);
int octpipe_group_info(const octpipe_group_t* g, int* submitThreads, int* slabsPlacedOnGpuNode);
uint64_t octpipe_group_serial_submit_count(const octpipe_group_t* g);
const char* octpipe_group_backend(const octpipe_group_t* g);   /* "rccl" or "copy" */
uint64_t octpipe_group_broadcast_count(const octpipe_group_t* g);
const char* octpipe_group_last_error(void);
int octpipe_group_set_params(octpipe_group_t* g, const OctPipeParams* params);
int octpipe_group_update_resample_curve(octpipe_group_t* g, const float* curve, int size);
int octpipe_group_update_dispersion_curve(octpipe_group_t* g, const float* curve, int size);
int octpipe_group_update_window_curve(octpipe_group_t* g, const float* curve, int size);
int octpipe_group_update_postprocess_background(octpipe_group_t* g, const float* background, int size);
int octpipe_group_set_mean_line(octpipe_group_t* g, const float* meanLineComplex, int pin);
int octpipe_group_process(octpipe_group_t* g, const void* h_inputSignal);          /* octCudaPipeline: whole buffer in host memory */
int octpipe_group_process_device(octpipe_group_t* g, const void* const* d_slabs);  /* slab i resident on devices[i] */
int octpipe_group_broadcast_calibration(octpipe_group_t* g);
int octpipe_group_synchronize(octpipe_group_t* g);
int octpipe_group_copy_processed_to_host(octpipe_group_t* g, float* dst /* S/2 floats, slabs back to back */);

/* ------------------------------------------------------------------ dispersion estimation
 * What the Dispersion Estimator extension of the reference does (docs/docs/plugin-dispersionestimator.md; the chain it repeats is
 * processing.md:80-109): process M A-scans of one grabbed raw buffer once per candidate dispersion coefficient pair (d2, d3), reduce
 * every processed A-scan to an image metric, keep the candidate with the best mean.  Candidate c uses the phasor e^{i theta} with
 * theta = octpipe_dispersion_curve(d0, d1, d2[c], d3[c], N) (octalgorithmparameters.cpp:206-222, fillDispersivePhase cu:624-634).
 *
 * Value of depth bin k of an A-scan: the number the product itself would write into the processed volume under the handle's current
 * unpack, rolling average, resampling curve / interpolation, window and grey-value settings, with that phasor applied (also when
 * params.dispersionCompensation is 0), fixed-pattern-noise removal, post-process background, B-scan flip and sinusoidal
 * correction off, and signalLogScaling = !linear.  Metric of an A-scan over the bins k in [ignoreFirstSamples, N/2):
 *   SUM_ABOVE_THRESHOLD      sum of v[k] over v[k] > threshold
 *   SAMPLES_ABOVE_THRESHOLD  count of v[k] > threshold
 *   PEAK_VALUE               max v[k]
 *   MEAN_SOBEL               sum of |v[k+1] - v[k-1]| over k in [ignoreFirstSamples+1, N/2-2] (1-D axial Sobel derivative; this
 *                            library's definition, the extension's source is not published)
 * score[c] = mean of the M per-A-scan metrics.  Deterministic: two identical calls return the same bits, whatever the number of
 * candidates per call.  Only A-scans firstAscan-1 .. firstAscan+M of `raw` are read (the Lanczos taps reach the neighbours; the
 * first-line quirk of cu:313 holds as in the whole buffer).
 *
 * The calls are enqueued on the handle's compute stream behind everything already enqueued there and return once the scores are on
 * the host.  They change nothing the processing chain reads or writes (curves, LUTs, mean line, one-shot flags, processed / display /
 * volume buffers, kernel timing); their scratch belongs to the handle.  samplesPerLine = 256, 512, 1024, 2048 and 4096 only, every
 * other length returns OCTPIPE_ERR_UNSUPPORTED.  Inside a callback: OCTPIPE_ERR_IN_CALLBACK. */
enum { OCTPIPE_METRIC_SUM_ABOVE_THRESHOLD = 0, OCTPIPE_METRIC_SAMPLES_ABOVE_THRESHOLD = 1,
       OCTPIPE_METRIC_PEAK_VALUE = 2, OCTPIPE_METRIC_MEAN_SOBEL = 3 };
typedef struct OctPipeDispersionMetric {
	uint32_t firstAscan;          /* buffer-local index of the first A-scan used */
	uint32_t ascanCount;          /* M >= 1, firstAscan + M <= A*B */
	uint32_t ignoreFirstSamples;  /* depth bins [0, ignore) are not scored; ignore < N/2 - 2 */
	int32_t  linear;              /* 1: linear values (cu:723-741 form), 0: log values (cu:699-721 form) */
	int32_t  metric;              /* OCTPIPE_METRIC_* */
	float    threshold;           /* the two *_ABOVE_THRESHOLD metrics only */
	float    d0, d1;              /* held fixed for every candidate */
} OctPipeDispersionMetric;
/* score[c] for K arbitrary candidates (d2[c], d3[c]); raw = one whole raw buffer in the handle's layout and sample format
 * (octpipe_raw_buffer_bytes), in host (rawIsDevice = 0) or device memory */
int octpipe_dispersion_scores(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m,
                              const float* d2, const float* d3, unsigned candidates, float* scores);
/* The extension's two-step search: d2 over [d2Start, d2End] with d3 = 0, then d3 over [d3Start, d3End] with the best d2.  Candidate i
 * of a range is (float)(start + (end - start) * (double)i / (samples - 1)) (start alone for samples == 1); the best is the first
 * maximum, a NaN score never wins, all-NaN scores return OCTPIPE_ERR_INVALID_ARGUMENT.  d2Scores / d3Scores: `samples` floats each
 * or NULL. */
int octpipe_estimate_dispersion(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m,
                                float d2Start, float d2End, float d3Start, float d3End, unsigned samples,
                                float* d2Scores, float* d3Scores, float* bestD2, float* bestD3);

/* ------------------------------------------------------------------ phase extraction / k-linearisation calibration
 * What the Phase Extraction Extension of the reference does (docs/docs/plugin-phaseextraction.md): average the raw spectra of a
 * calibration signal, isolate its peak in depth, unwrap the phase of that band and invert it into the resampling curve that makes
 * the signal linear in k.  The extension's source is not published; the steps below are this library's definition.
 *
 * 1. octpipe_phase_accumulate reads A-scans firstAscan .. firstAscan+ascanCount-1 of one raw buffer in the handle's layout and sample
 *    format (octpipe_raw_buffer_bytes), in host (rawIsDevice = 0) or device memory; only those rows are read, and only they are
 *    copied from host memory.  Each sample is decoded to the integer the processing chain converts to float: every format, with the
 *    >> 4 of the bitshift in force at the call.  The exception is uint32 (AUTO, bitDepth > 16) under bitshift, which the chain
 *    decodes as v * 2^-32: there the integer is v and scale = 2^-32 is applied by the mean (the bitshift in force at that call).
 *    The integers are added exactly into a per-handle int64[N] accumulator, and the handle keeps the A-scan count: any split of the
 *    A-scans over calls gives the same bits.  A call that would take the count to 2^31 returns OCTPIPE_ERR_INVALID_ARGUMENT, so does
 *    ascanCount = 0 or firstAscan + ascanCount > A*B.  octpipe_phase_reset clears the accumulator.  Every samplesPerLine.
 * 2. octpipe_phase_mean: mean[n] = (float)(((double)S[n] / (double)count) * scale); a count of 0 returns OCTPIPE_ERR_INVALID_ARGUMENT.
 * 3. octpipe_extract_resample_curve (samplesPerLine = 256, 512, 1024, 2048, 4096; otherwise OCTPIPE_ERR_UNSUPPORTED), with
 *    x(n) = mean[n] - (1/N) sum mean (mean: N floats, all finite, or NULL for the accumulated mean), a = ignoreFirst, b = N-1-ignoreLast:
 *      windowRaw: x(n) *= 0.5 - 0.5 cos(2 pi n / (N-1));
 *      X[k] = sum_n x(n) e^{-2 pi i k n / N}; spectrum[k] = |X[k]|, k < N/2 (the depth bins of the processed A-scan);
 *      w(k) = 0.5 - 0.5 cos(2 pi (k-s) / (e-s)) on [s, e] with hannPeak, 1 on [s, e] without, 0 elsewhere (negative bins included);
 *      z(n) = (1/N) sum_k w(k) X[k] e^{+2 pi i k n / N}; envelope[n] = |z(n)|, wrapped phase pw(n) = atan2(Im z, Re z);
 *      J(n) = -1 if pw(n) - pw(n-1) > pi, +1 if < -pi, else 0; K(n) = sum_{m <= n} J(m);
 *      phase[n] = phi(n) = pw(n) - pw(a) + 2 pi (K(n) - K(a)) (float64 on the device);
 *      psi(n) = a + phi(n) (b - a) / phi(b) (phi(b) zero or not finite: OCTPIPE_ERR_INVALID_ARGUMENT, no calibration signal in the band);
 *      monotone from the anchor: n >= a: max of psi over [a, n]; n < a: min of psi over [n, a];
 *      curve[j] = 0 if j < psi(0), N-1 if j >= psi(N-1), else n* + (j - psi(n*)) / (psi(n*+1) - psi(n*)) with n* the largest n <= N-2
 *      where psi(n) <= j;
 *      coeffs: least squares (host, float64) of curve[j], j in [a, b], on {1, t, t^2, t^3}, t = j/(N-1) -- the parametrisation of
 *      octpipe_resample_curve, so they can go straight into params.c0..c3.  spectrum (N/2), envelope, phase (N) and coeffs (4) may be
 *      NULL.  Bitwise deterministic.
 * 4. The calls run on the handle's compute stream behind what is already enqueued there and return once their results are on the
 *    host.  They change nothing the processing chain reads or writes (curves, LUT, mean line, one-shot flags, processed / display
 *    buffers, kernel timing).  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.  Bad bands, ranges or pointers return
 *    OCTPIPE_ERR_INVALID_ARGUMENT naming the field.  octpipe_destroy frees the accumulator. */
typedef struct OctPipePhaseExtraction {
	uint32_t peakStart;    /* first bin of the calibration peak, 2 <= peakStart */
	uint32_t peakEnd;      /* last bin, inclusive: peakStart + 2 <= peakEnd <= N/2 - 1 */
	int32_t  windowRaw;    /* 1: Hann over the whole averaged interferogram before the forward transform */
	int32_t  hannPeak;     /* 1: Hann over [peakStart, peakEnd]; 0: rectangular */
	uint32_t ignoreFirst;  /* anchors and fit range: j in [a, b], a = ignoreFirst, b = N-1-ignoreLast, b - a >= 8 */
	uint32_t ignoreLast;
} OctPipePhaseExtraction;  /* 24 bytes */
int octpipe_phase_reset(octpipe_t* h);
int octpipe_phase_accumulate(octpipe_t* h, const void* raw, int rawIsDevice, uint32_t firstAscan, uint32_t ascanCount);
int octpipe_phase_mean(octpipe_t* h, float* mean /* N */, uint64_t* ascans /* may be NULL */);
int octpipe_extract_resample_curve(octpipe_t* h, const float* mean /* N floats; NULL: the accumulated mean */,
                                   const OctPipePhaseExtraction* x,
                                   float* spectrum /* N/2 or NULL */, float* envelope /* N or NULL */,
                                   float* phase /* N or NULL */, float* curve /* N */, float* coeffs /* 4 or NULL */);

/* ------------------------------------------------------------------ image statistics
 * What the Image Statistics extension of the reference shows during an acquisition (docs/docs/plugin-imagestatistics.md): a live
 * histogram of processed or raw data inside a region of interest.  The extension's source is not published; this is the definition.
 *
 * Region: element (b, a, s) for b in [firstBscan, +bscanCount), a in [firstAscan, +ascanCount), s in [firstSample, +sampleCount);
 * buffer-local A-scan index b*A + a, as the stored layout has it (a flipped B-scan is stored flipped).  Sources:
 *   processed, data = NULL: the float32 volume octpipe_get_processed_device returns at the time of the call, slot `buffer`
 *     (0xFFFFFFFF: the slot the last process call wrote; with buffersPerVolume = 1 and float streaming on, the one of the two
 *     buffers the last call wrote); s in [0, N/2);
 *   processed, data set: one buffer [B][A][N/2] of the caller's floats, host (dataIsDevice = 0) or device memory; buffer must be 0 or
 *     0xFFFFFFFF;
 *   raw: one raw buffer in the handle's layout and sample format (octpipe_raw_buffer_bytes), host or device; s in [0, N).
 * A host source is staged in bounded chunks; only the region's A-scans travel.  Every samplesPerLine the handle accepts.
 *
 * Processed values: NaN and +-inf count in nonFinite and nowhere else.  Every finite value enters count, min, max, mean and stddev,
 * whatever the histogram range.  Histogram: scale = (float)((double)bins / ((double)hi - (double)lo)) (clamped to FLT_MAX); v < lo
 * goes to underflow, v > hi to overflow, otherwise to bin min((int)floorf(t), bins - 1), t = (v - lo) * scale, the sub and the mul
 * each rounded to float32 (no v*scale - lo*scale): v == hi lands in the last bin, as in numpy's histogram.  autoRange: lo / hi =
 * min / max of the region's finite values, found on the device; lo == hi gives scale = 0 (every finite value in bin 0); no finite
 * value gives lo = hi = NaN and an all-zero histogram.
 * Raw values: x = the integer decode_sample hands over (the bitshift in force applied in every format but unsigned 32 bit, which is
 * the stored value): the integer octpipe_phase_accumulate sums.  x < lo goes to underflow; otherwise b = (x - lo) / binWidth in
 * 64-bit integers, b >= bins goes to overflow.  autoRange: lo = min, binWidth = max(1, ceil((max - min + 1) / bins)).  out->hi =
 * lo + bins * binWidth, nonFinite = 0.  (12-bit data, bins = 4096, lo = 0, binWidth = 1: one bin per code, the top code's count is
 * the saturation count.)
 * Moments in float64 (stddev: population standard deviation), in an order fixed by the region's shape alone: the same values give
 * the same bits from host or device memory and on any device.  Histogram counts are exact.
 * Limits: 1 <= bins <= 4096; without autoRange lo < hi, both finite (processed), binWidth >= 1 (raw); a non-empty region inside the
 * buffer.  Otherwise OCTPIPE_ERR_INVALID_ARGUMENT naming the field.
 * The work is enqueued on the compute stream behind what is already there; the calls return once the results are on the host.  They
 * change nothing the processing chain reads or writes (curves, LUTs, mean line, one-shot flags, processed / display / volume
 * buffers, kernel timing).  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.  The scratch belongs to the handle (freed in
 * octpipe_destroy). */
typedef struct OctPipeStatsRegion {   /* 7 x uint32 = 28 bytes */
	uint32_t buffer;        /* processed source only: slot in the volume; 0xFFFFFFFF = the slot the last process call wrote */
	uint32_t firstBscan, bscanCount;   /* B-scans of the buffer */
	uint32_t firstAscan, ascanCount;   /* A-scans within each of those B-scans */
	uint32_t firstSample, sampleCount; /* depth bins [0, N/2) for processed data, raw samples [0, N) for raw data */
} OctPipeStatsRegion;

typedef struct OctPipeImageStatistics {  /* 11 x 8 = 88 bytes */
	uint64_t count;       /* values that enter the moments: finite values (processed), every sample (raw) */
	uint64_t underflow, overflow, nonFinite;
	double   min, max, mean, stddev;  /* over `count` values; stddev = population standard deviation; all NaN when count = 0 */
	double   lo, hi, binWidth;        /* the range the histogram used (after autoRange); processed binWidth = (hi - lo) / bins */
} OctPipeImageStatistics;

int octpipe_processed_statistics(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                                 const OctPipeStatsRegion* r, unsigned bins, int autoRange, float lo, float hi,
                                 uint64_t* histogram /* bins, or NULL */, OctPipeImageStatistics* out);
int octpipe_raw_statistics(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeStatsRegion* r,
                           unsigned bins, int autoRange, int64_t lo, uint32_t binWidth,
                           uint64_t* histogram /* bins, or NULL */, OctPipeImageStatistics* out);

/* ------------------------------------------------------------------ peak analysis
 * What the Peak Detector and Axial PSF Analyzer extensions of the reference report (docs/docs/plugin-peakdetector.md,
 * plugin-axialpsfanalyzer.md): the A-scans of a region averaged into one A-scan, the depth of its highest value, its width at half
 * maximum and a Gaussian fit -- batched over groups of A-scans.  The extensions' source is not published; this is the definition.
 *
 * Region and source: those of octpipe_processed_statistics (the same OctPipeStatsRegion; data = NULL: the handle's processed volume,
 * slot `buffer`, 0xFFFFFFFF = the slot the last process call wrote; otherwise one caller buffer [B][A][N/2] of float32 in host or
 * device memory; the stored layout, a flipped B-scan is stored flipped).  Depth positions in the results are absolute depth bins.
 * Groups: G = ascansPerGroup >= 1 divides ascanCount.  Group q = b * (ascanCount / G) + j covers A-scans firstAscan + jG ..
 *   firstAscan + jG + G - 1 of B-scan firstBscan + b; Q = bscanCount * ascanCount / G groups.  G = ascanCount: one averaged A-scan per
 *   B-scan (the extensions); G = 1: one result per A-scan (a surface map).
 * Averaged A-scan m[s], s in the window [s0, s1] = [firstSample, firstSample + sampleCount - 1]: the group is cut into chunks of 64
 *   consecutive A-scans (the last may be shorter); a chunk partial is the float64 sum of its values added one after another in A-scan
 *   order (starting from the first value); T = the float64 sum of the partials in chunk order (starting from the first partial);
 *   m = (float)(T / G), one float64 division and one rounding.  For G <= 64 that is the plain sequential float64 sum.  NaN and inf
 *   propagate as in IEEE arithmetic.
 * Analysis of one averaged A-scan, float64 on the float32 values:
 *   1. a non-finite m[s] in the window: NONFINITE, every other field NaN (integers 0).  Stop.
 *   2. k = the smallest s where m reaches its maximum, value = m[k].  !(value > threshold): NO_PEAK, index and value reported, the
 *      rest NaN.  Stop.
 *   3. position = k + (0.5 (m[k-1] - m[k+1])) / d if s0 < k < s1 and d = (m[k-1] - 2 m[k]) + m[k+1] < 0; otherwise k.
 *   4. half-maximum width against zero (defined when value > 0, otherwise WIDTH_UNDEFINED and left / right / fwhm NaN): half =
 *      0.5 value; l = k, while l > s0 and m[l-1] > half: l -= 1; left = l - (m[l] - half) / (m[l] - m[l-1]) if l > s0, else s0 and
 *      LEFT_OPEN.  r = k, while r < s1 and m[r+1] > half: r += 1; right = r + (m[r] - half) / (m[r] - m[r+1]) if r < s1, else s1 and
 *      RIGHT_OPEN.  fwhm = right - left.
 *   5. Gaussian fit (fitGaussian != 0): f(z) = A exp(-(z - mu)^2 / (2 sigma^2)) + c over the window [max(s0, k - w), min(s1, k + w)],
 *      w = fitHalfWidth if non-zero, else min(256, max(4, ceil(1.5 fwhm))) with the width defined, else 16.  Fewer than 5 samples:
 *      FIT_SKIPPED.  Start: c0 = min of m over the fit window, A0 = value - c0, mu0 = position, sigma0 = max(0.5, fwhm / (2 sqrt(2 ln 2)))
 *      (1 with the width undefined).  Levenberg-Marquardt: r = m - f, C = sum r^2, H = J^T J, g = J^T r; (H + lambda diag(H)) delta = g
 *      solved by Gaussian elimination with partial pivoting, lambda0 = 1e-3; C(p + delta) < C(p) accepts (lambda = max(lambda / 10,
 *      1e-15)), otherwise rejects (lambda *= 10); a zero or non-finite pivot rejects.  FIT_CONVERGED after an accepted step with
 *      C(p) - C(p') <= 1e-12 C(p) or max_i |delta_i| / (|p_i| + 1e-12) <= 1e-10, or at once when C = 0; FIT_STALLED when lambda > 1e15;
 *      FIT_MAX_ITER after maxIterations solves (0: 100; at most 1000).  Reported, from the last accepted parameters: amplitude, center,
 *      sigma = |sigma|, offset, fitFwhm = 2 sqrt(2 ln 2) sigma, rms = sqrt(C / n), the window (fitFirst, fitCount), the solves done.
 *      Fit off: the fit fields NaN, no FIT_* bit, fitFirst = fitCount = iterations = 0.
 * Every output is a function of the values and the region's shape alone: the same values give the same bits from host or device
 * memory, from another slot, in a repeated call.  Steps 1 to 4 are float64 adds and one division each, in a fixed order, multiplied
 * only by 0.5 and 2: the averaged A-scan, index, value, position, left, right, fwhm and the bits of steps 1 to 4 are exact against a
 * float64 restatement.  The fit's sums are reduced in a fixed order too; against another implementation they agree to rounding.
 * A Gaussian FWHM is meaningful on linearly scaled values (signalLogScaling = 0); the call analyses whatever values are stored.
 * Limits: 3 <= sampleCount <= 4096 (a longer window: OCTPIPE_ERR_UNSUPPORTED); threshold not NaN (-inf is allowed); maxIterations
 * <= 1000; a non-empty region inside the buffer.  Otherwise OCTPIPE_ERR_INVALID_ARGUMENT naming the field.
 * The work is enqueued on the compute stream behind what is already there; the call returns once the results are on the host.  It
 * changes nothing the processing chain reads or writes.  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.  The scratch belongs to the
 * handle (freed in octpipe_destroy). */
enum {
	OCTPIPE_PEAK_NO_PEAK = 1u << 0,
	OCTPIPE_PEAK_NONFINITE = 1u << 1,
	OCTPIPE_PEAK_WIDTH_UNDEFINED = 1u << 2,
	OCTPIPE_PEAK_LEFT_OPEN = 1u << 3,
	OCTPIPE_PEAK_RIGHT_OPEN = 1u << 4,
	OCTPIPE_PEAK_FIT_CONVERGED = 1u << 8,
	OCTPIPE_PEAK_FIT_MAX_ITER = 1u << 9,
	OCTPIPE_PEAK_FIT_STALLED = 1u << 10,
	OCTPIPE_PEAK_FIT_SKIPPED = 1u << 11
};

typedef struct OctPipePeakSettings {  /* 5 x 4 = 20 bytes */
	uint32_t ascansPerGroup;  /* G >= 1, divides ascanCount */
	float    threshold;       /* minimum value of a peak (NaN: invalid; -inf: every finite maximum) */
	int32_t  fitGaussian;     /* != 0: step 5 */
	uint32_t fitHalfWidth;    /* 0: from the half-maximum width */
	uint32_t maxIterations;   /* 0: 100; at most 1000 */
} OctPipePeakSettings;

typedef struct OctPipePeak {  /* 6 x 4 + 10 x 8 = 104 bytes */
	uint32_t status;          /* OCTPIPE_PEAK_* bits */
	uint32_t index;           /* k, absolute depth bin */
	float    value;           /* m[k] */
	uint32_t fitFirst, fitCount, iterations;      /* the fit window and the solves done */
	double   position, left, right, fwhm;         /* steps 3 and 4, absolute depth bins */
	double   amplitude, center, sigma, offset;    /* step 5: A, mu, |sigma|, c */
	double   fitFwhm, rms;                        /* 2 sqrt(2 ln 2) sigma, sqrt(C / n) */
} OctPipePeak;

int octpipe_peak_analysis(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                          const OctPipeStatsRegion* r, const OctPipePeakSettings* s,
                          OctPipePeak* peaks /* Q */, float* averaged /* Q x sampleCount, or NULL */);

/* ------------------------------------------------------------------ volume rendering
 * The reference's third output window (docs/docs/visualization.md; src/glwindow3d.cpp, src/raycastvolume.cpp and the fragment shaders
 * under octproz/shaders/) as one call: the handle's 8-bit volume view buffer (octpipe_get_volume_view_buffer), or a uint8 volume of the
 * caller's, ray-cast into an RGBA image in a device buffer the handle owns.  The reference holds no test vectors for it and its shaders
 * need a GL context: parity is unpinned, and THIS COMMENT IS THE DEFINITION.  tests/render_model.py restates it in
 * numpy, csrc/volume_render.h implements it.  All arithmetic below is float32 unless it says "host" (double on the host, rounded once).
 *
 * Voxels.  `voxels` is [dims[2]][dims[1]][dims[0]] uint8, dims = (x, y, z), x fastest.  voxels = NULL is the handle's volume view buffer
 * [N/2][B*buffersPerVolume][A]: dims = (A, B*buffersPerVolume, N/2), i.e. the A-scan index runs along the box's x axis, the B-scan index
 * along y and the depth along z (raycastvolume.cpp:227-229 called with width = N/2, height = A, depth = B*buffersPerVolume,
 * glwindow3d.cpp:467-478 / octprozmainwindow.cpp:61-67, 801-804: size = (height, depth, width)).
 *
 * Per pixel (px, py), 0 <= px < width, 0 <= py < height, row 0 at the BOTTOM of the picture (image[py][px][4]):
 * 1. Camera (glwindow3d.cpp:293-311, every shader's main()).  f = focal length = 1 / tan(fovDegrees / 2) (host), aspect = width / height
 *    (host).  c = ((2 (px + 0.5) / width - 1) aspect, 2 (py + 0.5) / height - 1, -f).  With V = viewMatrix (row-major, V[r][c]) the ray
 *    direction is d[j] = (c[0] V[0][j] + c[1] V[1][j]) + c[2] V[2][j], every product rounded on its own (the row vector (c, 0) times
 *    V), and the ray origin is o = -R^-1 t (host; R = the upper left 3 x 3 of V, t = its fourth column: the fourth column of V^-1).
 *    Box (raycastvolume.cpp:192-220): e[i] = dims[i] stretch[i], extent[i] = e[i] / max(e), top = extent / 2, bottom = -top.
 *    Slab test, per axis with inv = 1 / d[i]: a = inv (top[i] - o[i]), b = inv (bottom[i] - o[i]); t_0 = max(0, largest of the three
 *    min(a, b)), t_1 = smallest of the three max(a, b); min and max return the other operand when one is NaN.  Unless t_1 > t_0 the pixel
 *    is (background, 1) and nothing below happens (the reference rasterises only the cube's faces: such a pixel keeps the clear colour).
 * 2. March.  start = (o + d t_0 - bottom) / (top - bottom), stop likewise with t_1 (texture coordinates, 0 .. 1 per axis); ray = stop -
 *    start, L = |ray| = sqrt(x^2 + y^2 + z^2), stepVector = stepLength ray / L.  K = ceil(L / stepLength), limited to 0 .. 1733 (=
 *    ceil(sqrt(3) / 0.001)): the number of k >= 0 with L - k stepLength > 0.  Sample k sits at p_k = start' + k stepVector and carries the
 *    remaining length r_k = L - k stepLength.  (The shaders keep two running float accumulators; the closed forms make the trip count an
 *    integer known before the loop.)  Jitter: start' = start + stepVector j, j = 0 for jitterSeed = 0, else j = (h >> 24) / 255 with, in
 *    uint32 arithmetic, h = px * 0x9E3779B1 + py * 0x85EBCA77 + jitterSeed * 0xC2B2AE3D; h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12;
 *    h *= 0x297A2D39; h ^= h >> 15.  (The reference reads an unseeded random R8 texture, nearest, one texel per pixel.)
 * 3. Voxel fetch I(p) (GL_LINEAR, GL_CLAMP_TO_EDGE on an R8 texture, with exact weights).  Per axis u = p[i] dims[i] - 0.5, limited to
 *    -1 .. dims[i] (NaN: -1); i0 = floor(u), w = u - i0; the two texels are clamp(i0, 0, dims[i] - 1) and clamp(i0 + 1, 0, dims[i] - 1).
 *    Blend the bytes (as floats) a + w (b - a) along x (four pairs), then along y (two), then along z; I = that blend / 255.  The colour
 *    table (LUT) is fetched the same way in one dimension, per channel, from its `width` RGBA entries; its alpha channel is never used.
 *    pow(x, y) below is 0 for x <= 0, else 2^(y log2 x).  normalize(v) = v / |v|, and (0, 0, 0) for |v| = 0 (GLSL leaves that undefined).
 *    transfer(i): rgb = (i, i, i) (DMIP: i + (1 - i) (0.1, 0, 0.2)), or LUT(i) when lutEnabled; alpha = pow(i, alphaExponent).
 *    normal(p, h) = -normalize(sum of e_n I(p + h e_n)) over the four tetrahedron corners e_n = 0.577350269 (+--, --+, -+-, +++) in this
 *    order.  shade(colour, p; h, Ia, kd, ks) = (Ia + kd max(0, N.Lv)) colour + ks pow(max(0, N.H), 600), Lv = normalize(lightPosition - p),
 *    Vw = -normalize(ray), H = normalize(Lv + Vw), N = normal(p, h).  (The shaders mix texture and camera coordinates here; so does this.)
 * 4. Modes.  A sample "counts" when I > threshold (strictly).
 *    MIP (maximum_intensity_projection.frag): m = 0; for k < K while m < 0.99: a counting sample with I > m sets m = I.  C = transfer(m).
 *    DMIP (depth_mip.frag): as MIP, remembering p_k of the last update (initially start').  C = transfer(m) with its own dark colour;
 *      depth = |p_max - start'| / |stop - start'|; all four channels of C times (1 - depthWeight) + 2 depthWeight (1 - depth).
 *    XRAY (xray.frag): all K samples; m = sqrt(sum / count) over the counting samples, 0 without one.  C = transfer(m).
 *    ALPHA_BLENDING (alpha_blending.frag): C = 0; for k < K while C.a < 0.9, counting samples only: c = transfer(I);
 *      C.rgb = c.a c.rgb + (1 - c.a) C.a C.rgb; C.a = c.a + (1 - c.a) C.a; C.rgb = C.a C.rgb pow(2.25, r_k / L) / 1.75 (the depth cue;
 *      quirk: the colour is multiplied by its alpha every step); then, shadingEnabled, C.rgb = shade(C.rgb, p_k; 0.005, 0.75, 0.5, 1.0)
 *      (quirk: inside the accumulation loop).
 *    MIDA (mida.frag): C = 0, m = 0; for k < K while C.a < 0.9, counting samples with I > m: c = transfer(I); w = 1 - (I - m); m = I;
 *      q = (1 - w C.a) c.a; C.rgb = w C.rgb + q c.rgb; C.a = w C.a + q; then, shadingEnabled, C.rgb = shade(C.rgb, p_k; 0.005, 0.75,
 *      0.35, 0.2) (quirk: inside the loop).
 *    MIP, DMIP, XRAY, ALPHA_BLENDING, MIDA end with C.rgb = C.a C.rgb + (1 - C.a) pow(background, gamma) (per channel; the power on the
 *      host), out = pow(C.rgb, 1 / gamma) (1 / gamma on the host).  shadingEnabled is ignored by MIP, DMIP and XRAY, as their shaders ignore it.
 *    ISOSURFACE (isosurface.frag): out = background unless some k < K counts; at the first, q = p_k - 0.5 stepVector, then
 *      q -= (I(q) > threshold ? 0.25 : -0.25) stepVector, and out = pow(shade(material, q; 0.001, 0.2, 0.7, 1.5), 1 / gamma), where for
 *      smoothFactor = n > 0 the normal is normalize(sum over the (2n + 1)^3 offsets (x, y, z) 0.001, x, y, z = -n .. n, x outermost, of
 *      normal(q + offset, 0.001), divided by their number); the sum starts at zero (the shader leaves it uninitialised).  Always shaded,
 *      never through the LUT: shadingEnabled, lutEnabled, alphaExponent and depthWeight are ignored.
 * 5. Output.  Each of out's three channels limited to 0 .. 1 (NaN: 0), as a normalised framebuffer stores it; alpha = 1.
 *    OCTPIPE_RENDER_RGBA_F32: four floats per pixel.  OCTPIPE_RENDER_RGBA_U8: four bytes, (uint8)(c * 255 + 0.5).
 * 6. OCT Depth (oct_depth.frag over the depth texture of compute_sample_depths.glsl), mode 6, through octpipe_render_oct_depth only: every
 *    sample is coloured by its depth below the detected sample surface.  tests/depth_render_model.py restates this step in numpy,
 *    csrc/volume_depth.h implements it.
 *    Surface map (the pre-pass).  T = 1.5f * threshold, one float product (glwindow3d.cpp:184).  With Z = dims[2], first = (int)(Z -
 *    Z / 32.0f) evaluated in float: s(x, y) is the largest i in 1 .. first with (float)voxel[i][y][x] / 255.0f > T (strictly, float32
 *    on both sides), and 0 when there is none; index 0 and the indices above `first` are never examined.  s is a uint16 per column.
 *    Every column is processed (the reference dispatches X / 16 by Y / 16 groups and so skips the remainder columns).
 *    Depth field.  D(x, y, i) = 1.0f - (float)(s - 1 - i) * (1.0f / (float)Z) for 1 <= i < s, else 0: the surface voxel itself is 0, the
 *    voxel below it (the next smaller index; what the shader calls "above" the surface are the larger indices) is 1, then D falls by
 *    1 / Z per voxel; index 0 and everything above `first` are 0 (the reference leaves those texels of its float volume unwritten, and
 *    reaches the other values by repeated float subtraction; the closed form is the definition here).  D is never stored: Dtex(p) is
 *    the fetch of step 3 applied to D -- the indices and weights of I(p), the blend order x, y, z, no division by 255 -- computed from
 *    the four entries of s under the sample.
 *    March.  Steps 1, 2 and 5 as above, but from the far end: stop' = stop + j stepVector, sample k sits at q_k = stop' - k stepVector,
 *    for all k < K (no early exit).  C = 0, Dold = 1.  Per sample: I = I(q_k), D = Dtex(q_k), dd = |D - Dold|, Dold = D (every sample).
 *    The sample counts when I > threshold and I < 0.9 and D > 0.1 and dd < 1.01f * stepLength (dd guards against the jump of D at the
 *    surface).  A counting sample has c.rgb = (D, D, D), c.a = pow(D, alphaExponent), or with lutEnabled c.rgb = LUT(D - 0.05), c.a =
 *    pow(I, alphaExponent); then C.rgb = c.a c.rgb + (1 - c.a) C.a C.rgb; C.a = c.a + (1 - c.a) C.a; C.rgb = C.rgb / C.a; then,
 *    shadingEnabled, C.rgb = shade(C.rgb, q_k; 0.005, 0.75, 0.5, 1.0) with ray = stop - start (quirk: inside the loop).  The end is that
 *    of the other blending modes: C.rgb = C.a C.rgb + (1 - C.a) pow(background, gamma), out = pow(C.rgb, 1 / gamma).  depthWeight,
 *    smoothFactor and material are ignored.  (The reference's depth_colors.png is not shipped: any table goes through
 *    octpipe_update_render_lut.)
 *
 * Ranges (the reference's control panel, src/controlpanel.cpp:115-163): width, height 1 .. 4096; stretch 0.1 .. 9999; stepLength
 * 0.001 .. 10; threshold, depthWeight 0 .. 1; alphaExponent, gamma 0.1 .. 10; smoothFactor 0 .. 3; fovDegrees in (0, 180) exclusive;
 * background, material 0 .. 1; lightPosition and viewMatrix finite, the matrix's upper left 3 x 3 invertible; dims 1 .. 4096 each.
 * Anything else, NaN included: OCTPIPE_ERR_INVALID_ARGUMENT naming the field.  voxels = NULL on a handle without a volume view buffer
 * (no buffer processed with volumeViewEnabled, octpipe_get_volume_view_buffer never called), or lutEnabled in a mode that reads the LUT
 * before octpipe_update_render_lut: OCTPIPE_ERR_NOT_INITIALIZED.
 *
 * octpipe_render_volume enqueues on the compute stream behind what is already there (a render after octpipe_process_device sees that
 * buffer's voxels without a host synchronise) and returns without waiting for the kernel (host voxels are first copied into a staging
 * buffer of the handle; the call returns once that copy has left the caller's memory).  *d_image stays valid until the next render or
 * octpipe_destroy; octpipe_copy_rendered_to_host copies the last image (`bytes` must equal its size) and waits for it.  Nothing the
 * processing chain reads or writes is touched.  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.
 *
 * octpipe_render_oct_depth is octpipe_render_volume for mode 6 (octpipe_render_modes.h), with the same contract (stream ordering, staging
 * of host voxels, image ownership, octpipe_copy_rendered_to_host, error codes and ranges): it enqueues the surface pre-pass and the ray
 * cast back to back on the compute stream.  settings->mode must be that mode, and octpipe_render_volume keeps refusing it: in both
 * cases OCTPIPE_ERR_INVALID_ARGUMENT naming `mode`.  Besides the image the handle keeps only the surface map, 2 X Y bytes; nothing
 * proportional to the voxel count is allocated.
 * octpipe_volume_surface_map is the pre-pass on its own (surface detection, flattening, en face below the surface): s(x, y) of the
 * volume for depthThreshold = T itself (0 .. 1.5; anything else, NaN included: OCTPIPE_ERR_INVALID_ARGUMENT naming depthThreshold) into
 * `map`, host memory for dims[0] * dims[1] entries, [y][x]; it waits for the result. */
enum {
	OCTPIPE_RENDER_MIP = 0,
	OCTPIPE_RENDER_DMIP = 1,
	OCTPIPE_RENDER_XRAY = 2,
	OCTPIPE_RENDER_ALPHA_BLENDING = 3,
	OCTPIPE_RENDER_MIDA = 4,
	OCTPIPE_RENDER_ISOSURFACE = 5
};
#include "octpipe_render_modes.h"  /* mode 6, taken by octpipe_render_oct_depth alone */
enum {
	OCTPIPE_RENDER_RGBA_F32 = 0,
	OCTPIPE_RENDER_RGBA_U8 = 1
};

typedef struct OctPipeRenderSettings {  /* 42 x 4 = 168 bytes */
	uint32_t mode;             /* OCTPIPE_RENDER_MIP ... _ISOSURFACE (octpipe_render_oct_depth: mode 6, octpipe_render_modes.h) */
	uint32_t width, height;    /* viewport in pixels */
	float    viewMatrix[16];   /* row-major 4 x 4 (octpipe_render_view_matrix) */
	float    fovDegrees;       /* vertical field of view */
	float    stretch[3];       /* spacing of the voxels along x, y, z */
	float    stepLength;
	float    threshold;
	float    depthWeight;
	float    alphaExponent;
	float    gamma;
	int32_t  smoothFactor;
	int32_t  shadingEnabled, lutEnabled;
	float    background[3], material[3], lightPosition[3];
	uint32_t jitterSeed;       /* 0: no jitter */
	uint32_t outputFormat;     /* OCTPIPE_RENDER_RGBA_F32 / _U8 */
} OctPipeRenderSettings;

/* The reference's state after start-up: mode MIP (glwindow3d.cpp:96), 512 x 512, the view matrix of the identity rotation at viewPos
 * (0, 0), distExp -500 (glwindow3d.h:236), fov 50 (glwindow3d.h:206), stretch 1, 1, 1 (raycastvolume.cpp:99-101), stepLength 0.01
 * (glwindow3d.cpp:98), threshold 0.5 (glwindow3d.cpp:97), depthWeight 0.7 (glwindow3d.cpp:84), alphaExponent 2 (glwindow3d.cpp:85),
 * gamma 2.2 (glwindow3d.h:219), smoothFactor 1 (glwindow3d.cpp:86), shading on (glwindow3d.cpp:87), LUT off (glwindow3d.cpp:88),
 * background black (glwindow3d.cpp:89), material 1, 1, 1 (glwindow3d.h:214), light at 1, 3, 3 (glwindow3d.h:213); no jitter, RGBA_F32. */
void octpipe_default_render_settings(OctPipeRenderSettings* s);
/* glwindow3d.cpp:301-303: translate(viewX, viewY, -4 exp(distExp / 600)) times the rotation of the quaternion (w, x, y, z), which is
 * normalised first (zero or not finite: OCTPIPE_ERR_INVALID_ARGUMENT).  Computed in double, rounded once; row-major. */
int octpipe_render_view_matrix(const float quaternion[4], float viewX, float viewY, float distExp, float out[16]);
/* the 1-D colour table: `width` (2 ... 4096) RGBA byte quadruples, copied on the compute stream */
int octpipe_update_render_lut(octpipe_t* h, const uint8_t* rgba, unsigned width);
int octpipe_render_volume(octpipe_t* h, const uint8_t* voxels /* NULL: the handle's volume view buffer */, int voxelsAreDevice,
                          const uint32_t dims[3] /* x, y, z of `voxels`; ignored for NULL */, const OctPipeRenderSettings* s,
                          void** d_image /* may be NULL */, size_t* bytes /* may be NULL */);
int octpipe_render_oct_depth(octpipe_t* h, const uint8_t* voxels /* NULL: the handle's volume view buffer */, int voxelsAreDevice,
                             const uint32_t dims[3] /* x, y, z of `voxels`; ignored for NULL */, const OctPipeRenderSettings* s,
                             void** d_image /* may be NULL */, size_t* bytes /* may be NULL */);
int octpipe_volume_surface_map(octpipe_t* h, const uint8_t* voxels /* NULL: the handle's volume view buffer */, int voxelsAreDevice,
                               const uint32_t dims[3], float depthThreshold, uint16_t* map /* host, dims[0] * dims[1] */);
int octpipe_copy_rendered_to_host(octpipe_t* h, void* dst, size_t bytes);

/* ------------------------------------------------------------------ surface views
 * What a user does with a curved or tilted sample: find the first interface of every A-scan, smooth that map, then cut an en face
 * slab that follows it, or shift every A-scan so that the surface becomes a straight line (flattening).  All of it on the float32
 * processed volume, and chainable on the device: detect -> smooth -> en face / flatten without a host round trip.  The reference has
 * no counterpart: parity is unpinned, and THIS COMMENT IS THE DEFINITION.  tests/surface_model.py restates it in
 * numpy, csrc/surface_views.h implements it.
 *
 * Source and region: those of octpipe_processed_statistics (the same OctPipeStatsRegion; data = NULL: the handle's processed volume,
 * slot `buffer`, 0xFFFFFFFF = the slot the last process call wrote; otherwise one caller buffer [B][A][N/2] of float32 in host or device
 * memory, buffer 0 or 0xFFFFFFFF; the stored layout).  v[d] below is the value of depth bin d of the A-scan in question.  The window is
 * W = [s0, s1] = [firstSample, firstSample + sampleCount - 1]; no call reads a value outside W.
 * Surface: int32 [bscanCount][ascanCount], dense over the region (entry b * ascanCount + a belongs to A-scan firstAscan + a of B-scan
 * firstBscan + b).  Entries are ABSOLUTE depth bins (not relative to firstSample).  Any negative entry means "no surface here";
 * outputs write -1 for it.
 * Memory: every surface and every result lies in host memory (...IsDevice = 0) or device memory (!= 0).  A host source is staged in
 * bounded chunks, only the region's A-scans travel; a host surface is copied whole.
 *
 * octpipe_surface_detect.  s(b, a) = the smallest d with s0 <= d <= s1 - run + 1 and v[d + i] > threshold for every 0 <= i < run; -1
 *   when there is none.  The compare is a strict float32 compare: NaN never exceeds, +inf exceeds every finite threshold, a value equal to
 *   the threshold does not.  The caller skips the top of the depth range with firstSample.  Limits: 1 <= run <= 64, run <= sampleCount,
 *   threshold not NaN (+-inf allowed).
 * octpipe_surface_smooth (no handle state besides scratch; the map is rows x cols, row-major).  out[r][c] = the lower median of the
 *   non-negative entries among surface[r'][c'], |r' - r| <= radius, |c' - c| <= radius, 0 <= r' < rows, 0 <= c' < cols: element (n - 1) / 2
 *   (integer division) of those n entries sorted ascending; -1 for n = 0.  A hole is filled from its neighbours; radius = 0 only
 *   canonicalises negatives to -1.  Limits: radius <= 3; rows, cols >= 1, rows * cols <= 2^28; out must not be the input pointer.
 * octpipe_surface_enface.  For an A-scan with surface entry s >= 0, D = the bins s + offset ... s + offset + thickness - 1 (64-bit
 *   integer arithmetic) that lie inside W.  s < 0 or D empty: the output is `fill` (its bits as given).  Otherwise
 *     function 0 (averaging): the float64 sum of the values of D, added one after another in increasing depth starting from the first,
 *       divided once by |D| in float64 and rounded once to float32; NaN and inf behave as in IEEE arithmetic;
 *     function 1 (MIP): NaN if any value of D is NaN; otherwise the value at the smallest depth among those that no other value of D
 *       exceeds (which settles -0 against +0).
 *   A NaN result is stored as the canonical quiet NaN 0x7FC00000 in both functions.  Output: float32 [bscanCount][ascanCount].
 *   Limits: 1 <= thickness <= 4096; function 0 or 1 (the codes of displayFunctionEnFaceView).
 * octpipe_flatten.  out[b][a][j], 0 <= j < outDepth, = v[s - anchor + j] when s >= 0 and that bin lies inside W, else `fill`.  Values
 *   and fill are copied bit by bit.  The surface lands in row `anchor` of the output, which may be negative or beyond outDepth.
 *   Output: float32 [bscanCount][ascanCount][outDepth].  Limits: 1 <= outDepth <= 8192.
 * Every output is a function of the values, the surface and the region's shape alone: the same values give the same bits from host or
 * device memory, from another slot, in a repeated call.
 * A NULL pointer, a limit above, a region that is empty or leaves the buffer: OCTPIPE_ERR_INVALID_ARGUMENT naming the field.
 * The work is enqueued on the compute stream behind what is already there (a call after octpipe_process_device sees that buffer
 * without a host synchronise).  A call with a host result returns once that result is filled; with a device result it returns without
 * waiting for the kernel (host inputs have left the caller's memory by then).  The calls change nothing the processing chain reads or
 * writes (processed / display / volume buffers, kernel timing).  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.  The scratch belongs to
 * the handle (freed in octpipe_destroy). */
typedef struct OctPipeSurfaceDetectSettings {  /* 2 x 4 = 8 bytes */
	float    threshold;   /* a bin is "above" when v > threshold */
	uint32_t run;         /* consecutive bins above the threshold that make a surface, 1 ... 64 */
} OctPipeSurfaceDetectSettings;

typedef struct OctPipeSurfaceEnfaceSettings {  /* 4 x 4 = 16 bytes */
	int32_t  offset;      /* first bin of the slab relative to the surface (negative: above it) */
	uint32_t thickness;   /* bins of the slab, 1 ... 4096 */
	int32_t  function;    /* 0: averaging, 1: MIP */
	float    fill;        /* output where there is no surface or no bin of the slab inside the window */
} OctPipeSurfaceEnfaceSettings;

typedef struct OctPipeFlattenSettings {  /* 3 x 4 = 12 bytes */
	int32_t  anchor;      /* output row the surface lands in */
	uint32_t outDepth;    /* rows of the output, 1 ... 8192 */
	float    fill;        /* output where the source bin is outside the window or there is no surface */
} OctPipeFlattenSettings;

int octpipe_surface_detect(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                           const OctPipeStatsRegion* r, const OctPipeSurfaceDetectSettings* s,
                           int32_t* surface /* bscanCount x ascanCount */, int surfaceIsDevice);
int octpipe_surface_smooth(octpipe_t* h, const int32_t* surface, int surfaceIsDevice, uint32_t rows, uint32_t cols, uint32_t radius,
                           int32_t* out /* rows x cols */, int outIsDevice);
int octpipe_surface_enface(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                           const OctPipeStatsRegion* r, const int32_t* surface, int surfaceIsDevice,
                           const OctPipeSurfaceEnfaceSettings* s, float* out /* bscanCount x ascanCount */, int outIsDevice);
int octpipe_flatten(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                    const OctPipeStatsRegion* r, const int32_t* surface, int surfaceIsDevice,
                    const OctPipeFlattenSettings* s, float* out /* bscanCount x ascanCount x outDepth */, int outIsDevice);

/* ------------------------------------------------------------------ boundary tracing
 * What octpipe_surface_detect cannot do: a layer boundary on which neighbouring A-scans agree, and a second boundary below the first.
 * Every B-scan of the region is segmented by graph search (Chiu et al. 2010 and successors): the path from its first to its last
 * A-scan that minimises a cost made of the vertical intensity gradient and a penalty on depth changes, with the depth change between
 * neighbouring A-scans limited.  A band around a guide surface restricts the search: a detected and smoothed first interface as the guide
 * and a band below it finds the next layer.  On the float32 processed volume, chainable on the device: detect -> smooth -> trace
 * (guided) -> en face / flatten / attenuation en face.  The reference has no counterpart: parity is unpinned, and
 * THIS COMMENT IS THE DEFINITION.  tests/boundary_model.py restates it in numpy, csrc/boundary_trace.h implements it; results are held
 * bit for bit.
 *
 * Source, region, window W = [s0, s1], surfaces and memory: those of the surface views.  v[a][d] is depth bin d of A-scan a (0 <= a <
 * ascanCount) of the B-scan in question; no call reads a value outside W; B-scans are independent of one another.
 * Guide: NULL (with guideIsDevice = 0), or int32 [bscanCount][ascanCount] of absolute bins, negative = none, in host or device memory.
 *   With a guide the node coordinate is r in [bandLo, bandHi] and node (a, r) stands for bin d = guide[a] + r.  With guide = NULL the
 *   guide counts as 0 everywhere and the band as [s0, s1]; bandLo and bandHi are ignored.  H = the number of nodes per A-scan (bandHi -
 *   bandLo + 1, or sampleCount).
 * Node cost, float32 throughout.  If guide[a] < 0 or d lies outside W: c(a, r) = +0.  Otherwise, with cl(i) = i clamped into W and
 *   k = halfWidth,
 *     up = v[cl(d)] + v[cl(d + 1)] + ... + v[cl(d + k - 1)]      starting from the first term, the others added one after another in
 *     dn = v[cl(d - 1)] + v[cl(d - 2)] + ... + v[cl(d - k)]      that order, each sum rounded to float32
 *     g = up - dn;   g not finite: c = +0;   otherwise c = -g for polarity +1 (dark above, bright below), c = g for polarity -1.
 * Recurrence.  p_j = fl32(smoothness * j), 0 <= j <= m = maxStep: one rounded float32 product, not contracted into the sum below.
 *   E(0, r) = c(0, r).  For a >= 1: E(a, r) = t* + c(a, r), where t* is the smallest of t_j = E(a - 1, r + j) + p_|j| over |j| <= m with
 *   r + j inside the band (j = 0 included; p_0 = +0 is added like the others).  The candidates are compared with a strict float32 `<`
 *   in the order j = 0, -1, +1, -2, +2, ...: t* starts as t_0 and a later candidate replaces it only where it compares smaller, so equal
 *   values keep the smallest |j| and then the negative j, and t* carries the bits of the chosen candidate (a select, not fminf).
 *   Overflow to +-inf follows IEEE arithmetic and the same rule.
 * Path.  At the last A-scan the smallest r among those no other E compares smaller than (the scan starts at the first node of the band
 *   and replaces only on a strict `<`); then back through the recorded choices j.
 * Output.  surface[b][a] = guide[a] + r of the path where guide[a] >= 0 and that bin lies inside W, else -1: int32
 *   [bscanCount][ascanCount], which octpipe_surface_smooth / _enface, octpipe_flatten, octpipe_angiogram_enface and
 *   octpipe_attenuation_enface take as it is, and this call as a guide.  pathCost (may be NULL): float32 [bscanCount], the E of the
 *   path's node at the last A-scan with its own bits; it lies where surface lies (surfaceIsDevice).
 * Limits: bandLo <= bandHi, both within +-65536 (with a guide); 1 <= halfWidth <= 8; polarity +1 or -1; 1 <= maxStep <= 7; smoothness
 *   finite and >= 0; 1 <= ascanCount <= 65536: otherwise OCTPIPE_ERR_INVALID_ARGUMENT naming the field.  1 <= H <= 1024; a larger H:
 *   OCTPIPE_ERR_UNSUPPORTED.  A host source is staged B-scan by B-scan (whole B-scans per slice).
 * Every output is a function of the values, the guide, the settings and the region's shape alone: the same values give the same bits
 * from host or device memory, from another slot, in a repeated call.  Errors (a NULL region, settings or surface; a guide that is NULL
 * with guideIsDevice set; argument checks come before the handle's), ordering on the compute stream, host and device results, side
 * effects (none on what the processing chain reads or writes), callbacks and scratch: as in the surface views. */
typedef struct OctPipeBoundaryTraceSettings {  /* 6 x 4 = 24 bytes */
	int32_t  bandLo;      /* first node relative to the guide, -65536 ... 65536 (ignored without a guide) */
	int32_t  bandHi;      /* last node relative to the guide, bandLo ... 65536 (ignored without a guide) */
	uint32_t halfWidth;   /* k: bins on either side of the gradient, 1 ... 8 */
	int32_t  polarity;    /* +1: dark above and bright below, -1: the reverse */
	uint32_t maxStep;     /* m: largest depth change between neighbouring A-scans, 1 ... 7 */
	float    smoothness;  /* lambda: cost per bin of depth change, finite, >= 0 */
} OctPipeBoundaryTraceSettings;

int octpipe_trace_boundary(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                           const OctPipeStatsRegion* r, const int32_t* guide /* bscanCount x ascanCount, or NULL */, int guideIsDevice,
                           const OctPipeBoundaryTraceSettings* s, int32_t* surface /* bscanCount x ascanCount */,
                           float* pathCost /* bscanCount, or NULL */, int surfaceIsDevice);

/* ------------------------------------------------------------------ angiography
 * What a scan protocol that records every slow-axis position several times is for: the contrast between the repeated B-scans (flow
 * decorrelates the speckle, static tissue does not), as a volume and as an en face projection of a slab that may follow the tissue
 * surface.  On the float32 processed volume, chainable on the device behind the surface views: detect -> smooth -> angiogram en face.
 * The reference has no counterpart: parity is unpinned, and THIS COMMENT IS THE DEFINITION.
 * tests/angio_model.py restates it in numpy, csrc/angiogram.h implements it.
 *
 * Source and region: those of octpipe_processed_statistics (the same OctPipeStatsRegion; data = NULL: the handle's processed volume,
 * slot `buffer`, 0xFFFFFFFF = the slot the last process call wrote; otherwise one caller buffer [B][A][N/2] of float32 in host or device
 * memory, buffer 0 or 0xFFFFFFFF; the stored layout).  A host source is staged in bounded chunks of whole positions (at least one), only
 * the region's A-scans travel.
 *
 * Repeats.  M = repeats, 2 <= M <= 8, and M divides bscanCount.  Position p, 0 <= p < P = bscanCount / M, owns B-scans firstBscan + p M + m,
 *   0 <= m < M: consecutive B-scans of one buffer.  For A-scan a of the region and depth bin d of the window W = [s0, s1] =
 *   [firstSample, firstSample + sampleCount - 1], v_m is the float32 value of repeat m, converted exactly to float64.  No call reads a
 *   value outside W or outside the region's A-scans.
 * Mean.  mu = (((v_0 + v_1) + v_2) + ...) / M in float64, one division.  mu32 = (float)mu.
 * Contrast c, in float64; every product is rounded before it is added (no fused multiply-add):
 *   method 0, speckle variance:  d_m = v_m - mu;  c = (((d_0 d_0 + d_1 d_1) + d_2 d_2) + ...) / M.
 *   method 1, amplitude decorrelation (meaningful on linearly scaled data; the call analyses whatever is stored):  for 0 <= m <= M - 2,
 *     n_m = v_m v_{m+1} and q_m = 0.5 (v_m v_m) + 0.5 (v_{m+1} v_{m+1});  t_m = 1 when q_m == 0, otherwise n_m / q_m;
 *     c = 1 - (((t_0 + t_1) + ...) / (M - 1)).
 *   method 2, differential (on log-scaled data: the log-ratio contrast):  c = (((|v_1 - v_0| + |v_2 - v_1|) + ...) / (M - 1)).
 *   c32 = (float)c.  NaN and inf behave as in IEEE arithmetic; a NaN result is stored as the canonical quiet NaN 0x7FC00000.
 * Mask.  With mask != 0, c32 is replaced by `masked` (its bits as given) wherever !(mu32 > threshold): a strict float32 compare, so a NaN
 *   mean is masked.  threshold must not be NaN when mask != 0 (+-inf allowed).
 *
 * octpipe_angiogram.  out: float32 [P][ascanCount][sampleCount], c32 after the mask, dense over the region.  mean (may be NULL): the same
 *   shape, mu32 with a NaN canonical.  Both in host memory (outIsDevice = 0) or both in device memory.
 * octpipe_angiogram_enface.  The contrast of one slab, projected, without the volume ever being written: float32 [P][ascanCount].
 *   Surface: NULL (with surfaceIsDevice = 0) means s = firstSample for every A-scan, a fixed-depth slab.  Otherwise int32
 *     [bscanCount][ascanCount], exactly what octpipe_surface_detect / _smooth return for the same region (absolute bins, negative = none),
 *     in host or device memory; position p uses the row of its first repeat, row p M.
 *   Slab (OctPipeSurfaceEnfaceSettings): D = the bins s + offset ... s + offset + thickness - 1 (64-bit integer arithmetic) that lie inside
 *     W.  s < 0 or D empty: the output is `fill` (its bits as given).  Otherwise the bins of D are numbered i = 0, 1, ... in increasing
 *     depth and x_i is the bin's c32 after the mask.
 *   function 0 (averaging): partial L_j, 0 <= j < 64, is the float64 sum of x_j, x_{j+64}, x_{j+128}, ... added in that order starting
 *     from the first; S is the float64 sum of the existing partials in increasing j starting from L_0; the result is (float)(S / |D|), a NaN
 *     canonical.
 *   function 1 (MIP): NaN (canonical) if any x_i is NaN; otherwise the x_i with the smallest i among those that no other exceeds.
 *   Limits: 1 <= thickness <= 4096; function 0 or 1.
 * Every output is a function of the values, the surface and the region's shape alone: the same values give the same bits from host or
 * device memory, from another slot, in a repeated call.
 * A NULL region / settings / out, repeats outside [2, 8] or not dividing bscanCount, an unknown method, a NaN threshold with the mask on,
 * a surface that is NULL with surfaceIsDevice set, a thickness or function outside its limits, a buffer other than 0 / 0xFFFFFFFF with
 * data, a region that is empty or leaves the buffer: OCTPIPE_ERR_INVALID_ARGUMENT naming the field; these checks come before the handle's.
 * The work is enqueued on the compute stream behind what is already there.  A call with a host result returns once that result is
 * filled; with a device result it returns without waiting for the kernel (host inputs have left the caller's memory by then).  The calls
 * change nothing the processing chain reads or writes.  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.  The scratch belongs to the handle
 * (freed in octpipe_destroy). */
typedef struct OctPipeAngioSettings {  /* 5 x 4 = 20 bytes */
	uint32_t repeats;     /* M: B-scans per slow-axis position, 2 ... 8 */
	int32_t  method;      /* 0: speckle variance, 1: amplitude decorrelation, 2: differential */
	int32_t  mask;        /* != 0: replace the contrast by `masked` where the mean does not exceed `threshold` */
	float    threshold;
	float    masked;
} OctPipeAngioSettings;

int octpipe_angiogram(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                      const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                      float* out /* P x ascanCount x sampleCount */, float* mean /* the same, or NULL */, int outIsDevice);
int octpipe_angiogram_enface(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                             const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                             const int32_t* surface /* bscanCount x ascanCount, or NULL: firstSample */, int surfaceIsDevice,
                             const OctPipeSurfaceEnfaceSettings* slab, float* out /* P x ascanCount */, int outIsDevice);

/* ------------------------------------------------------------------ repeat registration
 * What the angiography needs on a live sample: between two repeats the sample moves axially by a few depth bins (breathing, heartbeat,
 * stage drift), and bin d of one repeat then shows the tissue of bin d + 2 of the next, so every static interface lights up as flow.
 * octpipe_repeat_shifts estimates the axial shift of every repeat against the first one; the _registered forms of the two angiography
 * calls take the contrast from the shifted bins.  All of it on the device and chainable without a host round trip: repeat shifts ->
 * angiogram (en face) registered.  The reference has no counterpart: parity is unpinned, and THIS COMMENT IS THE
 * DEFINITION.  tests/register_model.py restates it in numpy, csrc/repeat_register.h implements it.
 *
 * Source, region, window W = [s0, s1], repeats M (2 ... 8, divides bscanCount), positions p and P: those of the angiography section.
 * Groups.  G = ascansPerGroup >= 1 divides ascanCount; Qp = ascanCount / G groups per B-scan, as in the peak analysis: group j covers
 *   A-scans firstAscan + jG .. firstAscan + jG + G - 1.  G = ascanCount: one shift per repeated B-scan (the usual bulk-motion model);
 *   G = 1: one per A-scan.
 * Profile.  P_m[s], s in W, of group j of repeat m of position p: the averaged A-scan of that group exactly as the peak analysis section
 *   defines it (chunks of 64 consecutive A-scans, float64 chunk partials added in A-scan order, partials added in chunk order,
 *   (float)(T / G)): what octpipe_peak_analysis returns as `averaged` for group (p M + m) Qp + j of the same region.
 * Cost.  R = maxShift, 1 <= R <= 64, and sampleCount >= 2R + 1.  The inner window s0 + R ... s1 - R holds K = sampleCount - 2R bins,
 *   numbered i = 0 ... K - 1 in increasing depth; it is the same for every lag, so the costs need no normalisation.  For m >= 1 and every
 *   lag d in [-R, R]: term t_i = |(double)P_m[s0 + R + i + d] - (double)P_0[s0 + R + i]|; partial L_j, 0 <= j < 64, is the float64 sum of
 *   t_j, t_{j+64}, t_{j+128}, ... added in that order starting from the first; C_m(d) is the float64 sum of the existing partials in
 *   increasing j starting from L_0 (the partial scheme of octpipe_angiogram_enface, function 0).
 * Shift.  If any value of P_0 or of P_m inside W is non-finite: shift_m = 0 and every C_m(d) is reported as the canonical quiet NaN
 *   0x7FF8000000000000.  Otherwise shift_m = the d with the smallest C_m(d); among equal costs the smallest |d|, then the negative one.
 *   shift_0 = 0 always.  Meaning: bin s + shift_m of repeat m shows what bin s of repeat 0 shows.
 *
 * octpipe_repeat_shifts.  shifts: int32 [P][M][Qp], in host (shiftsIsDevice = 0) or device memory.  costs (may be NULL): float64
 *   [P][M - 1][Qp][2R + 1] in the same memory as shifts, lag d at index d + R.
 *   Limits: 3 <= sampleCount <= 4096 as in the peak analysis (a longer window: OCTPIPE_ERR_UNSUPPORTED).
 *
 * Registered contrast.  shifts: int32 [P][M][Qp] in host or device memory, what octpipe_repeat_shifts returns for the same region, M and
 *   G = registration->ascansPerGroup.  ANY values are accepted, a non-zero entry for m = 0 included; everything below is 64-bit integer
 *   arithmetic.  For an A-scan of group j with shifts d_m, the covered window is Wc = [s0 + max_m(-d_m), s1 - max_m(d_m)], which may be
 *   empty.  For a bin s of W inside Wc, v_m is the value of repeat m at bin s + d_m (a bin of W); mean, contrast, mask and NaN
 *   canonicalisation are exactly those of the angiography section.
 * octpipe_angiogram_registered.  The arguments and the output shape of octpipe_angiogram; the bins of W outside Wc hold
 *   registration->fill (its bits as given) in both out and mean.
 * octpipe_angiogram_enface_registered.  The arguments of octpipe_angiogram_enface; D is the slab's bins inside W and inside Wc (still one
 *   contiguous run, so the numbering i and the partials are unchanged).  s < 0 or D empty: the output is the slab's fill.
 *   registration->fill is not used by this call.
 * With all shifts zero both calls write the bits of the unregistered calls.
 * Every output is a function of the values, the shifts, the surface and the region's shape alone: the same values give the same bits
 * from host or device memory, from another slot, in a repeated call.
 * A NULL region / settings / shifts / registration / out, a shifts that is NULL with shiftsIsDevice set, repeats outside [2, 8] or not
 * dividing bscanCount, ascansPerGroup = 0 or not dividing ascanCount, maxShift outside [1, 64], sampleCount < 2 maxShift + 1 or < 3, and
 * everything the angiography calls refuse: OCTPIPE_ERR_INVALID_ARGUMENT naming the field; these checks (and the one for sampleCount >
 * 4096) come before the handle's.
 * A host source is staged in bounded chunks of whole positions; host shifts are uploaded whole.  The work is enqueued on the compute
 * stream behind what is already there.  A call with a host result returns once that result is filled; with a device result it returns
 * without waiting for the kernel (host inputs have left the caller's memory by then).  The calls change nothing the processing chain
 * reads or writes.  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.  The scratch belongs to the handle (freed in octpipe_destroy). */
typedef struct OctPipeRepeatShiftSettings {  /* 3 x 4 = 12 bytes */
	uint32_t repeats;         /* M: B-scans per slow-axis position, 2 ... 8 */
	uint32_t ascansPerGroup;  /* G >= 1, divides ascanCount */
	uint32_t maxShift;        /* R: the lags searched are -R ... R, 1 ... 64 */
} OctPipeRepeatShiftSettings;

typedef struct OctPipeAngioRegistration {  /* 2 x 4 = 8 bytes */
	uint32_t ascansPerGroup;  /* G of the shifts */
	float    fill;            /* octpipe_angiogram_registered: out and mean where a bin of the window is not covered by every repeat */
} OctPipeAngioRegistration;

int octpipe_repeat_shifts(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                          const OctPipeStatsRegion* r, const OctPipeRepeatShiftSettings* s,
                          int32_t* shifts /* P x M x Qp */, int shiftsIsDevice, double* costs /* P x (M - 1) x Qp x (2R + 1), or NULL */);
int octpipe_angiogram_registered(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                                 const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                 float* out /* P x ascanCount x sampleCount */, float* mean /* the same, or NULL */, int outIsDevice,
                                 const int32_t* shifts /* P x M x Qp */, int shiftsIsDevice, const OctPipeAngioRegistration* registration);
int octpipe_angiogram_enface_registered(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                                        const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                        const int32_t* surface /* bscanCount x ascanCount, or NULL: firstSample */, int surfaceIsDevice,
                                        const OctPipeSurfaceEnfaceSettings* slab, float* out /* P x ascanCount */, int outIsDevice,
                                        const int32_t* shifts /* P x M x Qp */, int shiftsIsDevice, const OctPipeAngioRegistration* registration);

/* ------------------------------------------------------------------ attenuation
 * The standard quantitative read-out of a structural OCT volume: the depth-resolved attenuation coefficient of Vermeer et al. 2014
 * (PAPERS.md), mu[i] = I[i] / (2 Delta sum_{j > i} I[j]), for every bin of a region, as a volume and as an en face projection of a slab
 * that may follow the tissue surface.  On the float32 processed volume, chainable on the device behind the surface views: detect ->
 * smooth -> attenuation en face.  The reference has no counterpart: parity is unpinned, and THIS COMMENT IS THE
 * DEFINITION.  tests/attenuation_model.py restates it in numpy, csrc/attenuation.h implements it.
 *
 * Source and region: those of octpipe_processed_statistics (the same OctPipeStatsRegion; data = NULL: the handle's processed volume,
 * slot `buffer`, 0xFFFFFFFF = the slot the last process call wrote; otherwise one caller buffer [B][A][N/2] of float32 in host or device
 * memory, buffer 0 or 0xFFFFFFFF; the stored layout).  A host source is staged in bounded chunks, only the region's A-scans travel.
 * The window is W = [s0, s1] = [firstSample, firstSample + sampleCount - 1], n = sampleCount, and bin i = d - s0 for depth bin d of W; v[i]
 * is the float32 value of bin i of the A-scan in question.  No call reads a value outside W or outside the region's A-scans.  `out` must
 * not overlap the source.
 * Gain table.  depthGain = NULL (with gainIsDevice = 0): none.  Otherwise n float32 entries g[i], one per bin of W, in host
 *   (gainIsDevice = 0) or device memory: the correction of the sensitivity roll-off, for instance from the averaged A-scans of
 *   octpipe_peak_analysis.  ANY values are accepted.
 *
 * All arithmetic is float64 (every float32 converted exactly) with no fused multiply-add: every product is rounded before it is added.
 * Intensity of bin i, with a = mapScale, b = mapOffset:
 *   1. x = (double)v[i] * a + b.
 *   2. J = x for scale 0 (the mapped value is an intensity), x * x for scale 1 (an amplitude), pow2(x) for scale 2 (log2 of an intensity).
 *   3. K = J - (double)noise.
 *   4. L = K * (double)g[i] with a gain table, else L = K.
 *   5. I = L > 0 ? L : +0.0.
 *   A NaN or negative L therefore gives +0: a NaN bin does not poison the A-scan above it.  +inf stays.
 * pow2(y), defined so that host and device agree bit for bit: +inf for y >= 1024; +0 for y < -1000; NaN for a NaN y.  Otherwise m = rint(y)
 *   (ties to even), f = y - m, t = f * 0x1.62e42fefa39efp-1 (ln 2), p = c_13, then for k = 12 ... 0: p = c_k + t * p, with c_k the double
 *   nearest 1 / k!; the result is ldexp(p, m).  (Within 2 ulp of exp2 over [-60, 60].)
 * Sum below a bin.  The order is fixed; it is the one of a wave of 64 lanes that hold four consecutive bins each.  The bins of W are cut
 *   into chunks of 256, anchored at s0: chunk k, lane l in 0 .. 63 and j in 0 .. 3 is bin 256 k + 4 l + j; bins >= n count as I = +0.
 *   C = (double)tail at the start.  For k from the last chunk down to 0:
 *     1. Q_l = ((I_{l,3} + I_{l,2}) + I_{l,1}) + I_{l,0}.
 *     2. t_l = Q_l; then for s = 1, 2, 4, 8, 16, 32, all lanes at once from the previous step's values: t_l = t_l + t_{l+s} where
 *        l + s <= 63, else unchanged.
 *     3. R_63 = C, and R_l = t_{l+1} + C for l < 63.
 *     4. below_{l,3} = R_l;  below_{l,2} = below_{l,3} + I_{l,3};  below_{l,1} = below_{l,2} + I_{l,2};  below_{l,0} = below_{l,1} + I_{l,1}.
 *     5. C = t_0 + C.
 * Result.  den = (2.0 * (double)pixelSize) * below.  den > 0: mu32 = (float)(I / den), a NaN result stored as the canonical quiet NaN
 *   0x7FC00000.  Otherwise (nothing below the bin): `undefined`, its bits as given.
 *
 * octpipe_attenuation.  out: float32 [bscanCount][ascanCount][sampleCount], mu32, dense over the region, in host (outIsDevice = 0) or
 *   device memory.
 * octpipe_attenuation_enface.  The coefficient of one slab, projected, without the volume ever being written: float32
 *   [bscanCount][ascanCount].  By definition it is what octpipe_surface_enface returns for the volume octpipe_attenuation writes for the
 *   same region, with the same OctPipeSurfaceEnfaceSettings: the slab, `fill`, the averaging (the sequential float64 sum in increasing
 *   depth) and the MIP are those of the surface views section.
 *   Surface: NULL (with surfaceIsDevice = 0) means s = firstSample for every A-scan, a fixed-depth slab.  Otherwise int32
 *     [bscanCount][ascanCount], what octpipe_surface_detect / _smooth return for the same region (absolute bins, negative = none), in
 *     host or device memory.
 *   An A-scan is read only from the first bin of its slab down to the end of W.
 *   Limits: 1 <= thickness <= 4096; function 0 or 1.
 * Every output is a function of the values, the settings, the gain table, the surface and the region's shape alone: the same values give
 * the same bits from host or device memory, from another slot, in a repeated call.
 * A NULL region / settings / out, a scale outside 0 .. 2, a pixelSize that is not finite and > 0, a NaN noise, a tail that is negative or
 * NaN, a mapScale or mapOffset that is not finite, reserved != 0, a depthGain that is NULL with gainIsDevice set, a surface that is NULL
 * with surfaceIsDevice set, a thickness or function outside its limits, a buffer other than 0 / 0xFFFFFFFF with data, a region that is
 * empty or leaves the buffer: OCTPIPE_ERR_INVALID_ARGUMENT naming the field; these checks (the region's extent excepted) come before the
 * handle's.
 * The work is enqueued on the compute stream behind what is already there.  A call with a host result returns once that result is
 * filled; with a device result it returns without waiting for the kernel (host inputs have left the caller's memory by then).  The calls
 * change nothing the processing chain reads or writes.  Inside a callback: OCTPIPE_ERR_IN_CALLBACK.  The scratch belongs to the handle
 * (freed in octpipe_destroy). */
typedef struct OctPipeAttenuationSettings {  /* 2 x 8 + 6 x 4 = 40 bytes */
	double   mapScale, mapOffset;  /* a, b of the linearising map x = v * a + b; finite */
	int32_t  scale;       /* what x is: 0 an intensity, 1 an amplitude (squared), 2 log2 of an intensity */
	float    pixelSize;   /* Delta: the length of one depth bin in the sample (mu comes out in its inverse unit); finite and > 0 */
	float    noise;       /* the noise floor in intensity units, subtracted from every bin; not NaN */
	float    tail;        /* the intensity below the window; >= 0, not NaN; 0 if unknown */
	float    undefined;   /* the output where the sum below a bin is zero; its bits as given */
	uint32_t reserved;    /* must be 0 */
} OctPipeAttenuationSettings;

int octpipe_attenuation(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                        const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s,
                        const float* depthGain /* sampleCount entries, or NULL */, int gainIsDevice,
                        float* out /* bscanCount x ascanCount x sampleCount */, int outIsDevice);
int octpipe_attenuation_enface(octpipe_t* h, const float* data /* NULL: the handle's processed volume */, int dataIsDevice,
                               const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s,
                               const float* depthGain /* sampleCount entries, or NULL */, int gainIsDevice,
                               const int32_t* surface /* bscanCount x ascanCount, or NULL: firstSample */, int surfaceIsDevice,
                               const OctPipeSurfaceEnfaceSettings* slab, float* out /* bscanCount x ascanCount */, int outIsDevice);

/* ------------------------------------------------------------------ measurement helper
 * Average duration in ms of the dominant (fused) kernel since the last reset, measured with HIP
 * events on the handle's own stream around each launch while timing is enabled (enable != 0: a boolean).
 * octpipe_set_kernel_timing_stride(h, n): only every n-th launch carries events from then on (a timed launch costs the stream 2-4 us on
 * MI355X, profiles/r5f_fold_flush16_ab.txt); n = 1 (the default after every enable) times each launch.  (Until round 5 `enable = n > 1`
 * meant the stride: a caller passing any non-zero value as a boolean silently got sparse timing -- ADVICE r5.)
 * ON THE COMPUTE LANES THIS IS NOT A KERNEL DURATION.  While consecutive octpipe_process_device buffers alternate between the handle's
 * two compute lanes (csrc/lanes.h: an even buffersPerVolume and nothing that keeps the buffer on one stream), the start event of a timed
 * launch is taken when its lane accepts the dispatch, which is while the other lane's kernel still holds the chip: the interval spans the
 * wait for the compute units plus the kernel, about twice the kernel's duration in a steady stream of buffers (0.27-0.29 ms for a
 * 0.146 ms kernel, profiles/lanes_ab.txt).  For the duration of the kernel alone keep the handle on one stream while measuring
 * (OCTPIPE_ROUTE_ONE_LANE of octpipe_debug.h, or any of the conditions of lanes.h) or read a kernel trace; the time per buffer is the
 * wall time of a run of buffers. */
int octpipe_enable_kernel_timing(octpipe_t* h, int enable);
int octpipe_set_kernel_timing_stride(octpipe_t* h, unsigned everyNth);
int octpipe_kernel_timing(octpipe_t* h, double* avgMs, unsigned* launches, int reset);

#ifdef __cplusplus
}
#endif
#endif /* OCTPIPE_H */
