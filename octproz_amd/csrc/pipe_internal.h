// pipe_internal.h -- what the translation units of the C-ABI implementation share (round 5: octpipe_api.hip was one 1 800-line file):
// the per-handle state (everything the reference keeps in the file-scope globals of cuda_code.cu, cu:39-105), the error convention
// and the helpers that cross file borders.  Not installed, not part of the boundary (include/octpipe.h is).
//   octpipe_api.hip    handle life cycle, the chain of one buffer (launchFused / processDeviceRaw), result delivery, debug hooks
//   pipe_calib.hip     curves, look-up tables, twiddles, per-length tables, calibration blob, mean line (cu:636-657, cu:1433-1445)
//   pipe_display.hip   display-frame extraction (cu:1223-1308, cu:1571-1578)
//   pipe_dispersion.hip dispersion estimation: candidate sweep over a staged copy of a few A-scans (dispersion_sweep.h)
//   pipe_phase.hip     phase extraction: integer accumulation of raw A-scans, resampling curve from their mean (phase_extract.h)
//   pipe_stats.hip     image statistics: histogram and moments of a region of a processed or raw buffer (image_stats.h)
//   pipe_peak.hip      peak analysis: averaged A-scans of groups of a region, peak, half-maximum width, Gaussian fit (peak_analysis.h)
//   pipe_render.hip    volume rendering: the ray caster over the 8-bit volume view or a caller's voxels (volume_render.h)
//   pipe_surface.hip   surface views: surface detection and smoothing, surface-following en face slabs, flattening (surface_views.h)
//   pipe_angio.hip     angiography: contrast between repeated B-scans as a volume and as an en face slab (angiogram.h); repeat
//                      registration: the axial shifts of the repeated B-scans, the same two calls on the shifted bins (repeat_register.h)
//   pipe_attenuation.hip depth-resolved attenuation: the coefficient of every bin as a volume and as an en face slab (attenuation.h)
//   pipe_boundary.hip  boundary tracing: the minimum-cost path through every B-scan of a region (boundary_trace.h)
//   pipe_region.hip    what the statistics, the peak analysis, the surface views, the angiography and the attenuation share: region checks, the processed
//                      source, host staging of a region's rows, a host surface on its way in, a result's place and its way to the host
//   route.h            which implementation a buffer runs on (pure functions)
// This file also holds what the nine families of analysis calls (dispersion ... boundary tracing) share: their device scratch (DeviceScratch, grow, release),
// the optional device timing behind the octpipe_debug_* entry points (StreamTimer) and the entry check (enterCall).
#pragma once
#include <dlfcn.h>
#include <sys/stat.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/octpipe.h"
#include "../../include/octpipe_debug.h"
#include "display_kernels.h"
#include "host_luts.h"
#include "lanes.h"
#include "launch.h"
#include "route.h"
#include "sample_decode.h"
#include "sinus_plan.h"

namespace octimpl {

extern thread_local std::string g_lastError;
extern thread_local bool t_inCallback;  // this thread is inside a data / event callback of the pipeline (hipLaunchHostFunc)

inline int fail(int code, const std::string& msg) {
	g_lastError = msg;
	return code;
}

#define HIP_TRY(expr)                                                                                         \
	do {                                                                                                      \
		hipError_t _e = (expr);                                                                               \
		if (_e != hipSuccess) {                                                                               \
			return octimpl::fail(_e == hipErrorOutOfMemory ? OCTPIPE_ERR_OUT_OF_MEMORY : OCTPIPE_ERR_DEVICE,  \
			                     std::string(#expr) + ": " + hipGetErrorString(_e));                          \
		}                                                                                                     \
	} while (0)

struct CalibrationHeader {  // layout of the calibration blob (octpipe_export_calibration)
	uint32_t magic, version, samplesPerLine, fixedPatternNoiseDetermined;
};
constexpr uint32_t kCalibMagic = 0x4F435443u;  // "OCTC"

struct TimedLaunch { hipEvent_t start, stop; };
// the image route of an otherwise eligible buffer (lanes.h), kept with what it was chosen from (octpipe_api.hip laneFacts)
struct LanePlanCache {
	bool valid = false, prepared = false, error = false;
	int kind = 0;
	unsigned route = 0, state = 0;
	OctPipeParams params{};
};

// cu:718 / cu:739 rewritten as one multiply-add on log2(P) resp. sqrt(P): value = sA * s + sB; constants in double
inline void grayscaleScaling(const OctPipeParams& p, int N, bool logScale, float* sA, float* sB) {
	const double half = (double)(N / 2), range = (double)p.signalGrayscaleMax - (double)p.signalGrayscaleMin;
	const double coeff = p.signalMultiplicator, addend = p.signalAddend, mn = p.signalGrayscaleMin;
	if (logScale) {
		*sA = (float)(coeff * 10.0 * log10(2.0) / range);
		*sB = (float)(coeff * ((-10.0 * log10(half) - mn) / range + addend));
	} else {
		*sA = (float)(coeff / (half * range));
		*sB = (float)(coeff * (-mn / range + addend));
	}
}

// Device scratch of one of the analysis calls: slots grown on demand (grow), owned by the handle, released in octpipe_destroy.
// Each call's state names its slots; SLOTS is the most any of them has.
struct DeviceScratch {
	enum { SLOTS = 11 };
	void* p[SLOTS] = {};
	size_t bytes[SLOTS] = {};
	template <class T> T* as(int slot) const { return static_cast<T*>(p[slot]); }
};
struct SweepScratch : DeviceScratch {  // dispersion sweep (pipe_dispersion.hip)
	enum { RAW, ROWS, GATHERED, LUT, LANCZOS, TWIDDLE, COEF, PHASOR, THETA, METRIC, SCORES, COUNT };
};
struct PhaseState : DeviceScratch {  // phase extraction (pipe_phase.hip)
	enum { ACC, STAGE, EXTRACT, COUNT };  // int64[N] column sums | host rows in transit | mean, outputs and status of one extraction
	uint64_t count = 0;  // A-scans in ACC
};
struct StatsState : DeviceScratch {  // image statistics (pipe_stats.hip)
	enum { PARTS, SLAB, OUT, STAGE, COUNT };  // segment partials | per-workgroup counts | result + uint64 histogram, under / overflow |
	                                          // host rows in transit
};
struct PeakState : DeviceScratch {  // peak analysis (pipe_peak.hip)
	enum { PARTS, OUT, AVG, STAGE, COUNT };  // float64 chunk partials | OctPipePeak results | averaged A-scans | host rows in transit
};
struct RenderState : DeviceScratch {  // volume rendering (pipe_render.hip)
	enum { IMAGE, LUT, STAGE, SURFACE, COUNT };  // the rendered RGBA image | the colour table | host voxels in transit | the OCT Depth
	                                             // mode's surface map, uint16 [Y][X]
	size_t imageBytes = 0;  // size of the last rendered image (0: none yet)
	unsigned lutWidth = 0;  // entries of the colour table (0: none yet)
};
struct SurfaceState : DeviceScratch {  // surface views (pipe_surface.hip)
	enum { STAGE, SURF_IN, SURF_OUT, OUT, COUNT };  // host rows in transit | a host surface on its way in | a surface result on its way to
	                                                // the host | an en face image or a slice of flattened rows on its way to the host
};
struct AngioState : DeviceScratch {  // angiography and repeat registration (pipe_angio.hip)
	enum { STAGE, SURF_IN, SHIFTS_IN, OUT, MEAN, PARTS, SHIFTS_OUT, COSTS_OUT, COUNT };  // host rows in transit | a host surface / host shifts on
	                                            // their way in | an en face image or a slice of contrast rows / of mean rows on its way to the
	                                            // host | the shift estimate: float64 chunk partials, shifts / costs on their way to the host
};
struct AttenuationState : DeviceScratch {  // depth-resolved attenuation (pipe_attenuation.hip)
	enum { STAGE, GAIN_IN, SURF_IN, OUT, COUNT };  // host rows in transit | a host gain table / a host surface on their way in | an en face
	                                               // image or a slice of coefficient rows (of sums) on its way to the host
};
struct BoundaryState : DeviceScratch {  // boundary tracing (pipe_boundary.hip)
	enum { STAGE, GUIDE_IN, SURF_OUT, COST_OUT, CHOICES, COUNT };  // host rows in transit | a host guide on its way in | the surface / the path
	                                                               // costs on their way to the host | the 4-bit choices of one launch
};
static_assert(BoundaryState::COUNT <= DeviceScratch::SLOTS, "raise DeviceScratch::SLOTS");
static_assert(SweepScratch::COUNT <= DeviceScratch::SLOTS && PhaseState::COUNT <= DeviceScratch::SLOTS && StatsState::COUNT <= DeviceScratch::SLOTS &&
                  PeakState::COUNT <= DeviceScratch::SLOTS && RenderState::COUNT <= DeviceScratch::SLOTS && SurfaceState::COUNT <= DeviceScratch::SLOTS &&
                  AngioState::COUNT <= DeviceScratch::SLOTS && AttenuationState::COUNT <= DeviceScratch::SLOTS, "raise DeviceScratch::SLOTS");

// Device time of a call's work on a stream, for the octpipe_debug_* entry points: nothing at all unless wanted.  begin / end may
// repeat (the last pair counts); elapsedMs, after the stream has been synchronised, leaves *ms alone unless wanted.  `what` prefixes the messages.
class StreamTimer {
	const bool wanted;
	const char* const what;
	hipEvent_t ev[2] = {nullptr, nullptr};
	int record(hipEvent_t e, hipStream_t stream) const {
		if (wanted && hipEventRecord(e, stream) != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, std::string(what) + ": event record");
		return OCTPIPE_OK;
	}

public:
	StreamTimer(bool wanted, const char* what) : wanted(wanted), what(what) {}
	StreamTimer(const StreamTimer&) = delete;
	~StreamTimer() {
		for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
	}
	int begin(hipStream_t stream) {
		if (wanted && !ev[0]) HIP_TRY(hipEventCreate(&ev[0]));
		if (wanted && !ev[1]) HIP_TRY(hipEventCreate(&ev[1]));
		return record(ev[0], stream);
	}
	int end(hipStream_t stream) const { return record(ev[1], stream); }
	hipError_t elapsedMs(double* ms) const {
		if (!wanted) return hipSuccess;
		float f = 0.0f;
		const hipError_t e = hipEventElapsedTime(&f, ev[0], ev[1]);
		if (e == hipSuccess) *ms = f;
		return e;
	}
};

// what a call that reads a region of one buffer reads (pipe_region.hip): the source container, its memory, the region
struct RegionSource {
	const char* what;
	int src;                 // oct::ST_F32 (processed float32) or PH_* (raw containers)
	bool packed;
	const void* mem;         // the buffer (device), or the caller's host buffer
	bool device;
	unsigned N, A, B, L;     // samplesPerLine, A-scans, B-scans, elements per row
	OctPipeStatsRegion r;
};

}  // namespace octimpl

struct octpipe {
	int device = 0;
	OctPipeAcquisitionParams acq{};
	OctPipeParams params{};
	int N = 0, A = 0, B = 0, log2n = 0, bytesPerSample = 0, sampleFormat = OCTPIPE_FORMAT_AUTO;
	size_t S = 0;  // samplesPerBuffer

	hipStream_t stream = nullptr;      // compute stream (all kernels of the chain)
	// the second compute lane (lanes.h): eligible buffers of odd slots run their whole chain here -- processDeviceRaw points `stream`
	// at it for the duration of the call -- with no event between the lanes; joinLanes orders the two before anything else runs
	hipStream_t lane1 = nullptr;
	hipEvent_t laneDone[2] = {nullptr, nullptr};  // [0] compute stream -> lane 1 waits, [1] lane 1 -> the compute stream waits
	bool lane1Pending = false;     // lane 1 holds work the compute stream has not been ordered behind
	bool streamForeign = false;    // the compute stream holds work other than eligible buffers that lane 1 has not been ordered behind
	bool streamExposed = false;    // octpipe_get_stream / octpipe_set_stream were called: lanes off for good
	bool groupMember = false;      // member of an octpipe_group: lanes off
	uint64_t laneOverlapped = 0, laneJoins = 0;  // octpipe_debug_lane_stats
	octimpl::LanePlanCache lanePlan;
	hipStream_t copyStream = nullptr;  // H2D of the raw buffer
	hipStream_t outStream = nullptr;   // result delivery: quantiser, both D2H copies, data callbacks (cu:1357-1386)
	hipEvent_t chainDone = nullptr;    // compute stream: the processed slot of the current buffer is complete
	std::vector<hipEvent_t> destRead;  // result stream: everything that reads processed destination d has finished
	std::vector<char> destReadPending;
	float* d_processedAlt = nullptr;   // second processed buffer (buffersPerVolume == 1 with float streaming, see octpipe.h)
	float* d_processedCur = nullptr;   // the one of the two the last buffer went to
	int altCur = 0;
	unsigned route = 0;                // OCTPIPE_ROUTE_* (octpipe_debug_set_route)
	int lastGrid = 0;
	unsigned lastPath = 0;  // OCTPIPE_PATH_* of the last image launch
	bool ownStream = true;
	hipEvent_t h2dDone[2] = {nullptr, nullptr};   // raw slot filled
	hipEvent_t slotFree[2] = {nullptr, nullptr};  // fused kernel finished reading the raw slot
	bool slotUsed[2] = {false, false};
	int slot = 0;
	int lastInputSlot = -1;  // raw slot of the last octpipe_process[_async] call

	void* d_raw[2] = {nullptr, nullptr};
	float* d_prepared = nullptr;   // S floats (uint8/uint32 input, Lanczos): lazily allocated
	float* d_processed = nullptr;  // S/2 * buffersPerVolume
	float* d_sinusTmp = nullptr;   // S/2, lazily
	void* d_output = nullptr;      // quantised output, lazily
	float4* d_lut = nullptr;
	float4* d_cubicW = nullptr;    // [N] Catmull-Rom tap weights of the resampling curve (oct_tap_weights_kernel, FusedArgs::cubicW)
	f2* d_twiddle = nullptr;
	f2* d_meanLine = nullptr;
	float* d_postBg = nullptr;
	float* d_bgTerm = nullptr;       // weight * d_postBg + offset for the removal inside the fused kernels' store
	unsigned bgVersion = 1, bgTermVersion = 0;  // d_postBg content / what d_bgTerm was computed from
	float bgTermWeight = 0.0f, bgTermOffset = 0.0f;
	float* d_sinusCurve = nullptr;
	uint32_t* d_sinusEnt = nullptr;  // work list of the correction inside the fused kernel's store (sinus_plan.h), [sinusM][4]; nullptr: no plan for this A
	unsigned sinusM = 0, sinusBlocksPerWave = 0;
	f2* d_spectrum = nullptr;  // FPN / debug scratch, lazily
	size_t spectrumLines = 0;
	float4* d_segs = nullptr;
	float* d_dispBscan = nullptr;
	float* d_dispEnFace = nullptr;
	uint64_t displaySig = 0;          // display settings of the last full extraction from the volume (0 = none yet)
	uint8_t* d_volumeView = nullptr;  // [N/2][B*buffersPerVolume][A] uint8, lazily (cu:914-941 into a plain buffer)
	bool libfft = false;       // no fused kernel for this length: gather -> hipFFT -> epilogue through a complex buffer (side_kernels.h)
	f2* d_cplx = nullptr;      // libfft: [A*B][N] complex
	void* fftLib = nullptr;
	bool fftLazy = false;      // libhipfft.so not bound yet: the length runs a kernel compiled for it; bound on the first launch that needs the library route
	int (*fftPlan1d)(void**, int, int, int) = nullptr;       // hipfftHandle is an opaque pointer
	int (*fftSetStream)(void*, hipStream_t) = nullptr;
	int (*fftExecC2C)(void*, void*, void*, int) = nullptr;
	int (*fftDestroy)(void*) = nullptr;
	void* fftPlan[2] = {nullptr, nullptr};
	size_t fftPlanBatch[2] = {0, 0};
	bool mixed = false;        // samplesPerLine == 1664: mixed-radix kernel (mixed1664.h); Bluestein stays for Lanczos
	float* d_lanczosW = nullptr;   // [N][16] Lanczos tap weights (uploaded with the LUT while that interpolation is selected)
	float4* d_lutPlain = nullptr;  // mixed: the LUT without the Bluestein chirp folded in
	f2* d_twMixed = nullptr;       // mixed: W_1664^{n2 k1}, [32][52]
	bool mixedN = false;           // a generic mixed-radix plan exists for this length (mixedn_kernel.h): every variant but Lanczos runs on it
	int mxnPasses = 0, mxnRadix[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	bool mixedStatic = false;      // ... and a static-plan instance of it (mixedn_static.h, one wave per A-scan) for this length
	oct::mxs::PlanDesc mxsPlan{};
	std::string rtcMessage;        // why this length has no static-plan kernel although a plan exists (hiprtc not loadable ...)
	std::string arch;              // gcnArchName of the device (key of the run-time compiled code objects)
	f2* d_twMixedStatic = nullptr;
	f2* d_twMixedN = nullptr;      // W_N^j, j < N
	f2* d_twTeam = nullptr;        // N = 4096: twiddles of the 16 x 16 x 16 plan of the one-A-scan-per-team kernel (team_kernel.h)
	bool bluestein = false;    // samplesPerLine is not a power of two: log2n = log2 of the padded length M
	f2* d_filter = nullptr;    // [M] Bluestein filter spectrum
	f2* d_outChirp = nullptr;  // [N] c[k] / M

	std::vector<float> resample, dispersion, window, phase;  // host copies (N each, phase 2N); zero like cu:1082-1085
	std::vector<float> h_postBg;                             // host shadow of the recorded background
	bool lutDirty = true;

	unsigned bufferNumberInVolume = 0;
	bool fpnDetermined = false;
	bool pinMean = false;
	bool forcePrepared = false;
	unsigned streamedBuffers = 0, streamingBufferNumber = 0, floatStreamingBufferNumber = 0;

	void* h_buffer[2] = {nullptr, nullptr};
	bool h_bufferRegistered[2] = {false, false};
	void* h_stream[2] = {nullptr, nullptr};
	void* h_floatStream[2] = {nullptr, nullptr};
	bool floatStreamingRegistered = false;
	size_t streamBytes = 0, floatStreamBytes = 0;

	octpipe_data_callback onStreaming = nullptr, onFloatStreaming = nullptr;
	octpipe_event_callback onBackground = nullptr;
	void* user = nullptr;

	bool timing = false;
	unsigned timingStride = 1, timingCounter = 0;  // every timingStride-th launch of the dominant kernel is timed
	std::vector<octimpl::TimedLaunch> timed;
	double timedMs = 0.0;
	unsigned timedLaunches = 0;

	octimpl::SweepScratch sweep;  // octpipe_dispersion_scores / octpipe_estimate_dispersion
	octimpl::PhaseState phaseState;  // octpipe_phase_* / octpipe_extract_resample_curve
	octimpl::StatsState statsState;  // octpipe_processed_statistics / octpipe_raw_statistics
	octimpl::PeakState peakState;    // octpipe_peak_analysis
	octimpl::RenderState renderState;  // octpipe_render_volume
	octimpl::SurfaceState surfaceState;  // octpipe_surface_detect / _smooth / _enface, octpipe_flatten
	octimpl::AngioState angioState;      // octpipe_angiogram / _enface, with and without _registered; octpipe_repeat_shifts
	octimpl::AttenuationState attenuationState;  // octpipe_attenuation / _enface
	octimpl::BoundaryState boundaryState;        // octpipe_trace_boundary
};

namespace octimpl {

// octpipe_api.hip
int uploadSync(octpipe* h, void* dst, const void* src, size_t bytes);
int downloadSync(octpipe* h, void* dst, const void* src, size_t bytes);
int ensure(octpipe* h, void** p, size_t bytes);   // lazily allocated, zero-filled device buffer
// how every entry point but octpipe_process_device starts: the device, and the compute stream ordered behind the second lane (joinLanes)
int setDevice(octpipe* h);
// the compute stream waits for what lane 1 holds (one event pair, only if it holds any); from here on the caller's work on the compute
// stream counts as foreign to the lanes: lane 1 waits for it before its next buffer
int joinLanes(octpipe* h);
size_t rawBytes(const octpipe* h);
int launchPrepare(octpipe* h, const void* d_raw, float* d_out, size_t count, int rollingW);
// oct_lib_gather_kernel over `lines` prepared rows (k-linearisation x window x the LUT's phasor, complex output)
int launchGatherRows(octpipe* h, const float* rows, f2* out, const float4* lut, size_t lines, int rs, const float* lanczosW);
// pipe_calib.hip
float4 lutEntry(const octpipe* h, int j, bool unitPhasor);
void lanczosWeights(const std::vector<float4>& lut, std::vector<float>& w);
int fusedTwiddles(int log2n, std::vector<f2>& tw);
int uploadLut(octpipe* h);
int uploadTwiddles(octpipe* h);
int uploadBluesteinTables(octpipe* h);
int bindFftLibrary(octpipe* h);
int uploadTeamTables(octpipe* h);
int uploadMixedNTable(octpipe* h);
int uploadMixedTables(octpipe* h);
// pipe_dispersion.hip
const f2* planTwiddles(octpipe* h, int* rc);  // the handle's Plan<LOG2N> twiddle tables on the device (N = 256 ... 4096)
// pipe_region.hip
// j.r = *r after checking that the region is non-empty and inside [B][A][j.L] (error messages name the field)
int checkRegion(octpipe* h, RegionSource& j, const OctPipeStatsRegion* r);
// the processed source: data (host or device), or the handle's volume at slot j.r.buffer (0xFFFFFFFF: the slot the last call wrote)
int resolveProcessed(octpipe* h, RegionSource& j, const float* data, int dataIsDevice);
// bytes of elements [e0, e1) of a buffer in the source's container, and the byte offset of element e0 (packed: from the sample pair)
size_t regionElemBytes(const RegionSource& j, uint64_t e0, uint64_t e1, size_t* off);
// region rows [r0, r1) (r = b * ascanCount + a) of the host source copied on the compute stream to stage rows 0 .., row by row
// (parity: packed rows of odd length, each B-scan run at its own sample parity 4 elements apart, image_stats.h StatsArgs)
int stageRegionRows(octpipe* h, const RegionSource& j, char* stage, unsigned r0, unsigned r1, bool parity);
// what the surface views and the angiography share besides: how many bytes of a host source's rows, or of a volume result on its way to
// the host, one slice holds; the thickest en face slab (OctPipeSurfaceEnfaceSettings); a HIP error as the call's own
constexpr size_t kSliceBytes = 64ull << 20;
constexpr unsigned kMaxThickness = 4096;
inline int deviceError(const RegionSource& j, hipError_t e) { return fail(OCTPIPE_ERR_DEVICE, std::string(j.what) + ": " + hipGetErrorString(e)); }
// a surface the kernels can read: the caller's device memory, or a whole copy of the caller's host memory in `slot` of the call's scratch
int surfaceIn(octpipe* h, const RegionSource& j, DeviceScratch& s, int slot, const int32_t* surface, int isDevice, size_t entries, const int32_t** dev);
// where the kernels write a result of `bytes`: the caller's device memory, or `slot` of the call's scratch for a host result
int resultOut(octpipe* h, DeviceScratch& s, int slot, void* out, int isDevice, size_t bytes, void** dev);
// the end of a call: a host result (hostOut; `bytes` of it still at dev, 0 where it has left in slices) comes home and the call waits for it;
// a timed call waits in any case
int finish(octpipe* h, const RegionSource& j, const StreamTimer& timer, double* kernelMs, void* hostOut, const void* dev, size_t bytes);
// pipe_display.hip
uint64_t displaySignature(const OctPipeParams& p);
int updateDisplay(octpipe* h, bool bscan, unsigned frameNrB, unsigned framesB, int fnB, bool enface, unsigned frameNrE, unsigned framesE, int fnE,
                  bool currentBufferOnly = false);

// slot `slot` of a call's scratch with room for `bytes`: nothing if it is large enough; otherwise it waits for what the compute stream
// may still read there, frees and allocates
inline int grow(octpipe* h, DeviceScratch& s, int slot, size_t bytes) {
	if (s.bytes[slot] >= bytes) return OCTPIPE_OK;
	if (s.p[slot]) {
		HIP_TRY(hipStreamSynchronize(h->stream));
		HIP_TRY(hipFree(s.p[slot]));
		s.p[slot] = nullptr;
		s.bytes[slot] = 0;
	}
	HIP_TRY(hipMalloc(&s.p[slot], bytes));
	s.bytes[slot] = bytes;
	return OCTPIPE_OK;
}
inline void release(DeviceScratch& s) {
	for (int i = 0; i < DeviceScratch::SLOTS; ++i) {
		if (s.p[i]) hipFree(s.p[i]);
		s.p[i] = nullptr;
		s.bytes[i] = 0;
	}
}

// how every analysis call starts: null handle, inside a callback, `check` (a test of the handle that comes before any device work), the device
inline int enterCall(octpipe* h, const char* what, int (*check)(const octpipe*) = nullptr) {
	if (!h) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, std::string(what) + ": null handle");
	if (t_inCallback) return fail(OCTPIPE_ERR_IN_CALLBACK, std::string(what) + " from inside a pipeline callback");
	if (check)
		if (int rc = check(h)) return rc;
	return setDevice(h);
}

}  // namespace octimpl
