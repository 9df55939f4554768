// pipe_surface.hip -- surface views (include/octpipe.h "surface views"): surface detection, smoothing, surface-following en face
// slabs and flattening of the float32 processed volume (surface_views.h).
//
//   octpipe_surface_detect   oct_surface_detect_kernel       region rows -> int32 surface
//   octpipe_surface_smooth   oct_surface_smooth_kernel<R>    int32 map -> int32 map
//   octpipe_surface_enface   oct_surface_enface_kernel<FN>   region rows + surface -> float32 image
//   octpipe_flatten          oct_flatten_kernel<LOADS>       region rows + surface -> float32 volume
// The region and the processed source are pipe_region.hip's (shared with the image statistics and the peak analysis).  The three
// calls that read the volume go over the region's rows in slices: one slice for a device source and a device result; otherwise as many
// rows as kSliceBytes of staged source rows (host source) and of flattened rows on their way to the host (host result) allow.  A host
// surface is uploaded whole, a host surface or image result is downloaded whole (4 bytes per A-scan).  Everything runs on the handle's
// compute stream behind what is already enqueued there and touches nothing the processing chain reads or writes; the scratch belongs to
// the handle (SurfaceState, released in octpipe_destroy).
#include <algorithm>

#include "pipe_internal.h"
#include "surface_views.h"

namespace oct {
hipError_t launch_surface_detect(const SurfArgs& a, float threshold, unsigned run, int32_t* out, hipStream_t s);
hipError_t launch_surface_smooth(const int32_t* in, unsigned rows, unsigned cols, unsigned radius, int32_t* out, hipStream_t s);
hipError_t launch_surface_enface(int function, const EnfaceArgs& a, hipStream_t s);
hipError_t launch_flatten(unsigned loads, const FlattenArgs& a, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr unsigned kMaxRun = 64, kMaxRadius = 3, kMaxOutDepth = 8192;  // (kSliceBytes, kMaxThickness, deviceError: pipe_internal.h)
constexpr unsigned long long kMaxMap = 1ull << 28;
constexpr unsigned kFlattenLoads = 1;  // the form octpipe_flatten uses

// the source of one call and how its rows are walked
struct Job : RegionSource {
	unsigned rows;
};

// entry checks, region and source of the three calls that read the volume
int open(octpipe* h, Job& j, const char* what, const float* data, int dataIsDevice, const OctPipeStatsRegion* r) {
	if (data && r->buffer != 0 && r->buffer != 0xFFFFFFFFu)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, std::string(what) + ": buffer must be 0 or 0xFFFFFFFF when data is given");
	int rc = enterCall(h, what);
	if (rc) return rc;
	j.what = what;
	j.src = oct::ST_F32;
	j.L = (unsigned)(h->N / 2);
	if ((rc = checkRegion(h, j, r))) return rc;
	j.rows = j.r.bscanCount * j.r.ascanCount;  // <= A * B
	return resolveProcessed(h, j, data, dataIsDevice);
}

oct::SurfArgs sourceArgs(const Job& j) {
	oct::SurfArgs a{};
	a.A = j.A;
	a.fb = j.r.firstBscan;
	a.fa = j.r.firstAscan;
	a.ac = j.r.ascanCount;
	a.L = j.L;
	a.s0 = j.r.firstSample;
	a.cnt = j.r.sampleCount;
	return a;
}

// the region's rows in slices of at most `sliceRows`: a host source's rows staged, then launch(args of the slice)
template <class Launch>
int overRows(octpipe* h, const Job& j, unsigned sliceRows, Launch launch) {
	int rc;
	oct::SurfArgs a = sourceArgs(j);
	const size_t rowBytes = sizeof(float) * (size_t)j.L;
	char* stage = nullptr;
	if (!j.device) {
		sliceRows = (unsigned)std::min<size_t>(sliceRows, std::max<size_t>(1, kSliceBytes / rowBytes));
		if ((rc = grow(h, h->surfaceState, SurfaceState::STAGE, (size_t)sliceRows * rowBytes))) return rc;
		stage = h->surfaceState.as<char>(SurfaceState::STAGE);
	}
	for (unsigned r0 = 0; r0 < j.rows; r0 += sliceRows) {
		const unsigned r1 = (unsigned)std::min<unsigned long long>(j.rows, (unsigned long long)r0 + sliceRows);
		if (!j.device && (rc = stageRegionRows(h, j, stage, r0, r1, false))) return rc;
		a.src = j.device ? static_cast<const float*>(j.mem) : reinterpret_cast<const float*>(stage);
		a.staged = j.device ? 0 : 1;
		a.r0 = r0;
		a.rFirst = r0;
		a.rCount = r1 - r0;
		if ((rc = launch(a))) return rc;
	}
	return OCTPIPE_OK;
}

int detectEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeSurfaceDetectSettings* s, int32_t* surface,
                int surfaceIsDevice, double* kernelMs) {
	const std::string w("surface detect");
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!surface) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL");
	const OctPipeSurfaceDetectSettings st = *s;
	if (std::isnan(st.threshold)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": threshold is NaN");
	if (st.run < 1 || st.run > kMaxRun) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": run must lie in [1, 64]");
	Job j{};
	int rc = open(h, j, "surface detect", data, dataIsDevice, r);
	if (rc) return rc;
	if (st.run > j.r.sampleCount)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": run = " + std::to_string(st.run) + " must not exceed the region's sampleCount = " +
		                                              std::to_string(j.r.sampleCount));
	const size_t bytes = sizeof(int32_t) * (size_t)j.rows;
	void* dOut = nullptr;
	if ((rc = resultOut(h, h->surfaceState, SurfaceState::SURF_OUT, surface, surfaceIsDevice, bytes, &dOut))) return rc;
	StreamTimer timer(kernelMs != nullptr, j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	rc = overRows(h, j, j.rows, [&](const oct::SurfArgs& a) -> int {
		HIP_TRY(oct::launch_surface_detect(a, st.threshold, st.run, static_cast<int32_t*>(dOut), h->stream));
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	return finish(h, j, timer, kernelMs, surfaceIsDevice ? nullptr : surface, dOut, bytes);
}

int smoothEntry(octpipe* h, const int32_t* surface, int surfaceIsDevice, uint32_t rows, uint32_t cols, uint32_t radius, int32_t* out, int outIsDevice,
                double* kernelMs) {
	const std::string w("surface smooth");
	if (!surface) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	if (out == surface) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out must not be the input surface");
	if (radius > kMaxRadius) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": radius must lie in [0, 3]");
	if (rows < 1 || cols < 1 || (unsigned long long)rows * cols > kMaxMap)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": rows / cols must be at least 1 and rows * cols at most 2^28");
	int rc = enterCall(h, "surface smooth");
	if (rc) return rc;
	Job j{};
	j.what = "surface smooth";
	const size_t entries = (size_t)rows * cols, bytes = sizeof(int32_t) * entries;
	void* dOut = nullptr;
	if ((rc = resultOut(h, h->surfaceState, SurfaceState::SURF_OUT, out, outIsDevice, bytes, &dOut))) return rc;
	StreamTimer timer(kernelMs != nullptr, j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	const int32_t* dIn = nullptr;
	if ((rc = surfaceIn(h, j, h->surfaceState, SurfaceState::SURF_IN, surface, surfaceIsDevice, entries, &dIn))) return rc;
	HIP_TRY(oct::launch_surface_smooth(dIn, rows, cols, radius, static_cast<int32_t*>(dOut), h->stream));
	if ((rc = timer.end(h->stream))) return rc;
	return finish(h, j, timer, kernelMs, outIsDevice ? nullptr : out, dOut, bytes);
}

int enfaceEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface, int surfaceIsDevice,
                const OctPipeSurfaceEnfaceSettings* s, float* out, int outIsDevice, double* kernelMs) {
	const std::string w("surface enface");
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!surface) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	const OctPipeSurfaceEnfaceSettings st = *s;
	if (st.thickness < 1 || st.thickness > kMaxThickness) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": thickness must lie in [1, 4096]");
	if (st.function != 0 && st.function != 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": function must be 0 (averaging) or 1 (MIP)");
	Job j{};
	int rc = open(h, j, "surface enface", data, dataIsDevice, r);
	if (rc) return rc;
	const size_t bytes = sizeof(float) * (size_t)j.rows;
	void* dOut = nullptr;
	if ((rc = resultOut(h, h->surfaceState, SurfaceState::OUT, out, outIsDevice, bytes, &dOut))) return rc;
	StreamTimer timer(kernelMs != nullptr, j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::EnfaceArgs e{};
	if ((rc = surfaceIn(h, j, h->surfaceState, SurfaceState::SURF_IN, surface, surfaceIsDevice, j.rows, &e.surface))) return rc;
	e.offset = st.offset;
	e.thickness = st.thickness;
	e.fill = st.fill;
	e.out = static_cast<float*>(dOut);
	rc = overRows(h, j, j.rows, [&](const oct::SurfArgs& a) -> int {
		e.g = a;
		HIP_TRY(oct::launch_surface_enface(st.function, e, h->stream));
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	return finish(h, j, timer, kernelMs, outIsDevice ? nullptr : out, dOut, bytes);
}

int flattenEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface, int surfaceIsDevice,
                 const OctPipeFlattenSettings* s, float* out, int outIsDevice, unsigned loads, double* kernelMs) {
	const std::string w("flatten");
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!surface) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	const OctPipeFlattenSettings st = *s;
	if (st.outDepth < 1 || st.outDepth > kMaxOutDepth) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": outDepth must lie in [1, 8192]");
	if (loads > 2) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": loads must be 0, 1 or 2");
	if (loads == 0) loads = kFlattenLoads;
	Job j{};
	int rc = open(h, j, "flatten", data, dataIsDevice, r);
	if (rc) return rc;
	const size_t outRowBytes = sizeof(float) * (size_t)st.outDepth;
	// a host result leaves in slices of whole rows through the OUT slot
	unsigned sliceRows = j.rows;
	if (!outIsDevice) {
		sliceRows = (unsigned)std::min<size_t>(j.rows, std::max<size_t>(1, kSliceBytes / outRowBytes));
		if ((rc = grow(h, h->surfaceState, SurfaceState::OUT, (size_t)sliceRows * outRowBytes))) return rc;
	}
	StreamTimer timer(kernelMs != nullptr, j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::FlattenArgs f{};
	if ((rc = surfaceIn(h, j, h->surfaceState, SurfaceState::SURF_IN, surface, surfaceIsDevice, j.rows, &f.surface))) return rc;
	f.anchor = st.anchor;
	f.outDepth = st.outDepth;
	f.fill = st.fill;
	rc = overRows(h, j, sliceRows, [&](const oct::SurfArgs& a) -> int {
		f.g = a;
		f.out = outIsDevice ? out : h->surfaceState.as<float>(SurfaceState::OUT);
		f.o0 = outIsDevice ? 0 : a.rFirst;
		HIP_TRY(oct::launch_flatten(loads, f, h->stream));
		if (!outIsDevice)
			HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(out) + (size_t)a.rFirst * outRowBytes, f.out, (size_t)a.rCount * outRowBytes,
			                       hipMemcpyDeviceToHost, h->stream));
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	return finish(h, j, timer, kernelMs, outIsDevice ? nullptr : out, nullptr, 0);  // (the rows have left slice by slice)
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_surface_detect(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeSurfaceDetectSettings* s,
                           int32_t* surface, int surfaceIsDevice) {
	return detectEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, nullptr);
}

int octpipe_surface_smooth(octpipe_t* h, const int32_t* surface, int surfaceIsDevice, uint32_t rows, uint32_t cols, uint32_t radius, int32_t* out,
                           int outIsDevice) {
	return smoothEntry(h, surface, surfaceIsDevice, rows, cols, radius, out, outIsDevice, nullptr);
}

int octpipe_surface_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface, int surfaceIsDevice,
                           const OctPipeSurfaceEnfaceSettings* s, float* out, int outIsDevice) {
	return enfaceEntry(h, data, dataIsDevice, r, surface, surfaceIsDevice, s, out, outIsDevice, nullptr);
}

int octpipe_flatten(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface, int surfaceIsDevice,
                    const OctPipeFlattenSettings* s, float* out, int outIsDevice) {
	return flattenEntry(h, data, dataIsDevice, r, surface, surfaceIsDevice, s, out, outIsDevice, 0, nullptr);
}

int octpipe_debug_surface_detect(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeSurfaceDetectSettings* s,
                                 int32_t* surface, int surfaceIsDevice, double* kernelMs) {
	return detectEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, kernelMs);
}

int octpipe_debug_surface_smooth(octpipe_t* h, const int32_t* surface, int surfaceIsDevice, uint32_t rows, uint32_t cols, uint32_t radius, int32_t* out,
                                 int outIsDevice, double* kernelMs) {
	return smoothEntry(h, surface, surfaceIsDevice, rows, cols, radius, out, outIsDevice, kernelMs);
}

int octpipe_debug_surface_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface,
                                 int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* s, float* out, int outIsDevice, double* kernelMs) {
	return enfaceEntry(h, data, dataIsDevice, r, surface, surfaceIsDevice, s, out, outIsDevice, kernelMs);
}

int octpipe_debug_flatten(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* surface, int surfaceIsDevice,
                          const OctPipeFlattenSettings* s, float* out, int outIsDevice, unsigned loads, double* kernelMs) {
	return flattenEntry(h, data, dataIsDevice, r, surface, surfaceIsDevice, s, out, outIsDevice, loads, kernelMs);
}

}  // extern "C"
