// pipe_attenuation.hip -- depth-resolved attenuation (include/octpipe.h "attenuation"): the attenuation coefficient of every bin of a region
// of the float32 processed volume, its en face projection under a surface, and the float64 sums below every bin (attenuation.h).
//
//   octpipe_attenuation                 oct_atten_volume_kernel<SCALE, GAIN, false>   region rows -> float32 coefficient volume
//   octpipe_attenuation_enface          oct_atten_enface_kernel<SCALE, GAIN, FN>      region rows (+ surface) -> float32 image
//   octpipe_debug_attenuation_sums      oct_atten_volume_kernel<SCALE, GAIN, true>    region rows -> float64 sums below every bin
// The region and the processed source are pipe_region.hip's.  Every call goes over the region's rows in slices: one slice for a device
// source and a device result; otherwise as many rows as kSliceBytes of staged source rows (host source) and of result rows on their way
// to the host (host result of a volume call) allow.  A host gain table and a host surface are uploaded whole, a host image is downloaded
// whole.  Everything runs on the handle's compute stream behind what is already enqueued there and touches nothing the processing chain
// reads or writes; the scratch belongs to the handle (AttenuationState, released in octpipe_destroy).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "attenuation.h"
#include "pipe_internal.h"

namespace oct {
hipError_t launch_atten_volume(int scale, bool sums, const AttenVolumeArgs& a, hipStream_t s);
hipError_t launch_atten_enface(int scale, int function, const AttenEnfaceArgs& a, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

// the source of one call and how its rows are walked
struct Job : RegionSource {
	unsigned rows;
};

// the checks that need no handle; every message names the field
int checkArguments(const std::string& w, const float* data, const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s, const float* gain,
                   int gainIsDevice, const void* out) {
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	if (s->scale < 0 || s->scale > 2) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": scale must be 0 (intensity), 1 (amplitude) or 2 (log2 of an intensity)");
	if (!std::isfinite(s->pixelSize) || !(s->pixelSize > 0.0f)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": pixelSize must be finite and > 0");
	if (std::isnan(s->noise)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": noise is NaN");
	if (std::isnan(s->tail) || s->tail < 0.0f) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": tail must be >= 0 and not NaN");
	if (!std::isfinite(s->mapScale)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": mapScale must be finite");
	if (!std::isfinite(s->mapOffset)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": mapOffset must be finite");
	if (s->reserved != 0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": reserved must be 0");
	if (!gain && gainIsDevice) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": depthGain is NULL but gainIsDevice is set");
	if (data && r->buffer != 0 && r->buffer != 0xFFFFFFFFu)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": buffer must be 0 or 0xFFFFFFFF when data is given");
	return OCTPIPE_OK;
}

// entry, region and source
int open(octpipe* h, Job& j, const char* what, const float* data, int dataIsDevice, const OctPipeStatsRegion* r) {
	int rc = enterCall(h, what);
	if (rc) return rc;
	j.what = what;
	j.src = oct::ST_F32;
	j.L = (unsigned)(h->N / 2);
	if ((rc = checkRegion(h, j, r))) return rc;
	j.rows = j.r.bscanCount * j.r.ascanCount;  // <= A * B
	return resolveProcessed(h, j, data, dataIsDevice);
}

// what the kernels need besides the rows: the settings in float64, the gain table on the device (a host table is uploaded whole)
int settingsArgs(octpipe* h, const Job& j, const OctPipeAttenuationSettings& s, const float* gain, int gainIsDevice, oct::AttenArgs& n) {
	n.a = s.mapScale;
	n.b = s.mapOffset;
	n.noise = (double)s.noise;
	n.tail = (double)s.tail;
	n.twoDelta = 2.0 * (double)s.pixelSize;
	std::memcpy(&n.undefined, &s.undefined, sizeof(n.undefined));
	n.gain = gain;
	if (gain && !gainIsDevice) {
		const size_t bytes = sizeof(float) * (size_t)j.r.sampleCount;
		if (int rc = grow(h, h->attenuationState, AttenuationState::GAIN_IN, bytes)) return rc;
		float* d = h->attenuationState.as<float>(AttenuationState::GAIN_IN);
		if (hipError_t e = hipMemcpyAsync(d, gain, bytes, hipMemcpyHostToDevice, h->stream); e != hipSuccess) return deviceError(j, e);
		n.gain = d;
	}
	return OCTPIPE_OK;
}

// the region's rows in slices of at most `sliceRows`: a host source's rows staged, then launch(n with the slice's rows)
template <class Launch>
int overRows(octpipe* h, const Job& j, oct::AttenArgs& n, unsigned sliceRows, Launch launch) {
	int rc;
	oct::SurfArgs& a = n.g;
	a.A = j.A;
	a.fb = j.r.firstBscan;
	a.fa = j.r.firstAscan;
	a.ac = j.r.ascanCount;
	a.L = j.L;
	a.s0 = j.r.firstSample;
	a.cnt = j.r.sampleCount;
	const size_t rowBytes = sizeof(float) * (size_t)j.L;
	char* stage = nullptr;
	if (!j.device) {
		sliceRows = (unsigned)std::min<size_t>(sliceRows, std::max<size_t>(1, kSliceBytes / rowBytes));
		if ((rc = grow(h, h->attenuationState, AttenuationState::STAGE, (size_t)sliceRows * rowBytes))) return rc;
		stage = h->attenuationState.as<char>(AttenuationState::STAGE);
	}
	for (unsigned r0 = 0; r0 < j.rows; r0 += sliceRows) {
		const unsigned r1 = (unsigned)std::min<unsigned long long>(j.rows, (unsigned long long)r0 + sliceRows);
		if (!j.device && (rc = stageRegionRows(h, j, stage, r0, r1, false))) return rc;
		a.src = j.device ? static_cast<const float*>(j.mem) : reinterpret_cast<const float*>(stage);
		a.staged = j.device ? 0 : 1;
		a.r0 = r0;
		a.rFirst = r0;
		a.rCount = r1 - r0;
		if ((rc = launch())) return rc;
	}
	return OCTPIPE_OK;
}

// the volume call (out: float32 mu32) and, with `sums`, the debug entry that writes the float64 sums below every bin instead
int volumeEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s, const float* gain,
                int gainIsDevice, void* out, int outIsDevice, bool sums, double* kernelMs) {
	const char* what = sums ? "attenuation sums" : "attenuation";
	int rc = checkArguments(what, data, r, s, gain, gainIsDevice, out);
	if (rc) return rc;
	const OctPipeAttenuationSettings st = *s;
	Job j{};
	if ((rc = open(h, j, what, data, dataIsDevice, r))) return rc;
	AttenuationState& mem = h->attenuationState;
	const size_t outRowBytes = (sums ? sizeof(double) : sizeof(float)) * (size_t)j.r.sampleCount;
	// a host result leaves in slices of whole rows through the OUT slot
	unsigned sliceRows = j.rows;
	if (!outIsDevice) {
		sliceRows = (unsigned)std::min<size_t>(j.rows, std::max<size_t>(1, kSliceBytes / outRowBytes));
		if ((rc = grow(h, mem, AttenuationState::OUT, (size_t)sliceRows * outRowBytes))) return rc;
	}
	StreamTimer timer(kernelMs != nullptr, what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::AttenVolumeArgs v{};
	if ((rc = settingsArgs(h, j, st, gain, gainIsDevice, v.n))) return rc;
	rc = overRows(h, j, v.n, sliceRows, [&]() -> int {
		v.out = outIsDevice ? out : mem.p[AttenuationState::OUT];
		v.o0 = outIsDevice ? 0 : v.n.g.rFirst;
		HIP_TRY(oct::launch_atten_volume(st.scale, sums, v, h->stream));
		if (!outIsDevice)
			HIP_TRY(hipMemcpyAsync(static_cast<char*>(out) + (size_t)v.n.g.rFirst * outRowBytes, v.out, (size_t)v.n.g.rCount * outRowBytes,
			                       hipMemcpyDeviceToHost, h->stream));
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	return finish(h, j, timer, kernelMs, outIsDevice ? nullptr : out, nullptr, 0);  // (the rows have left slice by slice)
}

int enfaceEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s, const float* gain,
                int gainIsDevice, const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice,
                double* kernelMs) {
	const char* what = "attenuation enface";
	const std::string w(what);
	int rc = checkArguments(w, data, r, s, gain, gainIsDevice, out);
	if (rc) return rc;
	if (!slab) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": slab settings is NULL");
	if (!surface && surfaceIsDevice) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL but surfaceIsDevice is set");
	const OctPipeAttenuationSettings st = *s;
	const OctPipeSurfaceEnfaceSettings sl = *slab;
	if (sl.thickness < 1 || sl.thickness > kMaxThickness) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": thickness must lie in [1, 4096]");
	if (sl.function != 0 && sl.function != 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": function must be 0 (averaging) or 1 (MIP)");
	Job j{};
	if ((rc = open(h, j, what, data, dataIsDevice, r))) return rc;
	AttenuationState& mem = h->attenuationState;
	const size_t bytes = sizeof(float) * (size_t)j.rows;
	void* dOut = nullptr;
	if ((rc = resultOut(h, mem, AttenuationState::OUT, out, outIsDevice, bytes, &dOut))) return rc;
	StreamTimer timer(kernelMs != nullptr, what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::AttenEnfaceArgs e{};
	if ((rc = settingsArgs(h, j, st, gain, gainIsDevice, e.n))) return rc;
	// (no surface: firstSample everywhere)
	if (surface && (rc = surfaceIn(h, j, mem, AttenuationState::SURF_IN, surface, surfaceIsDevice, j.rows, &e.surface))) return rc;
	e.offset = sl.offset;
	e.thickness = sl.thickness;
	e.fill = sl.fill;
	e.cap = (std::min(sl.thickness, j.r.sampleCount) + 3u) & ~3u;  // whole quads; <= kMaxThickness: 16 KiB of LDS per wave at the most
	e.out = static_cast<float*>(dOut);
	rc = overRows(h, j, e.n, j.rows, [&]() -> int {
		HIP_TRY(oct::launch_atten_enface(st.scale, sl.function, e, h->stream));
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	return finish(h, j, timer, kernelMs, outIsDevice ? nullptr : out, dOut, bytes);
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_attenuation(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s,
                        const float* depthGain, int gainIsDevice, float* out, int outIsDevice) {
	return volumeEntry(h, data, dataIsDevice, r, s, depthGain, gainIsDevice, out, outIsDevice, false, nullptr);
}

int octpipe_attenuation_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s,
                               const float* depthGain, int gainIsDevice, const int32_t* surface, int surfaceIsDevice,
                               const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice) {
	return enfaceEntry(h, data, dataIsDevice, r, s, depthGain, gainIsDevice, surface, surfaceIsDevice, slab, out, outIsDevice, nullptr);
}

int octpipe_debug_attenuation(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAttenuationSettings* s,
                              const float* depthGain, int gainIsDevice, float* out, int outIsDevice, double* kernelMs) {
	return volumeEntry(h, data, dataIsDevice, r, s, depthGain, gainIsDevice, out, outIsDevice, false, kernelMs);
}

int octpipe_debug_attenuation_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                     const OctPipeAttenuationSettings* s, const float* depthGain, int gainIsDevice, const int32_t* surface,
                                     int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice, double* kernelMs) {
	return enfaceEntry(h, data, dataIsDevice, r, s, depthGain, gainIsDevice, surface, surfaceIsDevice, slab, out, outIsDevice, kernelMs);
}

int octpipe_debug_attenuation_sums(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                   const OctPipeAttenuationSettings* s, const float* depthGain, int gainIsDevice, double* out, int outIsDevice) {
	return volumeEntry(h, data, dataIsDevice, r, s, depthGain, gainIsDevice, out, outIsDevice, true, nullptr);
}

}  // extern "C"
