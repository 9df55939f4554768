// pipe_angio.hip -- OCT angiography (include/octpipe.h "angiography"): the contrast between the repeated B-scans of every slow-axis
// position of the float32 processed volume (angiogram.h).
//
//   octpipe_angiogram          oct_angio_volume_kernel<METHOD, M>       region rows -> float32 contrast volume (and mean volume)
//   octpipe_angiogram_enface   oct_angio_enface_kernel<METHOD, FN, M>   region rows (+ surface) -> float32 image (thin slabs: its team form)
// The region and the processed source are pipe_region.hip's.  Both calls go over the region's positions in slices: one slice for a device
// source and a device result; otherwise as many whole positions (at least one) as kSliceBytes of staged source rows (host source) and of
// contrast rows on their way to the host (host result of the volume call) allow.  A host surface is uploaded whole, a host image is
// downloaded whole.  Everything runs on the handle's compute stream behind what is already enqueued there and touches nothing the
// processing chain reads or writes; the scratch belongs to the handle (AngioState, released in octpipe_destroy).
#include <algorithm>

#include "angiogram.h"
#include "pipe_internal.h"

namespace oct {
hipError_t launch_angio_volume(int method, const AngioVolumeArgs& a, hipStream_t s);
hipError_t launch_angio_enface(int method, int function, bool team, const AngioEnfaceArgs& a, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr unsigned kMinRepeats = oct::ANGIO_MIN_REPEATS, kMaxRepeats = oct::ANGIO_MAX_REPEATS;  // (kSliceBytes, kMaxThickness: pipe_internal.h)
// the thickest slab octpipe_angiogram_enface gives to the kernel's team form: all it takes (faster than the full-wave form at 16 and at 64
// bins in the same-run comparison of profiles/angio_bench.json)
constexpr unsigned kTeamMaxThickness = oct::ANGIO_TEAM_BINS;

// the source of one call and how its positions are walked
struct Job : RegionSource {
	unsigned M, P;     // repeats, positions
	unsigned rows;     // output rows: P * ascanCount
	double* kernelMs;
};

// the checks of both calls that need no handle
int checkArguments(const std::string& w, const float* data, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, const void* out) {
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	if (s->repeats < kMinRepeats || s->repeats > kMaxRepeats) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": repeats must lie in [2, 8]");
	if (r->bscanCount % s->repeats)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": repeats = " + std::to_string(s->repeats) + " must divide the region's bscanCount = " +
		                                              std::to_string(r->bscanCount));
	if (s->method < 0 || s->method > 2)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": method must be 0 (speckle variance), 1 (amplitude decorrelation) or 2 (differential)");
	if (s->mask && std::isnan(s->threshold)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": threshold is NaN");
	if (data && r->buffer != 0 && r->buffer != 0xFFFFFFFFu)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": buffer must be 0 or 0xFFFFFFFF when data is given");
	return OCTPIPE_OK;
}

// entry, region and source
int open(octpipe* h, Job& j, const char* what, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings& s,
         double* kernelMs) {
	int rc = enterCall(h, what);
	if (rc) return rc;
	j.what = what;
	j.src = oct::ST_F32;
	j.L = (unsigned)(h->N / 2);
	j.kernelMs = kernelMs;
	if ((rc = checkRegion(h, j, r))) return rc;
	j.M = s.repeats;
	j.P = j.r.bscanCount / j.M;
	j.rows = j.P * j.r.ascanCount;  // <= A * B
	return resolveProcessed(h, j, data, dataIsDevice);
}

oct::AngioArgs sourceArgs(const Job& j, const OctPipeAngioSettings& s) {
	oct::AngioArgs n{};
	n.g.A = j.A;
	n.g.fb = j.r.firstBscan;
	n.g.fa = j.r.firstAscan;
	n.g.ac = j.r.ascanCount;
	n.g.L = j.L;
	n.g.s0 = j.r.firstSample;
	n.g.cnt = j.r.sampleCount;
	n.M = s.repeats;
	n.mask = s.mask != 0;
	n.threshold = s.threshold;
	n.masked = s.masked;
	return n;
}

// the region's positions in slices of at most `slicePos`: a host source's rows staged, then launch(args of the slice, first position, positions)
template <class Launch>
int overPositions(octpipe* h, const Job& j, const OctPipeAngioSettings& s, unsigned slicePos, Launch launch) {
	int rc;
	oct::AngioArgs n = sourceArgs(j, s);
	const unsigned ac = j.r.ascanCount;
	const size_t posBytes = sizeof(float) * (size_t)j.L * j.M * ac;  // the source rows of one position
	char* stage = nullptr;
	if (!j.device) {
		slicePos = (unsigned)std::min<size_t>(slicePos, std::max<size_t>(1, kSliceBytes / posBytes));
		if ((rc = grow(h, h->angioState, AngioState::STAGE, (size_t)slicePos * posBytes))) return rc;
		stage = h->angioState.as<char>(AngioState::STAGE);
	}
	for (unsigned p0 = 0; p0 < j.P; p0 += slicePos) {
		const unsigned p1 = (unsigned)std::min<unsigned long long>(j.P, (unsigned long long)p0 + slicePos);
		const unsigned r0 = p0 * j.M * ac, r1 = p1 * j.M * ac;  // region rows, <= A * B
		if (!j.device && (rc = stageRegionRows(h, j, stage, r0, r1, false))) return rc;
		n.g.src = j.device ? static_cast<const float*>(j.mem) : reinterpret_cast<const float*>(stage);
		n.g.staged = j.device ? 0 : 1;
		n.g.r0 = r0;
		n.g.rFirst = p0 * ac;
		n.g.rCount = (p1 - p0) * ac;
		if ((rc = launch(n))) return rc;
	}
	return OCTPIPE_OK;
}

int volumeEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, float* out, float* mean,
                int outIsDevice, double* kernelMs) {
	int rc = checkArguments("angiogram", data, r, s, out);
	if (rc) return rc;
	const OctPipeAngioSettings st = *s;
	Job j{};
	if ((rc = open(h, j, "angiogram", data, dataIsDevice, r, st, kernelMs))) return rc;
	const size_t outRowBytes = sizeof(float) * (size_t)j.r.sampleCount, outPosBytes = outRowBytes * j.r.ascanCount;
	// a host result leaves in slices of whole positions through the OUT and MEAN slots
	unsigned slicePos = j.P;
	if (!outIsDevice) {
		slicePos = (unsigned)std::min<size_t>(j.P, std::max<size_t>(1, kSliceBytes / outPosBytes));
		if ((rc = grow(h, h->angioState, AngioState::OUT, (size_t)slicePos * outPosBytes))) return rc;
		if (mean && (rc = grow(h, h->angioState, AngioState::MEAN, (size_t)slicePos * outPosBytes))) return rc;
	}
	StreamTimer timer(kernelMs != nullptr, j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	rc = overPositions(h, j, st, slicePos, [&](const oct::AngioArgs& n) -> int {
		oct::AngioVolumeArgs v{};
		v.n = n;
		v.out = outIsDevice ? out : h->angioState.as<float>(AngioState::OUT);
		v.mean = !mean ? nullptr : outIsDevice ? mean : h->angioState.as<float>(AngioState::MEAN);
		v.o0 = outIsDevice ? 0 : n.g.rFirst;
		HIP_TRY(oct::launch_angio_volume(st.method, v, h->stream));
		if (!outIsDevice) {
			const size_t off = (size_t)n.g.rFirst * outRowBytes, len = (size_t)n.g.rCount * outRowBytes;
			HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(out) + off, v.out, len, hipMemcpyDeviceToHost, h->stream));
			if (mean) HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(mean) + off, v.mean, len, hipMemcpyDeviceToHost, h->stream));
		}
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	hipError_t e = hipSuccess;
	if (!outIsDevice || kernelMs) e = hipStreamSynchronize(h->stream);
	if (e == hipSuccess) e = timer.elapsedMs(kernelMs);
	if (e != hipSuccess) return deviceError(j, e);
	return OCTPIPE_OK;
}

int enfaceEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, const int32_t* surface,
                int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice, unsigned form, double* kernelMs) {
	const std::string w("angiogram enface");
	int rc = checkArguments(w, data, r, s, out);
	if (rc) return rc;
	if (!slab) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": slab settings is NULL");
	if (!surface && surfaceIsDevice) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL but surfaceIsDevice is set");
	const OctPipeAngioSettings st = *s;
	const OctPipeSurfaceEnfaceSettings sl = *slab;
	if (sl.thickness < 1 || sl.thickness > kMaxThickness) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": thickness must lie in [1, 4096]");
	if (sl.function != 0 && sl.function != 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": function must be 0 (averaging) or 1 (MIP)");
	if (form > 2 || (form == 2 && sl.thickness > oct::ANGIO_TEAM_BINS))
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": form must be 0, 1 or 2, and 2 (teams of 16 lanes) takes a thickness of at most 64");
	const bool team = form == 2 || (form == 0 && sl.thickness <= kTeamMaxThickness);
	Job j{};
	if ((rc = open(h, j, "angiogram enface", data, dataIsDevice, r, st, kernelMs))) return rc;
	const size_t bytes = sizeof(float) * (size_t)j.rows;
	float* dOut = out;
	if (!outIsDevice) {
		if ((rc = grow(h, h->angioState, AngioState::OUT, bytes))) return rc;
		dOut = h->angioState.as<float>(AngioState::OUT);
	}
	StreamTimer timer(kernelMs != nullptr, j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::AngioEnfaceArgs e{};
	e.surface = surface;
	if (surface && !surfaceIsDevice) {  // a host surface is uploaded whole
		const size_t sBytes = sizeof(int32_t) * (size_t)j.r.bscanCount * j.r.ascanCount;
		if ((rc = grow(h, h->angioState, AngioState::SURF_IN, sBytes))) return rc;
		int32_t* d = h->angioState.as<int32_t>(AngioState::SURF_IN);
		if (hipError_t err = hipMemcpyAsync(d, surface, sBytes, hipMemcpyHostToDevice, h->stream); err != hipSuccess) return deviceError(j, err);
		e.surface = d;
	}
	e.offset = sl.offset;
	e.thickness = sl.thickness;
	e.fill = sl.fill;
	e.out = dOut;
	rc = overPositions(h, j, st, j.P, [&](const oct::AngioArgs& n) -> int {
		e.n = n;
		HIP_TRY(oct::launch_angio_enface(st.method, sl.function, team, e, h->stream));
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	hipError_t err = hipSuccess;
	if (!outIsDevice) err = hipMemcpyAsync(out, dOut, bytes, hipMemcpyDeviceToHost, h->stream);
	if (err == hipSuccess && (!outIsDevice || kernelMs)) err = hipStreamSynchronize(h->stream);
	if (err == hipSuccess) err = timer.elapsedMs(kernelMs);
	if (err != hipSuccess) return deviceError(j, err);
	return OCTPIPE_OK;
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_angiogram(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, float* out,
                      float* mean, int outIsDevice) {
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, nullptr);
}

int octpipe_angiogram_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                             const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice) {
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, 0, nullptr);
}

int octpipe_debug_angiogram(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, float* out,
                            float* mean, int outIsDevice, double* kernelMs) {
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, kernelMs);
}

int octpipe_debug_angiogram_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                   const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice,
                                   unsigned form, double* kernelMs) {
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, form, kernelMs);
}

}  // extern "C"
