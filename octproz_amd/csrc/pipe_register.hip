// pipe_register.hip -- repeat registration (include/octpipe.h "repeat registration"): the axial shift of every repeated B-scan against the
// first one of its position, and the angiography's contrast taken from the shifted bins (repeat_register.h).
//
//   octpipe_repeat_shifts                 G <= 64: oct_register_search_kernel<false> builds the M profiles of every (position, group) from the
//                                         source rows and searches the lags (one pass over the region).
//                                         G > 64:  oct_peak_partials_kernel (the peak analysis' stage A, one wave per chunk of 64 A-scans and
//                                         tile of 256 bins) writes the float64 chunk partials, oct_register_search_kernel<true> adds them in
//                                         chunk order: few positions with large groups still fill the device.
//   octpipe_angiogram_registered          oct_register_volume_kernel<METHOD, M>
//   octpipe_angiogram_enface_registered   oct_register_enface_kernel<METHOD, FN, M> (thin slabs: its team form)
// The region and the processed source are pipe_region.hip's.  Every call goes over the region's positions in slices: one slice for a device
// source (and a device result); otherwise as many whole positions (at least one) as kSliceBytes of staged source rows, of chunk partials
// and of contrast rows on their way to the host allow.  Host shifts and a host surface are uploaded whole; host shifts, costs and images are
// downloaded whole.  Everything runs on the handle's compute stream behind what is already enqueued there and touches nothing the
// processing chain reads or writes; the scratch belongs to the handle (RegisterState, released in octpipe_destroy).
#include <algorithm>

#include "pipe_internal.h"
#include "repeat_register.h"

namespace oct {
hipError_t launch_peak_partials(const PeakArgs& a, hipStream_t s);
hipError_t launch_register_search(bool fromPartials, const RegSearchArgs& a, hipStream_t s);
hipError_t launch_register_volume(int method, const RegVolumeArgs& a, hipStream_t s);
hipError_t launch_register_enface(int method, int function, bool team, const RegEnfaceArgs& a, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr unsigned kMinRepeats = oct::ANGIO_MIN_REPEATS, kMaxRepeats = oct::ANGIO_MAX_REPEATS;
constexpr unsigned kTeamMaxThickness = oct::ANGIO_TEAM_BINS;  // (as octpipe_angiogram_enface)

// the source of one call and how its positions are walked
struct Job : RegionSource {
	unsigned M, P, G, Qp;  // repeats, positions, A-scans per group, groups per B-scan
	unsigned rows;         // output rows: P * ascanCount
};

// the checks on repeats and groups that need no handle
int checkRepeats(const std::string& w, const float* data, const OctPipeStatsRegion* r, unsigned repeats, unsigned G) {
	if (repeats < kMinRepeats || repeats > kMaxRepeats) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": repeats must lie in [2, 8]");
	if (r->bscanCount % repeats)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": repeats = " + std::to_string(repeats) + " must divide the region's bscanCount = " +
		                                              std::to_string(r->bscanCount));
	if (G < 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": ascansPerGroup must be >= 1");
	if (r->ascanCount % G)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": ascansPerGroup = " + std::to_string(G) + " must divide the region's ascanCount = " +
		                                              std::to_string(r->ascanCount));
	if (data && r->buffer != 0 && r->buffer != 0xFFFFFFFFu)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": buffer must be 0 or 0xFFFFFFFF when data is given");
	return OCTPIPE_OK;
}

// the checks of the two registered angiography calls that need no handle
int checkRegistered(const std::string& w, const float* data, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, const void* out,
                    const int32_t* shifts, int shiftsIsDevice, const OctPipeAngioRegistration* reg) {
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	if (!shifts) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + (shiftsIsDevice ? ": shifts is NULL but shiftsIsDevice is set" : ": shifts is NULL"));
	if (!reg) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": registration is NULL");
	if (s->method < 0 || s->method > 2)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": method must be 0 (speckle variance), 1 (amplitude decorrelation) or 2 (differential)");
	if (s->mask && std::isnan(s->threshold)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": threshold is NaN");
	return checkRepeats(w, data, r, s->repeats, reg->ascansPerGroup);
}

// entry, region and source
int open(octpipe* h, Job& j, const char* what, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, unsigned repeats, unsigned G) {
	int rc = enterCall(h, what);
	if (rc) return rc;
	j.what = what;
	j.src = oct::ST_F32;
	j.L = (unsigned)(h->N / 2);
	if ((rc = checkRegion(h, j, r))) return rc;
	j.M = repeats;
	j.P = j.r.bscanCount / j.M;
	j.G = G;
	j.Qp = j.r.ascanCount / G;
	j.rows = j.P * j.r.ascanCount;  // <= A * B
	return resolveProcessed(h, j, data, dataIsDevice);
}

size_t positionBytes(const Job& j) { return sizeof(float) * (size_t)j.L * j.M * j.r.ascanCount; }  // the source rows of one position

// the staging slot for `slicePos` positions of a host source (nullptr: a device source); slicePos comes back bounded by kSliceBytes
int stageFor(octpipe* h, const Job& j, unsigned& slicePos, char** stage) {
	*stage = nullptr;
	if (j.device) return OCTPIPE_OK;
	slicePos = (unsigned)std::min<size_t>(slicePos, std::max<size_t>(1, kSliceBytes / positionBytes(j)));
	if (int rc = grow(h, h->registerState, RegisterState::STAGE, (size_t)slicePos * positionBytes(j) + 16)) return rc;
	*stage = h->registerState.as<char>(RegisterState::STAGE);
	return OCTPIPE_OK;
}

// host shifts on their way in (uploaded whole); device shifts as they are
int shiftsOnDevice(octpipe* h, const Job& j, const int32_t* shifts, int shiftsIsDevice, const int32_t** d) {
	*d = shifts;
	if (shiftsIsDevice) return OCTPIPE_OK;
	const size_t bytes = sizeof(int32_t) * (size_t)j.P * j.M * j.Qp;
	if (int rc = grow(h, h->registerState, RegisterState::SHIFTS_IN, bytes)) return rc;
	int32_t* mem = h->registerState.as<int32_t>(RegisterState::SHIFTS_IN);
	if (hipError_t e = hipMemcpyAsync(mem, shifts, bytes, hipMemcpyHostToDevice, h->stream); e != hipSuccess) return deviceError(j, e);
	*d = mem;
	return OCTPIPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the shift estimate
int estimateEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeRepeatShiftSettings* s, int32_t* shifts,
                  int shiftsIsDevice, double* costs, double* kernelMs) {
	const char* what = "repeat shifts";
	const std::string w(what);
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!shifts) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + (shiftsIsDevice ? ": shifts is NULL but shiftsIsDevice is set" : ": shifts is NULL"));
	const OctPipeRepeatShiftSettings st = *s;
	int rc = checkRepeats(w, data, r, st.repeats, st.ascansPerGroup);
	if (rc) return rc;
	if (st.maxShift < 1 || st.maxShift > oct::REG_MAX_SHIFT) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": maxShift must lie in [1, 64]");
	if (r->sampleCount > oct::PEAK_MAX_SAMPLES)
		return fail(OCTPIPE_ERR_UNSUPPORTED, w + ": region sampleCount must be at most 4096 (depth window of " + std::to_string(r->sampleCount) + ")");
	if (r->sampleCount < 3 || r->sampleCount < 2 * st.maxShift + 1)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region sampleCount must be at least 3 and at least 2 maxShift + 1 = " +
		                                              std::to_string(2 * st.maxShift + 1));
	Job j{};
	if ((rc = open(h, j, what, data, dataIsDevice, r, st.repeats, st.ascansPerGroup))) return rc;
	const unsigned cnt = j.r.sampleCount, ac = j.r.ascanCount, lags = 2 * st.maxShift + 1;
	const unsigned chunks = (j.G + oct::PEAK_CHUNK - 1) / oct::PEAK_CHUNK;
	const bool fromPartials = j.G > oct::PEAK_CHUNK;
	RegisterState& mem = h->registerState;
	const size_t shiftBytes = sizeof(int32_t) * (size_t)j.P * j.M * j.Qp, costBytes = sizeof(double) * (size_t)j.P * (j.M - 1) * j.Qp * lags;
	int32_t* dShifts = shifts;
	double* dCosts = costs;
	if (!shiftsIsDevice) {
		if ((rc = grow(h, mem, RegisterState::SHIFTS_OUT, shiftBytes))) return rc;
		dShifts = mem.as<int32_t>(RegisterState::SHIFTS_OUT);
		if (costs) {
			if ((rc = grow(h, mem, RegisterState::COSTS_OUT, costBytes))) return rc;
			dCosts = mem.as<double>(RegisterState::COSTS_OUT);
		}
	}
	unsigned slicePos = j.P;
	char* stage;
	if ((rc = stageFor(h, j, slicePos, &stage))) return rc;
	const size_t posPartBytes = sizeof(double) * (size_t)chunks * cnt * j.M * j.Qp;  // the chunk partials of one position
	if (fromPartials) {
		slicePos = (unsigned)std::min<size_t>(slicePos, std::max<size_t>(1, kSliceBytes / posPartBytes));
		if ((rc = grow(h, mem, RegisterState::PARTS, (size_t)slicePos * posPartBytes))) return rc;
	}
	oct::RegSearchArgs a{};
	a.k.A = j.A;
	a.k.fb = j.r.firstBscan;
	a.k.fa = j.r.firstAscan;
	a.k.ac = ac;
	a.k.L = j.L;
	a.k.s0 = j.r.firstSample;
	a.k.cnt = cnt;
	a.k.G = j.G;
	a.k.chunks = chunks;
	a.k.parts = fromPartials ? mem.as<double>(RegisterState::PARTS) : nullptr;
	a.M = j.M;
	a.Qp = j.Qp;
	a.R = st.maxShift;
	a.shifts = dShifts;
	a.costs = dCosts;
	StreamTimer timer(kernelMs != nullptr, what);
	if ((rc = timer.begin(h->stream))) return rc;
	for (unsigned p0 = 0; p0 < j.P; p0 += slicePos) {
		const unsigned p1 = (unsigned)std::min<unsigned long long>(j.P, (unsigned long long)p0 + slicePos);
		const unsigned r0 = p0 * j.M * ac, r1 = p1 * j.M * ac;  // region rows, <= A * B
		if (!j.device && (rc = stageRegionRows(h, j, stage, r0, r1, false))) return rc;
		a.k.src = j.device ? static_cast<const float*>(j.mem) : reinterpret_cast<const float*>(stage);
		a.k.staged = j.device ? 0 : 1;
		a.k.r0 = r0;
		a.k.vec = a.k.L % 4 == 0 && a.k.s0 % 4 == 0 && reinterpret_cast<uintptr_t>(a.k.src) % 16 == 0 ? 1 : 0;
		a.k.pFirst = p0 * j.M * j.Qp;  // the first group (of the peak analysis' numbering) whose partials are in `parts`
		if (fromPartials) {
			a.k.gFirst = a.k.pFirst * chunks;
			a.k.gCount = (p1 - p0) * j.M * j.Qp * chunks;
			HIP_TRY(oct::launch_peak_partials(a.k, h->stream));
		}
		a.pFirst = p0;
		a.pCount = p1 - p0;
		HIP_TRY(oct::launch_register_search(fromPartials, a, h->stream));
	}
	if ((rc = timer.end(h->stream))) return rc;
	hipError_t e = hipSuccess;
	if (!shiftsIsDevice) {
		e = hipMemcpyAsync(shifts, dShifts, shiftBytes, hipMemcpyDeviceToHost, h->stream);
		if (e == hipSuccess && costs) e = hipMemcpyAsync(costs, dCosts, costBytes, hipMemcpyDeviceToHost, h->stream);
	}
	if (e == hipSuccess && (!shiftsIsDevice || kernelMs)) e = hipStreamSynchronize(h->stream);
	if (e == hipSuccess) e = timer.elapsedMs(kernelMs);
	if (e != hipSuccess) return deviceError(j, e);
	return OCTPIPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the registered calls
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

// the region's positions in slices of at most `slicePos`: a host source's rows staged, then launch(args of the slice)
template <class Launch>
int overPositions(octpipe* h, const Job& j, const OctPipeAngioSettings& s, unsigned slicePos, Launch launch) {
	int rc;
	oct::AngioArgs n = sourceArgs(j, s);
	const unsigned ac = j.r.ascanCount;
	char* stage;
	if ((rc = stageFor(h, j, slicePos, &stage))) return rc;
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
                int outIsDevice, const int32_t* shifts, int shiftsIsDevice, const OctPipeAngioRegistration* reg, double* kernelMs) {
	const char* what = "angiogram registered";
	int rc = checkRegistered(what, data, r, s, out, shifts, shiftsIsDevice, reg);
	if (rc) return rc;
	const OctPipeAngioSettings st = *s;
	const OctPipeAngioRegistration rg = *reg;
	Job j{};
	if ((rc = open(h, j, what, data, dataIsDevice, r, st.repeats, rg.ascansPerGroup))) return rc;
	RegisterState& mem = h->registerState;
	const size_t outRowBytes = sizeof(float) * (size_t)j.r.sampleCount, outPosBytes = outRowBytes * j.r.ascanCount;
	// a host result leaves in slices of whole positions through the OUT and MEAN slots
	unsigned slicePos = j.P;
	if (!outIsDevice) {
		slicePos = (unsigned)std::min<size_t>(j.P, std::max<size_t>(1, kSliceBytes / outPosBytes));
		if ((rc = grow(h, mem, RegisterState::OUT, (size_t)slicePos * outPosBytes))) return rc;
		if (mean && (rc = grow(h, mem, RegisterState::MEAN, (size_t)slicePos * outPosBytes))) return rc;
	}
	StreamTimer timer(kernelMs != nullptr, what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::RegVolumeArgs v{};
	if ((rc = shiftsOnDevice(h, j, shifts, shiftsIsDevice, &v.s.shifts))) return rc;
	v.s.G = j.G;
	v.s.Qp = j.Qp;
	v.fill = rg.fill;
	rc = overPositions(h, j, st, slicePos, [&](const oct::AngioArgs& n) -> int {
		v.v.n = n;
		v.v.out = outIsDevice ? out : mem.as<float>(RegisterState::OUT);
		v.v.mean = !mean ? nullptr : outIsDevice ? mean : mem.as<float>(RegisterState::MEAN);
		v.v.o0 = outIsDevice ? 0 : n.g.rFirst;
		HIP_TRY(oct::launch_register_volume(st.method, v, h->stream));
		if (!outIsDevice) {
			const size_t off = (size_t)n.g.rFirst * outRowBytes, len = (size_t)n.g.rCount * outRowBytes;
			HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(out) + off, v.v.out, len, hipMemcpyDeviceToHost, h->stream));
			if (mean) HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(mean) + off, v.v.mean, len, hipMemcpyDeviceToHost, h->stream));
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
                int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice, const int32_t* shifts, int shiftsIsDevice,
                const OctPipeAngioRegistration* reg, unsigned form, double* kernelMs) {
	const char* what = "angiogram enface registered";
	const std::string w(what);
	int rc = checkRegistered(w, data, r, s, out, shifts, shiftsIsDevice, reg);
	if (rc) return rc;
	if (!slab) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": slab settings is NULL");
	if (!surface && surfaceIsDevice) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL but surfaceIsDevice is set");
	const OctPipeAngioSettings st = *s;
	const OctPipeSurfaceEnfaceSettings sl = *slab;
	const OctPipeAngioRegistration rg = *reg;
	if (sl.thickness < 1 || sl.thickness > kMaxThickness) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": thickness must lie in [1, 4096]");
	if (sl.function != 0 && sl.function != 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": function must be 0 (averaging) or 1 (MIP)");
	if (form > 2 || (form == 2 && sl.thickness > oct::ANGIO_TEAM_BINS))
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": form must be 0, 1 or 2, and 2 (teams of 16 lanes) takes a thickness of at most 64");
	const bool team = form == 2 || (form == 0 && sl.thickness <= kTeamMaxThickness);
	Job j{};
	if ((rc = open(h, j, what, data, dataIsDevice, r, st.repeats, rg.ascansPerGroup))) return rc;
	RegisterState& mem = h->registerState;
	const size_t bytes = sizeof(float) * (size_t)j.rows;
	float* dOut = out;
	if (!outIsDevice) {
		if ((rc = grow(h, mem, RegisterState::OUT, bytes))) return rc;
		dOut = mem.as<float>(RegisterState::OUT);
	}
	StreamTimer timer(kernelMs != nullptr, what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::RegEnfaceArgs e{};
	if ((rc = shiftsOnDevice(h, j, shifts, shiftsIsDevice, &e.s.shifts))) return rc;
	e.s.G = j.G;
	e.s.Qp = j.Qp;
	e.e.surface = surface;
	if (surface && !surfaceIsDevice) {  // a host surface is uploaded whole
		const size_t sBytes = sizeof(int32_t) * (size_t)j.r.bscanCount * j.r.ascanCount;
		if ((rc = grow(h, mem, RegisterState::SURF_IN, sBytes))) return rc;
		int32_t* d = mem.as<int32_t>(RegisterState::SURF_IN);
		if (hipError_t err = hipMemcpyAsync(d, surface, sBytes, hipMemcpyHostToDevice, h->stream); err != hipSuccess) return deviceError(j, err);
		e.e.surface = d;
	}
	e.e.offset = sl.offset;
	e.e.thickness = sl.thickness;
	e.e.fill = sl.fill;
	e.e.out = dOut;
	rc = overPositions(h, j, st, j.P, [&](const oct::AngioArgs& n) -> int {
		e.e.n = n;
		HIP_TRY(oct::launch_register_enface(st.method, sl.function, team, e, h->stream));
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

int octpipe_repeat_shifts(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeRepeatShiftSettings* s,
                          int32_t* shifts, int shiftsIsDevice, double* costs) {
	return estimateEntry(h, data, dataIsDevice, r, s, shifts, shiftsIsDevice, costs, nullptr);
}

int octpipe_angiogram_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                 float* out, float* mean, int outIsDevice, const int32_t* shifts, int shiftsIsDevice,
                                 const OctPipeAngioRegistration* registration) {
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, shifts, shiftsIsDevice, registration, nullptr);
}

int octpipe_angiogram_enface_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                        const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out,
                                        int outIsDevice, const int32_t* shifts, int shiftsIsDevice, const OctPipeAngioRegistration* registration) {
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, shifts, shiftsIsDevice, registration, 0, nullptr);
}

int octpipe_debug_repeat_shifts(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeRepeatShiftSettings* s,
                                int32_t* shifts, int shiftsIsDevice, double* costs, double* kernelMs) {
	return estimateEntry(h, data, dataIsDevice, r, s, shifts, shiftsIsDevice, costs, kernelMs);
}

int octpipe_debug_angiogram_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                       float* out, float* mean, int outIsDevice, const int32_t* shifts, int shiftsIsDevice,
                                       const OctPipeAngioRegistration* registration, double* kernelMs) {
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, shifts, shiftsIsDevice, registration, kernelMs);
}

int octpipe_debug_angiogram_enface_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                              const OctPipeAngioSettings* s, const int32_t* surface, int surfaceIsDevice,
                                              const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice, const int32_t* shifts,
                                              int shiftsIsDevice, const OctPipeAngioRegistration* registration, unsigned form, double* kernelMs) {
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, shifts, shiftsIsDevice, registration, form,
	                   kernelMs);
}

}  // extern "C"
