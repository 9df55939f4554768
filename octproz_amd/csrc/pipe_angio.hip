// pipe_angio.hip -- OCT angiography (include/octpipe.h "angiography"): the contrast between the repeated B-scans of every slow-axis
// position of the float32 processed volume (angiogram.h); and the repeat registration (include/octpipe.h "repeat registration"): the axial
// shift of every repeated B-scan against the first one of its position, and the same contrast taken from the shifted bins
// (repeat_register.h).  One host path: a registered call is the plain call plus its shifts.
//
//   octpipe_angiogram                     oct_angio_volume_kernel<METHOD, M>       region rows -> float32 contrast volume (and mean volume)
//   octpipe_angiogram_enface              oct_angio_enface_kernel<METHOD, FN, M>   region rows (+ surface) -> float32 image (thin slabs: its team form)
//   octpipe_angiogram_registered          oct_register_volume_kernel<METHOD, M>
//   octpipe_angiogram_enface_registered   oct_register_enface_kernel<METHOD, FN, M> (thin slabs: its team form)
//   octpipe_repeat_shifts                 G <= 64: oct_register_search_kernel<false> builds the M profiles of every (position, group) from the
//                                         source rows and searches the lags (one pass over the region).
//                                         G > 64:  oct_peak_partials_kernel (the peak analysis' stage A, one wave per chunk of 64 A-scans and
//                                         tile of 256 bins) writes the float64 chunk partials, oct_register_search_kernel<true> adds them in
//                                         chunk order: few positions with large groups still fill the device.
// The region and the processed source are pipe_region.hip's.  Every call goes over the region's positions in slices: one slice for a device
// source (and a device result); otherwise as many whole positions (at least one) as kSliceBytes of staged source rows (host source), of
// chunk partials and of contrast rows on their way to the host (host result of a volume call) allow.  Host shifts and a host surface are
// uploaded whole; host shifts, costs and images are downloaded whole.  Everything runs on the handle's compute stream behind what is already
// enqueued there and touches nothing the processing chain reads or writes; the scratch belongs to the handle (AngioState, released in
// octpipe_destroy): all five calls share its slots, one call after the other in stream order.
#include <algorithm>

#include "pipe_internal.h"
#include "repeat_register.h"

namespace oct {
hipError_t launch_angio_volume(int method, const AngioVolumeArgs& a, hipStream_t s);
hipError_t launch_angio_enface(int method, int function, bool team, const AngioEnfaceArgs& a, hipStream_t s);
hipError_t launch_peak_partials(const PeakArgs& a, hipStream_t s);
hipError_t launch_register_search(bool fromPartials, const RegSearchArgs& a, hipStream_t s);
hipError_t launch_register_volume(int method, const RegVolumeArgs& a, hipStream_t s);
hipError_t launch_register_enface(int method, int function, bool team, const RegEnfaceArgs& a, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr unsigned kMinRepeats = oct::ANGIO_MIN_REPEATS, kMaxRepeats = oct::ANGIO_MAX_REPEATS;  // (kSliceBytes, kMaxThickness: pipe_internal.h)
// the thickest slab the en face calls give to the kernel's team form: all it takes (faster than the full-wave form at 16 and at 64
// bins in the same-run comparison of profiles/angio_bench.json)
constexpr unsigned kTeamMaxThickness = oct::ANGIO_TEAM_BINS;

// the source of one call and how its positions are walked
struct Job : RegionSource {
	unsigned M, P;   // repeats, positions
	unsigned G, Qp;  // A-scans per group, groups per B-scan: only of a call that registers or estimates (else 0)
	unsigned rows;   // output rows: P * ascanCount
};

// what makes an angiography call a registered one (no Registration: the plain call)
struct Registration {
	const int32_t* shifts;
	int shiftsIsDevice;
	const OctPipeAngioRegistration* settings;
};

// the checks that need no handle, in pieces: every call keeps the order in which its own fire
int checkRepeats(const std::string& w, const OctPipeStatsRegion* r, unsigned repeats) {
	if (repeats < kMinRepeats || repeats > kMaxRepeats) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": repeats must lie in [2, 8]");
	if (r->bscanCount % repeats)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": repeats = " + std::to_string(repeats) + " must divide the region's bscanCount = " +
		                                              std::to_string(r->bscanCount));
	return OCTPIPE_OK;
}

int checkGroups(const std::string& w, const OctPipeStatsRegion* r, unsigned G) {
	if (G < 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": ascansPerGroup must be >= 1");
	if (r->ascanCount % G)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": ascansPerGroup = " + std::to_string(G) + " must divide the region's ascanCount = " +
		                                              std::to_string(r->ascanCount));
	return OCTPIPE_OK;
}

int checkBuffer(const std::string& w, const float* data, const OctPipeStatsRegion* r) {
	if (data && r->buffer != 0 && r->buffer != 0xFFFFFFFFu)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": buffer must be 0 or 0xFFFFFFFF when data is given");
	return OCTPIPE_OK;
}

const char* shiftsNull(int shiftsIsDevice) { return shiftsIsDevice ? ": shifts is NULL but shiftsIsDevice is set" : ": shifts is NULL"; }

// the four angiography calls.  The plain ones check the repeats before the method; the registered ones check shifts, registration, method
// and threshold before the repeats and the groups.
int checkArguments(const std::string& w, const float* data, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, const void* out,
                   const Registration* reg) {
	int rc;
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	if (reg && !reg->shifts) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + shiftsNull(reg->shiftsIsDevice));
	if (reg && !reg->settings) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": registration is NULL");
	if (!reg && (rc = checkRepeats(w, r, s->repeats))) return rc;
	if (s->method < 0 || s->method > 2)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": method must be 0 (speckle variance), 1 (amplitude decorrelation) or 2 (differential)");
	if (s->mask && std::isnan(s->threshold)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": threshold is NaN");
	if (reg && (rc = checkRepeats(w, r, s->repeats))) return rc;
	if (reg && (rc = checkGroups(w, r, reg->settings->ascansPerGroup))) return rc;
	return checkBuffer(w, data, r);
}

// entry, region and source (G = 0: a call without groups)
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
	j.Qp = G ? j.r.ascanCount / G : 0;
	j.rows = j.P * j.r.ascanCount;  // <= A * B
	return resolveProcessed(h, j, data, dataIsDevice);
}

// the staging slot for `slicePos` positions of a host source (nullptr: a device source); slicePos comes back bounded by kSliceBytes.
// Nothing reads past the last staged row: the kernels' 16-byte loads are taken only where the row length and firstSample are multiples
// of 4 and stay inside their row, and shifted bins are read only inside the covered window.  The 16 bytes behind it are the margin the
// registration's slot had.
int stageFor(octpipe* h, const Job& j, unsigned& slicePos, char** stage) {
	*stage = nullptr;
	if (j.device) return OCTPIPE_OK;
	const size_t posBytes = sizeof(float) * (size_t)j.L * j.M * j.r.ascanCount;  // the source rows of one position
	slicePos = (unsigned)std::min<size_t>(slicePos, std::max<size_t>(1, kSliceBytes / posBytes));
	if (int rc = grow(h, h->angioState, AngioState::STAGE, (size_t)slicePos * posBytes + 16)) return rc;
	*stage = h->angioState.as<char>(AngioState::STAGE);
	return OCTPIPE_OK;
}

// host shifts on their way in (uploaded whole); device shifts as they are
int shiftsOnDevice(octpipe* h, const Job& j, const Registration& reg, oct::RegShiftArgs& s) {
	s.G = j.G;
	s.Qp = j.Qp;
	s.shifts = reg.shifts;
	if (reg.shiftsIsDevice) return OCTPIPE_OK;
	const size_t bytes = sizeof(int32_t) * (size_t)j.P * j.M * j.Qp;
	if (int rc = grow(h, h->angioState, AngioState::SHIFTS_IN, bytes)) return rc;
	int32_t* mem = h->angioState.as<int32_t>(AngioState::SHIFTS_IN);
	if (hipError_t e = hipMemcpyAsync(mem, reg.shifts, bytes, hipMemcpyHostToDevice, h->stream); e != hipSuccess) return deviceError(j, e);
	s.shifts = mem;
	return OCTPIPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the shift estimate
int estimateEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeRepeatShiftSettings* s, int32_t* shifts,
                  int shiftsIsDevice, double* costs, double* kernelMs) {
	const char* what = "repeat shifts";
	const std::string w(what);
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!shifts) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + shiftsNull(shiftsIsDevice));
	const OctPipeRepeatShiftSettings st = *s;
	int rc;
	if ((rc = checkRepeats(w, r, st.repeats)) || (rc = checkGroups(w, r, st.ascansPerGroup)) || (rc = checkBuffer(w, data, r))) return rc;
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
	AngioState& mem = h->angioState;
	const size_t shiftBytes = sizeof(int32_t) * (size_t)j.P * j.M * j.Qp, costBytes = sizeof(double) * (size_t)j.P * (j.M - 1) * j.Qp * lags;
	int32_t* dShifts = shifts;
	double* dCosts = costs;
	if (!shiftsIsDevice) {
		if ((rc = grow(h, mem, AngioState::SHIFTS_OUT, shiftBytes))) return rc;
		dShifts = mem.as<int32_t>(AngioState::SHIFTS_OUT);
		if (costs) {
			if ((rc = grow(h, mem, AngioState::COSTS_OUT, costBytes))) return rc;
			dCosts = mem.as<double>(AngioState::COSTS_OUT);
		}
	}
	unsigned slicePos = j.P;
	char* stage;
	if ((rc = stageFor(h, j, slicePos, &stage))) return rc;
	const size_t posPartBytes = sizeof(double) * (size_t)chunks * cnt * j.M * j.Qp;  // the chunk partials of one position
	if (fromPartials) {
		slicePos = (unsigned)std::min<size_t>(slicePos, std::max<size_t>(1, kSliceBytes / posPartBytes));
		if ((rc = grow(h, mem, AngioState::PARTS, (size_t)slicePos * posPartBytes))) return rc;
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
	a.k.parts = fromPartials ? mem.as<double>(AngioState::PARTS) : nullptr;
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

// ---------------------------------------------------------------------------------------------------------------- the angiography calls
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
                int outIsDevice, const Registration* reg, double* kernelMs) {
	const char* what = reg ? "angiogram registered" : "angiogram";
	int rc = checkArguments(what, data, r, s, out, reg);
	if (rc) return rc;
	const OctPipeAngioSettings st = *s;
	const OctPipeAngioRegistration rg = reg ? *reg->settings : OctPipeAngioRegistration{};
	Job j{};
	if ((rc = open(h, j, what, data, dataIsDevice, r, st.repeats, rg.ascansPerGroup))) return rc;
	AngioState& mem = h->angioState;
	const size_t outRowBytes = sizeof(float) * (size_t)j.r.sampleCount, outPosBytes = outRowBytes * j.r.ascanCount;
	// a host result leaves in slices of whole positions through the OUT and MEAN slots
	unsigned slicePos = j.P;
	if (!outIsDevice) {
		slicePos = (unsigned)std::min<size_t>(j.P, std::max<size_t>(1, kSliceBytes / outPosBytes));
		if ((rc = grow(h, mem, AngioState::OUT, (size_t)slicePos * outPosBytes))) return rc;
		if (mean && (rc = grow(h, mem, AngioState::MEAN, (size_t)slicePos * outPosBytes))) return rc;
	}
	StreamTimer timer(kernelMs != nullptr, what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::RegVolumeArgs rv{};  // (rv.v alone: the plain call)
	if (reg && (rc = shiftsOnDevice(h, j, *reg, rv.s))) return rc;
	rv.fill = rg.fill;
	rc = overPositions(h, j, st, slicePos, [&](const oct::AngioArgs& n) -> int {
		oct::AngioVolumeArgs& v = rv.v;
		v.n = n;
		v.out = outIsDevice ? out : mem.as<float>(AngioState::OUT);
		v.mean = !mean ? nullptr : outIsDevice ? mean : mem.as<float>(AngioState::MEAN);
		v.o0 = outIsDevice ? 0 : n.g.rFirst;
		if (reg) HIP_TRY(oct::launch_register_volume(st.method, rv, h->stream));
		else HIP_TRY(oct::launch_angio_volume(st.method, v, h->stream));
		if (!outIsDevice) {
			const size_t off = (size_t)n.g.rFirst * outRowBytes, len = (size_t)n.g.rCount * outRowBytes;
			HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(out) + off, v.out, len, hipMemcpyDeviceToHost, h->stream));
			if (mean) HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(mean) + off, v.mean, len, hipMemcpyDeviceToHost, h->stream));
		}
		return OCTPIPE_OK;
	});
	if (rc) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	return finish(h, j, timer, kernelMs, outIsDevice ? nullptr : out, nullptr, 0);  // (the rows have left slice by slice)
}

int enfaceEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, const int32_t* surface,
                int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice, const Registration* reg, unsigned form,
                double* kernelMs) {
	const char* what = reg ? "angiogram enface registered" : "angiogram enface";
	const std::string w(what);
	int rc = checkArguments(w, data, r, s, out, reg);
	if (rc) return rc;
	if (!slab) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": slab settings is NULL");
	if (!surface && surfaceIsDevice) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL but surfaceIsDevice is set");
	const OctPipeAngioSettings st = *s;
	const OctPipeSurfaceEnfaceSettings sl = *slab;
	const OctPipeAngioRegistration rg = reg ? *reg->settings : OctPipeAngioRegistration{};
	if (sl.thickness < 1 || sl.thickness > kMaxThickness) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": thickness must lie in [1, 4096]");
	if (sl.function != 0 && sl.function != 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": function must be 0 (averaging) or 1 (MIP)");
	if (form > 2 || (form == 2 && sl.thickness > oct::ANGIO_TEAM_BINS))
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": form must be 0, 1 or 2, and 2 (teams of 16 lanes) takes a thickness of at most 64");
	const bool team = form == 2 || (form == 0 && sl.thickness <= kTeamMaxThickness);
	Job j{};
	if ((rc = open(h, j, what, data, dataIsDevice, r, st.repeats, rg.ascansPerGroup))) return rc;
	AngioState& mem = h->angioState;
	const size_t bytes = sizeof(float) * (size_t)j.rows;
	void* dOut = nullptr;
	if ((rc = resultOut(h, mem, AngioState::OUT, out, outIsDevice, bytes, &dOut))) return rc;
	StreamTimer timer(kernelMs != nullptr, what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::RegEnfaceArgs re{};  // (re.e alone: the plain call)
	if (reg && (rc = shiftsOnDevice(h, j, *reg, re.s))) return rc;
	oct::AngioEnfaceArgs& e = re.e;
	// (no surface: firstSample everywhere)
	if (surface && (rc = surfaceIn(h, j, mem, AngioState::SURF_IN, surface, surfaceIsDevice, (size_t)j.r.bscanCount * j.r.ascanCount, &e.surface)))
		return rc;
	e.offset = sl.offset;
	e.thickness = sl.thickness;
	e.fill = sl.fill;
	e.out = static_cast<float*>(dOut);
	rc = overPositions(h, j, st, j.P, [&](const oct::AngioArgs& n) -> int {
		e.n = n;
		if (reg) HIP_TRY(oct::launch_register_enface(st.method, sl.function, team, re, h->stream));
		else HIP_TRY(oct::launch_angio_enface(st.method, sl.function, team, e, h->stream));
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

int octpipe_angiogram(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, float* out,
                      float* mean, int outIsDevice) {
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, nullptr, nullptr);
}

int octpipe_angiogram_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                             const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice) {
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, nullptr, 0, nullptr);
}

int octpipe_debug_angiogram(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s, float* out,
                            float* mean, int outIsDevice, double* kernelMs) {
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, nullptr, kernelMs);
}

int octpipe_debug_angiogram_enface(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                   const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice,
                                   unsigned form, double* kernelMs) {
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, nullptr, form, kernelMs);
}

int octpipe_repeat_shifts(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeRepeatShiftSettings* s,
                          int32_t* shifts, int shiftsIsDevice, double* costs) {
	return estimateEntry(h, data, dataIsDevice, r, s, shifts, shiftsIsDevice, costs, nullptr);
}

int octpipe_angiogram_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                 float* out, float* mean, int outIsDevice, const int32_t* shifts, int shiftsIsDevice,
                                 const OctPipeAngioRegistration* registration) {
	const Registration reg{shifts, shiftsIsDevice, registration};
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, &reg, nullptr);
}

int octpipe_angiogram_enface_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                        const int32_t* surface, int surfaceIsDevice, const OctPipeSurfaceEnfaceSettings* slab, float* out,
                                        int outIsDevice, const int32_t* shifts, int shiftsIsDevice, const OctPipeAngioRegistration* registration) {
	const Registration reg{shifts, shiftsIsDevice, registration};
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, &reg, 0, nullptr);
}

int octpipe_debug_repeat_shifts(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeRepeatShiftSettings* s,
                                int32_t* shifts, int shiftsIsDevice, double* costs, double* kernelMs) {
	return estimateEntry(h, data, dataIsDevice, r, s, shifts, shiftsIsDevice, costs, kernelMs);
}

int octpipe_debug_angiogram_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipeAngioSettings* s,
                                       float* out, float* mean, int outIsDevice, const int32_t* shifts, int shiftsIsDevice,
                                       const OctPipeAngioRegistration* registration, double* kernelMs) {
	const Registration reg{shifts, shiftsIsDevice, registration};
	return volumeEntry(h, data, dataIsDevice, r, s, out, mean, outIsDevice, &reg, kernelMs);
}

int octpipe_debug_angiogram_enface_registered(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r,
                                              const OctPipeAngioSettings* s, const int32_t* surface, int surfaceIsDevice,
                                              const OctPipeSurfaceEnfaceSettings* slab, float* out, int outIsDevice, const int32_t* shifts,
                                              int shiftsIsDevice, const OctPipeAngioRegistration* registration, unsigned form, double* kernelMs) {
	const Registration reg{shifts, shiftsIsDevice, registration};
	return enfaceEntry(h, data, dataIsDevice, r, s, surface, surfaceIsDevice, slab, out, outIsDevice, &reg, form, kernelMs);
}

}  // extern "C"
