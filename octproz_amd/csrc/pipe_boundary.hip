// pipe_boundary.hip -- boundary tracing (include/octpipe.h "boundary tracing"): the minimum-cost path through every B-scan of a region
// of the float32 processed volume (boundary_trace.h).
//
//   octpipe_trace_boundary   oct_boundary_trace_kernel<WAVE, CHLDS>   region rows [+ guide] -> int32 surface [+ float32 path costs]
// The region and the processed source are pipe_region.hip's.  A launch covers whole B-scans, one workgroup each.  The region's B-scans
// go in chunks: one chunk for a device source with the choices in LDS; otherwise as many B-scans as kSliceBytes of staged source rows
// (host source) and of 4-bit choices (the scratch forms) allow, at least one.  A host guide is uploaded whole, host results are
// downloaded whole.  Everything runs on the handle's compute stream behind what is already enqueued there and touches nothing the
// processing chain reads or writes; the scratch belongs to the handle (BoundaryState, released in octpipe_destroy).
#include <algorithm>

#include "pipe_internal.h"
#include "boundary_trace.h"

namespace oct {
hipError_t launch_boundary_trace(unsigned form, const TraceArgs& a, unsigned bscans, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr int kMaxBand = 65536;
constexpr unsigned kMaxAscans = 65536;
enum { FORM_AUTO, FORM_WAVE_LDS, FORM_WAVE_SCRATCH, FORM_GROUP_LDS, FORM_GROUP_SCRATCH, FORM_COUNT };

int traceEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* guide, int guideIsDevice,
               const OctPipeBoundaryTraceSettings* s, int32_t* surface, float* pathCost, int surfaceIsDevice, unsigned form, double* kernelMs) {
	const std::string w("trace boundary");
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!surface) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": surface is NULL");
	if (!guide && guideIsDevice) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": guide is NULL with guideIsDevice set");
	const OctPipeBoundaryTraceSettings st = *s;
	if (guide) {
		if (st.bandLo < -kMaxBand || st.bandLo > kMaxBand) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": bandLo must lie in [-65536, 65536]");
		if (st.bandHi < -kMaxBand || st.bandHi > kMaxBand) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": bandHi must lie in [-65536, 65536]");
		if (st.bandLo > st.bandHi) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": bandLo must not exceed bandHi");
	}
	if (st.halfWidth < 1 || st.halfWidth > oct::TRACE_MAX_K) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": halfWidth must lie in [1, 8]");
	if (st.polarity != 1 && st.polarity != -1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": polarity must be +1 or -1");
	if (st.maxStep < 1 || st.maxStep > oct::TRACE_MAX_M) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": maxStep must lie in [1, 7]");
	if (!std::isfinite(st.smoothness) || st.smoothness < 0.0f) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": smoothness must be finite and >= 0");
	if (r->ascanCount > kMaxAscans) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region ascanCount must not exceed 65536");
	if (form >= FORM_COUNT) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": form must be 0 ... 4");
	const unsigned long long H = guide ? (unsigned long long)((long long)st.bandHi - st.bandLo + 1) : r->sampleCount;
	if (H > oct::TRACE_MAX_H)
		return fail(OCTPIPE_ERR_UNSUPPORTED, w + ": " + std::to_string(H) + " nodes per A-scan (bandHi - bandLo + 1, or sampleCount without a guide), at most 1024");
	if (data && r->buffer != 0 && r->buffer != 0xFFFFFFFFu)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": buffer must be 0 or 0xFFFFFFFF when data is given");
	int rc = enterCall(h, "trace boundary");
	if (rc) return rc;
	RegionSource j{};
	j.what = "trace boundary";
	j.src = oct::ST_F32;
	j.L = (unsigned)(h->N / 2);
	if ((rc = checkRegion(h, j, r))) return rc;
	if ((rc = resolveProcessed(h, j, data, dataIsDevice))) return rc;
	const unsigned ac = j.r.ascanCount, bc = j.r.bscanCount, rows = ac * bc;

	// the form: one wave where the nodes fit one, the choices in LDS where they fit
	const size_t choiceBytes = (size_t)ac * ((H + 1) / 2);  // of one B-scan
	const bool waveFits = H <= oct::TRACE_WAVE_H;
	if (form == FORM_AUTO) {
		if (waveFits) form = choiceBytes <= oct::TRACE_CH_WAVE ? FORM_WAVE_LDS : FORM_WAVE_SCRATCH;
		else form = choiceBytes <= oct::TRACE_CH_WG ? FORM_GROUP_LDS : FORM_GROUP_SCRATCH;
	} else {
		const bool wave = form == FORM_WAVE_LDS || form == FORM_WAVE_SCRATCH;
		const size_t room = form == FORM_WAVE_LDS ? oct::TRACE_CH_WAVE : form == FORM_GROUP_LDS ? oct::TRACE_CH_WG : ~(size_t)0;
		if ((wave && !waveFits) || choiceBytes > room)
			return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": form = " + std::to_string(form) + " does not apply to " + std::to_string(H) + " nodes and " +
			                                              std::to_string(ac) + " A-scans");
	}
	const bool scratch = form == FORM_WAVE_SCRATCH || form == FORM_GROUP_SCRATCH;

	BoundaryState& mem = h->boundaryState;
	const size_t rowBytes = sizeof(float) * (size_t)j.L, surfBytes = sizeof(int32_t) * (size_t)rows, costBytes = sizeof(float) * (size_t)bc;
	unsigned chunk = bc;  // B-scans per launch
	if (!j.device) chunk = (unsigned)std::min<size_t>(chunk, std::max<size_t>(1, kSliceBytes / (rowBytes * ac)));
	if (scratch) chunk = (unsigned)std::min<size_t>(chunk, std::max<size_t>(1, kSliceBytes / choiceBytes));
	if (!j.device && (rc = grow(h, mem, BoundaryState::STAGE, (size_t)chunk * ac * rowBytes))) return rc;
	if (scratch && (rc = grow(h, mem, BoundaryState::CHOICES, (size_t)chunk * choiceBytes))) return rc;
	void *dSurf = nullptr, *dCost = nullptr;
	if ((rc = resultOut(h, mem, BoundaryState::SURF_OUT, surface, surfaceIsDevice, surfBytes, &dSurf))) return rc;
	if (pathCost && (rc = resultOut(h, mem, BoundaryState::COST_OUT, pathCost, surfaceIsDevice, costBytes, &dCost))) return rc;

	StreamTimer timer(kernelMs != nullptr, j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	oct::TraceArgs t{};
	if (guide && (rc = surfaceIn(h, j, mem, BoundaryState::GUIDE_IN, guide, guideIsDevice, rows, &t.guide))) return rc;
	t.g.A = j.A;
	t.g.fb = j.r.firstBscan;
	t.g.fa = j.r.firstAscan;
	t.g.ac = ac;
	t.g.L = j.L;
	t.g.s0 = j.r.firstSample;
	t.g.cnt = j.r.sampleCount;
	t.surface = static_cast<int32_t*>(dSurf);
	t.pathCost = static_cast<float*>(dCost);
	t.choices = scratch ? mem.as<uint8_t>(BoundaryState::CHOICES) : nullptr;
	t.lo = guide ? st.bandLo : (int)j.r.firstSample;
	t.H = (unsigned)H;
	t.k = st.halfWidth;
	t.m = st.maxStep;
	t.negate = st.polarity > 0 ? 1 : 0;
	for (unsigned i = 0; i <= oct::TRACE_MAX_M; i++) {
		volatile float p = st.smoothness * (float)i;  // one rounded product
		t.p[i] = p;
	}
	char* stage = j.device ? nullptr : mem.as<char>(BoundaryState::STAGE);
	for (unsigned b0 = 0; b0 < bc; b0 += chunk) {
		const unsigned nb = std::min(chunk, bc - b0);
		if (!j.device && (rc = stageRegionRows(h, j, stage, b0 * ac, (b0 + nb) * ac, false))) return rc;
		t.g.src = j.device ? static_cast<const float*>(j.mem) : reinterpret_cast<const float*>(stage);
		t.g.staged = j.device ? 0 : 1;
		t.g.r0 = b0 * ac;
		t.g.rFirst = b0 * ac;
		t.g.rCount = nb * ac;
		t.bFirst = b0;
		HIP_TRY(oct::launch_boundary_trace(form, t, nb, h->stream));
	}
	if ((rc = timer.end(h->stream))) return rc;
	if (pathCost && !surfaceIsDevice) HIP_TRY(hipMemcpyAsync(pathCost, dCost, costBytes, hipMemcpyDeviceToHost, h->stream));
	return finish(h, j, timer, kernelMs, surfaceIsDevice ? nullptr : surface, dSurf, surfBytes);
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_trace_boundary(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* guide, int guideIsDevice,
                           const OctPipeBoundaryTraceSettings* s, int32_t* surface, float* pathCost, int surfaceIsDevice) {
	return traceEntry(h, data, dataIsDevice, r, guide, guideIsDevice, s, surface, pathCost, surfaceIsDevice, 0, nullptr);
}

int octpipe_debug_trace_boundary(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const int32_t* guide,
                                 int guideIsDevice, const OctPipeBoundaryTraceSettings* s, int32_t* surface, float* pathCost, int surfaceIsDevice,
                                 unsigned form, double* kernelMs) {
	return traceEntry(h, data, dataIsDevice, r, guide, guideIsDevice, s, surface, pathCost, surfaceIsDevice, form, kernelMs);
}

}  // extern "C"
