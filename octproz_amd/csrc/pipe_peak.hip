// pipe_peak.hip -- peak analysis of groups of A-scans of a region (include/octpipe.h "peak analysis"; reference docs:
// docs/docs/plugin-peakdetector.md, plugin-axialpsfanalyzer.md).
//
//   G <= 64: oct_peak_kernel<FIT, false> builds every group's averaged A-scan from the source rows and analyses it (one pass).
//   G > 64:  oct_peak_partials_kernel writes the float64 partials of every (group, chunk of 64 A-scans), then
//            oct_peak_kernel<FIT, true> sums them; groups go in batches whose partials fit kPartBytes.
// The region and the processed source are pipe_region.hip's (shared with the image statistics).  A host source is staged in slices
// of whole groups (G <= 64) or whole chunks (G > 64), only the region's rows, so every sum sees the same values in the same order as
// from a device source.  Everything runs on the handle's compute stream behind what is already enqueued there and touches nothing
// the processing chain reads or writes; the scratch belongs to the handle (PeakState, released in octpipe_destroy).
#include <algorithm>
#include <limits>

#include "pipe_internal.h"
#include "peak_analysis.h"

namespace oct {
hipError_t launch_peak_partials(const PeakArgs& a, hipStream_t s);
hipError_t launch_peak(bool fit, bool fromPartials, unsigned waves, const PeakArgs& a, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr size_t kStageBytes = 64ull << 20;  // host rows staged per slice (at least one group or chunk)
constexpr size_t kPartBytes = 64ull << 20;   // float64 partials of one batch of groups (at least one group)
constexpr unsigned kMaxIterations = 1000;
constexpr const char* kWhat = "peak analysis";

int launchB(octpipe* h, bool fit, bool fromPartials, const oct::PeakArgs& a) {
	const unsigned waves = a.cnt > 1024 ? 1 : 4;  // (LDS per workgroup at most 16 KiB)
	HIP_TRY(oct::launch_peak(fit, fromPartials, waves, a, h->stream));
	return OCTPIPE_OK;
}

bool vecOk(const oct::PeakArgs& a) { return a.L % 4 == 0 && a.s0 % 4 == 0 && reinterpret_cast<uintptr_t>(a.src) % 16 == 0; }

// the device work of the whole call
int enqueue(octpipe* h, const RegionSource& j, const OctPipePeakSettings& st, unsigned Q, OctPipePeak* dPeaks, float* dAvg) {
	const unsigned G = st.ascansPerGroup, cnt = j.r.sampleCount, chunks = (G + oct::PEAK_CHUNK - 1) / oct::PEAK_CHUNK;
	const bool fit = st.fitGaussian != 0;
	oct::PeakArgs a{};
	a.A = j.A;
	a.fb = j.r.firstBscan;
	a.fa = j.r.firstAscan;
	a.ac = j.r.ascanCount;
	a.L = j.L;
	a.s0 = j.r.firstSample;
	a.cnt = cnt;
	a.G = G;
	a.chunks = chunks;
	a.threshold = st.threshold;
	a.fitHalfWidth = st.fitHalfWidth;
	a.maxIter = st.maxIterations ? st.maxIterations : 100u;
	a.peaks = dPeaks;
	a.averaged = dAvg;
	int rc;
	PeakState& mem = h->peakState;
	char* stage = nullptr;
	const size_t rowBytes = sizeof(float) * (size_t)j.L;
	if (!j.device) {
		const size_t unitRows = G <= oct::PEAK_CHUNK ? G : oct::PEAK_CHUNK;
		const size_t units = std::max<size_t>(1, kStageBytes / (rowBytes * unitRows));
		if ((rc = grow(h, mem, PeakState::STAGE, units * unitRows * rowBytes + 16))) return rc;
		stage = mem.as<char>(PeakState::STAGE);
	}
	auto setSource = [&](unsigned r0) {
		a.src = j.device ? static_cast<const float*>(j.mem) : reinterpret_cast<const float*>(stage);
		a.staged = j.device ? 0 : 1;
		a.r0 = r0;
		a.vec = vecOk(a) ? 1 : 0;
	};
	if (G <= oct::PEAK_CHUNK) {
		if (j.device) {
			setSource(0);
			a.qFirst = 0;
			a.qCount = Q;
			return launchB(h, fit, false, a);
		}
		const unsigned sliceGroups = (unsigned)std::max<size_t>(1, kStageBytes / (rowBytes * G));
		for (unsigned q0 = 0; q0 < Q; q0 += sliceGroups) {
			const unsigned q1 = std::min(Q, q0 + sliceGroups);
			if ((rc = stageRegionRows(h, j, stage, q0 * G, q1 * G, false))) return rc;
			setSource(q0 * G);
			a.qFirst = q0;
			a.qCount = q1 - q0;
			if ((rc = launchB(h, fit, false, a))) return rc;
		}
		return OCTPIPE_OK;
	}
	// G > 64: batches of groups whose partials fit kPartBytes
	const size_t groupPartBytes = sizeof(double) * (size_t)chunks * cnt;
	const unsigned batch = (unsigned)std::min<size_t>(Q, std::max<size_t>(1, kPartBytes / groupPartBytes));
	if ((rc = grow(h, mem, PeakState::PARTS, groupPartBytes * batch))) return rc;
	a.parts = mem.as<double>(PeakState::PARTS);
	const unsigned sliceChunks = j.device ? 0u : (unsigned)std::max<size_t>(1, kStageBytes / (rowBytes * oct::PEAK_CHUNK));
	for (unsigned q0 = 0; q0 < Q; q0 += batch) {
		const unsigned q1 = std::min(Q, q0 + batch);
		a.pFirst = q0;
		const unsigned g0 = q0 * chunks, g1 = q1 * chunks;
		if (j.device) {
			setSource(0);
			a.gFirst = g0;
			a.gCount = g1 - g0;
			HIP_TRY(oct::launch_peak_partials(a, h->stream));
		} else {
			for (unsigned ga = g0; ga < g1; ga += sliceChunks) {
				const unsigned gb = std::min(g1, ga + sliceChunks);
				// region rows of chunks [ga, gb): from the first row of chunk ga to the last row of chunk gb - 1
				const unsigned ra = (ga / chunks) * G + (ga % chunks) * oct::PEAK_CHUNK;
				const unsigned qe = (gb - 1) / chunks, ce = (gb - 1) % chunks;
				const unsigned rb = qe * G + std::min(G, (ce + 1) * oct::PEAK_CHUNK);
				if ((rc = stageRegionRows(h, j, stage, ra, rb, false))) return rc;
				setSource(ra);
				a.gFirst = ga;
				a.gCount = gb - ga;
				HIP_TRY(oct::launch_peak_partials(a, h->stream));
			}
		}
		a.qFirst = q0;
		a.qCount = q1 - q0;
		if ((rc = launchB(h, fit, true, a))) return rc;
	}
	return OCTPIPE_OK;
}

int entry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipePeakSettings* s, OctPipePeak* peaks,
          float* averaged, double* kernelMs) {
	// (the checks that need no handle come first)
	const std::string w(kWhat);
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region is NULL");
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	if (!peaks) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": peaks is NULL");
	const OctPipePeakSettings st = *s;
	if (std::isnan(st.threshold)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": threshold is NaN");
	if (st.maxIterations > kMaxIterations) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": maxIterations must be at most 1000");
	if (st.ascansPerGroup < 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": ascansPerGroup must be >= 1");
	if (data && r->buffer != 0 && r->buffer != 0xFFFFFFFFu)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": buffer must be 0 or 0xFFFFFFFF when data is given");
	int rc = enterCall(h, kWhat);
	if (rc) return rc;
	RegionSource j{};
	j.what = kWhat;
	j.src = oct::ST_F32;
	j.L = (unsigned)(h->N / 2);
	if ((rc = checkRegion(h, j, r))) return rc;
	if (j.r.sampleCount < 3) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region sampleCount must be at least 3");
	if (j.r.sampleCount > oct::PEAK_MAX_SAMPLES)
		return fail(OCTPIPE_ERR_UNSUPPORTED, w + ": region sampleCount must be at most 4096 (depth window of " + std::to_string(j.r.sampleCount) + ")");
	if (j.r.ascanCount % st.ascansPerGroup)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": ascansPerGroup = " + std::to_string(st.ascansPerGroup) + " must divide the region's ascanCount = " +
		                                              std::to_string(j.r.ascanCount));
	if ((rc = resolveProcessed(h, j, data, dataIsDevice))) return rc;
	const unsigned Q = j.r.bscanCount * (j.r.ascanCount / st.ascansPerGroup);
	const size_t avgBytes = sizeof(float) * (size_t)Q * j.r.sampleCount;
	PeakState& mem = h->peakState;
	if ((rc = grow(h, mem, PeakState::OUT, sizeof(OctPipePeak) * (size_t)Q))) return rc;
	if (averaged && (rc = grow(h, mem, PeakState::AVG, avgBytes))) return rc;
	StreamTimer timer(kernelMs != nullptr, kWhat);
	if ((rc = timer.begin(h->stream))) return rc;
	OctPipePeak* dPeaks = mem.as<OctPipePeak>(PeakState::OUT);
	float* dAvg = averaged ? mem.as<float>(PeakState::AVG) : nullptr;
	if ((rc = enqueue(h, j, st, Q, dPeaks, dAvg))) return rc;
	if ((rc = timer.end(h->stream))) return rc;
	if (averaged)
		if (hipError_t e = hipMemcpyAsync(averaged, dAvg, avgBytes, hipMemcpyDeviceToHost, h->stream); e != hipSuccess) return deviceError(j, e);
	return finish(h, j, timer, kernelMs, peaks, dPeaks, sizeof(OctPipePeak) * (size_t)Q);
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_peak_analysis(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipePeakSettings* s,
                          OctPipePeak* peaks, float* averaged) {
	return entry(h, data, dataIsDevice, r, s, peaks, averaged, nullptr);
}

int octpipe_debug_peak_analysis(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, const OctPipePeakSettings* s,
                                OctPipePeak* peaks, float* averaged, double* kernelMs) {
	return entry(h, data, dataIsDevice, r, s, peaks, averaged, kernelMs);
}

}  // extern "C"
