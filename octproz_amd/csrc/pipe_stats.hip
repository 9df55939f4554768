// pipe_stats.hip -- image statistics of a region (include/octpipe.h "image statistics"; reference docs:
// docs/docs/plugin-imagestatistics.md).
//
//   octpipe_processed_statistics   oct_stats_kernel<ST_F32> over the handle's processed volume or a caller's float buffer
//   octpipe_raw_statistics         oct_stats_kernel<PH_*> over one raw buffer in the handle's sample format
// The region, the processed source (slot rules, caller buffer) and the host staging are pipe_region.hip's, shared with the peak
// analysis.  Explicit range: one pass (moments and histogram) and the finish kernel.  autoRange: the moments pass, the finish kernel (which
// derives the range on the device), the histogram pass that reads it.  A host source is staged in slices of whole segments, only
// the region's rows, so the segment partials -- and the bits of the moments -- are those of the device source.  Everything runs on
// the handle's compute stream behind what is already enqueued there and touches nothing the processing chain reads or writes; the
// scratch belongs to the handle (StatsState, released in octpipe_destroy).
#include <algorithm>
#include <cfloat>
#include <limits>

#include "pipe_internal.h"
#include "image_stats.h"

namespace oct {
hipError_t launch_stats(int src, bool vec, unsigned groups, size_t lds, const StatsArgs& a, hipStream_t s);
hipError_t launch_stats_hist_sum(const unsigned* slab, unsigned rows, unsigned cols, unsigned long long* histOut, hipStream_t s);
hipError_t launch_stats_finish(const StatsFinishArgs& f, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr size_t kStageBytes = 64ull << 20;  // host rows staged per slice (at least one segment)
constexpr unsigned kMaxGroups = 2048;        // workgroups of a pass: 8 per CU of an MI355X ...
constexpr unsigned kMaxGroupsWide = 1024;    // ... 4 per CU above 512 bins (each stores bins + 2 counts into the slab)
constexpr uint32_t kLastSlot = 0xFFFFFFFFu;

// what one call reads: the source (RegionSource, pipe_internal.h) and the region's item space
struct Job : RegionSource {
	unsigned V, G, rows, segRows, segments;
	unsigned bins;
};

int validate(octpipe* h, Job& j, const OctPipeStatsRegion* r, unsigned bins) {
	j.bins = bins;
	int rc = checkRegion(h, j, r);
	if (rc) return rc;
	j.V = oct::format_vector(j.src);
	j.G = (r->sampleCount + j.V - 1) / j.V;
	j.rows = r->bscanCount * r->ascanCount;  // <= A * B
	// segment size from the shape alone: STATS_SEG_TARGET segments where each still gives every lane an item, at most STATS_SEG_VALUES values
	const uint64_t items = (uint64_t)j.rows * j.G;
	const uint64_t segItems = std::min<uint64_t>(oct::STATS_SEG_VALUES / j.V, std::max<uint64_t>(oct::STATS_THREADS, (items + oct::STATS_SEG_TARGET - 1) / oct::STATS_SEG_TARGET));
	j.segRows = (unsigned)std::max<uint64_t>(1, segItems / j.G);
	j.segments = (j.rows + j.segRows - 1) / j.segRows;
	return OCTPIPE_OK;
}

oct::StatsArgs baseArgs(octpipe* h, const Job& j) {
	oct::StatsArgs a{};
	a.A = j.A;
	a.fb = j.r.firstBscan;
	a.fa = j.r.firstAscan;
	a.ac = j.r.ascanCount;
	a.L = j.L;
	a.s0 = j.r.firstSample;
	a.cnt = j.r.sampleCount;
	a.G = j.G;
	a.mG = oct::stats_magic(j.G);
	a.mAc = oct::stats_magic(j.r.ascanCount);
	a.rows = j.rows;
	a.segRows = j.segRows;
	a.bitshift = h->params.bitshift ? 1 : 0;
	a.bins = j.bins;
	a.parts = h->statsState.as<oct::StatsPart>(StatsState::PARTS);
	a.slab = h->statsState.as<unsigned>(StatsState::SLAB);
	return a;
}

// workgroups of a histogram pass at most; a workgroup's uint32 counters stay below 2^31 (each holds at most the values of the
// segments it takes)
unsigned groupCap(const Job& j) {
	const uint64_t values = (uint64_t)j.rows * j.r.sampleCount;
	const unsigned cap = j.bins > 512 ? kMaxGroupsWide : kMaxGroups;
	return (unsigned)std::max<uint64_t>(cap, (values >> 31) + 1);
}

int launch(octpipe* h, const Job& j, oct::StatsArgs& a, unsigned segFirst, unsigned segCount) {
	// the vector form: every item one aligned load (16 bytes; packed: 12 bytes of dword alignment, element index % 8 == 0)
	const uintptr_t base = reinterpret_cast<uintptr_t>(a.src);
	const bool vec = !a.parity && a.L % j.V == 0 && a.s0 % j.V == 0 && base % (j.packed ? 4 : 16) == 0;
	a.segFirst = segFirst;
	a.segCount = segCount;
	const unsigned groups = std::min(segCount, groupCap(j));
	HIP_TRY(oct::launch_stats(j.src, vec, groups, a.hist ? sizeof(unsigned) * j.bins : 0, a, h->stream));
	if (a.hist) HIP_TRY(oct::launch_stats_hist_sum(a.slab, groups, j.bins + 2, a.histOut, h->stream));
	return OCTPIPE_OK;
}

// one pass over the region: the device source in one launch, a host source in slices of whole segments
int pass(octpipe* h, const Job& j, const oct::StatsArgs& proto) {
	oct::StatsArgs a = proto;
	if (j.device) {
		a.src = j.mem;
		a.staged = 0;
		return launch(h, j, a, 0, j.segments);
	}
	const uint64_t N = j.L;  // elements per row
	const bool parity = j.packed && (j.N & 1u);
	size_t off = 0;
	const size_t rowBytes = regionElemBytes(j, 0, N, &off) + 3;  // (packed: the partial sample pair on either side)
	const unsigned sliceSegs = (unsigned)std::max<size_t>(1, kStageBytes / (rowBytes * j.segRows + 64));
	const size_t sliceRows = std::min<size_t>((size_t)sliceSegs * j.segRows, j.rows);
	const unsigned ac = j.r.ascanCount;
	// the staging of one slice: rows * N elements, plus 4 per B-scan run for the parity spacing, plus a 16-byte tail
	const size_t maxRuns = sliceRows / ac + 2;
	size_t stageBytes = regionElemBytes(j, 0, (uint64_t)sliceRows * N + (parity ? 4 * maxRuns + 2 : 0), &off) + 16;
	int rc = grow(h, h->statsState, StatsState::STAGE, stageBytes);
	if (rc) return rc;
	char* stage = h->statsState.as<char>(StatsState::STAGE);
	a.src = stage;
	a.staged = 1;
	a.parity = parity ? 1 : 0;
	for (unsigned s0 = 0; s0 < j.segments; s0 += sliceSegs) {
		const unsigned segs = std::min(sliceSegs, j.segments - s0);
		const unsigned r0 = s0 * j.segRows, r1 = std::min<unsigned>(j.rows, (s0 + segs) * j.segRows);
		const unsigned bFirst = r0 / ac;
		if ((rc = stageRegionRows(h, j, stage, r0, r1, parity))) return rc;
		a.r0 = r0;
		a.bFirst = bFirst;
		if ((rc = launch(h, j, a, s0, segs))) return rc;
	}
	return OCTPIPE_OK;
}

// the whole call: passes, finish kernel, results to the host
int run(octpipe* h, Job& j, int autoRange, const oct::StatsRange& range, uint64_t* histogram, OctPipeImageStatistics* out, double* kernelMs) {
	int rc;
	StatsState& mem = h->statsState;
	if ((rc = grow(h, mem, StatsState::PARTS, sizeof(oct::StatsPart) * j.segments))) return rc;
	if ((rc = grow(h, mem, StatsState::OUT, sizeof(oct::StatsResult) + sizeof(uint64_t) * (oct::STATS_MAX_BINS + 2)))) return rc;
	if ((rc = grow(h, mem, StatsState::SLAB, sizeof(unsigned) * (size_t)groupCap(j) * (j.bins + 2)))) return rc;
	StreamTimer timer(kernelMs != nullptr, j.what);
	const std::string w(j.what);
	if ((rc = timer.begin(h->stream))) return rc;
	char* outBlock = mem.as<char>(StatsState::OUT);
	unsigned long long* dHist = reinterpret_cast<unsigned long long*>(outBlock + sizeof(oct::StatsResult));
	if (hipMemsetAsync(dHist, 0, sizeof(uint64_t) * (j.bins + 2), h->stream) != hipSuccess)
		return fail(OCTPIPE_ERR_DEVICE, w + ": memset");
	oct::StatsArgs a = baseArgs(h, j);
	a.histOut = dHist;
	oct::StatsFinishArgs f{};
	f.parts = a.parts;
	f.segments = j.segments;
	f.raw = j.src != oct::ST_F32;
	f.autoRange = autoRange;
	f.bins = j.bins;
	f.range = range;
	f.out = reinterpret_cast<oct::StatsResult*>(outBlock);
	a.range = range;
	a.moments = 1;
	a.hist = autoRange ? 0 : 1;
	if ((rc = pass(h, j, a))) return rc;
	if (hipError_t e = oct::launch_stats_finish(f, h->stream); e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, w + ": " + hipGetErrorString(e));
	if (autoRange) {
		a.moments = 0;
		a.hist = 1;
		a.devRange = &f.out->range;
		if ((rc = pass(h, j, a))) return rc;
	}
	if ((rc = timer.end(h->stream))) return rc;
	std::vector<char> block(sizeof(oct::StatsResult) + sizeof(uint64_t) * (j.bins + 2));
	hipError_t e = hipMemcpyAsync(block.data(), outBlock, block.size(), hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
	if (e == hipSuccess) e = timer.elapsedMs(kernelMs);
	if (e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, w + ": " + hipGetErrorString(e));
	oct::StatsResult res;
	std::memcpy(&res, block.data(), sizeof(res));
	std::vector<uint64_t> hist(j.bins + 2);
	std::memcpy(hist.data(), block.data() + sizeof(res), sizeof(uint64_t) * hist.size());
	const double nan = std::numeric_limits<double>::quiet_NaN();
	const oct::StatsPart& m = res.m;
	out->count = (uint64_t)m.n;
	out->underflow = hist[j.bins];
	out->overflow = hist[j.bins + 1];
	out->nonFinite = m.nonFinite;
	const bool any = m.n > 0.0;
	out->min = any ? m.mn : nan;
	out->max = any ? m.mx : nan;
	out->mean = any ? m.mean : nan;
	out->stddev = any ? std::sqrt(m.m2 / m.n) : nan;
	const oct::StatsRange& R = res.range;
	if (f.raw) {
		out->lo = (double)R.rlo;
		out->binWidth = (double)R.width;
		out->hi = (double)R.rlo + (double)j.bins * (double)R.width;
	} else {
		out->lo = (double)R.lo;
		out->hi = (double)R.hi;
		out->binWidth = ((double)R.hi - (double)R.lo) / (double)j.bins;
	}
	if (histogram) std::memcpy(histogram, hist.data(), sizeof(uint64_t) * j.bins);
	return OCTPIPE_OK;
}

float processedScale(unsigned bins, float lo, float hi) {
	if (lo == hi) return 0.0f;
	const double s = (double)bins / ((double)hi - (double)lo);
	return s > (double)FLT_MAX ? FLT_MAX : (float)s;
}

int processedEntry(octpipe* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange, float lo, float hi,
                   uint64_t* histogram, OctPipeImageStatistics* out, double* kernelMs) {
	// (the checks that need no handle come first)
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "processed statistics: region is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "processed statistics: out is NULL");
	if (bins < 1 || bins > oct::STATS_MAX_BINS) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "processed statistics: bins must lie in [1, 4096]");
	oct::StatsRange R{};
	if (!autoRange) {
		if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
			return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "processed statistics: need finite lo < hi (or autoRange)");
		R.lo = lo;
		R.hi = hi;
		R.scale = processedScale(bins, lo, hi);
	}
	if (data && r->buffer != 0 && r->buffer != kLastSlot)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "processed statistics: buffer must be 0 or 0xFFFFFFFF when data is given");
	int rc = enterCall(h, "processed statistics");
	if (rc) return rc;
	Job j{};
	j.what = "processed statistics";
	j.src = oct::ST_F32;
	j.L = (unsigned)(h->N / 2);
	if ((rc = validate(h, j, r, bins))) return rc;
	if ((rc = resolveProcessed(h, j, data, dataIsDevice))) return rc;
	return run(h, j, autoRange ? 1 : 0, R, histogram, out, kernelMs);
}

int rawEntry(octpipe* h, const void* raw, int rawIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange, int64_t lo, uint32_t binWidth,
             uint64_t* histogram, OctPipeImageStatistics* out, double* kernelMs) {
	if (!raw) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "raw statistics: raw is NULL");
	if (!r) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "raw statistics: region is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "raw statistics: out is NULL");
	if (bins < 1 || bins > oct::STATS_MAX_BINS) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "raw statistics: bins must lie in [1, 4096]");
	oct::StatsRange R{};
	if (!autoRange) {
		if (binWidth < 1) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "raw statistics: binWidth must be >= 1 (or autoRange)");
		R.rlo = lo;
		R.width = binWidth;
		R.limit = (uint64_t)binWidth * bins;
		R.invWidth = 1.0 / (double)binWidth;
	}
	int rc = enterCall(h, "raw statistics");
	if (rc) return rc;
	Job j{};
	j.what = "raw statistics";
	j.src = oct::ph_format(h->sampleFormat, h->acq.bitDepth);
	j.packed = oct::format_packed(j.src);
	j.L = (unsigned)h->N;
	if ((rc = validate(h, j, r, bins))) return rc;
	j.mem = raw;
	j.device = rawIsDevice != 0;
	return run(h, j, autoRange ? 1 : 0, R, histogram, out, kernelMs);
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_processed_statistics(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange, float lo,
                                 float hi, uint64_t* histogram, OctPipeImageStatistics* out) {
	return processedEntry(h, data, dataIsDevice, r, bins, autoRange, lo, hi, histogram, out, nullptr);
}

int octpipe_raw_statistics(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange, int64_t lo,
                           uint32_t binWidth, uint64_t* histogram, OctPipeImageStatistics* out) {
	return rawEntry(h, raw, rawIsDevice, r, bins, autoRange, lo, binWidth, histogram, out, nullptr);
}

int octpipe_debug_processed_statistics(octpipe_t* h, const float* data, int dataIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange,
                                       float lo, float hi, uint64_t* histogram, OctPipeImageStatistics* out, double* kernelMs) {
	return processedEntry(h, data, dataIsDevice, r, bins, autoRange, lo, hi, histogram, out, kernelMs);
}

int octpipe_debug_raw_statistics(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeStatsRegion* r, unsigned bins, int autoRange,
                                 int64_t lo, uint32_t binWidth, uint64_t* histogram, OctPipeImageStatistics* out, double* kernelMs) {
	return rawEntry(h, raw, rawIsDevice, r, bins, autoRange, lo, binWidth, histogram, out, kernelMs);
}

}  // extern "C"
