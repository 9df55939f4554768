// pipe_region.hip -- what the calls that read a region of a buffer share (include/octpipe.h "image statistics", "peak analysis"):
// the region's checks, the processed source (the handle's volume by slot, or a caller buffer) and the staging of a host source's
// region rows into device memory (pipe_stats.hip, pipe_peak.hip, pipe_surface.hip, pipe_angio.hip); for the last two also a host surface
// on its way in, the place of a result and the end of a call.
#include <algorithm>

#include "pipe_internal.h"

namespace octimpl {

int checkRegion(octpipe* h, RegionSource& j, const OctPipeStatsRegion* r) {
	const std::string w(j.what);
	j.r = *r;
	j.N = (unsigned)h->N;
	j.A = (unsigned)h->A;
	j.B = (unsigned)h->B;
	struct { uint32_t first, count, extent; const char* name; } ax[3] = {
		{r->firstBscan, r->bscanCount, j.B, "firstBscan / bscanCount"},
		{r->firstAscan, r->ascanCount, j.A, "firstAscan / ascanCount"},
		{r->firstSample, r->sampleCount, j.L, "firstSample / sampleCount"}};
	for (auto& x : ax)
		if (x.count < 1 || (uint64_t)x.first + x.count > x.extent)
			return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": region " + x.name + " must be a non-empty range inside [0, " + std::to_string(x.extent) + ")");
	return OCTPIPE_OK;
}

int resolveProcessed(octpipe* h, RegionSource& j, const float* data, int dataIsDevice) {
	const std::string w(j.what);
	if (data) {
		j.mem = data;
		j.device = dataIsDevice != 0;
		return OCTPIPE_OK;
	}
	const unsigned slot = j.r.buffer == 0xFFFFFFFFu ? h->bufferNumberInVolume : j.r.buffer;
	if (slot >= h->acq.buffersPerVolume)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": buffer must be below buffersPerVolume = " + std::to_string(h->acq.buffersPerVolume) +
		                                              " or 0xFFFFFFFF");
	if (!h->d_processedCur) return fail(OCTPIPE_ERR_NOT_INITIALIZED, w + ": no processed volume");
	j.mem = h->d_processedCur + (h->S / 2) * (size_t)slot;
	j.device = true;
	return OCTPIPE_OK;
}

size_t regionElemBytes(const RegionSource& j, uint64_t e0, uint64_t e1, size_t* off) {
	if (j.packed) {
		*off = (size_t)(e0 / 2 * 3);
		return (size_t)((e1 + 1) / 2 * 3) - *off;
	}
	const size_t eb = oct::format_elem_bytes(j.src);
	*off = (size_t)(e0 * eb);
	return (size_t)((e1 - e0) * eb);
}

int stageRegionRows(octpipe* h, const RegionSource& j, char* stage, unsigned r0, unsigned r1, bool parity) {
	const uint64_t N = j.L;  // elements per row
	const unsigned ac = j.r.ascanCount;
	const unsigned bFirst = r0 / ac;
	// one copy per B-scan run (runs of whole B-scans that follow each other in the buffer merge, except with parity spacing)
	size_t pendSrc = 0, pendDst = 0, pendLen = 0;
	int rc;
	auto flush = [&]() -> int {
		if (!pendLen) return OCTPIPE_OK;
		const hipError_t e = hipMemcpyAsync(stage + pendDst, static_cast<const char*>(j.mem) + pendSrc, pendLen, hipMemcpyHostToDevice, h->stream);
		pendLen = 0;
		if (e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, std::string(j.what) + ": " + hipGetErrorString(e));
		return OCTPIPE_OK;
	};
	for (unsigned b = bFirst; b * ac < r1; ++b) {
		const unsigned rk = std::max(r0, b * ac), rEnd = std::min(r1, (b + 1) * ac);
		const uint64_t rowIdx = ((uint64_t)j.r.firstBscan + b) * j.A + j.r.firstAscan + (rk - b * ac);
		const uint64_t srcE0 = rowIdx * N, srcE1 = srcE0 + (uint64_t)(rEnd - rk) * N;
		uint64_t dstE0 = (uint64_t)(rk - r0) * N;
		if (parity) dstE0 += 4ull * (b - bFirst) + ((rowIdx - rk + r0) & 1ull);
		size_t srcOff = 0, dstOff = 0;
		const size_t len = regionElemBytes(j, srcE0, srcE1, &srcOff);
		regionElemBytes(j, dstE0, dstE0 + 1, &dstOff);
		if (pendLen && !parity && pendSrc + pendLen == srcOff && pendDst + pendLen == dstOff) {
			pendLen += len;
			continue;
		}
		if ((rc = flush())) return rc;
		pendSrc = srcOff;
		pendDst = dstOff;
		pendLen = len;
	}
	return flush();
}

int surfaceIn(octpipe* h, const RegionSource& j, DeviceScratch& s, int slot, const int32_t* surface, int isDevice, size_t entries, const int32_t** dev) {
	if (isDevice) {
		*dev = surface;
		return OCTPIPE_OK;
	}
	int rc = grow(h, s, slot, sizeof(int32_t) * entries);
	if (rc) return rc;
	int32_t* d = s.as<int32_t>(slot);
	if (hipError_t e = hipMemcpyAsync(d, surface, sizeof(int32_t) * entries, hipMemcpyHostToDevice, h->stream); e != hipSuccess) return deviceError(j, e);
	*dev = d;
	return OCTPIPE_OK;
}

int resultOut(octpipe* h, DeviceScratch& s, int slot, void* out, int isDevice, size_t bytes, void** dev) {
	if (isDevice) {
		*dev = out;
		return OCTPIPE_OK;
	}
	int rc = grow(h, s, slot, bytes);
	if (rc) return rc;
	*dev = s.p[slot];
	return OCTPIPE_OK;
}

int finish(octpipe* h, const RegionSource& j, const StreamTimer& timer, double* kernelMs, void* hostOut, const void* dev, size_t bytes) {
	hipError_t e = hipSuccess;
	if (hostOut && bytes) e = hipMemcpyAsync(hostOut, dev, bytes, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess && (hostOut || kernelMs)) e = hipStreamSynchronize(h->stream);
	if (e == hipSuccess) e = timer.elapsedMs(kernelMs);
	if (e != hipSuccess) return deviceError(j, e);
	return OCTPIPE_OK;
}

}  // namespace octimpl
