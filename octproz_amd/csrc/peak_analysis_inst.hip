// peak_analysis_inst.hip -- instantiates the peak analysis kernels (peak_analysis.h): the chunk partials (stage A) and the per-group
// analysis with and without the fit, from the source rows or from the partials (stage B).
#include "peak_analysis.h"

namespace oct {

// stage A: one wave per (chunk, tile of 256 samples), lane l samples 4l .. 4l + 3 of the tile; float64 partials of the chunk's rows
__global__ __launch_bounds__(PEAK_THREADS) void oct_peak_partials_kernel(const PeakArgs a) {
	const unsigned lane = threadIdx.x & 63;
	const unsigned tiles = (a.cnt + PEAK_TILE - 1) / PEAK_TILE;
	const unsigned item = blockIdx.x * (PEAK_THREADS / 64) + (threadIdx.x >> 6);
	if (item >= a.gCount * tiles) return;
	const unsigned g = a.gFirst + item / tiles, tile = item % tiles;
	const unsigned q = g / a.chunks, c = g - q * a.chunks;
	const unsigned s = tile * PEAK_TILE + lane * 4;
	if (s >= a.cnt) return;
	const unsigned rowFirst = q * a.G + c * PEAK_CHUNK;
	const unsigned n = min(PEAK_CHUNK, a.G - c * PEAK_CHUNK);
	double v[4] = {-0.0, -0.0, -0.0, -0.0};
	peak_add_rows(a, peak_row(a, rowFirst), n, s, v);
	double* out = a.parts + ((size_t)(q - a.pFirst) * a.chunks + c) * a.cnt + s;
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (s + j < a.cnt) out[j] = v[j];
}

// stage A over the chunks [a.gFirst, a.gFirst + a.gCount): four (chunk, tile) items per workgroup
hipError_t launch_peak_partials(const PeakArgs& a, hipStream_t s) {
	const unsigned tiles = (a.cnt + PEAK_TILE - 1) / PEAK_TILE;
	const unsigned long long items = (unsigned long long)a.gCount * tiles;
	const unsigned groups = (unsigned)((items + PEAK_THREADS / 64 - 1) / (PEAK_THREADS / 64));
	hipLaunchKernelGGL(oct_peak_partials_kernel, dim3(groups), dim3(PEAK_THREADS), 0, s, a);
	return hipGetLastError();
}

// stage B over the groups [a.qFirst, a.qFirst + a.qCount): `waves` groups per workgroup, each with an LDS slice of a.cnt floats
hipError_t launch_peak(bool fit, bool fromPartials, unsigned waves, const PeakArgs& a, hipStream_t s) {
	const unsigned groups = (a.qCount + waves - 1) / waves;
	const size_t lds = sizeof(float) * a.cnt * waves;
	const dim3 grid(groups), block(64 * waves);
	if (fit) {
		if (fromPartials) hipLaunchKernelGGL((oct_peak_kernel<true, true>), grid, block, lds, s, a);
		else hipLaunchKernelGGL((oct_peak_kernel<true, false>), grid, block, lds, s, a);
	} else {
		if (fromPartials) hipLaunchKernelGGL((oct_peak_kernel<false, true>), grid, block, lds, s, a);
		else hipLaunchKernelGGL((oct_peak_kernel<false, false>), grid, block, lds, s, a);
	}
	return hipGetLastError();
}

}  // namespace oct
