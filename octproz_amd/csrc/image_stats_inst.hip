// image_stats_inst.hip -- instantiates the image statistics kernels (image_stats.h): one streaming kernel per source container
// (float32 processed, the eight raw containers) in a vector and a scalar form, the slab sum and the finish kernel.
#include "image_stats.h"

namespace oct {

// the slab rows of one pass summed into the uint64 histogram: thread = column, blockIdx.y = a run of rows, one atomic
// per non-zero (column, run of STATS_SUM_ROWS rows)
__global__ __launch_bounds__(STATS_THREADS) void oct_stats_hist_sum_kernel(const unsigned* slab, unsigned rows, unsigned cols,
                                                                            unsigned long long* histOut) {
	const unsigned col = blockIdx.x * STATS_THREADS + threadIdx.x;
	if (col >= cols) return;
	const unsigned r0 = blockIdx.y * STATS_SUM_ROWS;
	unsigned c[STATS_SUM_ROWS];
#pragma unroll
	for (int k = 0; k < STATS_SUM_ROWS; k++) c[k] = r0 + k < rows ? slab[(size_t)(r0 + k) * cols + col] : 0u;  // all loads in flight
	unsigned long long s = 0;
#pragma unroll
	for (int k = 0; k < STATS_SUM_ROWS; k++) s += c[k];
	if (s) atomicAdd(histOut + col, s);
}

__global__ __launch_bounds__(STATS_THREADS) void oct_stats_finish_kernel(const StatsFinishArgs f) {
	__shared__ StatsPart waveParts[STATS_THREADS / 64];
	const unsigned t = threadIdx.x;
	const unsigned per = (f.segments + STATS_THREADS - 1) / STATS_THREADS;
	StatsPart p;
	p.n = p.mean = p.m2 = 0.0;
	p.mn = __builtin_inf();
	p.mx = -__builtin_inf();
	p.nonFinite = 0;
	for (unsigned i = t * per; i < min(f.segments, (t + 1) * per); i++) p = stats_merge(p, f.parts[i]);
	p = stats_block_reduce(p, waveParts);
	if (t != 0) return;
	StatsRange R = f.range;
	if (f.autoRange) {
		if (f.raw) {
			// (the region is never empty: n >= 1)
			R.rlo = (long long)p.mn;
			const unsigned long long span = (unsigned long long)((long long)p.mx - R.rlo) + 1ull;
			unsigned long long w = (span + f.bins - 1) / f.bins;
			R.width = w < 1 ? 1 : w;
			R.limit = R.width * f.bins;
			R.invWidth = 1.0 / (double)R.width;
		} else if (p.n == 0.0) {
			R.lo = R.hi = __builtin_nanf("");
			R.scale = 0.0f;
		} else {
			R.lo = (float)p.mn;
			R.hi = (float)p.mx;
			const double s = R.lo == R.hi ? 0.0 : (double)f.bins / ((double)R.hi - (double)R.lo);
			R.scale = s > 3.4028234663852886e38 ? 3.4028234663852886e38f : (float)s;
		}
	}
	f.out->m = p;
	f.out->range = R;
}

namespace {

template <int F> hipError_t launchF(bool vec, unsigned groups, size_t lds, const StatsArgs& a, hipStream_t s) {
	if (vec) hipLaunchKernelGGL((oct_stats_kernel<F, true>), dim3(groups), dim3(STATS_THREADS), lds, s, a);
	else hipLaunchKernelGGL((oct_stats_kernel<F, false>), dim3(groups), dim3(STATS_THREADS), lds, s, a);
	return hipGetLastError();
}
template hipError_t launchF<ST_F32>(bool, unsigned, size_t, const StatsArgs&, hipStream_t);  // (its kernels stay the first of the code object)

}  // namespace

// src: ST_F32 or PH_*; lds: bins * 4 bytes when a.hist, else 0
hipError_t launch_stats(int src, bool vec, unsigned groups, size_t lds, const StatsArgs& a, hipStream_t s) {
	return with_format<ST_COUNT>(src, hipErrorInvalidValue, [&](auto F) { return launchF<F()>(vec, groups, lds, a, s); });
}

hipError_t launch_stats_hist_sum(const unsigned* slab, unsigned rows, unsigned cols, unsigned long long* histOut, hipStream_t s) {
	const dim3 grid((cols + STATS_THREADS - 1) / STATS_THREADS, (rows + STATS_SUM_ROWS - 1) / STATS_SUM_ROWS);
	hipLaunchKernelGGL(oct_stats_hist_sum_kernel, grid, dim3(STATS_THREADS), 0, s, slab, rows, cols, histOut);
	return hipGetLastError();
}

hipError_t launch_stats_finish(const StatsFinishArgs& f, hipStream_t s) {
	hipLaunchKernelGGL(oct_stats_finish_kernel, dim3(1), dim3(STATS_THREADS), 0, s, f);
	return hipGetLastError();
}

}  // namespace oct
