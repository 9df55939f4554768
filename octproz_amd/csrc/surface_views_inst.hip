// surface_views_inst.hip -- instantiates the surface view kernels (surface_views.h): detection, smoothing for every radius, both en
// face functions, both load forms of the flattening.
#include "surface_views.h"

namespace oct {

// one wave per A-scan; see surface_views.h
__global__ __launch_bounds__(SURF_THREADS) void oct_surface_detect_kernel(const SurfArgs a, const float threshold, const unsigned run,
                                                                           int32_t* __restrict__ out) {
	const unsigned lane = threadIdx.x & 63;
	const unsigned long long ri = (unsigned long long)blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6);
	if (ri >= a.rCount) return;
	const unsigned r = a.rFirst + (unsigned)ri;
	const float* p = surf_row(a, r) + a.s0;
	unsigned carry = 0;  // bins above the threshold that end the previous chunk (always below `run`)
	int hit = -1;        // relative to s0
	for (unsigned base = 0; base < a.cnt && hit < 0; base += DETECT_STEP) {
		bool above[DETECT_STEP / DETECT_LANES];
#pragma unroll
		for (unsigned c = 0; c < DETECT_STEP / DETECT_LANES; c++) {
			const unsigned i = base + c * DETECT_LANES + lane;
			above[c] = i < a.cnt ? p[i] > threshold : false;
		}
#pragma unroll
		for (unsigned c = 0; c < DETECT_STEP / DETECT_LANES; c++) {
			const unsigned first = base + c * DETECT_LANES;
			const unsigned long long m = __ballot(above[c]);
			if (hit >= 0 || first >= a.cnt) continue;
			const unsigned lead = ~m ? (unsigned)__builtin_ctzll(~m) : 64u;
			if (carry && carry + lead >= run) {
				hit = (int)(first - carry);
				continue;
			}
			const unsigned long long y = surf_runs(m, run);
			if (y) {
				hit = (int)(first + (unsigned)__builtin_ctzll(y));
				continue;
			}
			carry = ~m ? (unsigned)__builtin_clzll(~m) : 64u;
		}
	}
	if (lane == 0) out[r] = hit < 0 ? -1 : (int32_t)(a.s0 + (unsigned)hit);
}

hipError_t launch_surface_detect(const SurfArgs& a, float threshold, unsigned run, int32_t* out, hipStream_t s) {
	const unsigned groups = (a.rCount + SURF_THREADS / 64 - 1) / (SURF_THREADS / 64);
	hipLaunchKernelGGL(oct_surface_detect_kernel, dim3(groups), dim3(SURF_THREADS), 0, s, a, threshold, run, out);
	return hipGetLastError();
}

hipError_t launch_surface_smooth(const int32_t* in, unsigned rows, unsigned cols, unsigned radius, int32_t* out, hipStream_t s) {
	const unsigned long long n = (unsigned long long)rows * cols;
	const dim3 grid((unsigned)((n + SURF_THREADS - 1) / SURF_THREADS)), block(SURF_THREADS);
	switch (radius) {
	case 0: hipLaunchKernelGGL(oct_surface_smooth_kernel<0>, grid, block, 0, s, in, rows, cols, out); break;
	case 1: hipLaunchKernelGGL(oct_surface_smooth_kernel<1>, grid, block, 0, s, in, rows, cols, out); break;
	case 2: hipLaunchKernelGGL(oct_surface_smooth_kernel<2>, grid, block, 0, s, in, rows, cols, out); break;
	case 3: hipLaunchKernelGGL(oct_surface_smooth_kernel<3>, grid, block, 0, s, in, rows, cols, out); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

hipError_t launch_surface_enface(int function, const EnfaceArgs& a, hipStream_t s) {
	const dim3 grid((a.g.rCount + SURF_THREADS - 1) / SURF_THREADS), block(SURF_THREADS);
	if (function == 0) hipLaunchKernelGGL(oct_surface_enface_kernel<0>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(oct_surface_enface_kernel<1>, grid, block, 0, s, a);
	return hipGetLastError();
}

hipError_t launch_flatten(unsigned loads, const FlattenArgs& a, hipStream_t s) {
	const unsigned rowsPerGroup = FLAT_ROWS * (SURF_THREADS / 64);
	const dim3 grid((a.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
	if (loads == 2) hipLaunchKernelGGL(oct_flatten_kernel<2>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(oct_flatten_kernel<1>, grid, block, 0, s, a);
	return hipGetLastError();
}

}  // namespace oct
