// dispersion_sweep.h -- scoring of dispersion candidates (octpipe_dispersion_scores, include/octpipe.h "dispersion estimation").
//
// The Dispersion Estimator extension of the reference (docs/docs/plugin-dispersionestimator.md) processes M A-scans of one raw
// frame once per candidate (d2, d3) and reduces every processed A-scan to one image metric.  Between candidates only the phasor
// changes, so the front end (unpack, rolling average, k-linearisation, window: oct_prepare_rows_* + oct_lib_gather_kernel with a
// unit phasor) runs once per call and this kernel does the rest per (candidate, A-scan): one wave multiplies the prepared row by
// the candidate's phasor, transforms it with the in-register FFT of the product (fft_wave, kernels.h), scales |z| exactly as the
// product's epilogue does (cu:699-741) and reduces the N/2 values of the A-scan to one metric in registers.  Nothing of the
// transformed A-scan reaches memory but that one float.
//
// Metric over the bins k in [ignore, N/2) of one A-scan (values v[k] as the product writes them):
//   SUM_ABOVE_THRESHOLD      sum of v[k] > threshold
//   SAMPLES_ABOVE_THRESHOLD  count of v[k] > threshold
//   PEAK_VALUE               max v[k]
//   MEAN_SOBEL               sum of |v[k+1] - v[k-1]|, k in [ignore+1, N/2-2] (the neighbours go through the wave's LDS slice)
// Every sum runs in a fixed order (a lane's bins in register order, then a butterfly across the wave): two calls give the same
// bits, and so does any split of the candidate list over launches.
#pragma once
#include "kernels.h"

namespace oct {

enum { SWEEP_SUM_ABOVE = 0, SWEEP_SAMPLES_ABOVE = 1, SWEEP_PEAK = 2, SWEEP_SOBEL = 3 };

struct SweepArgs {
	const f2* rows;     // [M][N] prepared rows: x = resampled sample * window, y = 0 (oct_lib_gather_kernel with a unit phasor)
	const f2* phasor;   // [K][N] e^{i theta_c[j]} of the candidates (oct_sweep_phasor_kernel)
	const f2* twiddle;  // the canonical per-pass tables of Plan<LOG2N> (uploadTwiddles)
	float* metric;      // [K][M]
	unsigned K, M;
	int ignore, metricKind, logScale;
	float threshold, sA, sB;
};

// one wave per (candidate, A-scan); a workgroup's waves share the twiddle table in LDS.  N = 4096 holds 64 complex points per lane
// (128 VGPRs of data): 4 waves per workgroup like the Bluestein kernel at that length
template <int LOG2N> constexpr int sweep_waves() { return LOG2N >= 12 ? 4 : 8; }
template <int LOG2N> constexpr int sweep_lds_bytes() { return tw_lds_bytes<LOG2N>() + sweep_waves<LOG2N>() * wave_lds_bytes<(1 << LOG2N)>(); }

OCT_DEV float wave_sum(float x) {
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s);  // a + b == b + a: every lane ends with the same bits
	return x;
}
OCT_DEV float wave_max(float x) {
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) x = fmaxf(x, __shfl_xor(x, s));
	return x;
}
OCT_DEV int wave_sum_int(int x) {
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s);
	return x;
}

template <int LOG2N>
__global__ __launch_bounds__(sweep_waves<LOG2N>() * 64) void oct_dispersion_sweep_kernel(const SweepArgs a) {
	constexpr int N = 1 << LOG2N, P = N / 64, HALF = N / 2;
	constexpr int WAVES = sweep_waves<LOG2N>(), THREADS = WAVES * 64;
	constexpr int RL = LastRadix<LOG2N>::value, NBL = P / RL;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	f2* tw = reinterpret_cast<f2*>(smem);
	const int tid = threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	char* wbase = smem + tw_lds_bytes<LOG2N>() + wave * wave_lds_bytes<N>();
	f2* xbuf = reinterpret_cast<f2*>(wbase);
	float* vals = reinterpret_cast<float*>(wbase);  // MEAN_SOBEL: the A-scan's N/2 values (the transform's exchange buffer is dead by then)
	fill_twiddles<LOG2N>(tw, a.twiddle, tid, THREADS);
	__syncthreads();

	const unsigned total = a.K * a.M, wavesTotal = gridDim.x * (unsigned)WAVES;
	for (unsigned item = blockIdx.x * (unsigned)WAVES + (unsigned)wave; item < total; item += wavesTotal) {
		const unsigned c = item / a.M, m = item - c * a.M;  // consecutive waves: one candidate's phasor, neighbouring rows
		const f2* y = a.rows + (size_t)m * N + lane;
		const f2* ph = a.phasor + (size_t)c * N + lane;
		f2 v[P];
#pragma unroll
		for (int q = 0; q < P; q++) {
			// the product's gather: (y w) * phasor per component (oct_lib_gather_kernel, the non-LDS-LUT form of oct_fused_kernel)
			const float yw = y[64 * q].x;
			const f2 w = ph[64 * q];
			v[q] = f2{yw * w.x, yw * w.y};
		}
		wave_sync_lds();
		fft_wave<LOG2N, true>(v, xbuf, tw, lane);  // bin lane + 64 m + u N/RL in v[m + u NBL], u < RL/2

		// the product's epilogue without mean line (fixed-pattern-noise removal is off for every candidate)
		float o[P / 2];
#pragma unroll
		for (int u = 0; u < RL / 2; u++)
#pragma unroll
			for (int mm = 0; mm < NBL; mm++) {
				const f2 z = v[mm + u * NBL];
				const float p = z.x * z.x + z.y * z.y;
				const float s = a.logScale ? __builtin_amdgcn_logf(p) : __builtin_amdgcn_sqrtf(p);
				o[mm + u * NBL] = a.sA * s + a.sB;
			}
		float result;
		if (a.metricKind == SWEEP_SOBEL) {
			wave_sync_lds();
#pragma unroll
			for (int u = 0; u < RL / 2; u++)
#pragma unroll
				for (int mm = 0; mm < NBL; mm++) vals[fft_bin<LOG2N>(lane, mm, u)] = o[mm + u * NBL];
			wave_sync_lds();
			float acc = 0.0f;
#pragma unroll
			for (int u = 0; u < RL / 2; u++)
#pragma unroll
				for (int mm = 0; mm < NBL; mm++) {
					const int k = fft_bin<LOG2N>(lane, mm, u);
					// (k - 1 >= 0 and k + 1 < N/2 inside the range; the clamped indices keep the reads in the slice for the others)
					const float d = fabsf(vals[min(k + 1, HALF - 1)] - vals[max(k - 1, 0)]);
					if (k >= a.ignore + 1 && k <= HALF - 2) acc += d;
				}
			result = wave_sum(acc);
		} else if (a.metricKind == SWEEP_PEAK) {
			// (fmaxf drops a NaN; the metric keeps it, like the sums do: a candidate whose phase is not a number never wins)
			float best = -INFINITY;
			int nan = 0;
#pragma unroll
			for (int u = 0; u < RL / 2; u++)
#pragma unroll
				for (int mm = 0; mm < NBL; mm++)
					if (fft_bin<LOG2N>(lane, mm, u) >= a.ignore) {
						best = fmaxf(best, o[mm + u * NBL]);
						nan |= o[mm + u * NBL] != o[mm + u * NBL];
					}
			result = wave_sum_int(nan) ? __builtin_nanf("") : wave_max(best);
		} else if (a.metricKind == SWEEP_SAMPLES_ABOVE) {
			int cnt = 0;
#pragma unroll
			for (int u = 0; u < RL / 2; u++)
#pragma unroll
				for (int mm = 0; mm < NBL; mm++) cnt += (fft_bin<LOG2N>(lane, mm, u) >= a.ignore && o[mm + u * NBL] > a.threshold) ? 1 : 0;
			result = (float)wave_sum_int(cnt);
		} else {
			float acc = 0.0f;
#pragma unroll
			for (int u = 0; u < RL / 2; u++)
#pragma unroll
				for (int mm = 0; mm < NBL; mm++)
					if (fft_bin<LOG2N>(lane, mm, u) >= a.ignore && o[mm + u * NBL] > a.threshold) acc += o[mm + u * NBL];
			result = wave_sum(acc);
		}
		if (lane == 0) a.metric[(size_t)c * a.M + m] = result;
		wave_sync_lds();
	}
}

// one instance per transform length (dispersion_sweep_inst.hip, compiled once per OCT_LOG2N)
#define OCT_DECL_SWEEP(L) hipError_t launch_dispersion_sweep_##L(const SweepArgs& a, hipStream_t stream);
OCT_DECL_SWEEP(8)
OCT_DECL_SWEEP(9)
OCT_DECL_SWEEP(10)
OCT_DECL_SWEEP(11)
OCT_DECL_SWEEP(12)
#undef OCT_DECL_SWEEP
inline hipError_t launch_dispersion_sweep(int log2n, const SweepArgs& a, hipStream_t stream) {
	switch (log2n) {
	case 8: return launch_dispersion_sweep_8(a, stream);
	case 9: return launch_dispersion_sweep_9(a, stream);
	case 10: return launch_dispersion_sweep_10(a, stream);
	case 11: return launch_dispersion_sweep_11(a, stream);
	case 12: return launch_dispersion_sweep_12(a, stream);
	default: return hipErrorNotSupported;
	}
}

}  // namespace oct
