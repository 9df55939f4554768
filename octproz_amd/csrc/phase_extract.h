// phase_extract.h -- k-linearisation calibration (include/octpipe.h "phase extraction"; the reference's Phase Extraction Extension,
// docs/docs/plugin-phaseextraction.md).
//
// oct_phase_accumulate_kernel: the exact integer sum of the decoded samples of a run of A-scans into an int64[N] accumulator.  A pure
// streaming read: every lane owns fixed columns of the row (one 16-byte load per row, 12 bytes for packed 12 bit), keeps int32
// partials over at most PHASE_TILE rows (so that 16-bit samples cannot overflow them) and widens them to int64; the row offsets of
// a workgroup are combined in LDS, and every workgroup adds one 64-bit atomic per column.  Integer sums do not depend on order: any
// split of the A-scans over calls or workgroups gives the same bits.  Rows whose length or address does not allow the vector loads
// (row bytes and base both multiples of 16; packed 12 bit: N a multiple of 8 and a dword-aligned base) take the same kernel with
// one sample per load.
//
// oct_phase_extract_kernel<LOG2N>: one wave, latency only.  Forward transform of the averaged interferogram (conjugate of fft_wave),
// band window in bin order, natural-order reload, inverse transform, float64 atan2, integer jump scan, normalisation, monotone
// envelope from the anchor outwards (prefix max / suffix min) and the inversion by binary search -- every step over the LDS copy.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "sample_decode.h"

namespace oct {

// ------------------------------------------------------------------ accumulate
constexpr int PHASE_THREADS = 256;
constexpr int PHASE_TILE = 16384;   // rows per int32 partial: 16384 * 2^16 = 2^30
constexpr int PHASE_UNROLL = 4;     // rows whose loads are in flight together

struct PhaseAccArgs {
	const void* raw;           // sample 0 of row 0 of the buffer (packed: byte 0)
	unsigned long long* acc;   // [N] int64 sums (two's complement)
	size_t firstRow;           // buffer-local index of the first A-scan
	unsigned rows, N;
	unsigned chunks;           // loads per row: N / V (vector form) or N
	unsigned rowsPerPass;      // rows a workgroup covers side by side (chunks <= 256: 256 / chunks, else 1)
	unsigned colBlocks;        // workgroups across one row (chunks > 256)
	unsigned rowGroups;        // workgroups along the rows
	int bitshift;
};

template <int F, bool VEC>
__global__ __launch_bounds__(PHASE_THREADS) void oct_phase_accumulate_kernel(const PhaseAccArgs a) {
	typedef PhFmt<F> PF;
	constexpr int V = VEC ? PF::V : 1;
	typedef typename std::conditional<PF::WIDE, long long, int>::type Part;
	__shared__ long long red[PHASE_THREADS * 16];  // [rowOff][column] of a workgroup (rowsPerPass > 1: rowsPerPass * N <= 256 V)
	const unsigned t = threadIdx.x;
	const unsigned colBlk = blockIdx.x % a.colBlocks, rg = blockIdx.x / a.colBlocks;
	unsigned chunk, rowOff;
	bool active;
	if (a.rowsPerPass > 1) { chunk = t % a.chunks; rowOff = t / a.chunks; active = rowOff < a.rowsPerPass; }
	else { chunk = colBlk * PHASE_THREADS + t; rowOff = 0; active = chunk < a.chunks; }
	const int bitshift = a.bitshift;
	auto conv = [](auto v) { return (Part)v; };
	auto u32 = [](uint32_t v) { return (Part)v; };
	long long sum[V];
	Part part[V];
#pragma unroll
	for (int i = 0; i < V; i++) { sum[i] = 0; part[i] = 0; }
	// the V samples of load `chunk` of buffer row `row`
	auto load = [&](size_t row, Part (&x)[V]) {
		const size_t s0 = row * a.N + (size_t)chunk * V;
		if constexpr (!VEC) {
			x[0] = decode_sample(a.raw, s0, PF::BD, bitshift, PF::FMT, conv, u32);
		} else if constexpr (PF::CHUNK == 12) {
			const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.raw) + s0 / 2 * 3);
			const uint32_t c[3] = {__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1), __builtin_nontemporal_load(p + 2)};
#pragma unroll
			for (int i = 0; i < V; i++) x[i] = decode_sample(c, (size_t)i, PF::BD, bitshift, PF::FMT, conv, u32);
		} else {
			typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
			const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.raw) + s0 * (PF::BD / 8)));
#pragma unroll
			for (int i = 0; i < V; i++) x[i] = decode_sample(&c, (size_t)i, PF::BD, bitshift, PF::FMT, conv, u32);
		}
	};
	auto flush = [&]() {
#pragma unroll
		for (int i = 0; i < V; i++) { sum[i] += (long long)part[i]; part[i] = 0; }
	};
	if (active) {
		const size_t stride = (size_t)a.rowGroups * a.rowsPerPass;
		size_t r = (size_t)rg * a.rowsPerPass + rowOff;
		int inPart = 0;
		for (; r + (PHASE_UNROLL - 1) * stride < a.rows; r += PHASE_UNROLL * stride) {
			Part x[PHASE_UNROLL][V];
#pragma unroll
			for (int u = 0; u < PHASE_UNROLL; u++) load(a.firstRow + r + u * stride, x[u]);
#pragma unroll
			for (int u = 0; u < PHASE_UNROLL; u++)
#pragma unroll
				for (int i = 0; i < V; i++) part[i] += x[u][i];
			if (!PF::WIDE && (inPart += PHASE_UNROLL) >= PHASE_TILE) { flush(); inPart = 0; }
		}
		for (; r < a.rows; r += stride) {
			Part x[V];
			load(a.firstRow + r, x);
#pragma unroll
			for (int i = 0; i < V; i++) part[i] += x[i];
		}
		flush();
	}
	if (a.rowsPerPass > 1) {
		if (active)
#pragma unroll
			for (int i = 0; i < V; i++) red[rowOff * a.N + chunk * V + i] = sum[i];
		__syncthreads();
		for (unsigned col = t; col < a.N; col += PHASE_THREADS) {
			long long s = 0;
			for (unsigned q = 0; q < a.rowsPerPass; q++) s += red[q * a.N + col];
			atomicAdd(a.acc + col, (unsigned long long)s);
		}
	} else if (active) {
#pragma unroll
		for (int i = 0; i < V; i++) atomicAdd(a.acc + (size_t)chunk * V + i, (unsigned long long)sum[i]);
	}
}

// ------------------------------------------------------------------ extract
struct PhaseExtractArgs {
	const float* mean;   // [N] averaged interferogram
	const f2* twiddle;   // the canonical per-pass tables of Plan<LOG2N>
	float* spectrum;     // [N/2] |X[k]|
	float* envelope;     // [N]   |z(n)|
	float* phase;        // [N]   phi(n), unwrapped and referenced to the anchor
	float* curve;        // [N]   the resampling curve
	int* status;         // 0, or 1: phi(b) is zero or not finite (no calibration signal in the band)
	int peakStart, peakEnd, windowRaw, hannPeak, a, b;
};

template <int LOG2N> constexpr size_t phase_extract_lds_bytes() {
	return (size_t)tw_lds_bytes<LOG2N>() + wave_lds_bytes<(1 << LOG2N)>() + 16 * ((size_t)1 << LOG2N);
}

OCT_DEV double wave_sum_f64(double x) {
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s);
	return x;
}

template <int LOG2N>
__global__ __launch_bounds__(64) void oct_phase_extract_kernel(const PhaseExtractArgs g) {
	constexpr int N = 1 << LOG2N, P = N / 64, HALF = N / 2;
	constexpr int RL = LastRadix<LOG2N>::value, NBL = P / RL;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	f2* tw = reinterpret_cast<f2*>(smem);
	f2* xbuf = reinterpret_cast<f2*>(smem + tw_lds_bytes<LOG2N>());
	char* area = smem + tw_lds_bytes<LOG2N>() + wave_lds_bytes<N>();
	f2* spec = reinterpret_cast<f2*>(area);      // band-windowed spectrum in bin order; later K(n)
	int* jumps = reinterpret_cast<int*>(area);
	double* ph = reinterpret_cast<double*>(area + 8 * (size_t)N);  // wrapped phase -> phi -> psi -> the monotone psi
	const int lane = threadIdx.x;
	const int a = g.a, b = g.b;
	fill_twiddles<LOG2N>(tw, g.twiddle, lane, 64);

	// x(n) = mean[n] - (1/N) sum mean, optionally times the Hann window over the whole interferogram
	double s = 0.0;
	for (int i = 0; i < P; i++) s += (double)g.mean[lane * P + i];
	const double avg = wave_sum_f64(s) / (double)N;
	f2 v[P];
#pragma unroll
	for (int q = 0; q < P; q++) {
		const int n = lane + 64 * q;
		double x = (double)g.mean[n] - avg;
		if (g.windowRaw) x *= 0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)(N - 1));
		v[q] = f2{(float)x, 0.0f};
	}
	__syncthreads();
	fft_wave<LOG2N, false>(v, xbuf, tw, lane);  // sum_n x(n) e^{+2 pi i k n / N}: X[k] is its conjugate

	// |X[k]| below N/2, and w(k) X[k] in bin order
	const double span = (double)(g.peakEnd - g.peakStart);
#pragma unroll
	for (int u = 0; u < RL; u++)
#pragma unroll
		for (int m = 0; m < NBL; m++) {
			const int k = fft_bin<LOG2N>(lane, m, u);
			const f2 y = v[m + u * NBL];
			if (k < HALF) g.spectrum[k] = (float)sqrt((double)y.x * (double)y.x + (double)y.y * (double)y.y);
			float w = 0.0f;
			if (k >= g.peakStart && k <= g.peakEnd) w = g.hannPeak ? (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)(k - g.peakStart) / span)) : 1.0f;
			spec[k] = f2{w * y.x, -(w * y.y)};
		}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < P; q++) v[q] = spec[lane + 64 * q];
	__syncthreads();
	fft_wave<LOG2N, false>(v, xbuf, tw, lane);  // N z(n)

	// envelope and wrapped phase
#pragma unroll
	for (int u = 0; u < RL; u++)
#pragma unroll
		for (int m = 0; m < NBL; m++) {
			const int n = fft_bin<LOG2N>(lane, m, u);
			const double zx = (double)v[m + u * NBL].x / (double)N, zy = (double)v[m + u * NBL].y / (double)N;
			g.envelope[n] = (float)sqrt(zx * zx + zy * zy);
			ph[n] = atan2(zy, zx);
		}
	__syncthreads();

	// K(n) = sum_{m <= n} J(m) over the lane's contiguous segment [lane P, lane P + P), then across the wave
	const int n0 = lane * P;
	int local = 0;
	for (int i = 0; i < P; i++) {
		const int n = n0 + i;
		if (n == 0) continue;
		const double d = ph[n] - ph[n - 1];
		local += d > M_PI ? -1 : (d < -M_PI ? 1 : 0);
	}
	int k = (int)wave_inclusive_scan((uint32_t)local) - local;
	for (int i = 0; i < P; i++) {
		const int n = n0 + i;
		if (n > 0) {
			const double d = ph[n] - ph[n - 1];
			k += d > M_PI ? -1 : (d < -M_PI ? 1 : 0);
		}
		jumps[n] = k;
	}
	__syncthreads();
	const double phA = ph[a];
	const int kA = jumps[a];
	__syncthreads();
	for (int i = 0; i < P; i++) {
		const int n = n0 + i;
		ph[n] = (ph[n] - phA) + 2.0 * M_PI * (double)(jumps[n] - kA);
	}
	__syncthreads();
	for (int i = 0; i < P; i++) g.phase[n0 + i] = (float)ph[n0 + i];
	const double phB = ph[b];
	if (!(phB != 0.0) || !isfinite(phB)) {
		if (lane == 0) *g.status = 1;
		return;
	}
	if (lane == 0) *g.status = 0;
	// psi(n) = a + phi(n) (b - a) / phi(b); then monotone from the anchor outwards: a running max for n >= a, a running min
	// (from a downwards) for n < a
	const double scale = (double)(b - a) / phB;
	double hi = -INFINITY, lo = INFINITY;
	for (int i = 0; i < P; i++) {
		const int n = n0 + i;
		const double psi = (double)a + ph[n] * scale;
		ph[n] = psi;
		if (n >= a) hi = fmax(hi, psi);
		if (n <= a) lo = fmin(lo, psi);
	}
	// exclusive scans of the lane totals: max over lower lanes, min over higher lanes
	double hiIn = hi, loIn = lo;
#pragma unroll
	for (int sft = 1; sft < 64; sft <<= 1) {
		const double o = __shfl_up(hiIn, sft);
		if (lane >= sft) hiIn = fmax(hiIn, o);
		const double p = __shfl_down(loIn, sft);
		if (lane + sft < 64) loIn = fmin(loIn, p);
	}
	double runHi = __shfl_up(hiIn, 1), runLo = __shfl_down(loIn, 1);
	if (lane == 0) runHi = -INFINITY;
	if (lane == 63) runLo = INFINITY;
	for (int i = 0; i < P; i++) {
		const int n = n0 + i;
		if (n >= a) { runHi = fmax(runHi, ph[n]); ph[n] = runHi; }
	}
	for (int i = P - 1; i >= 0; i--) {
		const int n = n0 + i;
		if (n <= a) { runLo = fmin(runLo, ph[n]); if (n < a) ph[n] = runLo; }
	}
	__syncthreads();

	// the inverse: curve[j] = n* + (j - psi(n*)) / (psi(n*+1) - psi(n*)), n* the largest n <= N-2 with psi(n) <= j
	const double first = ph[0], last = ph[N - 1];
	for (int q = 0; q < P; q++) {
		const int j = lane + 64 * q;
		const double y = (double)j;
		float c;
		if (y < first) c = 0.0f;
		else if (y >= last) c = (float)(N - 1);
		else {
			int l = 0, h = N - 2;  // psi(l) <= j throughout
			while (l < h) {
				const int mid = (l + h + 1) >> 1;
				if (ph[mid] <= y) l = mid; else h = mid - 1;
			}
			c = (float)((double)l + (y - ph[l]) / (ph[l + 1] - ph[l]));
		}
		g.curve[j] = c;
	}
}

#define OCT_DECL_PHASE(L) hipError_t launch_phase_extract_##L(const PhaseExtractArgs& g, hipStream_t stream);
OCT_DECL_PHASE(8)
OCT_DECL_PHASE(9)
OCT_DECL_PHASE(10)
OCT_DECL_PHASE(11)
OCT_DECL_PHASE(12)
#undef OCT_DECL_PHASE
inline hipError_t launch_phase_extract(int log2n, const PhaseExtractArgs& g, hipStream_t stream) {
	switch (log2n) {
	case 8: return launch_phase_extract_8(g, stream);
	case 9: return launch_phase_extract_9(g, stream);
	case 10: return launch_phase_extract_10(g, stream);
	case 11: return launch_phase_extract_11(g, stream);
	case 12: return launch_phase_extract_12(g, stream);
	default: return hipErrorNotSupported;
	}
}

}  // namespace oct
