// surface_views.h -- surface detection, surface smoothing, surface-following en face slabs and flattening of the float32 processed
// volume (include/octpipe.h "surface views"; the reference has no counterpart, the header comment is the definition).
//
// The region's rows are region row r = b * ascanCount + a, as in peak_analysis.h: row r lives at element rowIdx(r) * L of the buffer
// (rowIdx = (fb + b) * A + fa + a), or at (r - r0) * L of a staged copy of the rows r0 .. of one launch.  The depth window is
// [s0, s0 + cnt).  A surface is int32 per region row, absolute depth bins, negative = none.
//
// oct_surface_detect_kernel (surface_views_inst.hip): one wave per A-scan, lanes along depth.  A step is DETECT_STEP = 256 bins: four
//   coalesced dword loads per lane (chunk c, lane l: bin 64 c + l of the step), issued together.  Each chunk's compare becomes a 64-bit
//   ballot; the run test is scalar work on that mask: a shift-and ladder finds the runs that lie inside the chunk, and `carry` (the
//   ones that end the previous chunk) joins a run across chunk and step borders.  The wave leaves the loop at its first hit, so an A-scan
//   is read down to the step of its surface.
// oct_surface_smooth_kernel<R>: one lane per entry, the (2R + 1)^2 window in registers (statically indexed); the lower median is the
//   entry whose count of smaller entries <= k < count of entries not larger, k = (n - 1) / 2 (holes and cells outside the map are
//   INT_MAX and sort behind every valid entry).
// oct_surface_enface_kernel<FN>: one lane per A-scan walks its slab in increasing depth (the definition fixes the order of the sum);
//   a lane reads consecutive addresses, neighbouring lanes rows L elements apart.
// oct_flatten_kernel<LOADS>: one wave per output row at a time, FLAT_ROWS rows per wave; the row's surface entry and shift are
//   wave-uniform.  The output row is cut into a head (up to the first 16-byte boundary), a body of aligned quads stored with one
//   16-byte store per lane and a tail; head and tail (at most 6 elements) are stored as dwords by the first lanes.  The shifted source
//   is only dword-aligned.  LOADS = 1: four dword loads per quad.  LOADS = 2: one aligned 16-byte load per lane where the aligned quad
//   lies wholly inside the window, the misaligned quad assembled from it and the next lane's (one lane shift; the last lane, and a lane
//   whose neighbour could not load wide, loads the second quad itself); quads that touch the window's ends take the dword loads.
// No kernel uses private memory, LDS or atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_regs.h"

namespace oct {

constexpr int SURF_THREADS = 256;       // four waves per workgroup in every kernel
constexpr unsigned DETECT_LANES = 64;   // bins of one ballot
constexpr unsigned DETECT_STEP = 256;   // bins of one step of the detection loop (four ballots)
constexpr unsigned FLAT_ROWS = 8;       // output rows per wave
constexpr unsigned SURF_NAN = 0x7FC00000u;

typedef float surf_f4 __attribute__((ext_vector_type(4)));

struct SurfArgs {                // the source rows of one launch
	const float* src;            // element 0 of the memory the rows are read from
	unsigned long long A;        // A-scans per B-scan of the buffer
	unsigned fb, fa, ac;         // region: first B-scan, first A-scan, A-scans per B-scan
	unsigned L, s0, cnt;         // elements per row, window [s0, s0 + cnt)
	int staged;                  // 1: src holds the region rows r0 .. one after another, L elements apart
	unsigned r0;
	unsigned rFirst, rCount;     // the region rows of this launch
};

struct EnfaceArgs {
	SurfArgs g;
	const int32_t* surface;      // [rows of the region]
	long long offset;
	unsigned thickness;
	float fill;
	float* out;                  // [rows of the region]
};

struct FlattenArgs {
	SurfArgs g;
	const int32_t* surface;      // [rows of the region]
	long long anchor;
	unsigned outDepth;
	float fill;
	float* out;                  // row o0 of the output at element 0
	unsigned o0;
};

// element 0 of region row r
OCT_DEV const float* surf_row(const SurfArgs& a, unsigned r) {
	unsigned long long row;
	if (a.staged) {
		row = r - a.r0;
	} else {
		const unsigned b = r / a.ac;
		row = ((unsigned long long)a.fb + b) * a.A + a.fa + (r - b * a.ac);
	}
	return a.src + row * a.L;
}

// bit i is set where bits i .. i + run - 1 of m are (1 <= run <= 64)
OCT_DEV unsigned long long surf_runs(unsigned long long m, unsigned run) {
	unsigned long long y = m;
	for (unsigned len = 1; len < run;) {
		const unsigned s = min(len, run - len);
		y &= y >> s;
		len += s;
	}
	return y;
}

template <int R>
__global__ __launch_bounds__(SURF_THREADS) void oct_surface_smooth_kernel(const int32_t* __restrict__ in, unsigned rows, unsigned cols,
                                                                            int32_t* __restrict__ out) {
	constexpr int W = 2 * R + 1, M = W * W;
	const unsigned long long i = (unsigned long long)blockIdx.x * SURF_THREADS + threadIdx.x;
	if (i >= (unsigned long long)rows * cols) return;
	const int r = (int)(i / cols), c = (int)(i - (unsigned long long)r * cols);
	int v[M];
	int n = 0;
#pragma unroll
	for (int dr = -R; dr <= R; dr++)
#pragma unroll
		for (int dc = -R; dc <= R; dc++) {
			const int rr = r + dr, cc = c + dc;
			int x = -1;
			if (rr >= 0 && rr < (int)rows && cc >= 0 && cc < (int)cols) x = in[(size_t)rr * cols + cc];
			n += x >= 0 ? 1 : 0;
			v[(dr + R) * W + dc + R] = x >= 0 ? x : 0x7FFFFFFF;
		}
	int res = -1;
	if (n > 0) {
		const int k = (n - 1) / 2;
#pragma unroll
		for (int p = 0; p < M; p++) {
			int less = 0, leq = 0;
#pragma unroll
			for (int q = 0; q < M; q++) {
				less += v[q] < v[p] ? 1 : 0;
				leq += v[q] <= v[p] ? 1 : 0;
			}
			if (less <= k && k < leq) res = v[p];
		}
	}
	out[i] = res;
}

template <int FN>
__global__ __launch_bounds__(SURF_THREADS) void oct_surface_enface_kernel(const EnfaceArgs a) {
	const unsigned i = blockIdx.x * SURF_THREADS + threadIdx.x;
	if (i >= a.g.rCount) return;
	const unsigned r = a.g.rFirst + i;
	const long long s = a.surface[r];
	float res = a.fill;
	const long long lo = max(s + a.offset, (long long)a.g.s0), hi = min(s + a.offset + (long long)a.thickness - 1, (long long)a.g.s0 + a.g.cnt - 1);
	if (s >= 0 && lo <= hi) {
		const float* p = surf_row(a.g, r);
		if (FN == 0) {
			double acc = (double)p[lo];
			for (long long d = lo + 1; d <= hi; d++) acc += (double)p[d];
			res = (float)(acc / (double)(hi - lo + 1));
		} else {
			float m = p[lo];
			bool nan = m != m;
			for (long long d = lo + 1; d <= hi; d++) {
				const float x = p[d];
				nan |= x != x;
				if (x > m) m = x;
			}
			res = nan ? __uint_as_float(SURF_NAN) : m;
		}
		if (res != res) res = __uint_as_float(SURF_NAN);
	}
	a.out[r] = res;
}

// one value of the flattened row: source bin k of the row at p, or the fill
OCT_DEV float flat_value(const float* p, long long k, long long kLo, long long kHi, float fill) { return k >= kLo && k <= kHi ? p[k] : fill; }

template <int LOADS>
__global__ __launch_bounds__(SURF_THREADS) void oct_flatten_kernel(const FlattenArgs a) {
	const unsigned lane = threadIdx.x & 63;
	const unsigned wave = blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6);
	const unsigned D = a.outDepth;
	for (unsigned it = 0; it < FLAT_ROWS; it++) {
		const unsigned long long ri = (unsigned long long)wave * FLAT_ROWS + it;
		if (ri >= a.g.rCount) return;
		const unsigned r = a.g.rFirst + (unsigned)ri;
		const long long s = __builtin_amdgcn_readfirstlane(a.surface[r]);
		const float* p = surf_row(a.g, r);
		float* o = a.out + (size_t)(r - a.o0) * D;
		// source bin of output element j: k = shift + j, readable inside [kLo, kHi] (empty without a surface)
		const long long shift = s - a.anchor;
		const long long kLo = s >= 0 ? (long long)a.g.s0 : 1, kHi = s >= 0 ? (long long)a.g.s0 + a.g.cnt - 1 : 0;
		const unsigned head = min(D, (unsigned)((4 - ((reinterpret_cast<uintptr_t>(o) >> 2) & 3)) & 3));
		const unsigned nq = (D - head) / 4, tail0 = head + 4 * nq;
		// what the aligned quad under element `head` of the source is short of it (the same for every quad of the row)
		const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(p + shift + head) >> 2) & 3);
		for (unsigned q0 = 0; q0 < nq; q0 += 64) {
			const unsigned q = q0 + lane;
			const bool active = q < nq;
			const unsigned j = head + 4 * q;
			const long long k = shift + j;
			surf_f4 x = {0.0f, 0.0f, 0.0f, 0.0f};
			bool done = false;
			if (LOADS == 2) {
				// the aligned quads X = [k - mis, k - mis + 3] and Y = X + 4: each read only where it lies wholly inside the window
				const bool wideX = active && k - mis >= kLo && k - mis + 3 <= kHi;
				surf_f4 X = {0.0f, 0.0f, 0.0f, 0.0f};
				if (wideX) X = *reinterpret_cast<const surf_f4*>(p + k - mis);
				if (mis == 0) {
					x = X;
					done = wideX;
				} else {
					surf_f4 Y;
#pragma unroll
					for (int c = 0; c < 4; c++) Y[c] = __shfl_down(X[c], 1);
					const bool nextWide = __shfl_down((int)wideX, 1) != 0 && lane < 63;
					const bool inside = active && k >= kLo && k + 3 <= kHi;
					done = wideX && inside && (nextWide || k - mis + 7 <= kHi);
					if (done && !nextWide) Y = *reinterpret_cast<const surf_f4*>(p + k - mis + 4);
					if (mis == 1) x = surf_f4{X[1], X[2], X[3], Y[0]};
					else if (mis == 2) x = surf_f4{X[2], X[3], Y[0], Y[1]};
					else x = surf_f4{X[3], Y[0], Y[1], Y[2]};
				}
			}
			if (active) {
				if (!done) {
#pragma unroll
					for (int c = 0; c < 4; c++) x[c] = flat_value(p, k + c, kLo, kHi, a.fill);
				}
				__builtin_nontemporal_store(x, reinterpret_cast<surf_f4*>(o + j));
			}
		}
		// head and tail as dwords
		const unsigned edge = head + (D - tail0);
		if (lane < edge) {
			const unsigned j = lane < head ? lane : tail0 + (lane - head);
			o[j] = flat_value(p, shift + j, kLo, kHi, a.fill);
		}
	}
}

}  // namespace oct
