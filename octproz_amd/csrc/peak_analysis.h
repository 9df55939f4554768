// peak_analysis.h -- averaged A-scans of groups of a region, their peak, half-maximum width and Gaussian fit (include/octpipe.h
// "peak analysis"; the reference's Peak Detector and Axial PSF Analyzer extensions, docs/docs/plugin-peakdetector.md,
// plugin-axialpsfanalyzer.md).
//
// The region's rows are region row r = b * ascanCount + a; group q holds rows qG .. qG + G - 1 (G divides ascanCount, so a group never
// leaves its B-scan and its rows are consecutive in the buffer).  Row r lives at element rowIdx(r) * L + s0 of the buffer
// (rowIdx = (fb + b) * A + fa + a), or at (r - r0) * L + s0 of a staged copy of the rows r0 .. of one launch.
//
// oct_peak_partials_kernel (stage A, only for G > 64): one wave per (chunk, tile of 256 samples); chunk c of group q is rows
//   qG + 64c .. (at most 64).  Lane l owns samples 4l .. 4l + 3 of the tile and adds the chunk's rows to them in row order in float64,
//   starting from -0.0 (the additive identity: the sum is the one that starts from the first value).  The vector form loads 16 bytes
//   per row where row length, window start and address allow; the scalar form loads value by value; both add the same values in the
//   same order.  Output: float64 partials [group of the batch][chunk][sampleCount].
// oct_peak_kernel<FIT, FROM_PARTIALS> (stage B): one wave per group, 1 or 4 waves per workgroup, no cross-wave traffic.  The wave builds
//   m in its LDS slice (sampleCount floats): from the source rows (G <= 64: the region is read once) or from the partials, each
//   sample's float64 sum divided once by G and rounded once.  Then on the slice: the non-finite ballot, the argmax (per lane the first
//   maximum of its strided samples, then a butterfly that keeps the larger value and on a tie the smaller index: every lane ends with
//   the same k), the parabola, the crossings (ballot scans over 64-sample blocks outward from k: the first sample at or below half
//   on either side) and, in the FIT instance, Levenberg-Marquardt: lanes stride over the fit window, the 15 float64 sums (10 of H,
//   4 of g, the cost) are reduced by a fixed xor butterfly, so every lane holds the same bits and solves the same 4 x 4 system.  Lane
//   0 stores the OctPipePeak.  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/octpipe.h"
#include "fft_regs.h"

namespace oct {

constexpr int PEAK_THREADS = 256;    // stage A: four waves, each its own (chunk, tile)
constexpr unsigned PEAK_CHUNK = 64;  // A-scans per chunk partial
constexpr unsigned PEAK_TILE = 256;  // samples of one stage-A wave (4 per lane)
constexpr unsigned PEAK_MAX_SAMPLES = 4096;
constexpr double PEAK_FWHM_PER_SIGMA = 2.3548200450309493;  // 2 sqrt(2 ln 2)

struct PeakArgs {
	const float* src;            // element 0 of the memory the rows are read from
	unsigned long long A;        // A-scans per B-scan of the buffer
	unsigned fb, fa, ac;         // region: first B-scan, first A-scan, A-scans per B-scan
	unsigned L, s0, cnt;         // elements per row, window [s0, s0 + cnt)
	int staged;                  // 1: src holds the region rows r0 .. one after another, L elements apart
	unsigned r0;
	int vec;                     // 16-byte loads (L % 4 == 0, s0 % 4 == 0, src 16-byte aligned)
	unsigned G, chunks;          // A-scans per group, chunks per group
	unsigned qFirst, qCount;     // stage B: the groups of this launch
	unsigned gFirst, gCount;     // stage A: the chunks of this launch, g = q * chunks + c
	unsigned pFirst;             // the first group whose partials are in `parts`
	double* parts;               // [groups of the batch][chunks][cnt]
	float threshold;
	unsigned fitHalfWidth, maxIter;  // (maxIter: 0 already replaced by 100)
	OctPipePeak* peaks;          // [Q]
	float* averaged;             // [Q][cnt], or null
};

// element s0 of region row r
OCT_DEV const float* peak_row(const PeakArgs& a, unsigned r) {
	unsigned long long row;
	if (a.staged) {
		row = r - a.r0;
	} else {
		const unsigned b = r / a.ac;
		row = ((unsigned long long)a.fb + b) * a.A + a.fa + (r - b * a.ac);
	}
	return a.src + row * a.L + a.s0;
}

// v[j] += rows[0 .. n)[s + j] in row order, j < 4, s + j < cnt (rows L elements apart)
OCT_DEV void peak_add_rows(const PeakArgs& a, const float* p, unsigned n, unsigned s, double v[4]) {
	typedef float f32x4 __attribute__((ext_vector_type(4)));
	constexpr unsigned U = 8;  // rows in flight
	const unsigned nv = min(4u, a.cnt - s);
	for (unsigned i0 = 0; i0 < n; i0 += U) {
		float x[U][4];
#pragma unroll
		for (unsigned u = 0; u < U; u++) {
			const float* q = p + (size_t)(i0 + u) * a.L + s;
#pragma unroll
			for (int j = 0; j < 4; j++) x[u][j] = 0.0f;
			if (i0 + u < n) {
				if (a.vec) {
					const f32x4 c = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q));
#pragma unroll
					for (int j = 0; j < 4; j++) x[u][j] = c[j];
				} else {
#pragma unroll
					for (int j = 0; j < 4; j++)
						if ((unsigned)j < nv) x[u][j] = q[j];
				}
			}
		}
#pragma unroll
		for (unsigned u = 0; u < U; u++)
			if (i0 + u < n) {
#pragma unroll
				for (int j = 0; j < 4; j++) v[j] += (double)x[u][j];
			}
	}
}

// (oct_peak_partials_kernel is defined in peak_analysis_inst.hip: a plain kernel, one definition)

// the wave's sum by a fixed xor butterfly: every lane ends with the same bits (x + y == y + x), which are then handed over as
// wave-uniform (scalar registers: the fit's state does not occupy vector registers)
OCT_DEV double peak_sum(double v) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
	const unsigned long long b = (unsigned long long)__double_as_longlong(v);
	const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
	return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

struct PeakFitSums {
	double h[10], g[4], c;  // H00 H01 H02 H03 H11 H12 H13 H22 H23 H33, g0..g3, the cost
};

// the cost alone at p (the test of a step)
OCT_DEV double peak_fit_cost(const float* m, unsigned s0, unsigned lo, unsigned n, const double p[4]) {
	const unsigned lane = threadIdx.x & 63;
	const double inv = 1.0 / p[2];
	double c = 0.0;
#pragma unroll 1
	for (unsigned i = lane; i < n; i += 64) {
		const double z = (double)(s0 + lo + i);
		const double u = (z - p[1]) * inv;
		const double e = exp(-0.5 * (u * u));
		const double r = (double)m[lo + i] - (p[0] * e + p[3]);
		c += r * r;
	}
	return peak_sum(c);
}

// the sums of one evaluation at p = (A, mu, sigma, c) over the window [lo, lo + n) of the slice (absolute depth s0 + i); the cost is
// the same bits peak_fit_cost gives
OCT_DEV void peak_fit_eval(const float* m, unsigned s0, unsigned lo, unsigned n, const double p[4], PeakFitSums& S) {
	const unsigned lane = threadIdx.x & 63;
#pragma unroll
	for (int i = 0; i < 10; i++) S.h[i] = 0.0;
#pragma unroll
	for (int i = 0; i < 4; i++) S.g[i] = 0.0;
	S.c = 0.0;
	const double inv = 1.0 / p[2];
#pragma unroll 1
	for (unsigned i = lane; i < n; i += 64) {
		const double z = (double)(s0 + lo + i);
		const double u = (z - p[1]) * inv;
		const double e = exp(-0.5 * (u * u));
		const double j0 = e, j1 = p[0] * e * u * inv, j2 = j1 * u;
		const double r = (double)m[lo + i] - (p[0] * e + p[3]);
		S.h[0] += j0 * j0;
		S.h[1] += j0 * j1;
		S.h[2] += j0 * j2;
		S.h[3] += j0;
		S.h[4] += j1 * j1;
		S.h[5] += j1 * j2;
		S.h[6] += j1;
		S.h[7] += j2 * j2;
		S.h[8] += j2;
		S.h[9] += 1.0;
		S.g[0] += j0 * r;
		S.g[1] += j1 * r;
		S.g[2] += j2 * r;
		S.g[3] += r;
		S.c += r * r;
	}
#pragma unroll
	for (int i = 0; i < 10; i++) S.h[i] = peak_sum(S.h[i]);
#pragma unroll
	for (int i = 0; i < 4; i++) S.g[i] = peak_sum(S.g[i]);
	S.c = peak_sum(S.c);
}

// (H + lambda diag(H)) delta = g by Gaussian elimination with partial pivoting (the first largest |pivot|); false: a zero or
// non-finite pivot
OCT_DEV bool peak_solve(const PeakFitSums& S, double lambda, double d[4]) {
	const double* h = S.h;
	const double* g = S.g;
	double M[4][5] = {{h[0], h[1], h[2], h[3], g[0]},
	                  {h[1], h[4], h[5], h[6], g[1]},
	                  {h[2], h[5], h[7], h[8], g[2]},
	                  {h[3], h[6], h[8], h[9], g[3]}};
#pragma unroll
	for (int i = 0; i < 4; i++) M[i][i] = M[i][i] + lambda * M[i][i];
	bool ok = true;
#pragma unroll
	for (int col = 0; col < 4; col++) {
		int piv = col;
		double best = fabs(M[col][col]);
#pragma unroll
		for (int r = col + 1; r < 4; r++) {
			const double v = fabs(M[r][col]);
			if (v > best) {
				best = v;
				piv = r;
			}
		}
#pragma unroll
		for (int r = col + 1; r < 4; r++)
			if (piv == r) {
#pragma unroll
				for (int k = col; k < 5; k++) {
					const double t = M[col][k];
					M[col][k] = M[r][k];
					M[r][k] = t;
				}
			}
		const double pv = M[col][col];
		if (pv == 0.0 || !__builtin_isfinite(pv)) ok = false;
#pragma unroll
		for (int r = col + 1; r < 4; r++) {
			const double f = M[r][col] / pv;
#pragma unroll
			for (int k = col; k < 5; k++) M[r][k] -= f * M[col][k];
		}
	}
#pragma unroll
	for (int i = 3; i >= 0; i--) {
		double t = M[i][4];
#pragma unroll
		for (int k = i + 1; k < 4; k++) t -= M[i][k] * d[k];
		d[i] = t / M[i][i];
	}
	return ok;
}

template <bool FIT, bool FROM_PARTIALS>
__global__ __launch_bounds__(PEAK_THREADS) void oct_peak_kernel(const PeakArgs a) {
	extern __shared__ float peak_lds[];  // [waves][cnt]
	const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const unsigned qi = blockIdx.x * (blockDim.x >> 6) + wave;
	if (qi >= a.qCount) return;
	const unsigned q = a.qFirst + qi;
	const unsigned cnt = a.cnt, s0 = a.s0;
	float* m = peak_lds + (size_t)wave * cnt;
	const double G = (double)a.G;

	// ---- the averaged A-scan
	for (unsigned s = lane * 4; s < cnt; s += 256) {
		double v[4] = {-0.0, -0.0, -0.0, -0.0};
		if constexpr (FROM_PARTIALS) {
			const double* p = a.parts + (size_t)(q - a.pFirst) * a.chunks * cnt + s;
			for (unsigned c = 0; c < a.chunks; c++) {
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (s + j < cnt) v[j] += p[(size_t)c * cnt + j];
			}
		} else {
			peak_add_rows(a, peak_row(a, q * a.G), a.G, s, v);
		}
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (s + j < cnt) {
				const float x = (float)(v[j] / G);
				m[s + j] = x;
				if (a.averaged) a.averaged[(size_t)q * cnt + s + j] = x;
			}
	}
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	__builtin_amdgcn_wave_barrier();

	const double nan = __builtin_nan("");
	unsigned status = 0, index = 0, fitFirst = 0, fitCount = 0, iters = 0;
	float value = __builtin_nanf("");
	double position = nan, left = nan, right = nan, fwhm = nan;
	double amp = nan, center = nan, sigma = nan, offset = nan, fitFwhm = nan, rms = nan;

	// ---- 1. non-finite values; 2. the first maximum
	bool bad = false;
	float best = -__builtin_inff();
	unsigned bi = 0xFFFFFFFFu;
	for (unsigned s = lane; s < cnt; s += 64) {
		const float x = m[s];
		bad |= !__builtin_isfinite(x);
		if (x > best) {
			best = x;
			bi = s;
		}
	}
	if (__ballot(bad)) {
		status = OCTPIPE_PEAK_NONFINITE;
	} else {
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			const float ob = __shfl_xor(best, off);
			const unsigned oi = __shfl_xor(bi, off);
			if (ob > best || (ob == best && oi < bi)) {
				best = ob;
				bi = oi;
			}
		}
		const unsigned k = bi;
		value = m[k];
		index = s0 + k;
		const double vk = (double)value;
		if (!(vk > (double)a.threshold)) {
			status = OCTPIPE_PEAK_NO_PEAK;
		} else {
			// ---- 3. the parabola
			position = (double)(s0 + k);
			if (k > 0 && k + 1 < cnt) {
				const double ml = (double)m[k - 1], mr = (double)m[k + 1];
				const double d = (ml - 2.0 * vk) + mr;
				if (d < 0.0) position = (double)(s0 + k) + (0.5 * (ml - mr)) / d;
			}
			// ---- 4. the crossings at half maximum
			const bool widthOk = vk > 0.0;
			if (!widthOk) {
				status |= OCTPIPE_PEAK_WIDTH_UNDEFINED;
			} else {
				const double half = 0.5 * vk;
				// left: the largest j < k with m[j] <= half; l = j + 1 (none: l = 0, open)
				int l = -1;
				for (int base = (int)k - 1; base >= 0; base -= 64) {
					const int j = base - (int)lane;
					const unsigned long long hit = __ballot(j >= 0 && (double)m[j >= 0 ? j : 0] <= half);
					if (hit) {
						l = base - __builtin_ctzll(hit) + 1;
						break;
					}
				}
				if (l <= 0) {
					left = (double)s0;
					status |= OCTPIPE_PEAK_LEFT_OPEN;
				} else {
					const double ml = (double)m[l];
					left = (double)(s0 + l) - (ml - half) / (ml - (double)m[l - 1]);
				}
				// right: the smallest j > k with m[j] <= half; r = j - 1 (none: r = cnt - 1, open)
				int r = -1;
				for (unsigned base = k + 1; base < cnt; base += 64) {
					const unsigned j = base + lane;
					const unsigned long long hit = __ballot(j < cnt && (double)m[j < cnt ? j : 0] <= half);
					if (hit) {
						r = (int)(base + __builtin_ctzll(hit)) - 1;
						break;
					}
				}
				if (r < 0) {
					right = (double)(s0 + cnt - 1);
					status |= OCTPIPE_PEAK_RIGHT_OPEN;
				} else {
					const double mr = (double)m[r];
					right = (double)(s0 + r) + (mr - half) / (mr - (double)m[r + 1]);
				}
				fwhm = right - left;
			}
			// ---- 5. the Gaussian fit
			if constexpr (FIT) {
				unsigned w = a.fitHalfWidth;
				if (!w) w = widthOk ? (unsigned)fmin(256.0, fmax(4.0, ceil(1.5 * fwhm))) : 16u;
				w = min(w, cnt);  // (the same window; k + w cannot wrap)
				const unsigned lo = k > w ? k - w : 0u;
				const unsigned hi = min(cnt - 1, k + w);
				const unsigned n = hi - lo + 1;
				fitFirst = s0 + lo;
				fitCount = n;
				if (n < 5) {
					status |= OCTPIPE_PEAK_FIT_SKIPPED;
				} else {
					float c0 = __builtin_inff();
					for (unsigned i = lane; i < n; i += 64) c0 = fminf(c0, m[lo + i]);
#pragma unroll
					for (int off = 32; off >= 1; off >>= 1) c0 = fminf(c0, __shfl_xor(c0, off));
					double p[4] = {vk - (double)c0, position, widthOk ? fmax(0.5, fwhm / PEAK_FWHM_PER_SIGMA) : 1.0, (double)c0};
					// H and g live in the wave's LDS record between the evaluation and the solves (carried through the loop in
					// registers they would double the fit's register budget)
					__shared__ PeakFitSums fitSums[PEAK_THREADS / 64];
					PeakFitSums& S = fitSums[wave];
					double cost = 0.0;
					double lambda = 1e-3;
					unsigned fst = 0;
					bool fresh = true;  // H, g and the cost wanted at p (one place in the code: the evaluation is inlined once)
					while (!fst) {
						if (fresh) {
							PeakFitSums E;
							peak_fit_eval(m, s0, lo, n, p, E);
							if (lane == 0) S = E;
							__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
							__builtin_amdgcn_wave_barrier();
							cost = E.c;
							fresh = false;
							if (cost == 0.0) {
								fst = OCTPIPE_PEAK_FIT_CONVERGED;
								break;
							}
						}
						if (iters >= a.maxIter) {
							fst = OCTPIPE_PEAK_FIT_MAX_ITER;
							break;
						}
						double d[4];
						const bool ok = peak_solve(S, lambda, d);
						iters++;
						double pn[4], cn = 0.0;
#pragma unroll
						for (int i = 0; i < 4; i++) pn[i] = p[i] + d[i];
						if (ok) cn = peak_fit_cost(m, s0, lo, n, pn);
						if (ok && cn < cost) {
							double rel = 0.0;
#pragma unroll
							for (int i = 0; i < 4; i++) rel = fmax(rel, fabs(d[i]) / (fabs(p[i]) + 1e-12));
							const bool conv = cost - cn <= 1e-12 * cost || rel <= 1e-10 || cn == 0.0;
#pragma unroll
							for (int i = 0; i < 4; i++) p[i] = pn[i];
							cost = cn;
							fresh = !conv;
							lambda = fmax(lambda / 10.0, 1e-15);
							if (conv) fst = OCTPIPE_PEAK_FIT_CONVERGED;
						} else {
							lambda *= 10.0;
							if (lambda > 1e15) fst = OCTPIPE_PEAK_FIT_STALLED;
						}
					}
					status |= fst;
					amp = p[0];
					center = p[1];
					sigma = fabs(p[2]);
					offset = p[3];
					fitFwhm = PEAK_FWHM_PER_SIGMA * sigma;
					rms = sqrt(cost / (double)n);
				}
			}
		}
	}
	if (lane == 0) {
		OctPipePeak* o = a.peaks + q;
		o->status = status;
		o->index = index;
		o->value = value;
		o->fitFirst = fitFirst;
		o->fitCount = fitCount;
		o->iterations = iters;
		o->position = position;
		o->left = left;
		o->right = right;
		o->fwhm = fwhm;
		o->amplitude = amp;
		o->center = center;
		o->sigma = sigma;
		o->offset = offset;
		o->fitFwhm = fitFwhm;
		o->rms = rms;
	}
}

}  // namespace oct
