// repeat_register.h -- bulk-motion registration of the repeated B-scans of the angiography (include/octpipe.h "repeat registration"; the
// reference has no counterpart, the header comment is the definition): the axial shift of every repeat against the first one, and the
// angiography's contrast taken from the shifted bins.
//
// Positions, repeats and rows are those of angiogram.h (AngioArgs, angio_row); groups and averaged A-scans are those of peak_analysis.h:
// group j of repeat m of position p is the peak analysis' group q = (p M + m) Qp + j of the same region, and its profile is built by the
// same code (peak_row, peak_add_rows; for G > 64 from the float64 chunk partials that oct_peak_partials_kernel wrote), so the bits are
// those of octpipe_peak_analysis' averaged A-scans.
//
// oct_register_search_kernel<FROM_PARTIALS>: one workgroup per (position, group), of four waves from G = 8 on and of one wave below (at
//   G = 1 three waves that read one row each and then wait cost more than they bring: 760 against 397 us on the bench's volume; at G = 32
//   and G = 512 four waves took 74 against 81 and 84 against 105 us).  Every wave builds a profile at a time in LDS (M x cnt floats in
//   all), lanes along depth: the M x G rows of a group are read by all waves at once.  Then threads go along the (repeat, lag) pairs, one
//   workgroup of pairs at a time (up to 64 pairs -- R = 8 and M <= 4 -- that is the first wave alone): a thread walks the inner window for its own lag in the
//   definition's order -- partial L_0 = t_0 + t_64 + ..., then L_1, ... (four partials in flight: four independent chains), each added
//   to the lane's sum as it completes -- reading P_0 as a broadcast and P_m at consecutive addresses across the lanes (no bank conflict).
//   Nothing crosses lanes until the costs are known: they go to a small LDS array, and per repeat one wave's strided scan and a xor
//   butterfly over the total order (cost, |d|, d) leave every lane with the same answer.  Lane 0 stores the shift.  (Lanes along depth with the partials
//   added across lanes afterwards was the first form: an LDS tile [lag][64] of float64 for the transposition, two barriers per batch of
//   lags and 17 KB of LDS per wave that held the occupancy at six waves per CU; it took 1.7 x ... 6 x the time of the peak analysis'
//   averaging pass over the same data, profiles/register_bench.json has the form kept.)
// oct_register_volume_kernel<METHOD, M>: oct_angio_volume_kernel with the M source rows displaced by the group's shifts: one wave per output
//   row at a time, the row cut at the 16-byte boundaries of `out` into head, quads and tail.  The M rows start at different alignments, so
//   every load is a dword load.  A quad wholly inside the covered window takes 4 x M loads and leaves as one 16-byte store (from the
//   4 x M values on it is angio_quad_out, which both volume kernels share); a quad wholly outside it is a store of `fill`; the at most
//   two quads across its borders are left to the step that follows the body, one bin per lane, together with head and tail.
//   (A second quad path for the border quads made nearly every wave run the float64 work of a step twice: 1.6 x the unregistered call
//   with the decorrelation.  One quad path with every bin clamped into the covered window gave the
//   loads per-lane addresses instead of immediate offsets: 1.2 ... 1.3 x with every method.)
// oct_register_enface_kernel<METHOD, FN, M>: the en face body of angiogram.h (angio_enface_wave) with REGISTERED set: the slab clipped
//   to the covered window and the rows displaced by the shifts reg_shifts reads.
// oct_register_enface_team_kernel<METHOD, FN, M>: oct_angio_enface_team_kernel with the same three changes, written out (see angiogram.h).
// Shifts are wave-uniform in every kernel but the team form (scalar registers).  No kernel uses private memory or atomics.
#pragma once
#include "angiogram.h"
#include "peak_analysis.h"

namespace oct {

constexpr unsigned REG_MAX_SHIFT = 64;
constexpr unsigned REG_SEARCH_THREADS = 256;  // at most four waves per (position, group): a profile each at a time, then 256 pairs at a time
constexpr unsigned REG_SEARCH_WIDE_G = 8;     // from this many A-scans per group on the search runs four waves per group, below it one
constexpr unsigned long long REG_NAN64 = 0x7FF8000000000000ull;

struct RegSearchArgs {
	PeakArgs k;              // the source and the groups: G, chunks, parts, pFirst as the peak analysis has them
	unsigned M, Qp, R;       // repeats, groups per B-scan, maxShift
	unsigned pFirst, pCount; // the positions of this launch
	int32_t* shifts;         // [P][M][Qp]
	double* costs;           // [P][M - 1][Qp][2R + 1], or nullptr
};

struct RegShiftArgs {
	const int32_t* shifts;   // [P][M][Qp]
	unsigned G, Qp;
};

struct RegVolumeArgs {
	AngioVolumeArgs v;
	RegShiftArgs s;
	float fill;
};

struct RegEnfaceArgs {
	AngioEnfaceArgs e;
	RegShiftArgs s;
};

// bytes of dynamic LDS of the search kernel: the profiles, then the costs of the (M - 1)(2R + 1) pairs
inline size_t reg_search_lds(unsigned M, unsigned cnt, unsigned R) {
	return ((sizeof(float) * (size_t)M * cnt + 7) & ~(size_t)7) + sizeof(double) * (size_t)(M - 1) * (2 * R + 1);
}

// (cost, |d|, d) of x before that of y
OCT_DEV bool reg_before(double cx, int dx, double cy, int dy) {
	if (cx != cy) return cx < cy;
	const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
	if (ax != ay) return ax < ay;
	return dx < dy;
}

template <bool FROM_PARTIALS>
__global__ __launch_bounds__(REG_SEARCH_THREADS) void oct_register_search_kernel(const RegSearchArgs a) {
	extern __shared__ __attribute__((aligned(16))) char reg_lds[];
	const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
	const unsigned item = blockIdx.x;  // < pCount * Qp
	const unsigned p = a.pFirst + item / a.Qp, j = item % a.Qp;
	const unsigned cnt = a.k.cnt, M = a.M, R = a.R;
	float* prof = reinterpret_cast<float*>(reg_lds);  // [M][cnt]
	double* pairCost = reinterpret_cast<double*>(reg_lds + ((sizeof(float) * (size_t)M * cnt + 7) & ~(size_t)7));  // [M - 1][2R + 1]
	const double G = (double)a.k.G;

	// ---- the M profiles (oct_peak_kernel's averaged A-scan), one wave each
	for (unsigned m = wave; m < M; m += waves) {
		const unsigned q = (p * M + m) * a.Qp + j;
		float* pm = prof + (size_t)m * cnt;
		for (unsigned s = lane * 4; s < cnt; s += 256) {
			double v[4] = {-0.0, -0.0, -0.0, -0.0};
			if constexpr (FROM_PARTIALS) {
				const double* pp = a.k.parts + (size_t)(q - a.k.pFirst) * a.k.chunks * cnt + s;
				for (unsigned c = 0; c < a.k.chunks; c++) {
#pragma unroll
					for (int i = 0; i < 4; i++)
						if (s + i < cnt) v[i] += pp[(size_t)c * cnt + i];
				}
			} else {
				peak_add_rows(a.k, peak_row(a.k, q * a.k.G), a.k.G, s, v);
			}
#pragma unroll
			for (int i = 0; i < 4; i++)
				if (s + i < cnt) pm[s + i] = (float)(v[i] / G);
		}
	}
	__syncthreads();

	// ---- a non-finite value anywhere in the window
	unsigned badMask = 0;  // bit m
	for (unsigned m = 0; m < M; m++) {
		bool bad = false;
		for (unsigned s = lane; s < cnt; s += 64) bad |= !__builtin_isfinite(prof[(size_t)m * cnt + s]);
		if (__ballot(bad)) badMask |= 1u << m;
	}

	const unsigned K = cnt - 2 * R, lags = 2 * R + 1, owners = min(K, 64u), pairs = (M - 1) * lags;
	const size_t out0 = ((size_t)p * M) * a.Qp + j;
	// ---- the cost of every (repeat, lag) pair: thread = pair (up to 64 pairs: the first wave alone)
	for (unsigned e0 = 0; e0 < pairs; e0 += blockDim.x) {
		const unsigned e = e0 + tid;
		if (e < pairs) {
			const unsigned m = 1 + e / lags, li = e - (m - 1) * lags;
			const float* p0 = prof + R;
			const float* pm = prof + (size_t)m * cnt + li;  // R + d = li
			double total = 0.0;
			for (unsigned j0 = 0; j0 < owners; j0 += 4) {
				double acc[4] = {0.0, 0.0, 0.0, 0.0};  // L_j0 ... L_j0+3 (every term is >= +0: 0 + t is t)
				for (unsigned i = j0; i < K; i += 64) {
#pragma unroll
					for (unsigned u = 0; u < 4; u++)
						if (i + u < K) acc[u] += __builtin_fabs((double)pm[i + u] - (double)p0[i + u]);
				}
#pragma unroll
				for (unsigned u = 0; u < 4; u++)
					if (j0 + u < owners) total = j0 + u == 0 ? acc[u] : total + acc[u];
			}
			if (badMask & (1u | (1u << m))) total = __longlong_as_double((long long)REG_NAN64);
			pairCost[e] = total;
			if (a.costs) a.costs[(((size_t)p * (M - 1) + (m - 1)) * a.Qp + j) * lags + li] = total;
		}
	}
	__syncthreads();
	// ---- the best lag of every repeat, one wave each
	if (tid == 0) a.shifts[out0] = 0;
	for (unsigned m = 1 + wave; m < M; m += waves) {
		double bestC = __builtin_inf();
		int bestD = 0x7FFFFFFF;
		if (!(badMask & (1u | (1u << m)))) {
			for (unsigned li = lane; li < lags; li += 64) {
				const double c = pairCost[(m - 1) * lags + li];
				const int d = (int)li - (int)R;
				if (reg_before(c, d, bestC, bestD)) {
					bestC = c;
					bestD = d;
				}
			}
		}
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			const double oc = __shfl_xor(bestC, off);
			const int od = __shfl_xor(bestD, off);
			if (reg_before(oc, od, bestC, bestD)) {
				bestC = oc;
				bestD = od;
			}
		}
		if (lane == 0) a.shifts[out0 + (size_t)m * a.Qp] = bestD == 0x7FFFFFFF ? 0 : bestD;
	}
}

// The shifts of output row (p, as): d[m], and the covered part [lo, hi] of the window as indices 0 ... cnt - 1 (lo > hi: none)
template <unsigned M>
OCT_DEV void reg_shifts(const RegShiftArgs& s, unsigned p, unsigned as, unsigned cnt, long long (&d)[M], long long& lo, long long& hi) {
	const int32_t* sp = s.shifts + ((size_t)p * M) * s.Qp + as / s.G;
	long long neg = -(long long)sp[0], pos = (long long)sp[0];
#pragma unroll
	for (unsigned m = 0; m < M; m++) {
		d[m] = (long long)sp[(size_t)m * s.Qp];
		neg = max(neg, -d[m]);
		pos = max(pos, d[m]);
	}
	lo = max(0ll, neg);
	hi = min((long long)cnt - 1, (long long)cnt - 1 - pos);
}

// one quad of the body at element j of the output row, every bin of it inside the covered window
template <int METHOD, unsigned M>
OCT_DEV void reg_quad(const RegVolumeArgs& a, const float* const (&row)[M], unsigned j, float* o, float* mu, bool muWide) {
	float v[M][4];
#pragma unroll
	for (unsigned m = 0; m < M; m++) {
#pragma unroll
		for (int c = 0; c < 4; c++) v[m][c] = row[m][j + c];
	}
	angio_quad_out<METHOD, M>(a.v.n, v, j, o, mu, muWide);
}

template <int METHOD, unsigned M>
__global__ __launch_bounds__(SURF_THREADS) void oct_register_volume_kernel(const RegVolumeArgs a) {
	const AngioArgs& n = a.v.n;
	const unsigned lane = threadIdx.x & 63;
	const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6));
	const unsigned D = n.g.cnt;
	for (unsigned it = 0; it < ANGIO_ROWS; it++) {
		const unsigned long long ri = (unsigned long long)wave * ANGIO_ROWS + it;
		if (ri >= n.g.rCount) return;
		const unsigned o = n.g.rFirst + (unsigned)ri;
		const unsigned p = o / n.g.ac, as = o - p * n.g.ac;
		long long d[M], lo, hi;
		reg_shifts<M>(a.s, p, as, D, d, lo, hi);
		size_t stride;
		const float* src = angio_row<M>(n, p, as, &stride) + n.g.s0;  // bin s0 of the first repeat
		const float* row[M];  // output bin k of the window reads row[m][k]; only for lo <= k <= hi, where every row[m] + k lies in the window
#pragma unroll
		for (unsigned m = 0; m < M; m++) row[m] = src + m * stride + d[m];
		float* out = a.v.out + (size_t)(o - a.v.o0) * D;
		float* mu = a.v.mean ? a.v.mean + (size_t)(o - a.v.o0) * D : nullptr;
		const unsigned head = min(D, (unsigned)((4 - ((reinterpret_cast<uintptr_t>(out) >> 2) & 3)) & 3));
		const unsigned nq = (D - head) / 4, tail0 = head + 4 * nq;
		const bool muWide = mu && ((reinterpret_cast<uintptr_t>(mu + head) >> 2) & 3) == 0;
		for (unsigned q0 = 0; q0 < nq; q0 += 64) {
			const unsigned q = q0 + lane;
			if (q < nq) {
				const unsigned j = head + 4 * q;
				if ((long long)j >= lo && (long long)j + 3 <= hi) {
					reg_quad<METHOD, M>(a, row, j, out, mu, muWide);
				} else if (lo > hi || (long long)j + 3 < lo || (long long)j > hi) {
					const surf_f4 f = {a.fill, a.fill, a.fill, a.fill};
					__builtin_nontemporal_store(f, reinterpret_cast<surf_f4*>(out + j));
					if (mu) {
#pragma unroll
						for (int c = 0; c < 4; c++) __builtin_nontemporal_store(a.fill, mu + j + c);
					}
				}  // (a quad across a border of the covered window: below)
			}
		}
		// one bin per lane: head and tail, then the (at most two) quads of the body that lie across a border of the covered window -- the one
		// that holds `lo` and the one that holds `hi`
		const unsigned edge = head + (D - tail0);
		unsigned j = 0xFFFFFFFFu;
		if (lane < edge) {
			j = lane < head ? lane : tail0 + (lane - head);
		} else if (lane < edge + 8 && lo <= hi) {
			const unsigned w = (lane - edge) >> 2, c = (lane - edge) & 3;
			const unsigned x = (unsigned)(w ? hi : lo);  // (0 <= lo <= hi < D here)
			if (x >= head && x < tail0) {
				const unsigned jq = head + ((x - head) & ~3u);
				const bool across = (long long)jq < lo || (long long)jq + 3 > hi;
				const bool twice = w == 1 && (unsigned)lo >= head && head + (((unsigned)lo - head) & ~3u) == jq;  // `lo` lies in the same quad
				if (across && !twice) j = jq + c;
			}
		}
		if (j != 0xFFFFFFFFu) {
			float c32 = a.fill, mu32 = a.fill;
			if ((long long)j >= lo && (long long)j <= hi) {
				float v[M];
#pragma unroll
				for (unsigned m = 0; m < M; m++) v[m] = row[m][j];
				angio_contrast<METHOD, M>(v, n, c32, mu32);
			}
			out[j] = c32;
			if (mu) mu[j] = mu32;
		}
	}
}

// the full-wave en face kernel: the body of angiogram.h with REGISTERED set
template <int METHOD, int FN, unsigned M>
__global__ __launch_bounds__(SURF_THREADS) void oct_register_enface_kernel(const RegEnfaceArgs r) {
	angio_enface_wave<METHOD, FN, M, true>(r.e, &r.s);
}

// The team form (oct_angio_enface_team_kernel): four output A-scans per wave, each with the shifts of its own group.
template <int METHOD, int FN, unsigned M>
__global__ __launch_bounds__(SURF_THREADS) void oct_register_enface_team_kernel(const RegEnfaceArgs r) {
	const AngioEnfaceArgs& a = r.e;
	const unsigned lane = threadIdx.x & 63, t = lane & (ANGIO_TEAM_LANES - 1), teamBase = lane & ~(ANGIO_TEAM_LANES - 1);
	const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6));
	const unsigned long long ri = (unsigned long long)wave * (64 / ANGIO_TEAM_LANES) + lane / ANGIO_TEAM_LANES;
	const bool live = ri < a.n.g.rCount;
	const unsigned o = a.n.g.rFirst + (live ? (unsigned)ri : 0u);  // (a team without an A-scan walks the launch's first and stores nothing)
	const unsigned p = o / a.n.g.ac, as = o - p * a.n.g.ac;
	long long d[M], clo, chi;
	reg_shifts<M>(r.s, p, as, a.n.g.cnt, d, clo, chi);
	const long long s = a.surface ? (long long)a.surface[(size_t)p * M * a.n.g.ac + as] : (long long)a.n.g.s0;
	const long long lo = max(s + a.offset, (long long)a.n.g.s0 + clo), hi = min(s + a.offset + (long long)a.thickness - 1, (long long)a.n.g.s0 + chi);
	const unsigned count = s >= 0 && lo <= hi ? (unsigned)(hi - lo + 1) : 0u;  // <= thickness <= ANGIO_TEAM_BINS
	size_t stride;
	const float* src = angio_row<M>(a.n, p, as, &stride);
	float x[ANGIO_TEAM_BINS / ANGIO_TEAM_LANES];
#pragma unroll
	for (unsigned c = 0; c < ANGIO_TEAM_BINS / ANGIO_TEAM_LANES; c++) {
		const unsigned i = c * ANGIO_TEAM_LANES + t;
		x[c] = 0.0f;
		if (i < count) {  // (count > 0: lo and the shifted bins lie in the window)
			float v[M];
#pragma unroll
			for (unsigned m = 0; m < M; m++) v[m] = src[(long long)(m * stride) + lo + d[m] + (long long)i];
			float mu32;
			angio_contrast<METHOD, M>(v, a.n, x[c], mu32);
		}
	}
	// the longest slab among the wave's teams bounds the walk
	unsigned longest = 0;
#pragma unroll
	for (unsigned k = 0; k < 64; k += ANGIO_TEAM_LANES) longest = max(longest, (unsigned)__builtin_amdgcn_readlane((int)count, (int)k));
	double sum = 0.0;
	float top = 0.0f;
	bool nan = false;
#pragma unroll
	for (unsigned c = 0; c < ANGIO_TEAM_BINS / ANGIO_TEAM_LANES; c++) {
		if (c * ANGIO_TEAM_LANES >= longest) break;
		for (unsigned j = 0; j < ANGIO_TEAM_LANES && c * ANGIO_TEAM_LANES + j < longest; j++) {
			const unsigned i = c * ANGIO_TEAM_LANES + j;
			const float xi = __shfl(x[c], (int)(teamBase + j));
			if (i < count) {
				if (FN == 0) {
					sum = i == 0 ? (double)xi : sum + (double)xi;
				} else {
					nan |= xi != xi;
					if (i == 0 || xi > top) top = xi;
				}
			}
		}
	}
	float res = a.fill;
	if (count) {
		res = FN == 0 ? (float)(sum / (double)count) : nan ? __uint_as_float(SURF_NAN) : top;
		if (res != res) res = __uint_as_float(SURF_NAN);
	}
	if (live && t == 0) a.out[o] = res;
}

}  // namespace oct
