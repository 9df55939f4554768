// angiogram.h -- OCT angiography on the float32 processed volume: the contrast between the M repeated B-scans of every slow-axis position
// as a volume, and as an en face projection of a slab (include/octpipe.h "angiography"; the reference has no counterpart, the header
// comment is the definition).
//
// The region's rows are those of surface_views.h (region row r = b * ascanCount + a; SurfArgs).  Position p owns the region's B-scans
// p M .. p M + M - 1; output row o = p * ascanCount + a has its M source rows one B-scan apart (A * L floats in the buffer, ascanCount * L
// in a staged copy, which always starts with the first repeat of a position).
//
// M is a template argument of every kernel (2 ... 8): the loads of a step are straight-line code, so the compiler issues all of them
// before the one wait in front of the arithmetic, and only M repeats are worked out.  (A run-time M, every loop unrolled to 8 and
// predicated, put each load into a branch of its own with its own wait, and ran the arithmetic of all 8 repeats behind selects.)
//
// angio_contrast<METHOD, M>: one bin from its M values.  Everything is float64 with contraction off: every product is rounded before it is
//   added, as the definition says.
// oct_angio_volume_kernel<METHOD, M>: one wave per output row at a time, ANGIO_ROWS rows per wave, lanes along depth.  The output row is
//   cut as oct_flatten_kernel cuts its row: a head up to the first 16-byte boundary of `out`, a body of quads, a tail; head and tail (at
//   most six bins) are one bin per lane with dword loads and stores.  The body is one step of 64 quads at a time: the M loads of a lane
//   are issued together (4 x M values in registers), then the four bins are worked out, then `out` (and `mean`) leave as one non-temporal
//   16-byte store each.  Where the quads of all M source rows are 16-byte aligned (N/2 and firstSample multiples of 4 -- the usual
//   case) each load is one 16-byte load; otherwise the row takes four dword loads per quad and repeat.  A `mean` whose rows are aligned
//   differently from `out` is stored as dwords.
// oct_angio_enface_kernel<METHOD, FN, M>: one wave per output A-scan, lanes along the slab: lane j owns bins j, j + 64, ... of the slab (M
//   coalesced dword loads per bin), which are the definition's partials L_j.  The partials are added (FN 0) or compared (FN 1) in lane
//   order with v_readlane, every lane doing the same scalar-indexed walk.  The contrast volume is never written.
// oct_angio_enface_team_kernel<METHOD, FN, M>: the same for slabs of at most 64 bins with four A-scans per wave (see there).
// The full-wave en face kernel is a one-line wrapper around angio_enface_wave<METHOD, FN, M, REGISTERED>, and so is the registered one of
// repeat_register.h (REGISTERED: the slab clipped to the covered window, the rows displaced by the group's shifts); the volume kernel
// shares angio_quad_out, the second half of a step of its body, with the registered one.  The team form is written out here and there:
// behind a shared body the compiler formed its per-lane row addresses differently (two instructions fewer, another opcode mix), and the
// same-process timing against the old text did not stay inside that text's own spread.
// No kernel uses private memory, LDS or atomics.
#pragma once
#include "surface_views.h"

namespace oct {

constexpr unsigned ANGIO_MIN_REPEATS = 2, ANGIO_MAX_REPEATS = 8;
constexpr unsigned ANGIO_ROWS = 2;  // output rows per wave of the volume kernel
constexpr unsigned ANGIO_TEAM_LANES = 16;  // the en face kernel's team form: lanes per output A-scan ...
constexpr unsigned ANGIO_TEAM_BINS = 64;   // ... and the thickest slab it takes

struct AngioArgs {
	SurfArgs g;          // the source; rFirst / rCount: the OUTPUT rows o = p * ascanCount + a of this launch
	unsigned M;          // repeats, 2 ... 8: the kernels' template argument (here for the launcher)
	int mask;
	float threshold, masked;
};

struct AngioVolumeArgs {
	AngioArgs n;
	float* out;          // row o0 of the output at element 0, rows of g.cnt floats
	float* mean;         // the same, or nullptr
	unsigned o0;
};

struct AngioEnfaceArgs {
	AngioArgs n;
	const int32_t* surface;  // [rows of the region], or nullptr: firstSample everywhere
	long long offset;
	unsigned thickness;
	float fill;
	float* out;              // [output rows of the region]
};

// element 0 of the first repeat's row of output row (p, a), and the distance to the next repeat's
template <unsigned M>
OCT_DEV const float* angio_row(const AngioArgs& n, unsigned p, unsigned a, size_t* stride) {
	const unsigned long long b = (unsigned long long)p * M;
	unsigned long long row;
	if (n.g.staged) {
		row = b * n.g.ac + a - n.g.r0;
		*stride = (size_t)n.g.ac * n.g.L;
	} else {
		row = ((unsigned long long)n.g.fb + b) * n.g.A + n.g.fa + a;
		*stride = (size_t)n.g.A * n.g.L;
	}
	return n.g.src + row * n.g.L;
}

// c32 after the mask and mu32 of one bin, both with a NaN canonical
template <int METHOD, unsigned M>
OCT_DEV void angio_contrast(const float (&v)[M], const AngioArgs& n, float& c32, float& mu32) {
#pragma clang fp contract(off)
	double sum = (double)v[0];
#pragma unroll
	for (unsigned m = 1; m < M; m++) sum += (double)v[m];
	const double mu = sum / (double)M;
	double c;
	if (METHOD == 0) {
		const double d0 = (double)v[0] - mu;
		double acc = d0 * d0;
#pragma unroll
		for (unsigned m = 1; m < M; m++) {
			const double d = (double)v[m] - mu;
			const double dd = d * d;
			acc += dd;
		}
		c = acc / (double)M;
	} else {
		double acc = 0.0;
#pragma unroll
		for (unsigned m = 0; m + 1 < M; m++) {
			const double x = (double)v[m], y = (double)v[m + 1];
			double t;
			if (METHOD == 1) {
				const double num = x * y, xx = x * x, yy = y * y;
				const double hx = 0.5 * xx, hy = 0.5 * yy;
				const double q = hx + hy;
				t = q == 0.0 ? 1.0 : num / q;
			} else {
				t = __builtin_fabs(y - x);
			}
			acc = m == 0 ? t : acc + t;
		}
		const double avg = acc / (double)(M - 1);
		c = METHOD == 1 ? 1.0 - avg : avg;
	}
	float cf = (float)c, mf = (float)mu;
	if (cf != cf) cf = __uint_as_float(SURF_NAN);
	if (n.mask && !(mf > n.threshold)) cf = n.masked;
	if (mf != mf) mf = __uint_as_float(SURF_NAN);
	c32 = cf;
	mu32 = mf;
}

// the second half of a step of the body, shared by both volume kernels: the quad at element j of the output row from its 4 x M values
template <int METHOD, unsigned M>
OCT_DEV void angio_quad_out(const AngioArgs& n, const float (&v)[M][4], unsigned j, float* o, float* mu, bool muWide) {
	surf_f4 cq, mq;
#pragma unroll
	for (int c = 0; c < 4; c++) {
		float col[M];
#pragma unroll
		for (unsigned m = 0; m < M; m++) {
			col[m] = v[m][c];
			asm volatile("" : "+v"(col[m]));  // (see below)
		}
		float c32, mu32;
		angio_contrast<METHOD, M>(col, n, c32, mu32);
		// one bin after the other (volatile statements keep their order, and a bin's values pass through one): the float64 work of four
		// bins interleaved costs up to 156 VGPRs (decorrelation, M = 8)
		asm volatile("" : "+v"(c32), "+v"(mu32));
		cq[c] = c32;
		mq[c] = mu32;
	}
	__builtin_nontemporal_store(cq, reinterpret_cast<surf_f4*>(o + j));
	if (mu) {
		if (muWide) {
			__builtin_nontemporal_store(mq, reinterpret_cast<surf_f4*>(mu + j));
		} else {
#pragma unroll
			for (int c = 0; c < 4; c++) __builtin_nontemporal_store(mq[c], mu + j + c);
		}
	}
}

// one step of the body: the quad at element j of the output row from the quads at src + m * stride + j
template <int METHOD, unsigned M, bool WIDE>
OCT_DEV void angio_quad(const AngioVolumeArgs& a, const float* src, size_t stride, unsigned j, float* o, float* mu, bool muWide) {
	float v[M][4];
#pragma unroll
	for (unsigned m = 0; m < M; m++) {
		const float* s = src + m * stride + j;
		if (WIDE) {
			const surf_f4 x = *reinterpret_cast<const surf_f4*>(s);
#pragma unroll
			for (int c = 0; c < 4; c++) v[m][c] = x[c];
		} else {
#pragma unroll
			for (int c = 0; c < 4; c++) v[m][c] = s[c];
		}
	}
	angio_quad_out<METHOD, M>(a.n, v, j, o, mu, muWide);
}

template <int METHOD, unsigned M>
__global__ __launch_bounds__(SURF_THREADS) void oct_angio_volume_kernel(const AngioVolumeArgs a) {
	const unsigned lane = threadIdx.x & 63;
	const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6));
	const unsigned D = a.n.g.cnt;
	for (unsigned it = 0; it < ANGIO_ROWS; it++) {
		const unsigned long long ri = (unsigned long long)wave * ANGIO_ROWS + it;
		if (ri >= a.n.g.rCount) return;
		const unsigned o = a.n.g.rFirst + (unsigned)ri;
		const unsigned p = o / a.n.g.ac, as = o - p * a.n.g.ac;
		size_t stride;
		const float* src = angio_row<M>(a.n, p, as, &stride) + a.n.g.s0;  // bin s0 of the first repeat
		float* out = a.out + (size_t)(o - a.o0) * D;
		float* mu = a.mean ? a.mean + (size_t)(o - a.o0) * D : nullptr;
		const unsigned head = min(D, (unsigned)((4 - ((reinterpret_cast<uintptr_t>(out) >> 2) & 3)) & 3));
		const unsigned nq = (D - head) / 4, tail0 = head + 4 * nq;
		// the body's quads of every repeat on a 16-byte boundary: the first one is, and so is the distance between two repeats
		const bool wide = ((reinterpret_cast<uintptr_t>(src + head) >> 2) & 3) == 0 && (stride & 3) == 0;
		const bool muWide = mu && ((reinterpret_cast<uintptr_t>(mu + head) >> 2) & 3) == 0;
		for (unsigned q0 = 0; q0 < nq; q0 += 64) {
			const unsigned q = q0 + lane;
			if (q < nq) {
				if (wide) angio_quad<METHOD, M, true>(a, src, stride, head + 4 * q, out, mu, muWide);
				else angio_quad<METHOD, M, false>(a, src, stride, head + 4 * q, out, mu, muWide);
			}
		}
		// head and tail, one bin per lane
		const unsigned edge = head + (D - tail0);
		if (lane < edge) {
			const unsigned j = lane < head ? lane : tail0 + (lane - head);
			float v[M];
#pragma unroll
			for (unsigned m = 0; m < M; m++) v[m] = src[m * stride + j];
			float c32, mu32;
			angio_contrast<METHOD, M>(v, a.n, c32, mu32);
			out[j] = c32;
			if (mu) mu[j] = mu32;
		}
	}
}

OCT_DEV double angio_readlane(double x, unsigned lane) {
	const int lo = __builtin_amdgcn_readlane(__double2loint(x), (int)lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), (int)lane);
	return __hiloint2double(hi, lo);
}

// the shifts of a registered call and what they leave of the window (repeat_register.h)
struct RegShiftArgs;
template <unsigned M>
OCT_DEV void reg_shifts(const RegShiftArgs& s, unsigned p, unsigned as, unsigned cnt, long long (&d)[M], long long& lo, long long& hi);

// The full-wave form of the en face kernel.  REGISTERED (oct_register_enface_kernel; sh: the shifts, else unused): the slab is clipped to
// the covered window and the M rows are displaced by the group's shifts, which are wave-uniform.
template <int METHOD, int FN, unsigned M, bool REGISTERED>
OCT_DEV void angio_enface_wave(const AngioEnfaceArgs& a, const RegShiftArgs* sh) {
	const unsigned lane = threadIdx.x & 63;
	const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6));
	if (wave >= a.n.g.rCount) return;
	const unsigned o = a.n.g.rFirst + wave;
	const unsigned p = o / a.n.g.ac, as = o - p * a.n.g.ac;
	long long d[M], clo, chi;  // REGISTERED: the shifts, the covered window
	if constexpr (REGISTERED) reg_shifts<M>(*sh, p, as, a.n.g.cnt, d, clo, chi);
	// the surface row of the position's first repeat
	const long long s = a.surface ? (long long)__builtin_amdgcn_readfirstlane(a.surface[(size_t)p * M * a.n.g.ac + as]) : (long long)a.n.g.s0;
	long long lo, hi;
	if constexpr (REGISTERED) {
		lo = max(s + a.offset, (long long)a.n.g.s0 + clo);
		hi = min(s + a.offset + (long long)a.thickness - 1, (long long)a.n.g.s0 + chi);
	} else {  // (its own expressions: the ones above with clo = 0, chi = cnt - 1 cost this form eight instructions)
		lo = max(s + a.offset, (long long)a.n.g.s0);
		hi = min(s + a.offset + (long long)a.thickness - 1, (long long)a.n.g.s0 + a.n.g.cnt - 1);
	}
	float res = a.fill;
	if (s >= 0 && lo <= hi) {
		const unsigned count = (unsigned)(hi - lo + 1);  // |D| <= 4096
		size_t stride;
		const float* src = angio_row<M>(a.n, p, as, &stride) + lo;  // bin 0 of the slab in the (unshifted) first repeat
		const float* row[M];  // REGISTERED: the displaced rows
		if constexpr (REGISTERED) {
#pragma unroll
			for (unsigned m = 0; m < M; m++) row[m] = src + m * stride + d[m];
		}
		double part = 0.0;   // FN 0: L_lane
		float best = 0.0f;   // FN 1: the lane's x that none of the lane's exceeds, and its i
		unsigned bestI = 0;
		bool nan = false;
		for (unsigned i0 = 0; i0 < count; i0 += 64) {
			const unsigned i = i0 + lane;
			if (i < count) {
				float v[M];
#pragma unroll
				for (unsigned m = 0; m < M; m++) {
					if constexpr (REGISTERED) v[m] = row[m][i];
					else v[m] = src[m * stride + i];
				}
				float x, mu32;
				angio_contrast<METHOD, M>(v, a.n, x, mu32);
				if (FN == 0) {
					part = i0 == 0 ? (double)x : part + (double)x;
				} else {
					nan |= x != x;
					if (i0 == 0 || x > best) {
						best = x;
						bestI = i;
					}
				}
			}
		}
		const unsigned lanes = min(count, 64u);  // lanes that own a bin
		if (FN == 0) {
			double sum = angio_readlane(part, 0);
			for (unsigned l = 1; l < lanes; l++) sum += angio_readlane(part, l);
			res = (float)(sum / (double)count);
		} else {
			float top = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, best), 0));
			unsigned topI = (unsigned)__builtin_amdgcn_readlane((int)bestI, 0);
			for (unsigned l = 1; l < lanes; l++) {
				const float x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, best), (int)l));
				const unsigned xi = (unsigned)__builtin_amdgcn_readlane((int)bestI, (int)l);
				if (x > top || (x == top && xi < topI)) {
					top = x;
					topI = xi;
				}
			}
			res = __ballot(nan) ? __uint_as_float(SURF_NAN) : top;
		}
		if (res != res) res = __uint_as_float(SURF_NAN);
	}
	if (lane == 0) a.out[o] = res;
}

template <int METHOD, int FN, unsigned M>
__global__ __launch_bounds__(SURF_THREADS) void oct_angio_enface_kernel(const AngioEnfaceArgs a) {
	angio_enface_wave<METHOD, FN, M, false>(a, nullptr);
}

// The team form for slabs of at most ANGIO_TEAM_BINS bins: four output A-scans per wave, one team of 16 lanes each.  Lane t of a team
// owns x_t, x_{t+16}, x_{t+32}, x_{t+48} in four registers; every partial L_j of the definition is then a single x_j, and the team adds (or
// compares) them in increasing j by fetching x_j from its lane t = j & 15 (one ds_bpermute per step, no LDS memory), as far as the longest
// slab of the wave's four A-scans goes.  Same bits as the full-wave form.
template <int METHOD, int FN, unsigned M>
__global__ __launch_bounds__(SURF_THREADS) void oct_angio_enface_team_kernel(const AngioEnfaceArgs a) {
	const unsigned lane = threadIdx.x & 63, t = lane & (ANGIO_TEAM_LANES - 1), teamBase = lane & ~(ANGIO_TEAM_LANES - 1);
	const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6));
	const unsigned long long ri = (unsigned long long)wave * (64 / ANGIO_TEAM_LANES) + lane / ANGIO_TEAM_LANES;
	const bool live = ri < a.n.g.rCount;
	const unsigned o = a.n.g.rFirst + (live ? (unsigned)ri : 0u);  // (a team without an A-scan walks the launch's first and stores nothing)
	const unsigned p = o / a.n.g.ac, as = o - p * a.n.g.ac;
	const long long s = a.surface ? (long long)a.surface[(size_t)p * M * a.n.g.ac + as] : (long long)a.n.g.s0;
	const long long lo = max(s + a.offset, (long long)a.n.g.s0), hi = min(s + a.offset + (long long)a.thickness - 1, (long long)a.n.g.s0 + a.n.g.cnt - 1);
	const unsigned count = s >= 0 && lo <= hi ? (unsigned)(hi - lo + 1) : 0u;  // <= thickness <= ANGIO_TEAM_BINS
	size_t stride;
	const float* src = angio_row<M>(a.n, p, as, &stride) + (count ? lo : (long long)a.n.g.s0);
	float x[ANGIO_TEAM_BINS / ANGIO_TEAM_LANES];
#pragma unroll
	for (unsigned c = 0; c < ANGIO_TEAM_BINS / ANGIO_TEAM_LANES; c++) {
		const unsigned i = c * ANGIO_TEAM_LANES + t;
		x[c] = 0.0f;
		if (i < count) {
			float v[M];
#pragma unroll
			for (unsigned m = 0; m < M; m++) v[m] = src[m * stride + i];
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
