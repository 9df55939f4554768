// image_stats.h -- histogram and moments of a region of a processed or raw buffer (include/octpipe.h "image statistics"; the
// reference's Image Statistics extension, docs/docs/plugin-imagestatistics.md).
//
// The region is read as an item space: region row r (r = b * ascanCount + a) holds G = ceil(sampleCount / V) items, item k the V
// values j = kV .. kV+V-1 of the row's window (values past sampleCount masked).  V is the container's vector width (PhFmt<F>::V,
// sample_decode.h: 4 for float32).  Rows are cut into segments of segRows rows, a number fixed by the region's shape alone; a
// segment is one workgroup's unit of work and leaves one moments partial.  Lane t of a workgroup takes items t, t + 256, ... of a
// segment in that order, so which value enters which lane's sums, and in which order, depends on the shape only: not on the CU
// count, not on the grid, not on where the values are in memory (the vector form loads an item with one 16-byte load -- 12 bytes
// for packed 12 bit -- the scalar form value by value, and both give the same bits).
//
// oct_stats_kernel<F, VEC>: one streaming pass.  Moments (a.moments): float64 per lane with a per-lane shift K (the lane's first
//   value of the segment): n, sum(x-K), sum((x-K)^2); lanes to (n, mean, M2), a fixed shuffle tree over the wave, the four waves in
//   index order, one StatsPart per segment.  Histogram (a.hist): one LDS copy of `bins` uint32 counters per workgroup (4096 bins =
//   16 KiB, so LDS never limits the 8 workgroups a CU can hold).  The LDS services one wave-instruction at a time, so the costly
//   case is many lanes of ONE instruction on one bin (a log-scaled image or a constant buffer): when every active lane of the wave
//   has the same bin, one lane adds the lane count.  At the end each workgroup stores its counts (and under- / overflow) into its row
//   of a slab; oct_stats_hist_sum_kernel sums the rows into the uint64 histogram: integer sums, exact in any order.
// oct_stats_finish_kernel: one workgroup merges the segment partials in index order (each lane a contiguous run, then the same
//   tree) and writes the StatsResult; with autoRange it also derives the range there, for the histogram pass that follows.
#pragma once
#include <type_traits>

#include "sample_decode.h"

namespace oct {

constexpr int STATS_THREADS = 256;
constexpr unsigned STATS_SEG_VALUES = 32768;  // values per segment (one partial each) at most, at least one row ...
constexpr unsigned STATS_SEG_TARGET = 2048;   // ... and as many segments as this where a segment still has one item per lane
constexpr unsigned STATS_MAX_BINS = 4096;
constexpr int STATS_SUM_ROWS = 16;  // slab rows one thread of oct_stats_hist_sum_kernel adds (loads in flight together)

// the range the histogram uses: processed (lo, hi, scale), raw (rlo, width; limit = bins * width, invWidth = 1 / width)
struct StatsRange {
	float lo, hi, scale;
	int pad;
	long long rlo;
	unsigned long long width, limit;
	double invWidth;
};

struct StatsPart {  // moments of a segment: finite values (processed) or every sample (raw)
	double n, mean, m2, mn, mx;
	unsigned long long nonFinite;
};

struct StatsResult {
	StatsPart m;
	StatsRange range;  // the range in use (autoRange: derived by the finish kernel)
};

struct StatsArgs {
	const void* src;               // element 0 of the memory the region is read from (packed: byte 0)
	// where value j of item k of region row r = b * ac + a is: buffer row rowIdx = (fb + b) * A + fa + a, and
	//   in the buffer itself (staged = 0): element rowIdx * L + s0 + k * V + j;
	//   in a staged copy of the rows r0 .. of one launch: element (r - r0) * L + s0 + k * V + j, plus for packed rows of odd length
	//   (parity = 1), whose B-scan runs are copied byte-wise each on its own sample parity, 4 * (b - bFirst) + ((rowIdx - r + r0) & 1)
	unsigned long long A;
	unsigned fb, fa, ac;
	unsigned L, s0, cnt;           // elements per row, sample window [s0, s0 + cnt)
	int staged, parity;
	unsigned r0, bFirst;
	unsigned G;                    // items per row
	unsigned long long mG, mAc;    // magic numbers of the divisions by G and ac (0: divisor 1)
	unsigned rows, segRows;        // region rows, rows per segment
	unsigned segFirst, segCount;   // the segments of this launch
	int bitshift;
	int moments, hist;
	unsigned bins;
	StatsRange range;              // explicit range, or ...
	const StatsRange* devRange;    // ... the one the finish kernel of the moments pass derived (autoRange)
	StatsPart* parts;              // [segments of the region]
	unsigned* slab;                // [workgroups][bins + 2]: each workgroup's counts, underflow, overflow (a.hist)
	unsigned long long* histOut;   // [bins + 2]: the sums (oct_stats_hist_sum_kernel)
};

// q = n / d for 32-bit n and d (Lemire, Kaser, Kurz 2019: m = floor((2^64 - 1) / d) + 1; m = 0 stands for d = 1)
inline unsigned long long stats_magic(unsigned d) { return d <= 1 ? 0ull : ~0ull / d + 1ull; }
OCT_DEV unsigned stats_div(unsigned n, unsigned long long m) { return m ? (unsigned)__umul64hi(m, (unsigned long long)n) : n; }

OCT_DEV StatsPart stats_merge(const StatsPart& A, const StatsPart& B) {
	StatsPart r;
	r.mn = fmin(A.mn, B.mn);
	r.mx = fmax(A.mx, B.mx);
	r.nonFinite = A.nonFinite + B.nonFinite;
	if (B.n == 0.0) { r.n = A.n; r.mean = A.mean; r.m2 = A.m2; return r; }
	if (A.n == 0.0) { r.n = B.n; r.mean = B.mean; r.m2 = B.m2; return r; }
	const double n = A.n + B.n, delta = B.mean - A.mean;
	r.n = n;
	r.mean = A.mean + delta * (B.n / n);
	r.m2 = A.m2 + B.m2 + delta * delta * (A.n * (B.n / n));
	return r;
}

OCT_DEV StatsPart stats_shfl_down(const StatsPart& p, int off) {
	StatsPart o;
	o.n = __shfl_down(p.n, off);
	o.mean = __shfl_down(p.mean, off);
	o.m2 = __shfl_down(p.m2, off);
	o.mn = __shfl_down(p.mn, off);
	o.mx = __shfl_down(p.mx, off);
	o.nonFinite = __shfl_down(p.nonFinite, off);
	return o;
}

// the partials of the workgroup's lanes merged in a fixed order (lane tree in the wave, then waves 0..3); valid in thread 0
OCT_DEV StatsPart stats_block_reduce(StatsPart p, StatsPart* sh) {
	const unsigned t = threadIdx.x;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const StatsPart o = stats_shfl_down(p, off);
		if ((t & 63) < (unsigned)off) p = stats_merge(p, o);
	}
	if ((t & 63) == 0) sh[t >> 6] = p;
	__syncthreads();
	if (t == 0)
		for (int w = 1; w < STATS_THREADS / 64; w++) p = stats_merge(p, sh[w]);
	__syncthreads();
	return p;
}

// per-lane moments with the shift K = the lane's first value
struct StatsLane {
	unsigned n;
	double K, s1, s2, mn, mx;
	unsigned long long nonFinite;
	OCT_DEV void reset() { n = 0; K = s1 = s2 = 0.0; mn = __builtin_inf(); mx = -__builtin_inf(); nonFinite = 0; }
	OCT_DEV void add(double x) {
		K = n ? K : x;
		const double d = x - K;
		s1 += d;
		s2 += d * d;
		n++;
		mn = fmin(mn, x);
		mx = fmax(mx, x);
	}
	OCT_DEV StatsPart part() const {
		StatsPart p;
		p.n = (double)n;
		p.mean = n ? K + s1 / (double)n : 0.0;
		p.m2 = n ? fmax(0.0, s2 - s1 * (s1 / (double)n)) : 0.0;
		p.mn = mn;
		p.mx = mx;
		p.nonFinite = nonFinite;
		return p;
	}
};

// bin of a processed value inside [lo, hi]: min((int)floorf((v - lo) * scale), bins - 1), the sub and the mul as two float32 roundings
OCT_DEV int stats_bin_f32(float v, const StatsRange& R, unsigned bins) {
	const float t = __fmul_rn(__fsub_rn(v, R.lo), R.scale);
	const float f = floorf(t);
	return f >= (float)(bins - 1) ? (int)bins - 1 : (int)f;
}

// bin of a raw value x >= rlo with d = x - rlo < limit: d / width, exact (the float64 quotient is off by at most one)
OCT_DEV int stats_bin_raw(unsigned long long d, const StatsRange& R) {
	if (R.width == 1) return (int)d;
	unsigned q = (unsigned)((double)d * R.invWidth);
	if ((unsigned long long)q * R.width > d) q--;
	else if ((unsigned long long)(q + 1) * R.width <= d) q++;
	return (int)q;
}

template <int F, bool VEC>
__global__ __launch_bounds__(STATS_THREADS) void oct_stats_kernel(const StatsArgs a) {
	typedef PhFmt<F> S;
	constexpr int V = S::V;
	constexpr int U = 32 / V > 1 ? 32 / V : 1;  // items per lane in flight: 32 values
	typedef typename std::conditional<F == ST_F32, float, typename std::conditional<F == PH_U32, long long, int>::type>::type Val;
	extern __shared__ unsigned stats_hist[];  // [bins] (a.hist)
	__shared__ StatsPart waveParts[STATS_THREADS / 64];
	__shared__ unsigned long long flow[2];
	const unsigned t = threadIdx.x, lane = t & 63;
	const StatsRange R = a.devRange ? *a.devRange : a.range;
	const unsigned bins = a.bins;
	if (a.hist) {
		for (unsigned i = t; i < bins; i += STATS_THREADS) stats_hist[i] = 0u;
		if (t < 2) flow[t] = 0ull;
	}
	__syncthreads();
	unsigned under = 0, over = 0;
	const int bitshift = a.bitshift;
	auto conv = [](auto v) { return (Val)v; };
	auto u32 = [](uint32_t v) { return (Val)v; };
	auto count = [&](int bin) {
		// wave-uniform call: one add of the lane count when every active lane has the same bin
		const unsigned long long act = __ballot(bin >= 0);
		if (act) {
			const int first = __builtin_ctzll(act);
			const int b0 = __builtin_amdgcn_readlane(bin, first);
			const unsigned long long same = __ballot(bin == b0);
			if (same == act) {
				if ((int)lane == first) atomicAdd(&stats_hist[b0], (unsigned)__popcll(act));
			} else if (bin >= 0) {
				atomicAdd(&stats_hist[bin], 1u);
			}
		}
	};
	const unsigned segEnd = a.segFirst + a.segCount;
	for (unsigned seg = a.segFirst + blockIdx.x; seg < segEnd; seg += gridDim.x) {
		const unsigned row0 = seg * a.segRows;
		const unsigned nrows = min(a.segRows, a.rows - row0);
		const unsigned items = nrows * a.G;
		StatsLane acc;
		acc.reset();
		for (unsigned q0 = 0; q0 < items; q0 += STATS_THREADS * U) {
			Val x[U][V];
			unsigned nv[U];  // values of the item inside the window (0: no item)
#pragma unroll
			for (int u = 0; u < U; u++) {
				const unsigned il = q0 + t + (unsigned)u * STATS_THREADS;
				nv[u] = 0;
#pragma unroll
				for (int j = 0; j < V; j++) x[u][j] = (Val)0;
				if (il < items) {
					const unsigned rr = stats_div(il, a.mG);
					const unsigned k = il - rr * a.G;
					const unsigned r = row0 + rr;
					const unsigned b = stats_div(r, a.mAc), ai = r - b * a.ac;
					const unsigned long long rowIdx = ((unsigned long long)a.fb + b) * a.A + a.fa + ai;
					unsigned long long e = (a.staged ? (unsigned long long)(r - a.r0) : rowIdx) * a.L + a.s0 + (unsigned long long)k * V;
					if (a.parity) e += 4ull * (b - a.bFirst) + ((rowIdx - r + a.r0) & 1ull);
					nv[u] = min((unsigned)V, a.cnt - k * V);
					if constexpr (F == ST_F32) {
						const float* p = reinterpret_cast<const float*>(a.src) + e;
						if constexpr (VEC) {
							typedef float f32x4 __attribute__((ext_vector_type(4)));
							const f32x4 c = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
#pragma unroll
							for (int j = 0; j < V; j++) x[u][j] = c[j];
						} else {
#pragma unroll
							for (int j = 0; j < V; j++)
								if ((unsigned)j < nv[u]) x[u][j] = p[j];
						}
					} else if constexpr (!VEC) {
#pragma unroll
						for (int j = 0; j < V; j++)
							if ((unsigned)j < nv[u]) x[u][j] = decode_sample(a.src, (size_t)(e + j), S::BD, bitshift, S::FMT, conv, u32);
					} else if constexpr (S::CHUNK == 12) {
						const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.src) + e / 2 * 3);
						const uint32_t c[3] = {__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1), __builtin_nontemporal_load(p + 2)};
#pragma unroll
						for (int j = 0; j < V; j++) x[u][j] = decode_sample(c, (size_t)j, S::BD, bitshift, S::FMT, conv, u32);
					} else {
						typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
						const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.src) + e * (S::BD / 8)));
#pragma unroll
						for (int j = 0; j < V; j++) x[u][j] = decode_sample(&c, (size_t)j, S::BD, bitshift, S::FMT, conv, u32);
					}
				}
			}
#pragma unroll
			for (int u = 0; u < U; u++) {
#pragma unroll
				for (int j = 0; j < V; j++) {
					const bool in = (unsigned)j < nv[u];
					int bin = -1;
					if constexpr (F == ST_F32) {
						const float v = x[u][j];
						const bool fin = in && __builtin_isfinite(v);
						if (a.moments) {
							if (fin) acc.add((double)v);
							else if (in) acc.nonFinite++;
						}
						if (a.hist && fin) {
							if (v < R.lo) under++;
							else if (v > R.hi) over++;
							else bin = stats_bin_f32(v, R, bins);
						}
					} else {
						const long long v = (long long)x[u][j];
						if (a.moments && in) acc.add((double)v);
						if (a.hist && in) {
							if (v < R.rlo) {
								under++;
							} else {
								const unsigned long long d = (unsigned long long)v - (unsigned long long)R.rlo;
								if (d >= R.limit) over++;
								else bin = stats_bin_raw(d, R);
							}
						}
					}
					if (a.hist) count(bin);
				}
			}
		}
		if (a.moments) {
			const StatsPart p = stats_block_reduce(acc.part(), waveParts);
			if (t == 0) a.parts[seg] = p;
		}
	}
	if (a.hist) {
		// under- / overflow: wave sums, one LDS add per wave; then the workgroup's counts go to its row of the slab with plain stores
		// (every workgroup adding into the same few KiB of global memory would serialise on them)
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			under += __shfl_down(under, off);
			over += __shfl_down(over, off);
		}
		if (lane == 0) {
			if (under) atomicAdd(&flow[0], (unsigned long long)under);
			if (over) atomicAdd(&flow[1], (unsigned long long)over);
		}
		__syncthreads();
		unsigned* row = a.slab + (size_t)blockIdx.x * (bins + 2);
		for (unsigned i = t; i < bins; i += STATS_THREADS) row[i] = stats_hist[i];
		if (t < 2) row[bins + t] = (unsigned)flow[t];
	}
}

struct StatsFinishArgs {
	const StatsPart* parts;
	unsigned segments;
	int raw;        // 1: raw source (autoRange: rlo / width), 0: processed (lo / hi / scale)
	int autoRange;
	unsigned bins;
	StatsRange range;  // explicit range (autoRange = 0)
	StatsResult* out;
};
// (oct_stats_hist_sum_kernel and oct_stats_finish_kernel are defined in image_stats_inst.hip: plain kernels, one definition each)

}  // namespace oct
