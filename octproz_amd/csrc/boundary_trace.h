// boundary_trace.h -- boundary tracing: the minimum-cost path through every B-scan of a region of the float32 processed volume
// (include/octpipe.h "boundary tracing"; the reference has no counterpart, the header comment is the definition).
//
// Rows, region and window are those of surface_views.h (SurfArgs, surf_row): region row r = b * ascanCount + a.  One launch covers
// whole B-scans; B-scan b of the region is one workgroup.  Lane r of the workgroup is node r of every column (A-scan): bin
// d = guide[a] + lo + r, H nodes, H <= threads.
//
// oct_boundary_trace_kernel<WAVE, CHLDS> (boundary_trace_inst.hip).  The forward pass is a chain of ascanCount dependent steps; a step
//   is kept short, bandwidth does not matter (a step reads H + 2k floats).
//   * The values a column needs are the H + 2k bins guide[a] + lo - k ... guide[a] + lo + H - 1 + k - 1, each clamped into the window:
//     lane i loads elements i and i + threads of that line.  The loads of column a + TRACE_PF are issued in step a into registers
//     (raw[a % TRACE_PF], statically indexed: the loop is unrolled TRACE_PF times) and written to the LDS line of column a + 1 in step a,
//     so TRACE_PF - 1 steps hide their latency.
//   * Node cost: lane r reads its 2k values from the LDS line (consecutive lanes consecutive dwords, no conflict) and adds them in the
//     order the definition fixes; every node does its own 2k adds.
//   * Recurrence: the previous column E(a - 1, .) lies in LDS, double-buffered; lane r reads its 1 + 2m neighbours, adds p_|j| and
//     keeps the first smallest by a select on a strict compare, in the order j = 0, -1, +1, -2, +2, ...  p_j comes from the host as
//     one rounded product each.
//   * One synchronisation per column: it covers the line of column a + 1 and E(a, .).  WAVE = true (H <= 64, one wave per B-scan): LDS
//     operations of one wave complete in order, so a wavefront-scope fence that keeps the compiler from moving them is enough and no
//     workgroup barrier is executed.  WAVE = false (H <= 1024, threads = H rounded up to a multiple of 64): one __syncthreads().
//   * Choices are 4-bit codes (0: j = 0, 2 i - 1: j = -i, 2 i: j = +i; m <= 7 gives at most 14).  Even lanes fetch the code of the next
//     lane with one lane shift and store a byte: column a at byte a * CB + r / 2, CB = (H + 1) / 2.  CHLDS = true: in LDS
//     (TRACE_CH_WAVE resp. TRACE_CH_WG bytes; the widest instance takes the CU's 160 KiB); CHLDS = false: in the handle's scratch, CB *
//     ascanCount bytes per B-scan of the launch.
//   * The walk back runs on lane 0 behind the forward pass: the smallest r among the minimal E of the last column, then one code per
//     column, and the surface entry of every column on the way.
// No kernel uses private memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surface_views.h"

namespace oct {

constexpr unsigned TRACE_MAX_H = 1024;      // nodes per A-scan
constexpr unsigned TRACE_MAX_K = 8;         // halfWidth
constexpr unsigned TRACE_MAX_M = 7;         // maxStep
constexpr unsigned TRACE_PF = 4;            // columns whose values are in flight
constexpr unsigned TRACE_WAVE_H = 64;       // the wave form's nodes
constexpr unsigned TRACE_CH_WAVE = 32768;   // bytes of choices in LDS, wave form
// workgroup form: what the CU's 160 KiB leave beside two lines and two columns
constexpr unsigned TRACE_CH_WG = 163840 - 2 * 4 * (TRACE_MAX_H + 2 * TRACE_MAX_K) - 2 * 4 * TRACE_MAX_H;

struct TraceArgs {
	SurfArgs g;                  // the source rows of this launch: whole B-scans, rFirst = bFirst * ac
	const int32_t* guide;        // [rows of the region] or nullptr (0 everywhere)
	int32_t* surface;            // [rows of the region]
	float* pathCost;             // [B-scans of the region] or nullptr
	uint8_t* choices;            // scratch of the launch (CHLDS = false): B-scan i of the launch at i * cb * ac
	unsigned bFirst;             // first B-scan of this launch
	int lo;                      // node r stands for bin guide + lo + r
	unsigned H, k, m;
	int negate;                  // 1: c = -g (polarity +1), 0: c = g
	float p[TRACE_MAX_M + 1];    // fl32(lambda * j)
};

template <bool WAVE>
OCT_DEV void trace_sync() {
	if (WAVE) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	} else {
		__syncthreads();
	}
}

// the bin of element i of column a's line, clamped into the window
OCT_DEV unsigned trace_bin(const TraceArgs& t, int guide, unsigned i) {
	const long long d = (long long)guide + t.lo - (long long)t.k + i;
	const long long s0 = t.g.s0, s1 = (long long)t.g.s0 + t.g.cnt - 1;
	return (unsigned)(d < s0 ? s0 : d > s1 ? s1 : d);
}

template <bool WAVE, bool CHLDS>
__global__ __launch_bounds__(WAVE ? 64 : 1024) void oct_boundary_trace_kernel(const TraceArgs t) {
	constexpr unsigned MAXH = WAVE ? TRACE_WAVE_H : TRACE_MAX_H;
	constexpr unsigned LINE = MAXH + 2 * TRACE_MAX_K;
	__shared__ float line[2][LINE];   // the clamped values of columns a, a + 1
	__shared__ float prev[2][MAXH];   // E(a - 1, .), E(a, .)
	__shared__ uint8_t chl[CHLDS ? (WAVE ? TRACE_CH_WAVE : TRACE_CH_WG) : 4];

	const unsigned lane = threadIdx.x, T = blockDim.x;
	const unsigned H = t.H, k = t.k, m = t.m, ac = t.g.ac;
	const unsigned b = t.bFirst + blockIdx.x;       // B-scan of the region
	const unsigned row0 = b * ac;                   // its first region row
	const unsigned cb = (H + 1) / 2;
	const unsigned n = H + 2 * k;                   // elements of a line, <= T + 16 <= 2 T
	const int32_t* guide = t.guide ? t.guide + row0 : nullptr;
	uint8_t* ch = CHLDS ? chl : t.choices + (size_t)blockIdx.x * cb * ac;
	const long long s0 = t.g.s0, s1 = (long long)t.g.s0 + t.g.cnt - 1;
	const float* const src = surf_row(t.g, row0);   // the rows of one B-scan follow each other, staged or not

	float raw0[TRACE_PF], raw1[TRACE_PF];
	int gd[TRACE_PF];
	auto fetch = [&](unsigned a, float& x0, float& x1, int& gg) {
		gg = guide ? guide[a] : 0;
		const float* p = src + (size_t)a * t.g.L;
		x0 = lane < n ? p[trace_bin(t, gg, lane)] : 0.0f;
		x1 = lane + T < n ? p[trace_bin(t, gg, lane + T)] : 0.0f;
	};
	auto put = [&](unsigned buf, float x0, float x1) {
		if (lane < n) line[buf][lane] = x0;
		if (lane + T < n) line[buf][lane + T] = x1;
	};

	// columns 0 .. TRACE_PF - 1 on their way; column 0 into its line
#pragma unroll
	for (unsigned u = 0; u < TRACE_PF; u++) {
		raw0[u] = raw1[u] = 0.0f;
		gd[u] = -1;
		if (u < ac) fetch(u, raw0[u], raw1[u], gd[u]);
	}
	put(0, raw0[0], raw1[0]);
	trace_sync<WAVE>();

	for (unsigned a0 = 0; a0 < ac; a0 += TRACE_PF) {
#pragma unroll
		for (unsigned u = 0; u < TRACE_PF; u++) {
			const unsigned a = a0 + u;
			if (a >= ac) break;
			const int gg = gd[u];
			// column a + 1 into its line, column a + TRACE_PF on its way in the registers column a leaves
			if (a + 1 < ac) put((a + 1) & 1, raw0[(u + 1) % TRACE_PF], raw1[(u + 1) % TRACE_PF]);
			if (a + TRACE_PF < ac) fetch(a + TRACE_PF, raw0[u], raw1[u], gd[u]);
			float E = 0.0f;
			unsigned code = 0;
			if (lane < H) {
				// node cost
				const long long d = (long long)gg + t.lo + lane;
				float c = 0.0f;
				if (gg >= 0 && d >= s0 && d <= s1) {
					const float* v = &line[a & 1][lane + k];   // v[i] = bin cl(d + i)
					float up = v[0], dn = v[-1];
					for (unsigned i = 1; i < k; i++) {
						up = up + v[i];
						dn = dn + v[-1 - (int)i];
					}
					const float gr = up - dn;
					if (__builtin_isfinite(gr)) c = t.negate ? -gr : gr;
				}
				E = c;
				if (a > 0) {
					const float* pv = prev[(a - 1) & 1];
					float best = pv[lane] + t.p[0];
#pragma unroll
					for (unsigned jj = 1; jj <= TRACE_MAX_M; jj++) {
						if (jj > m) break;
						if (lane >= jj) {
							const float cand = pv[lane - jj] + t.p[jj];
							if (cand < best) {
								best = cand;
								code = 2 * jj - 1;
							}
						}
						if (lane + jj < H) {
							const float cand = pv[lane + jj] + t.p[jj];
							if (cand < best) {
								best = cand;
								code = 2 * jj;
							}
						}
					}
					E = best + c;
				}
				prev[a & 1][lane] = E;
			}
			// two codes per byte: the even lane stores its own and the next lane's (the same wave; 0 past H)
			const unsigned next = (unsigned)__shfl_down((int)code, 1);
			if (a > 0 && !(lane & 1) && lane < H) ch[(size_t)a * cb + lane / 2] = (uint8_t)(code | (next << 4));
			trace_sync<WAVE>();
		}
	}

	// the walk back
	if (!CHLDS) {
		__threadfence_block();
		trace_sync<WAVE>();
	}
	if (lane != 0) return;
	const float* last = prev[(ac - 1) & 1];
	float best = last[0];
	unsigned r = 0;
	for (unsigned i = 1; i < H; i++) {
		const float e = last[i];
		if (e < best) {
			best = e;
			r = i;
		}
	}
	if (t.pathCost) t.pathCost[b] = best;
	int32_t* out = t.surface + row0;
	for (unsigned a = ac; a-- > 0;) {
		const int gg = guide ? guide[a] : 0;
		const long long d = (long long)gg + t.lo + r;
		out[a] = gg >= 0 && d >= s0 && d <= s1 ? (int32_t)d : -1;
		if (a > 0) {
			const unsigned code = (ch[(size_t)a * cb + r / 2] >> (4 * (r & 1))) & 15u;
			const unsigned jj = (code + 1) / 2;
			r = code == 0 ? r : (code & 1) ? r - jj : r + jj;
		}
	}
}

}  // namespace oct
