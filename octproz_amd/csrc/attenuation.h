// attenuation.h -- the depth-resolved attenuation coefficient of the float32 processed volume (Vermeer et al. 2014): as a volume, as the
// float64 sums below every bin, and as an en face projection of a slab (include/octpipe.h "attenuation"; the reference has no counterpart,
// the header comment is the definition).
//
// The region's rows are those of surface_views.h (region row r = b * ascanCount + a; SurfArgs).  The window's bins are numbered from s0
// and cut into chunks of ATT_CHUNK = 256, anchored at s0: lane l of the wave owns bins 256 k + 4 l .. + 3 of chunk k, one 16-byte piece.
//
// atten_pow2 / atten_intensity: one bin's intensity.  Everything is float64 with contraction off: every product is rounded before it is
//   added, as the definition says; the a = 1, b = 0 map runs the same operations.
// atten_chunk: one chunk of one A-scan.  The lane's four intensities become Q_l; the suffix sum over the lanes is six steps, each two
//   32-bit ds_bpermute_b32 (there is no 64-bit cross-lane move) and one float64 add in the lanes that have a partner; one more move
//   brings t_{l+1}, and t_0 is read with v_readfirstlane into the carry C, which is wave-uniform.  The definition's order is this one.
// oct_atten_volume_kernel<SCALE, GAIN, SUMS>: one wave per A-scan at a time, ATT_ROWS A-scans per wave, the chunk loop from the deep end;
//   the quad of the next (shallower) chunk is loaded before the current one is worked out.  The source quad of a lane is one 16-byte load
//   where the row's bin s0 lies on a 16-byte boundary and the quad lies wholly inside the window, else up to four dword loads (odd depth,
//   any firstSample, the window's last quad); the result is one non-temporal 16-byte store under the same two conditions on the output
//   row, else dword stores.  The lane-to-bin map is the definition's, so a misaligned row is not re-cut into head, body and tail as
//   oct_flatten_kernel does: it takes the dword forms throughout.  SUMS: the float64 sums `below` leave instead of mu32 (the debug entry).
// oct_atten_enface_kernel<SCALE, GAIN, FN>: one wave per A-scan, the same chunk loop from the deep end down to the chunk that holds the
//   slab's first bin; bins above the slab are not read (they only enter sums nobody asks for).  mu32 of the slab's bins goes to the wave's
//   piece of LDS (the loop meets them in decreasing depth, the projection wants them in increasing depth); then every lane walks the piece
//   in increasing depth, four bins per broadcast 16-byte read, adding (FN 0) or comparing (FN 1) one after the other: the sequential
//   float64 sum and the MIP of oct_surface_enface_kernel on the volume the volume kernel writes, which is never written.
// No kernel uses private memory or atomics; only the en face kernel uses LDS.
#pragma once
#include "surface_views.h"

namespace oct {

constexpr unsigned ATT_CHUNK = 256;  // bins of one step of the chunk loop: 64 lanes x one 16-byte piece
constexpr unsigned ATT_ROWS = 2;     // A-scans per wave of the volume kernel
constexpr unsigned ATT_LDS_WAVE_BYTES = 16384;  // the thickest slab (4096 bins of float32): beyond a quarter of it a workgroup is one wave

struct AttenArgs {
	SurfArgs g;          // the source rows of this launch
	double a, b;         // the linearising map
	double noise, tail;  // (double)noise, (double)tail
	double twoDelta;     // 2.0 * (double)pixelSize
	const float* gain;   // [g.cnt], or nullptr (the kernels' template argument says which)
	unsigned undefined;  // the bits of `undefined`
};

struct AttenVolumeArgs {
	AttenArgs n;
	void* out;           // row o0 of the output at element 0, rows of g.cnt floats (SUMS: doubles)
	unsigned o0;
};

struct AttenEnfaceArgs {
	AttenArgs n;
	const int32_t* surface;  // [rows of the region], or nullptr: firstSample everywhere
	long long offset;
	unsigned thickness;
	float fill;
	unsigned cap;            // floats of LDS per wave, >= min(thickness, g.cnt) and a multiple of 4
	float* out;              // [rows of the region]
};

// 2^y as the definition has it: the guards, then exp(f ln 2) by the degree-13 Taylor polynomial in Horner form and an exact scaling
OCT_DEV double atten_pow2(double y) {
#pragma clang fp contract(off)
	const bool inside = y >= -1000.0 && y < 1024.0;  // (false for NaN)
	const double yc = inside ? y : 0.0;
	const double m = __builtin_rint(yc);
	const double f = yc - m;
	const double t = f * 0x1.62e42fefa39efp-1;
	constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
	                          1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
	double p = c[13];
#pragma unroll
	for (int k = 12; k >= 0; k--) {
		const double tp = t * p;
		p = c[k] + tp;
	}
	const double r = __builtin_ldexp(p, (int)m);
	return inside ? r : y >= 1024.0 ? __builtin_inf() : y < -1000.0 ? 0.0 : y;
}

template <int SCALE, bool GAIN>
OCT_DEV double atten_intensity(const AttenArgs& n, float v, float g) {
#pragma clang fp contract(off)
	const double xv = (double)v * n.a;
	const double x = xv + n.b;
	double J;
	if (SCALE == 0) J = x;
	else if (SCALE == 1) J = x * x;
	else J = atten_pow2(x);
	const double K = J - n.noise;
	double L = K;
	if (GAIN) L = K * (double)g;
	return L > 0.0 ? L : 0.0;
}

// mu32 of one bin from its intensity and the sum below it
OCT_DEV float atten_mu(const AttenArgs& n, double I, double below) {
#pragma clang fp contract(off)
	const double den = n.twoDelta * below;
	float mu = (float)(I / den);
	if (mu != mu) mu = __uint_as_float(SURF_NAN);
	return den > 0.0 ? mu : __uint_as_float(n.undefined);
}

// x of lane (lane + s) & 63
OCT_DEV double atten_from_lane(double x, unsigned lane, unsigned s) {
	const int idx = (int)((lane + s) << 2);
	const int lo = __builtin_amdgcn_ds_bpermute(idx, __double2loint(x)), hi = __builtin_amdgcn_ds_bpermute(idx, __double2hiint(x));
	return __hiloint2double(hi, lo);
}

// the lane's four values at p[bin0 .. bin0 + 3], those with lo <= bin < hi; the others come back as 0.  wide: p + bin0 lies on a 16-byte
// boundary in every lane
OCT_DEV surf_f4 atten_load4(const float* p, unsigned bin0, unsigned lo, unsigned hi, bool wide) {
	surf_f4 x = {0.0f, 0.0f, 0.0f, 0.0f};
	if (wide && bin0 >= lo && bin0 + 3 < hi) {
		x = *reinterpret_cast<const surf_f4*>(p + bin0);
	} else {
#pragma unroll
		for (int c = 0; c < 4; c++)
			if (bin0 + c >= lo && bin0 + c < hi) x[c] = p[bin0 + c];
	}
	return x;
}

// One chunk of one A-scan: the lane's intensities I[0 .. 3] (bins outside [lo, cnt) count as +0) and the sums below[0 .. 3] of its four bins;
// the carry C moves on to the next (shallower) chunk.
template <int SCALE, bool GAIN>
OCT_DEV void atten_chunk(const AttenArgs& n, unsigned lane, unsigned bin0, unsigned lo, const surf_f4& v, const surf_f4& g, double& C, double (&I)[4],
                         double (&below)[4]) {
#pragma clang fp contract(off)
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const double x = atten_intensity<SCALE, GAIN>(n, v[c], g[c]);
		I[c] = bin0 + c >= lo && bin0 + c < n.g.cnt ? x : 0.0;
	}
	double t = ((I[3] + I[2]) + I[1]) + I[0];
#pragma unroll
	for (unsigned s = 1; s < 64; s *= 2) {
		const double other = atten_from_lane(t, lane, s);
		const double sum = t + other;
		t = lane + s <= 63 ? sum : t;
	}
	const double next = atten_from_lane(t, lane, 1);  // t_{l+1}
	const double R = lane == 63 ? C : next + C;
	below[3] = R;
	below[2] = below[3] + I[3];
	below[1] = below[2] + I[2];
	below[0] = below[1] + I[1];
	const double t0 = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(t)), __builtin_amdgcn_readfirstlane(__double2loint(t)));
	C = t0 + C;
}

template <int SCALE, bool GAIN, bool SUMS>
__global__ __launch_bounds__(SURF_THREADS) void oct_atten_volume_kernel(const AttenVolumeArgs a) {
	const unsigned lane = threadIdx.x & 63;
	const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SURF_THREADS / 64) + (threadIdx.x >> 6));
	const unsigned D = a.n.g.cnt;
	const unsigned chunks = (D + ATT_CHUNK - 1) / ATT_CHUNK;
	const bool gainWide = GAIN && (reinterpret_cast<uintptr_t>(a.n.gain) & 15) == 0;
	for (unsigned it = 0; it < ATT_ROWS; it++) {
		const unsigned long long ri = (unsigned long long)wave * ATT_ROWS + it;
		if (ri >= a.n.g.rCount) return;
		const unsigned r = a.n.g.rFirst + (unsigned)ri;
		const float* src = surf_row(a.n.g, r) + a.n.g.s0;  // bin 0 of the window
		const bool srcWide = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
		float* out = static_cast<float*>(a.out) + (size_t)(r - a.o0) * D;
		double* sums = static_cast<double*>(a.out) + (size_t)(r - a.o0) * D;
		const bool outWide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
		double C = a.n.tail;
		unsigned bin0 = (chunks - 1) * ATT_CHUNK + 4 * lane;
		surf_f4 v = atten_load4(src, bin0, 0, D, srcWide);
		for (unsigned k = chunks; k-- > 0; bin0 -= ATT_CHUNK) {
			surf_f4 vNext = {0.0f, 0.0f, 0.0f, 0.0f};
			if (k > 0) vNext = atten_load4(src, bin0 - ATT_CHUNK, 0, D, srcWide);
			surf_f4 g = {0.0f, 0.0f, 0.0f, 0.0f};
			if (GAIN) g = atten_load4(a.n.gain, bin0, 0, D, gainWide);
			double I[4], below[4];
			atten_chunk<SCALE, GAIN>(a.n, lane, bin0, 0, v, g, C, I, below);
			if (SUMS) {
#pragma unroll
				for (int c = 0; c < 4; c++)
					if (bin0 + c < D) sums[bin0 + c] = below[c];
			} else {
				surf_f4 mu;
#pragma unroll
				for (int c = 0; c < 4; c++) mu[c] = atten_mu(a.n, I[c], below[c]);
				if (outWide && bin0 + 3 < D) {
					__builtin_nontemporal_store(mu, reinterpret_cast<surf_f4*>(out + bin0));
				} else {
#pragma unroll
					for (int c = 0; c < 4; c++)
						if (bin0 + c < D) out[bin0 + c] = mu[c];
				}
			}
			v = vNext;
		}
	}
}

template <int SCALE, bool GAIN, int FN>
__global__ __launch_bounds__(SURF_THREADS) void oct_atten_enface_kernel(const AttenEnfaceArgs a) {
	extern __shared__ float atten_lds[];
	const unsigned lane = threadIdx.x & 63;
	const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
	if (wave >= a.n.g.rCount) return;
	const unsigned r = a.n.g.rFirst + wave;
	const unsigned D = a.n.g.cnt;
	const long long s = a.surface ? (long long)__builtin_amdgcn_readfirstlane(a.surface[r]) : (long long)a.n.g.s0;
	const long long lo = max(s + a.offset, (long long)a.n.g.s0), hi = min(s + a.offset + (long long)a.thickness - 1, (long long)a.n.g.s0 + D - 1);
	float res = a.fill;
	if (s >= 0 && lo <= hi) {
		const unsigned i0 = (unsigned)(lo - a.n.g.s0), i1 = (unsigned)(hi - a.n.g.s0);  // the slab's first and last bin of the window
		const unsigned count = i1 - i0 + 1;                                              // <= min(thickness, D) <= cap
		float* slab = atten_lds + (size_t)(threadIdx.x >> 6) * a.cap;
		const float* src = surf_row(a.n.g, r) + a.n.g.s0;
		const bool srcWide = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
		const bool gainWide = GAIN && (reinterpret_cast<uintptr_t>(a.n.gain) & 15) == 0;
		const unsigned chunks = (D + ATT_CHUNK - 1) / ATT_CHUNK, kFirst = i0 / ATT_CHUNK;
		double C = a.n.tail;
		unsigned bin0 = (chunks - 1) * ATT_CHUNK + 4 * lane;
		for (unsigned k = chunks; k-- > kFirst; bin0 -= ATT_CHUNK) {
			const surf_f4 v = atten_load4(src, bin0, i0, D, srcWide);
			surf_f4 g = {0.0f, 0.0f, 0.0f, 0.0f};
			if (GAIN) g = atten_load4(a.n.gain, bin0, i0, D, gainWide);
			double I[4], below[4];
			atten_chunk<SCALE, GAIN>(a.n, lane, bin0, i0, v, g, C, I, below);
			if (k * ATT_CHUNK <= i1) {  // the chunk holds bins of the slab
#pragma unroll
				for (int c = 0; c < 4; c++) {
					const float mu = atten_mu(a.n, I[c], below[c]);
					if (bin0 + c >= i0 && bin0 + c <= i1) slab[bin0 + c - i0] = mu;
				}
			}
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the wave's own LDS writes, read back by other lanes of the same wave
		// -0 + x is x and x > -inf is true for every x the walk keeps: the sum and the maximum that start from the slab's first value
		double sum = -0.0;
		float top = -__builtin_inff();
		bool nan = false;
		auto take = [&](float x) {
			if (FN == 0) {
				sum += (double)x;
			} else {
				nan |= x != x;
				if (x > top) top = x;
			}
		};
		const unsigned whole = count & ~3u;
		for (unsigned d = 0; d < whole; d += 4) {
			const surf_f4 x = *reinterpret_cast<const surf_f4*>(slab + d);  // every lane the same quad: one broadcast read
#pragma unroll
			for (int c = 0; c < 4; c++) take(x[c]);
		}
		for (unsigned d = whole; d < count; d++) take(slab[d]);
		res = FN == 0 ? (float)(sum / (double)count) : nan ? __uint_as_float(SURF_NAN) : top;
		if (res != res) res = __uint_as_float(SURF_NAN);
	}
	if (lane == 0) a.out[r] = res;
}

}  // namespace oct
