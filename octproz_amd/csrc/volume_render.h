// volume_render.h -- the ray caster of include/octpipe.h "volume rendering": one lane per pixel, a wave per 8 x 8 pixel tile, a
// workgroup of four waves per 16 x 16 tile; one kernel instance per (mode, shading, LUT).  The header comment of octpipe.h is the
// definition; the step numbers below are its.  Every voxel index is clamped to the array before it is used (step 3), so no position,
// NaN included, reads outside the volume; the march runs over the integer count K of step 2 and cannot run on.
//
// Four samples of a ray are fetched before the first of them is compared (8 byte loads each, 32 in flight per lane): the compare
// chain (running maximum, threshold, opacity) is sequential per ray, the fetches are not.  Samples past a ray's end or past its early
// termination are fetched and dropped; their addresses are clamped like any other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oct {

enum { RM_MIP = 0, RM_DMIP = 1, RM_XRAY = 2, RM_ALPHA = 3, RM_MIDA = 4, RM_ISO = 5 };
constexpr int RENDER_THREADS = 256;   // 16 x 16 pixels
constexpr int RENDER_MAX_STEPS = 1733;  // ceil(sqrt(3) / 0.001)
constexpr int RENDER_AHEAD = 4;       // samples in flight per lane

struct RenderArgs {
	const uint8_t* vox;
	const uint8_t* lut;  // RGBA quadruples
	void* image;
	unsigned nx, ny, nz, lutW;
	unsigned width, height, tilesX, tiles, tilesPerXcd;
	float rows[3][3];    // V[r][c], r, c < 3
	float origin[3], top[3];
	float focal, aspect;
	float stepLength, threshold, depthWeight, alphaExponent, invGamma;
	float bg[3], bgGamma[3], material[3], light[3];
	int smooth;
	unsigned jitterSeed, u8;
};

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float len3(V3 a) { return sqrtf(dot3(a, a)); }
__device__ __forceinline__ V3 normalize3(V3 a) {
	const float l = len3(a);
	return l > 0.0f ? v3(a.x / l, a.y / l, a.z / l) : v3(0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ float rpow(float x, float y) { return x > 0.0f ? powf(x, y) : 0.0f; }

// step 1: one component of the ray direction, every product rounded on its own (no fused multiply-add): a quarter turn of the camera about
// its axis then permutes the pixels' rays exactly
__device__ __forceinline__ float render_direction(float cx, float cy, float cz, float r0, float r1, float r2) {
#pragma clang fp contract(off)
	const float p0 = cx * r0, p1 = cy * r1, p2 = cz * r2;
	return (p0 + p1) + p2;
}

// step 3: the two clamped texel indices and the weight of one axis
__device__ __forceinline__ void render_axis(float p, unsigned n, unsigned& i0, unsigned& i1, float& w) {
	float u = p * (float)n - 0.5f;
	u = fminf(fmaxf(u, -1.0f), (float)n);  // (NaN -> -1)
	const float fl = floorf(u);
	w = u - fl;
	const int i = (int)fl, last = (int)n - 1;
	i0 = (unsigned)min(max(i, 0), last);
	i1 = (unsigned)min(max(i + 1, 0), last);
}

__device__ __forceinline__ float render_fetch(const RenderArgs& a, V3 p) {
	unsigned x0, x1, y0, y1, z0, z1;
	float wx, wy, wz;
	render_axis(p.x, a.nx, x0, x1, wx);
	render_axis(p.y, a.ny, y0, y1, wy);
	render_axis(p.z, a.nz, z0, z1, wz);
	const size_t r00 = ((size_t)z0 * a.ny + y0) * a.nx, r01 = ((size_t)z0 * a.ny + y1) * a.nx;
	const size_t r10 = ((size_t)z1 * a.ny + y0) * a.nx, r11 = ((size_t)z1 * a.ny + y1) * a.nx;
	const float a000 = (float)a.vox[r00 + x0], a001 = (float)a.vox[r00 + x1];
	const float a010 = (float)a.vox[r01 + x0], a011 = (float)a.vox[r01 + x1];
	const float a100 = (float)a.vox[r10 + x0], a101 = (float)a.vox[r10 + x1];
	const float a110 = (float)a.vox[r11 + x0], a111 = (float)a.vox[r11 + x1];
	const float b00 = a000 + wx * (a001 - a000), b01 = a010 + wx * (a011 - a010);
	const float b10 = a100 + wx * (a101 - a100), b11 = a110 + wx * (a111 - a110);
	const float c0 = b00 + wy * (b01 - b00), c1 = b10 + wy * (b11 - b10);
	return (c0 + wz * (c1 - c0)) / 255.0f;
}

__device__ __forceinline__ V3 render_lut(const RenderArgs& a, float i) {
	unsigned i0, i1;
	float w;
	render_axis(i, a.lutW, i0, i1, w);
	const uint8_t* e0 = a.lut + 4 * (size_t)i0;
	const uint8_t* e1 = a.lut + 4 * (size_t)i1;
	const float r0 = (float)e0[0], g0 = (float)e0[1], b0 = (float)e0[2];
	const float r1 = (float)e1[0], g1 = (float)e1[1], b1 = (float)e1[2];
	return v3((r0 + w * (r1 - r0)) / 255.0f, (g0 + w * (g1 - g0)) / 255.0f, (b0 + w * (b1 - b0)) / 255.0f);
}

template <int MODE, bool LUT>
__device__ __forceinline__ V3 render_transfer_rgb(const RenderArgs& a, float i) {
	if (LUT) return render_lut(a, i);
	if (MODE == RM_DMIP) return v3(i + (1.0f - i) * 0.1f, i, i + (1.0f - i) * 0.2f);
	return v3(i, i, i);
}

__device__ __forceinline__ V3 render_normal(const RenderArgs& a, V3 p, float h) {
	const float e = 0.577350269f, eh = e * h;
	const float i0 = render_fetch(a, v3(p.x + eh, p.y - eh, p.z - eh));
	const float i1 = render_fetch(a, v3(p.x - eh, p.y - eh, p.z + eh));
	const float i2 = render_fetch(a, v3(p.x - eh, p.y + eh, p.z - eh));
	const float i3 = render_fetch(a, v3(p.x + eh, p.y + eh, p.z + eh));
	V3 n = v3(0.0f, 0.0f, 0.0f);
	n = n + v3(e, -e, -e) * i0;
	n = n + v3(-e, -e, e) * i1;
	n = n + v3(-e, e, -e) * i2;
	n = n + v3(e, e, e) * i3;
	const V3 u = normalize3(n);
	return v3(-u.x, -u.y, -u.z);
}

__device__ __forceinline__ V3 render_shade(const RenderArgs& a, V3 colour, V3 p, V3 ray, V3 N, float Ia, float kd, float ks) {
	const V3 Lv = normalize3(v3(a.light[0], a.light[1], a.light[2]) - p);
	const V3 nr = normalize3(ray);
	const V3 Vw = v3(-nr.x, -nr.y, -nr.z);
	const V3 H = normalize3(Lv + Vw);
	const float d = Ia + kd * fmaxf(0.0f, dot3(N, Lv));
	const float s = ks * rpow(fmaxf(0.0f, dot3(N, H)), 600.0f);
	return v3(d * colour.x + s, d * colour.y + s, d * colour.z + s);
}

__device__ __forceinline__ float render_clamp01(float c) { return fminf(fmaxf(c, 0.0f), 1.0f); }  // (NaN -> 0)

__device__ __forceinline__ void render_store(const RenderArgs& a, unsigned px, unsigned py, V3 c) {
	const float r = render_clamp01(c.x), g = render_clamp01(c.y), b = render_clamp01(c.z);
	const size_t i = (size_t)py * a.width + px;
	if (a.u8) {
		uchar4 o;
		o.x = (unsigned char)(r * 255.0f + 0.5f);
		o.y = (unsigned char)(g * 255.0f + 0.5f);
		o.z = (unsigned char)(b * 255.0f + 0.5f);
		o.w = 255;
		reinterpret_cast<uchar4*>(a.image)[i] = o;
	} else {
		reinterpret_cast<float4*>(a.image)[i] = make_float4(r, g, b, 1.0f);
	}
}

template <int MODE, bool SHADE, bool LUT>
__global__ __launch_bounds__(RENDER_THREADS) void oct_render_kernel(const RenderArgs a) {
	// workgroups b, b + 8, b + 16 ... share an XCD (and its L2): give each XCD a contiguous run of tiles of the picture
	const unsigned tile = (blockIdx.x & 7u) * a.tilesPerXcd + (blockIdx.x >> 3);
	if (tile >= a.tiles) return;
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const unsigned px = (tile % a.tilesX) * 16u + (wave & 1u) * 8u + (lane & 7u);
	const unsigned py = (tile / a.tilesX) * 16u + (wave >> 1) * 8u + (lane >> 3);
	if (px >= a.width || py >= a.height) return;

	// step 1
	const float cx = (2.0f * ((float)px + 0.5f) / (float)a.width - 1.0f) * a.aspect;
	const float cy = 2.0f * ((float)py + 0.5f) / (float)a.height - 1.0f;
	const float cz = -a.focal;
	const V3 d = v3(render_direction(cx, cy, cz, a.rows[0][0], a.rows[1][0], a.rows[2][0]), render_direction(cx, cy, cz, a.rows[0][1], a.rows[1][1], a.rows[2][1]),
	                render_direction(cx, cy, cz, a.rows[0][2], a.rows[1][2], a.rows[2][2]));
	const V3 o = v3(a.origin[0], a.origin[1], a.origin[2]), top = v3(a.top[0], a.top[1], a.top[2]);
	const V3 bottom = v3(-top.x, -top.y, -top.z);
	const V3 inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const V3 ta = v3(inv.x * (top.x - o.x), inv.y * (top.y - o.y), inv.z * (top.z - o.z));
	const V3 tb = v3(inv.x * (bottom.x - o.x), inv.y * (bottom.y - o.y), inv.z * (bottom.z - o.z));
	const float t0 = fmaxf(0.0f, fmaxf(fmaxf(fminf(ta.x, tb.x), fminf(ta.y, tb.y)), fminf(ta.z, tb.z)));
	const float t1 = fminf(fminf(fmaxf(ta.x, tb.x), fmaxf(ta.y, tb.y)), fmaxf(ta.z, tb.z));
	if (!(t1 > t0)) {
		render_store(a, px, py, v3(a.bg[0], a.bg[1], a.bg[2]));
		return;
	}
	// step 2
	const V3 size = top - bottom;
	const V3 e0 = o + d * t0 - bottom, e1 = o + d * t1 - bottom;
	V3 start = v3(e0.x / size.x, e0.y / size.y, e0.z / size.z);
	const V3 stop = v3(e1.x / size.x, e1.y / size.y, e1.z / size.z);
	const V3 ray = stop - start;
	const float L = len3(ray);
	const V3 sv = v3(a.stepLength * ray.x / L, a.stepLength * ray.y / L, a.stepLength * ray.z / L);
	const float kf = ceilf(L / a.stepLength);
	const int K = kf > 0.0f ? (int)fminf(kf, (float)RENDER_MAX_STEPS) : 0;  // (NaN -> 0)
	if (a.jitterSeed) {
		unsigned h = px * 0x9E3779B1u + py * 0x85EBCA77u + a.jitterSeed * 0xC2B2AE3Du;
		h ^= h >> 15;
		h *= 0x2C1B3C6Du;
		h ^= h >> 12;
		h *= 0x297A2D39u;
		h ^= h >> 15;
		start = start + sv * ((float)(h >> 24) / 255.0f);
	}

	// step 4
	float m = 0.0f, sum = 0.0f;
	int count = 0;
	V3 C = v3(0.0f, 0.0f, 0.0f), pmax = start, hit = start;
	float Ca = 0.0f;
	bool done = false, found = false;
	for (int k0 = 0; k0 < K && !done; k0 += RENDER_AHEAD) {
		float I[RENDER_AHEAD];
#pragma unroll
		for (int j = 0; j < RENDER_AHEAD; j++) I[j] = render_fetch(a, start + sv * (float)(k0 + j));
#pragma unroll
		for (int j = 0; j < RENDER_AHEAD; j++) {
			const int k = k0 + j;
			if (k >= K || done) continue;
			const float i = I[j];
			if (MODE == RM_MIP || MODE == RM_DMIP) {
				if (i > m && i > a.threshold) {
					m = i;
					if (MODE == RM_DMIP) pmax = start + sv * (float)k;
				}
				done = !(m < 0.99f);
			} else if (MODE == RM_XRAY) {
				if (i > a.threshold) {
					sum += i;
					count++;
				}
			} else if (MODE == RM_ALPHA) {
				if (i > a.threshold) {
					const V3 c = render_transfer_rgb<MODE, LUT>(a, i);
					const float ca = rpow(i, a.alphaExponent);
					const float q = (1.0f - ca) * Ca;
					C = v3(ca * c.x + q * C.x, ca * c.y + q * C.y, ca * c.z + q * C.z);
					Ca = ca + (1.0f - ca) * Ca;
					const float cue = rpow(2.25f, (L - (float)k * a.stepLength) / L) / 1.75f;
					C = v3(Ca * C.x * cue, Ca * C.y * cue, Ca * C.z * cue);
					if (SHADE) {
						const V3 p = start + sv * (float)k;
						C = render_shade(a, C, p, ray, render_normal(a, p, 0.005f), 0.75f, 0.5f, 1.0f);
					}
				}
				done = !(Ca < 0.9f);
			} else if (MODE == RM_MIDA) {
				if (i > a.threshold && i > m) {
					const V3 c = render_transfer_rgb<MODE, LUT>(a, i);
					const float ca = rpow(i, a.alphaExponent);
					const float w = 1.0f - (i - m);
					m = i;
					const float q = (1.0f - w * Ca) * ca;
					C = v3(w * C.x + q * c.x, w * C.y + q * c.y, w * C.z + q * c.z);
					Ca = w * Ca + q;
					if (SHADE) {
						const V3 p = start + sv * (float)k;
						C = render_shade(a, C, p, ray, render_normal(a, p, 0.005f), 0.75f, 0.35f, 0.2f);
					}
				}
				done = !(Ca < 0.9f);
			} else {
				if (i > a.threshold) {
					hit = start + sv * (float)k;
					found = true;
					done = true;
				}
			}
		}
	}

	V3 out;
	if (MODE == RM_ISO) {
		if (!found) {
			render_store(a, px, py, v3(a.bg[0], a.bg[1], a.bg[2]));
			return;
		}
		V3 q = hit - sv * 0.5f;
		const float i2 = render_fetch(a, q);
		q = q - sv * (i2 > a.threshold ? 0.25f : -0.25f);
		V3 N;
		if (a.smooth > 0) {
			const int n = a.smooth;
			V3 acc = v3(0.0f, 0.0f, 0.0f);
			for (int x = -n; x <= n; x++)
				for (int y = -n; y <= n; y++)
					for (int z = -n; z <= n; z++)
						acc = acc + render_normal(a, v3(q.x + (float)x * 0.001f, q.y + (float)y * 0.001f, q.z + (float)z * 0.001f), 0.001f);
			const float cnt = (float)((2 * n + 1) * (2 * n + 1) * (2 * n + 1));
			N = normalize3(v3(acc.x / cnt, acc.y / cnt, acc.z / cnt));
		} else {
			N = render_normal(a, q, 0.001f);
		}
		out = render_shade(a, v3(a.material[0], a.material[1], a.material[2]), q, ray, N, 0.2f, 0.7f, 1.5f);
	} else {
		if (MODE == RM_MIP || MODE == RM_DMIP || MODE == RM_XRAY) {
			if (MODE == RM_XRAY) m = count > 0 ? sqrtf(sum / (float)count) : 0.0f;
			C = render_transfer_rgb<MODE, LUT>(a, m);
			Ca = rpow(m, a.alphaExponent);
			if (MODE == RM_DMIP) {
				const float depth = len3(pmax - start) / len3(stop - start);
				const float f = (1.0f - a.depthWeight) + 2.0f * a.depthWeight * (1.0f - depth);
				C = C * f;
				Ca *= f;
			}
		}
		out = v3(Ca * C.x + (1.0f - Ca) * a.bgGamma[0], Ca * C.y + (1.0f - Ca) * a.bgGamma[1], Ca * C.z + (1.0f - Ca) * a.bgGamma[2]);
	}
	render_store(a, px, py, v3(rpow(out.x, a.invGamma), rpow(out.y, a.invGamma), rpow(out.z, a.invGamma)));
}

}  // namespace oct
