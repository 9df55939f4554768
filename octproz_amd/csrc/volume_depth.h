// volume_depth.h -- the OCT Depth mode of include/octpipe.h "volume rendering" (step 4, OCT_DEPTH) and the surface map it is built on:
// oct_surface_kernel is the pre-pass (the reference's compute_sample_depths.glsl), oct_depth_kernel the ray cast (oct_depth.frag).
// The header comment of octpipe.h is the definition.
//
// The reference's pre-pass fills a float volume with the depth of every voxel below the detected surface, and the shader fetches that
// volume trilinearly next to the intensity.  That depth is a function of one integer per (x, y) column, the surface index s, so the
// pre-pass here writes a uint16 [Y][X] map (2 X Y bytes, nothing proportional to the voxel count) and the ray cast computes the eight
// texels of the depth fetch in registers from the four map entries of the sample's columns, with the indices and weights it already
// has for the intensity fetch.  Deliberate differences from the reference: every column is processed (the reference dispatches X / 16
// by Y / 16 groups and skips the remainder columns); the texels the reference leaves unwritten (index 0, indices above `start`) are
// 0; a texel's depth is the closed form 1 - (s - 1 - i) / Z, where the reference subtracts 1 / Z repeatedly.
//
// Steps 1 and 2 (pixel, camera, slab test, trip count, jitter) are restated from oct_render_kernel in render_pixel / render_ray
// rather than shared with it, so that the six existing modes keep compiling to the code they had.
#pragma once
#include "volume_render.h"

namespace oct {

constexpr int SURFACE_THREADS = 256;
constexpr int SURFACE_AHEAD = 8;  // slices in flight per lane

struct SurfaceArgs {
	const uint8_t* vox;
	uint16_t* map;
	unsigned columns;   // X * Y
	unsigned start;     // the first index examined: min((int)(Z - Z / 32.0f), Z - 1)
	unsigned firstHit;  // the smallest byte b with (float)b / 255.0f > T (256: none)
};

// One lane per column, x fastest: a wave reads 64 consecutive bytes of one z-slice (a slice is X * Y contiguous bytes, so the column
// index is the offset inside it).  The walk runs from `start` down to index 1 and stops at the column's first hit; AHEAD
// slices are loaded before the first of them is compared.  Index 0 and indices above `start` are never read.
template <int AHEAD>
__global__ __launch_bounds__(SURFACE_THREADS) void oct_surface_kernel(const SurfaceArgs a) {
	const unsigned c = blockIdx.x * SURFACE_THREADS + threadIdx.x;
	if (c >= a.columns) return;
	const uint8_t* col = a.vox + c;
	unsigned s = 0;
	for (int i0 = (int)a.start; i0 >= 1 && s == 0u; i0 -= AHEAD) {
		unsigned b[AHEAD];
#pragma unroll
		for (int j = 0; j < AHEAD; j++) {
			const int i = max(i0 - j, 1);  // (past the end of the walk: index 1 again, dropped below)
			b[j] = col[(size_t)i * a.columns];
		}
#pragma unroll
		for (int j = 0; j < AHEAD; j++)
			if (s == 0u && i0 - j >= 1 && b[j] >= a.firstHit) s = (unsigned)(i0 - j);
	}
	a.map[c] = (uint16_t)s;
}

struct DepthArgs {
	RenderArgs r;
	const uint16_t* map;  // s [Y][X]
	float invZ;           // 1.0f / (float)Z
	float ddMax;          // 1.01f * stepLength
};

__device__ __forceinline__ bool render_pixel(const RenderArgs& a, unsigned& px, unsigned& py) {
	const unsigned tile = (blockIdx.x & 7u) * a.tilesPerXcd + (blockIdx.x >> 3);
	if (tile >= a.tiles) return false;
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	px = (tile % a.tilesX) * 16u + (wave & 1u) * 8u + (lane & 7u);
	py = (tile / a.tilesX) * 16u + (wave >> 1) * 8u + (lane >> 3);
	return px < a.width && py < a.height;
}

struct RenderRay {
	V3 start, stop, ray, sv;
	float L, j;  // j: the jitter of step 2 (0 for jitterSeed = 0); the caller applies it to the end it marches from
	int K;
};
// steps 1 and 2; false: the pixel misses the box
__device__ __forceinline__ bool render_ray(const RenderArgs& a, unsigned px, unsigned py, RenderRay& r) {
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
	if (!(t1 > t0)) return false;
	const V3 size = top - bottom;
	const V3 e0 = o + d * t0 - bottom, e1 = o + d * t1 - bottom;
	r.start = v3(e0.x / size.x, e0.y / size.y, e0.z / size.z);
	r.stop = v3(e1.x / size.x, e1.y / size.y, e1.z / size.z);
	r.ray = r.stop - r.start;
	r.L = len3(r.ray);
	r.sv = v3(a.stepLength * r.ray.x / r.L, a.stepLength * r.ray.y / r.L, a.stepLength * r.ray.z / r.L);
	const float kf = ceilf(r.L / a.stepLength);
	r.K = kf > 0.0f ? (int)fminf(kf, (float)RENDER_MAX_STEPS) : 0;  // (NaN -> 0)
	r.j = 0.0f;
	if (a.jitterSeed) {
		unsigned h = px * 0x9E3779B1u + py * 0x85EBCA77u + a.jitterSeed * 0xC2B2AE3Du;
		h ^= h >> 15;
		h *= 0x2C1B3C6Du;
		h ^= h >> 12;
		h *= 0x297A2D39u;
		h ^= h >> 15;
		r.j = (float)(h >> 24) / 255.0f;
	}
	return true;
}

// D(x, y, i) of a column with surface index s
__device__ __forceinline__ float depth_texel(unsigned s, unsigned i, float invZ) {
	return (i >= 1u && i < s) ? 1.0f - (float)(s - 1u - i) * invZ : 0.0f;
}

// I(p) and Dtex(p): one set of clamped indices and weights (step 3), eight voxel bytes and four map entries
__device__ __forceinline__ void depth_fetch(const DepthArgs& da, V3 p, float& I, float& D) {
	const RenderArgs& a = da.r;
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
	const unsigned m0 = y0 * a.nx, m1 = y1 * a.nx;
	const unsigned s00 = da.map[m0 + x0], s01 = da.map[m0 + x1], s10 = da.map[m1 + x0], s11 = da.map[m1 + x1];
	{
		const float b00 = a000 + wx * (a001 - a000), b01 = a010 + wx * (a011 - a010);
		const float b10 = a100 + wx * (a101 - a100), b11 = a110 + wx * (a111 - a110);
		const float c0 = b00 + wy * (b01 - b00), c1 = b10 + wy * (b11 - b10);
		I = (c0 + wz * (c1 - c0)) / 255.0f;
	}
	{
		const float d000 = depth_texel(s00, z0, da.invZ), d001 = depth_texel(s01, z0, da.invZ);
		const float d010 = depth_texel(s10, z0, da.invZ), d011 = depth_texel(s11, z0, da.invZ);
		const float d100 = depth_texel(s00, z1, da.invZ), d101 = depth_texel(s01, z1, da.invZ);
		const float d110 = depth_texel(s10, z1, da.invZ), d111 = depth_texel(s11, z1, da.invZ);
		const float b00 = d000 + wx * (d001 - d000), b01 = d010 + wx * (d011 - d010);
		const float b10 = d100 + wx * (d101 - d100), b11 = d110 + wx * (d111 - d110);
		const float c0 = b00 + wy * (b01 - b00), c1 = b10 + wy * (b11 - b10);
		D = c0 + wz * (c1 - c0);
	}
}

// One lane per pixel, tiles as in oct_render_kernel.  The march runs from the far end over all K samples (the shader has no early
// exit); RENDER_AHEAD samples are fetched (12 loads each) before the first of them is compared, as the compare chain (the previous
// sample's depth, the blend) is sequential per ray and the fetches are not.  Samples past a ray's end are fetched and dropped.
template <bool SHADE, bool LUT>
__global__ __launch_bounds__(RENDER_THREADS) void oct_depth_kernel(const DepthArgs da) {
	const RenderArgs& a = da.r;
	unsigned px, py;
	if (!render_pixel(a, px, py)) return;
	RenderRay r;
	if (!render_ray(a, px, py, r)) {
		render_store(a, px, py, v3(a.bg[0], a.bg[1], a.bg[2]));
		return;
	}
	const V3 far = a.jitterSeed ? r.stop + r.sv * r.j : r.stop;
	V3 C = v3(0.0f, 0.0f, 0.0f);
	float Ca = 0.0f, Dold = 1.0f;
	for (int k0 = 0; k0 < r.K; k0 += RENDER_AHEAD) {
		float I[RENDER_AHEAD], D[RENDER_AHEAD];
#pragma unroll
		for (int j = 0; j < RENDER_AHEAD; j++) depth_fetch(da, far - r.sv * (float)(k0 + j), I[j], D[j]);
#pragma unroll
		for (int j = 0; j < RENDER_AHEAD; j++) {
			const int k = k0 + j;
			if (k >= r.K) continue;
			const float i = I[j], d = D[j];
			const float dd = fabsf(d - Dold);
			Dold = d;
			if (i > a.threshold && i < 0.9f && d > 0.1f && dd < da.ddMax) {
				const V3 c = LUT ? render_lut(a, d - 0.05f) : v3(d, d, d);
				const float ca = rpow(LUT ? i : d, a.alphaExponent);
				const float q = (1.0f - ca) * Ca;
				Ca = ca + q;
				C = v3((ca * c.x + q * C.x) / Ca, (ca * c.y + q * C.y) / Ca, (ca * c.z + q * C.z) / Ca);
				if (SHADE) {
					const V3 p = far - r.sv * (float)k;
					C = render_shade(a, C, p, r.ray, render_normal(a, p, 0.005f), 0.75f, 0.5f, 1.0f);
				}
			}
		}
	}
	const V3 out = v3(Ca * C.x + (1.0f - Ca) * a.bgGamma[0], Ca * C.y + (1.0f - Ca) * a.bgGamma[1], Ca * C.z + (1.0f - Ca) * a.bgGamma[2]);
	render_store(a, px, py, v3(rpow(out.x, a.invGamma), rpow(out.y, a.invGamma), rpow(out.z, a.invGamma)));
}

}  // namespace oct
