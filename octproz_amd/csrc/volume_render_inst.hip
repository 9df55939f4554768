// volume_render_inst.hip -- instantiates the ray caster (volume_render.h): MIP, DMIP and X-ray with and without the colour table (their
// shaders never shade), alpha blending and MIDA with and without shading and the colour table, the isosurface (always shaded, no table);
// and the OCT Depth mode (volume_depth.h): its surface pre-pass, and its ray cast with and without shading and the colour table.
#include "volume_depth.h"

namespace oct {

template <int MODE, bool SHADE, bool LUT>
static void render_go(const RenderArgs& a, hipStream_t s) {
	hipLaunchKernelGGL((oct_render_kernel<MODE, SHADE, LUT>), dim3(a.tilesPerXcd * 8u), dim3(RENDER_THREADS), 0, s, a);
}

template <int MODE>
static void render_plain(bool lut, const RenderArgs& a, hipStream_t s) {
	if (lut) render_go<MODE, false, true>(a, s);
	else render_go<MODE, false, false>(a, s);
}

template <int MODE>
static void render_shaded(bool shade, bool lut, const RenderArgs& a, hipStream_t s) {
	if (shade) {
		if (lut) render_go<MODE, true, true>(a, s);
		else render_go<MODE, true, false>(a, s);
	} else {
		render_plain<MODE>(lut, a, s);
	}
}

// one launch over the picture's 16 x 16 tiles; a.tiles, a.tilesX, a.tilesPerXcd are filled in here
hipError_t launch_render(int mode, bool shade, bool lut, RenderArgs a, hipStream_t s) {
	a.tilesX = (a.width + 15u) / 16u;
	a.tiles = a.tilesX * ((a.height + 15u) / 16u);
	a.tilesPerXcd = (a.tiles + 7u) / 8u;
	switch (mode) {
	case RM_MIP: render_plain<RM_MIP>(lut, a, s); break;
	case RM_DMIP: render_plain<RM_DMIP>(lut, a, s); break;
	case RM_XRAY: render_plain<RM_XRAY>(lut, a, s); break;
	case RM_ALPHA: render_shaded<RM_ALPHA>(shade, lut, a, s); break;
	case RM_MIDA: render_shaded<RM_MIDA>(shade, lut, a, s); break;
	case RM_ISO: render_go<RM_ISO, true, false>(a, s); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

// the pre-pass: one lane per (x, y) column
hipError_t launch_surface(SurfaceArgs a, hipStream_t s) {
	hipLaunchKernelGGL((oct_surface_kernel<SURFACE_AHEAD>), dim3((a.columns + SURFACE_THREADS - 1u) / SURFACE_THREADS), dim3(SURFACE_THREADS), 0, s, a);
	return hipGetLastError();
}

template <bool SHADE, bool LUT>
static void depth_go(const DepthArgs& a, hipStream_t s) {
	hipLaunchKernelGGL((oct_depth_kernel<SHADE, LUT>), dim3(a.r.tilesPerXcd * 8u), dim3(RENDER_THREADS), 0, s, a);
}

// the OCT Depth ray cast over the picture's 16 x 16 tiles, as launch_render
hipError_t launch_depth_render(bool shade, bool lut, DepthArgs a, hipStream_t s) {
	a.r.tilesX = (a.r.width + 15u) / 16u;
	a.r.tiles = a.r.tilesX * ((a.r.height + 15u) / 16u);
	a.r.tilesPerXcd = (a.r.tiles + 7u) / 8u;
	if (shade) {
		if (lut) depth_go<true, true>(a, s);
		else depth_go<true, false>(a, s);
	} else {
		if (lut) depth_go<false, true>(a, s);
		else depth_go<false, false>(a, s);
	}
	return hipGetLastError();
}

}  // namespace oct
