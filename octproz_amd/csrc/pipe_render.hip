// pipe_render.hip -- volume rendering (include/octpipe.h "volume rendering"; reference: src/glwindow3d.cpp, src/raycastvolume.cpp and
// the fragment shaders): the settings checks, the host side of the camera (focal length, ray origin, box), the colour table, and one
// launch of oct_render_kernel (volume_render.h) on the handle's compute stream behind what is already enqueued there.  The OCT Depth
// mode (volume_depth.h; reference: compute_sample_depths.glsl, oct_depth.frag) has its own entry point: the surface pre-pass and its ray
// cast back to back on that stream; octpipe_volume_surface_map is the pre-pass alone.  The image, the colour table, the staging copy of
// host voxels and the surface map belong to the handle (RenderState, released in octpipe_destroy); nothing the processing chain reads or
// writes is touched.
#include "pipe_internal.h"
#include "volume_depth.h"

namespace oct {
hipError_t launch_render(int mode, bool shade, bool lut, RenderArgs a, hipStream_t s);
hipError_t launch_surface(SurfaceArgs a, hipStream_t s);
hipError_t launch_depth_render(bool shade, bool lut, DepthArgs a, hipStream_t s);
}  // namespace oct

namespace octimpl {

namespace {

constexpr const char* kWhat = "volume rendering";
constexpr unsigned kMaxExtent = 4096;  // viewport, voxel array and colour table, per dimension

bool inRange(float v, float lo, float hi) { return v >= lo && v <= hi; }  // (false for NaN)

int bad(const char* field, const char* range) { return fail(OCTPIPE_ERR_INVALID_ARGUMENT, std::string(kWhat) + ": " + field + " must be " + range); }

// every field of the settings against its range; fills the camera part of the kernel's arguments
int checkSettings(const OctPipeRenderSettings& s, oct::RenderArgs& a, bool depth) {
	if (depth && s.mode != OCTPIPE_RENDER_OCT_DEPTH) return bad("mode", "OCTPIPE_RENDER_OCT_DEPTH in octpipe_render_oct_depth");
	if (!depth && s.mode > OCTPIPE_RENDER_ISOSURFACE)
		return bad("mode", "one of OCTPIPE_RENDER_MIP ... OCTPIPE_RENDER_ISOSURFACE (OCTPIPE_RENDER_OCT_DEPTH: octpipe_render_oct_depth)");
	if (s.width < 1 || s.width > kMaxExtent) return bad("width", "1 ... 4096");
	if (s.height < 1 || s.height > kMaxExtent) return bad("height", "1 ... 4096");
	for (float v : s.viewMatrix)
		if (!std::isfinite(v)) return bad("viewMatrix", "finite");
	if (!(s.fovDegrees > 0.0f && s.fovDegrees < 180.0f)) return bad("fovDegrees", "above 0 and below 180");
	for (float v : s.stretch)
		if (!inRange(v, 0.1f, 9999.0f)) return bad("stretch", "0.1 ... 9999");
	if (!inRange(s.stepLength, 0.001f, 10.0f)) return bad("stepLength", "0.001 ... 10");
	if (!inRange(s.threshold, 0.0f, 1.0f)) return bad("threshold", "0 ... 1");
	if (!inRange(s.depthWeight, 0.0f, 1.0f)) return bad("depthWeight", "0 ... 1");
	if (!inRange(s.alphaExponent, 0.1f, 10.0f)) return bad("alphaExponent", "0.1 ... 10");
	if (!inRange(s.gamma, 0.1f, 10.0f)) return bad("gamma", "0.1 ... 10");
	if (s.smoothFactor < 0 || s.smoothFactor > 3) return bad("smoothFactor", "0 ... 3");
	for (float v : s.background)
		if (!inRange(v, 0.0f, 1.0f)) return bad("background", "0 ... 1");
	for (float v : s.material)
		if (!inRange(v, 0.0f, 1.0f)) return bad("material", "0 ... 1");
	for (float v : s.lightPosition)
		if (!std::isfinite(v)) return bad("lightPosition", "finite");
	if (s.outputFormat > OCTPIPE_RENDER_RGBA_U8) return bad("outputFormat", "OCTPIPE_RENDER_RGBA_F32 or OCTPIPE_RENDER_RGBA_U8");
	// the ray origin: the fourth column of the inverse, -R^-1 t
	double R[3][3], t[3];
	for (int r = 0; r < 3; r++) {
		for (int c = 0; c < 3; c++) R[r][c] = s.viewMatrix[4 * r + c];
		t[r] = s.viewMatrix[4 * r + 3];
	}
	double cof[3][3];
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 3; c++) {
			const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
			cof[r][c] = R[r1][c1] * R[r2][c2] - R[r1][c2] * R[r2][c1];
		}
	const double det = R[0][0] * cof[0][0] + R[0][1] * cof[0][1] + R[0][2] * cof[0][2];
	if (!std::isfinite(det) || std::fabs(det) < 1e-12) return bad("viewMatrix", "invertible in its upper left 3 x 3");
	for (int i = 0; i < 3; i++) {
		double o = 0.0;
		for (int j = 0; j < 3; j++) o -= cof[j][i] / det * t[j];  // (R^-1)[i][j] = cof[j][i] / det
		if (!std::isfinite(o) || std::fabs(o) > 3.0e38) return bad("viewMatrix", "invertible in its upper left 3 x 3");
		a.origin[i] = (float)o;
		for (int j = 0; j < 3; j++) a.rows[i][j] = s.viewMatrix[4 * i + j];
	}
	a.focal = (float)(1.0 / std::tan((double)s.fovDegrees * M_PI / 180.0 / 2.0));
	a.aspect = (float)((double)s.width / (double)s.height);
	a.width = s.width;
	a.height = s.height;
	a.stepLength = s.stepLength;
	a.threshold = s.threshold;
	a.depthWeight = s.depthWeight;
	a.alphaExponent = s.alphaExponent;
	a.invGamma = (float)(1.0 / (double)s.gamma);
	for (int i = 0; i < 3; i++) {
		a.bg[i] = s.background[i];
		a.bgGamma[i] = s.background[i] > 0.0f ? (float)std::pow((double)s.background[i], (double)s.gamma) : 0.0f;
		a.material[i] = s.material[i];
		a.light[i] = s.lightPosition[i];
	}
	a.smooth = s.smoothFactor;
	a.jitterSeed = s.jitterSeed;
	a.u8 = s.outputFormat == OCTPIPE_RENDER_RGBA_U8 ? 1u : 0u;
	return OCTPIPE_OK;
}

// raycastvolume.cpp:192-220 in float32
void boxTop(const uint32_t dims[3], const float stretch[3], float top[3]) {
	float e[3], mx = 0.0f;
	for (int i = 0; i < 3; i++) {
		e[i] = (float)dims[i] * stretch[i];
		mx = std::max(mx, e[i]);
	}
	for (int i = 0; i < 3; i++) top[i] = (e[i] / mx) / 2.0f;
}

bool modeReadsLut(uint32_t mode) { return mode != OCTPIPE_RENDER_ISOSURFACE; }

// the caller's dims (the check that needs no handle): dm = dims, or zeros for voxels = NULL
int checkDims(const uint8_t* voxels, const uint32_t* dims, uint32_t dm[3]) {
	dm[0] = dm[1] = dm[2] = 0;
	if (!voxels) return OCTPIPE_OK;
	if (!dims) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, std::string(kWhat) + ": dims is NULL");
	for (int i = 0; i < 3; i++) {
		if (dims[i] < 1 || dims[i] > kMaxExtent) return bad("dims", "1 ... 4096 each");
		dm[i] = dims[i];
	}
	return OCTPIPE_OK;
}

// voxels = NULL: the handle's volume view and its dims
int ownVolumeDims(octpipe* h, const uint8_t* voxels, uint32_t dm[3]) {
	if (voxels) return OCTPIPE_OK;
	const std::string w(kWhat);
	if (!h->d_volumeView)
		return fail(OCTPIPE_ERR_NOT_INITIALIZED, w + ": voxels is NULL and the handle has no volume view buffer yet (process a buffer with volumeViewEnabled)");
	dm[0] = (uint32_t)h->A;
	dm[1] = (uint32_t)h->B * h->acq.buffersPerVolume;
	dm[2] = (uint32_t)(h->N / 2);
	for (int i = 0; i < 3; i++)
		if (dm[i] > kMaxExtent) return fail(OCTPIPE_ERR_UNSUPPORTED, w + ": the volume view exceeds 4096 voxels along an axis");
	return OCTPIPE_OK;
}

// the voxels on the device: the handle's volume view, the caller's device memory, or the staging copy of the caller's host memory
int deviceVoxels(octpipe* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dm[3], const uint8_t** out) {
	RenderState& rs = h->renderState;
	if (!voxels) {
		*out = h->d_volumeView;
	} else if (voxelsAreDevice) {
		*out = voxels;
	} else {
		const size_t voxelBytes = (size_t)dm[0] * dm[1] * dm[2];
		if (int rc = grow(h, rs, RenderState::STAGE, voxelBytes)) return rc;
		HIP_TRY(hipMemcpyAsync(rs.p[RenderState::STAGE], voxels, voxelBytes, hipMemcpyHostToDevice, h->stream));
		HIP_TRY(hipStreamSynchronize(h->stream));  // the caller's memory is free again when the call returns
		*out = rs.as<const uint8_t>(RenderState::STAGE);
	}
	return OCTPIPE_OK;
}

// the pre-pass of the OCT Depth mode on the compute stream: the surface map of `vox` for the depth threshold T into the handle's
// SURFACE slot (2 X Y bytes)
int enqueueSurface(octpipe* h, const uint8_t* vox, const uint32_t dm[3], float T) {
	RenderState& rs = h->renderState;
	const size_t columns = (size_t)dm[0] * dm[1];
	if (int rc = grow(h, rs, RenderState::SURFACE, columns * sizeof(uint16_t))) return rc;
	oct::SurfaceArgs sa{};
	sa.vox = vox;
	sa.map = rs.as<uint16_t>(RenderState::SURFACE);
	sa.columns = (unsigned)columns;
	const float z = (float)dm[2];
	sa.start = (unsigned)std::min((int)(z - z / 32.0f), (int)dm[2] - 1);
	sa.firstHit = 256u;
	for (unsigned b = 0; b < 256u; b++)
		if ((float)b / 255.0f > T) {
			sa.firstHit = b;
			break;
		}
	const hipError_t e = oct::launch_surface(sa, h->stream);
	if (e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, std::string(kWhat) + ": " + hipGetErrorString(e));
	return OCTPIPE_OK;
}

// octpipe_render_volume (depth = false) and octpipe_render_oct_depth (depth = true); kernelMs: the ray cast, prepassMs: the pre-pass
int entry(octpipe* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t* dims, const OctPipeRenderSettings* s, void** d_image, size_t* bytes,
          double* kernelMs, bool depth = false, double* prepassMs = nullptr) {
	// (the checks that need no handle come first)
	const std::string w(kWhat);
	if (!s) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": settings is NULL");
	const OctPipeRenderSettings st = *s;
	oct::RenderArgs a{};
	int rc = checkSettings(st, a, depth);
	if (rc) return rc;
	uint32_t dm[3];
	if ((rc = checkDims(voxels, dims, dm))) return rc;
	if ((rc = enterCall(h, kWhat))) return rc;
	RenderState& rs = h->renderState;
	if ((rc = ownVolumeDims(h, voxels, dm))) return rc;
	const bool lut = st.lutEnabled != 0 && modeReadsLut(st.mode);
	if (lut && !rs.lutWidth) return fail(OCTPIPE_ERR_NOT_INITIALIZED, w + ": lutEnabled without a colour table (octpipe_update_render_lut)");
	if ((rc = deviceVoxels(h, voxels, voxelsAreDevice, dm, &a.vox))) return rc;
	a.nx = dm[0];
	a.ny = dm[1];
	a.nz = dm[2];
	boxTop(dm, st.stretch, a.top);
	a.lut = lut ? rs.as<const uint8_t>(RenderState::LUT) : nullptr;
	a.lutW = lut ? rs.lutWidth : 0u;
	const size_t imageBytes = (size_t)st.width * st.height * (a.u8 ? 4u : 16u);
	if ((rc = grow(h, rs, RenderState::IMAGE, imageBytes))) return rc;
	a.image = rs.p[RenderState::IMAGE];
	StreamTimer timer(kernelMs != nullptr, kWhat), preTimer(depth && prepassMs != nullptr, kWhat);
	hipError_t e;
	if (depth) {
		if ((rc = preTimer.begin(h->stream))) return rc;
		if ((rc = enqueueSurface(h, a.vox, dm, 1.5f * st.threshold))) return rc;  // glwindow3d.cpp:184
		if ((rc = preTimer.end(h->stream))) return rc;
		oct::DepthArgs da{};
		da.r = a;
		da.map = rs.as<const uint16_t>(RenderState::SURFACE);
		da.invZ = 1.0f / (float)dm[2];
		da.ddMax = 1.01f * st.stepLength;
		if ((rc = timer.begin(h->stream))) return rc;
		e = oct::launch_depth_render(st.shadingEnabled != 0, lut, da, h->stream);
	} else {
		if ((rc = timer.begin(h->stream))) return rc;
		e = oct::launch_render((int)st.mode, st.shadingEnabled != 0, lut, a, h->stream);
	}
	if (e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, w + ": " + hipGetErrorString(e));
	rs.imageBytes = imageBytes;
	if (kernelMs || (depth && prepassMs)) {
		if ((rc = timer.end(h->stream))) return rc;
		e = hipStreamSynchronize(h->stream);
		if (e == hipSuccess) e = timer.elapsedMs(kernelMs);
		if (e == hipSuccess) e = preTimer.elapsedMs(prepassMs);
		if (e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, w + ": " + hipGetErrorString(e));
	}
	if (d_image) *d_image = rs.p[RenderState::IMAGE];
	if (bytes) *bytes = imageBytes;
	return OCTPIPE_OK;
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

void octpipe_default_render_settings(OctPipeRenderSettings* s) {
	if (!s) return;
	memset(s, 0, sizeof(*s));
	s->mode = OCTPIPE_RENDER_MIP;  // glwindow3d.cpp:96
	s->width = 512;
	s->height = 512;
	const float q[4] = {1.0f, 0.0f, 0.0f, 0.0f};
	octpipe_render_view_matrix(q, 0.0f, 0.0f, -500.0f, s->viewMatrix);  // glwindow3d.h:236, glwindow3d.cpp:301-303
	s->fovDegrees = 50.0f;  // glwindow3d.h:206
	for (int i = 0; i < 3; i++) {
		s->stretch[i] = 1.0f;     // raycastvolume.cpp:99-101
		s->background[i] = 0.0f;  // glwindow3d.cpp:89
		s->material[i] = 1.0f;    // glwindow3d.h:214
	}
	s->stepLength = 0.01f;    // glwindow3d.cpp:98
	s->threshold = 0.5f;      // glwindow3d.cpp:97
	s->depthWeight = 0.7f;    // glwindow3d.cpp:84
	s->alphaExponent = 2.0f;  // glwindow3d.cpp:85
	s->gamma = 2.2f;          // glwindow3d.h:219
	s->smoothFactor = 1;      // glwindow3d.cpp:86
	s->shadingEnabled = 1;    // glwindow3d.cpp:87
	s->lutEnabled = 0;        // glwindow3d.cpp:88
	s->lightPosition[0] = 1.0f;  // glwindow3d.h:213
	s->lightPosition[1] = 3.0f;
	s->lightPosition[2] = 3.0f;
	s->jitterSeed = 0;
	s->outputFormat = OCTPIPE_RENDER_RGBA_F32;
}

int octpipe_render_view_matrix(const float quaternion[4], float viewX, float viewY, float distExp, float out[16]) {
	const std::string w(kWhat);
	if (!quaternion) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": quaternion is NULL");
	if (!out) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": out is NULL");
	double q[4], n2 = 0.0;
	for (int i = 0; i < 4; i++) {
		q[i] = quaternion[i];
		n2 += q[i] * q[i];
	}
	if (!std::isfinite(n2) || n2 <= 0.0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": quaternion must be finite and not zero");
	if (!std::isfinite(viewX) || !std::isfinite(viewY)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": viewX, viewY must be finite");
	const double tz = -4.0 * std::exp((double)distExp / 600.0);
	if (!std::isfinite(tz)) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": distExp must be finite and small enough for exp(distExp / 600)");
	const double n = std::sqrt(n2), qw = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
	const double m[16] = {1 - 2 * (y * y + z * z), 2 * (x * y - qw * z),     2 * (x * z + qw * y),     viewX,
	                      2 * (x * y + qw * z),     1 - 2 * (x * x + z * z), 2 * (y * z - qw * x),     viewY,
	                      2 * (x * z - qw * y),     2 * (y * z + qw * x),     1 - 2 * (x * x + y * y), tz,
	                      0, 0, 0, 1};
	for (int i = 0; i < 16; i++) out[i] = (float)m[i];
	return OCTPIPE_OK;
}

int octpipe_update_render_lut(octpipe_t* h, const uint8_t* rgba, unsigned width) {
	const std::string w(kWhat);
	if (!rgba) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": rgba is NULL");
	if (width < 2 || width > kMaxExtent) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": the colour table's width must be 2 ... 4096");
	int rc = enterCall(h, kWhat);
	if (rc) return rc;
	// (always the full capacity, so that a later table never reallocates under a queued render)
	if ((rc = grow(h, h->renderState, RenderState::LUT, 4u * kMaxExtent))) return rc;
	HIP_TRY(hipMemcpyAsync(h->renderState.p[RenderState::LUT], rgba, 4u * (size_t)width, hipMemcpyHostToDevice, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	h->renderState.lutWidth = width;
	return OCTPIPE_OK;
}

int octpipe_render_volume(octpipe_t* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dims[3], const OctPipeRenderSettings* s,
                          void** d_image, size_t* bytes) {
	return entry(h, voxels, voxelsAreDevice, dims, s, d_image, bytes, nullptr);
}

int octpipe_debug_render_volume(octpipe_t* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dims[3], const OctPipeRenderSettings* s,
                                void** d_image, size_t* bytes, double* kernelMs) {
	return entry(h, voxels, voxelsAreDevice, dims, s, d_image, bytes, kernelMs);
}

int octpipe_render_oct_depth(octpipe_t* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dims[3], const OctPipeRenderSettings* s,
                             void** d_image, size_t* bytes) {
	return entry(h, voxels, voxelsAreDevice, dims, s, d_image, bytes, nullptr, true);
}

int octpipe_debug_render_oct_depth(octpipe_t* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dims[3], const OctPipeRenderSettings* s,
                                   void** d_image, size_t* bytes, double* prepassMs, double* raycastMs) {
	return entry(h, voxels, voxelsAreDevice, dims, s, d_image, bytes, raycastMs, true, prepassMs);
}

int octpipe_volume_surface_map(octpipe_t* h, const uint8_t* voxels, int voxelsAreDevice, const uint32_t dims[3], float depthThreshold, uint16_t* map) {
	const std::string w(kWhat);
	if (!inRange(depthThreshold, 0.0f, 1.5f)) return bad("depthThreshold", "0 ... 1.5");
	if (!map) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": map is NULL");
	uint32_t dm[3];
	int rc = checkDims(voxels, dims, dm);
	if (rc) return rc;
	if ((rc = enterCall(h, kWhat))) return rc;
	if ((rc = ownVolumeDims(h, voxels, dm))) return rc;
	const uint8_t* vox = nullptr;
	if ((rc = deviceVoxels(h, voxels, voxelsAreDevice, dm, &vox))) return rc;
	if ((rc = enqueueSurface(h, vox, dm, depthThreshold))) return rc;
	HIP_TRY(hipMemcpyAsync(map, h->renderState.p[RenderState::SURFACE], (size_t)dm[0] * dm[1] * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	return OCTPIPE_OK;
}

int octpipe_copy_rendered_to_host(octpipe_t* h, void* dst, size_t bytes) {
	const std::string w(kWhat);
	if (!dst) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": dst is NULL");
	int rc = enterCall(h, kWhat);
	if (rc) return rc;
	const RenderState& rs = h->renderState;
	if (!rs.imageBytes) return fail(OCTPIPE_ERR_NOT_INITIALIZED, w + ": nothing rendered yet");
	if (bytes != rs.imageBytes)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, w + ": bytes = " + std::to_string(bytes) + " but the last image has " + std::to_string(rs.imageBytes));
	HIP_TRY(hipMemcpyAsync(dst, rs.p[RenderState::IMAGE], bytes, hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	return OCTPIPE_OK;
}

}  // extern "C"
