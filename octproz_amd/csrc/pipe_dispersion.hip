// pipe_dispersion.hip -- dispersion estimation (include/octpipe.h "dispersion estimation"; reference docs:
// docs/docs/plugin-dispersionestimator.md, processing.md:80-109).
//
// One call scores K candidates (d2[c], d3[c]) on M A-scans of one raw buffer:
//   1. the A-scans firstAscan-1 .. firstAscan+M (the Lanczos taps reach into both neighbours) are copied into scratch of the handle;
//   2. the product's front end runs on them ONCE: launchPrepare (unpack, bitshift, rolling average) and oct_lib_gather_kernel
//      (k-linearisation x window) with a unit phasor -> M real rows;
//   3. per chunk of candidates: oct_sweep_phasor_kernel (the K x N phasors, theta in the host's operation order),
//      oct_dispersion_sweep_kernel<LOG2N> (dispersion_sweep.h: one wave per (candidate, A-scan), one float out) and
//      oct_sweep_reduce_kernel (the mean over the M A-scans in index order).
// Everything runs on the handle's compute stream behind what is already enqueued there, and touches nothing the processing chain
// reads or writes: the handle's LUT, curves, mean line, one-shot flags, volume / display buffers and timing counters stay as they are.
#include <algorithm>

#include "pipe_internal.h"
#include "dispersion_sweep.h"

namespace oct {

// theta_c[j] = ((c3 x + c2) x + c1) x + c0 with x = j and one fmaf per step: the host's Horner (host_luts.cpp horner_curve) on the
// coefficients it pre-divides (scaled_cubic_coeffs), hence the host curve bit for bit; the phasor in full precision (theta reaches
// hundreds of radians, where __sinf / __cosf lose every digit)
__global__ __launch_bounds__(256) void oct_sweep_phasor_kernel(const float4* coef, f2* phasor, float* theta, int N, unsigned K) {
	const size_t total = (size_t)K * (size_t)N;
	for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
		const size_t c = idx / (size_t)N;
		const float x = (float)(int)(idx - c * (size_t)N);
		const float4 k = coef[c];
		float r = 0.0f;
		r = fmaf(r, x, k.w);
		r = fmaf(r, x, k.z);
		r = fmaf(r, x, k.y);
		r = fmaf(r, x, k.x);
		phasor[idx] = f2{cosf(r), sinf(r)};
		if (theta) theta[idx] = r;
	}
}

// score[c] = mean of metric[c][0 .. M-1], summed in index order (float64 accumulator): the same bits for every launch shape
__global__ __launch_bounds__(256) void oct_sweep_reduce_kernel(const float* metric, float* scores, unsigned K, unsigned M) {
	const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= K) return;
	const float* row = metric + (size_t)c * M;
	double s = 0.0;
	for (unsigned m = 0; m < M; ++m) s += (double)row[m];
	scores[c] = (float)(s / (double)M);
}

}  // namespace oct

namespace octimpl {

namespace {

constexpr size_t kSweepScratchBytes = 64ull << 20;  // phasors + metric matrix of one chunk of candidates

int checkLength(const octpipe* h) {
	const int N = h->N;
	if (N < 256 || N > 4096 || (N & (N - 1)) || h->bluestein)
		return fail(OCTPIPE_ERR_UNSUPPORTED, "dispersion estimation supports samplesPerLine = 256, 512, 1024, 2048 and 4096 (got " + std::to_string(N) + ")");
	return OCTPIPE_OK;
}

int checkMetric(const octpipe* h, const OctPipeDispersionMetric* m) {
	const uint64_t lines = (uint64_t)h->A * (uint64_t)h->B;
	if (m->ascanCount < 1 || (uint64_t)m->firstAscan + (uint64_t)m->ascanCount > lines)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion metric: need ascanCount >= 1 and firstAscan + ascanCount <= A*B = " + std::to_string(lines));
	if (m->ignoreFirstSamples >= (uint32_t)(h->N / 2 - 2))
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion metric: ignoreFirstSamples must be below N/2 - 2 = " + std::to_string(h->N / 2 - 2));
	if (m->metric < OCTPIPE_METRIC_SUM_ABOVE_THRESHOLD || m->metric > OCTPIPE_METRIC_MEAN_SOBEL)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion metric: unknown metric " + std::to_string(m->metric));
	return OCTPIPE_OK;
}

// steps 1 and 2: the M prepared rows of the metric's A-scans in scratch GATHERED; *rows points at the first of them
int prepareRows(octpipe* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m, const f2** rows) {
	const OctPipeParams& p = h->params;
	const int N = h->N;
	// (rows of whole bytes: this call needs a power-of-two N, so packed 12-bit rows never start inside a byte triple; cf. phase_stage.h)
	const size_t lines = (size_t)h->A * (size_t)h->B, rowBytes = rawBytes(h) / lines;
	const size_t lo = m->firstAscan > 0 ? m->firstAscan - 1 : 0;
	const size_t hi = std::min((size_t)m->firstAscan + m->ascanCount, lines - 1);  // inclusive
	const size_t count = hi - lo + 1;
	int rc;
	if ((rc = grow(h, h->sweep, SweepScratch::RAW, rowBytes * count)) || (rc = grow(h, h->sweep, SweepScratch::ROWS, sizeof(float) * count * N)) ||
	    (rc = grow(h, h->sweep, SweepScratch::GATHERED, sizeof(f2) * count * N)) || (rc = grow(h, h->sweep, SweepScratch::LUT, sizeof(float4) * N)))
		return rc;
	HIP_TRY(hipMemcpyAsync(h->sweep.p[SweepScratch::RAW], static_cast<const char*>(raw) + lo * rowBytes, rowBytes * count,
	                       rawIsDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
	if ((rc = launchPrepare(h, h->sweep.p[SweepScratch::RAW], h->sweep.as<float>(SweepScratch::ROWS), count * (size_t)N,
	                        p.backgroundRemoval ? p.rollingAverageWindowSize : 0)))
		return rc;
	// the handle's k-linearisation and window with the phasor of "dispersion compensation off" (uploadLut's table, not the handle's copy)
	std::vector<float4> lut((size_t)N);
	for (int j = 0; j < N; ++j) lut[(size_t)j] = lutEntry(h, j, true);
	HIP_TRY(hipMemcpyAsync(h->sweep.p[SweepScratch::LUT], lut.data(), sizeof(float4) * N, hipMemcpyHostToDevice, h->stream));
	int rs = oct::RS_NONE;
	if (p.resampling) rs = p.resamplingInterpolation == OCTPIPE_INTERP_CUBIC ? oct::RS_CUBIC : p.resamplingInterpolation == OCTPIPE_INTERP_LANCZOS ? oct::RS_LANCZOS : oct::RS_LINEAR;
	std::vector<float> lz;
	const float* lanczosW = nullptr;
	if (rs == oct::RS_LANCZOS) {
		lanczosWeights(lut, lz);
		if ((rc = grow(h, h->sweep, SweepScratch::LANCZOS, sizeof(float) * lz.size()))) return rc;
		HIP_TRY(hipMemcpyAsync(h->sweep.p[SweepScratch::LANCZOS], lz.data(), sizeof(float) * lz.size(), hipMemcpyHostToDevice, h->stream));
		lanczosW = h->sweep.as<float>(SweepScratch::LANCZOS);
	}
	// (the gather's first-line offset of the Lanczos taps, cu:313, falls on staged row 0: buffer line 0 itself or the halo row in front)
	if ((rc = launchGatherRows(h, h->sweep.as<float>(SweepScratch::ROWS), h->sweep.as<f2>(SweepScratch::GATHERED), h->sweep.as<float4>(SweepScratch::LUT), count, rs,
	                           lanczosW)))
		return rc;
	HIP_TRY(hipStreamSynchronize(h->stream));  // lut / lz are stack vectors
	*rows = h->sweep.as<f2>(SweepScratch::GATHERED) + ((size_t)m->firstAscan - lo) * (size_t)N;
	return OCTPIPE_OK;
}

// the phasors of candidates [0, K) into scratch PHASOR (and THETA when wanted)
int launchPhasors(octpipe* h, float d0, float d1, const float* d2, const float* d3, unsigned K, bool withTheta) {
	const int N = h->N;
	std::vector<float4> coef(K);
	for (unsigned c = 0; c < K; ++c) {
		float k[4];
		octhost::scaled_cubic_coeffs(d0, d1, d2[c], d3[c], (unsigned)N, k);
		coef[c] = float4{k[0], k[1], k[2], k[3]};
	}
	int rc;
	if ((rc = grow(h, h->sweep, SweepScratch::COEF, sizeof(float4) * K)) || (rc = grow(h, h->sweep, SweepScratch::PHASOR, sizeof(f2) * K * (size_t)N))) return rc;
	if (withTheta && (rc = grow(h, h->sweep, SweepScratch::THETA, sizeof(float) * K * (size_t)N))) return rc;
	HIP_TRY(hipMemcpyAsync(h->sweep.p[SweepScratch::COEF], coef.data(), sizeof(float4) * K, hipMemcpyHostToDevice, h->stream));
	size_t blocks = ((size_t)K * N + 255) / 256;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(oct::oct_sweep_phasor_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, h->sweep.as<float4>(SweepScratch::COEF),
	                   h->sweep.as<f2>(SweepScratch::PHASOR), withTheta ? h->sweep.as<float>(SweepScratch::THETA) : nullptr, N, K);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(h->stream));  // coef is a stack vector
	return OCTPIPE_OK;
}

// step 3 over all K candidates, in chunks whose phasors and metric matrix fit the scratch budget.  scores: K floats (host);
// metrics: K x M floats (host) or NULL; sweepMs: summed device time of the sweep kernel launches or NULL
int scoreCandidates(octpipe* h, const f2* rows, const OctPipeDispersionMetric* m, const float* d2, const float* d3, unsigned K, float* scores, float* metrics,
                    double* sweepMs) {
	const int N = h->N;
	const unsigned M = m->ascanCount;
	int rc;
	const f2* tw = planTwiddles(h, &rc);
	if (rc) return rc;
	const size_t perCandidate = sizeof(f2) * (size_t)N + sizeof(float) * (size_t)M;
	size_t chunk = kSweepScratchBytes / perCandidate;
	if (chunk < 1) chunk = 1;
	if (chunk > K) chunk = K;
	if (chunk * (size_t)M > 0xffffffffull) chunk = 0xffffffffull / M;  // (the kernel's item index is 32 bits)
	if ((rc = grow(h, h->sweep, SweepScratch::METRIC, sizeof(float) * chunk * M)) || (rc = grow(h, h->sweep, SweepScratch::SCORES, sizeof(float) * chunk))) return rc;
	oct::SweepArgs a{};
	a.rows = rows;
	a.twiddle = tw;
	a.M = M;
	a.ignore = (int)m->ignoreFirstSamples;
	a.metricKind = m->metric;
	a.logScale = m->linear ? 0 : 1;
	a.threshold = m->threshold;
	grayscaleScaling(h->params, N, a.logScale != 0, &a.sA, &a.sB);  // (the handle's grey-value settings, the metric's scaling)
	StreamTimer timer(sweepMs != nullptr, "dispersion sweep");
	if (sweepMs) *sweepMs = 0.0;
	rc = OCTPIPE_OK;
	for (unsigned c0 = 0; c0 < K && !rc; c0 += (unsigned)chunk) {
		const unsigned k = (unsigned)std::min<size_t>(chunk, K - c0);
		if ((rc = launchPhasors(h, m->d0, m->d1, d2 + c0, d3 + c0, k, false))) break;
		a.phasor = h->sweep.as<f2>(SweepScratch::PHASOR);
		a.metric = h->sweep.as<float>(SweepScratch::METRIC);
		a.K = k;
		if ((rc = timer.begin(h->stream))) break;
		hipError_t e = oct::launch_dispersion_sweep(h->log2n, a, h->stream);
		if (e == hipSuccess && (rc = timer.end(h->stream))) break;
		if (e == hipSuccess) {
			hipLaunchKernelGGL(oct::oct_sweep_reduce_kernel, dim3((k + 255) / 256), dim3(256), 0, h->stream, a.metric, h->sweep.as<float>(SweepScratch::SCORES), k, M);
			e = hipGetLastError();
		}
		if (e == hipSuccess) e = hipMemcpyAsync(scores + c0, h->sweep.p[SweepScratch::SCORES], sizeof(float) * k, hipMemcpyDeviceToHost, h->stream);
		if (e == hipSuccess && metrics) e = hipMemcpyAsync(metrics + (size_t)c0 * M, a.metric, sizeof(float) * k * (size_t)M, hipMemcpyDeviceToHost, h->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
		double ms = 0.0;
		if (e == hipSuccess) e = timer.elapsedMs(&ms);
		if (sweepMs) *sweepMs += ms;
		if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? OCTPIPE_ERR_OUT_OF_MEMORY : OCTPIPE_ERR_DEVICE, std::string("dispersion sweep: ") + hipGetErrorString(e));
	}
	return rc;
}

int scoresEntry(octpipe* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m, const float* d2, const float* d3, unsigned K, float* scores,
                float* metrics, double* sweepMs) {
	int rc = enterCall(h, "dispersion scores", checkLength);
	if (rc) return rc;
	if (!raw || !m || !d2 || !d3 || !scores || K == 0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion scores: null argument or no candidates");
	if ((rc = checkMetric(h, m))) return rc;
	const f2* rows = nullptr;
	if ((rc = prepareRows(h, raw, rawIsDevice, m, &rows))) return rc;
	return scoreCandidates(h, rows, m, d2, d3, K, scores, metrics, sweepMs);
}

// candidate i of a range (the extension's sampling of [start, end])
float rangeCandidate(float start, float end, unsigned i, unsigned samples) {
	if (samples == 1) return start;
	return (float)(start + (end - start) * (double)i / (double)(samples - 1));
}
// the first maximum; a NaN never wins.  -1: every score is NaN
long firstMax(const std::vector<float>& s) {
	long best = -1;
	for (size_t i = 0; i < s.size(); ++i)
		if (!std::isnan(s[i]) && (best < 0 || s[i] > s[(size_t)best])) best = (long)i;
	return best;
}

}  // namespace

const f2* planTwiddles(octpipe* h, int* rc) {
	*rc = OCTPIPE_OK;
	if (h->d_twiddle) return h->d_twiddle;  // the handle's Plan<LOG2N> tables (every length but the forced library route)
	if (!h->sweep.p[SweepScratch::TWIDDLE]) {
		std::vector<f2> tw;
		if ((*rc = fusedTwiddles(h->log2n, tw))) return nullptr;
		if ((*rc = grow(h, h->sweep, SweepScratch::TWIDDLE, sizeof(f2) * tw.size()))) return nullptr;
		if ((*rc = uploadSync(h, h->sweep.p[SweepScratch::TWIDDLE], tw.data(), sizeof(f2) * tw.size()))) return nullptr;
	}
	return h->sweep.as<f2>(SweepScratch::TWIDDLE);
}

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_dispersion_scores(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m, const float* d2, const float* d3,
                              unsigned candidates, float* scores) {
	return scoresEntry(h, raw, rawIsDevice, m, d2, d3, candidates, scores, nullptr, nullptr);
}

int octpipe_estimate_dispersion(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m, float d2Start, float d2End, float d3Start,
                                float d3End, unsigned samples, float* d2Scores, float* d3Scores, float* bestD2, float* bestD3) {
	int rc = enterCall(h, "dispersion estimate", checkLength);
	if (rc) return rc;
	if (!raw || !m || !bestD2 || !bestD3 || samples == 0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion estimate: null argument or samples == 0");
	if (!std::isfinite(d2Start) || !std::isfinite(d2End) || !std::isfinite(d3Start) || !std::isfinite(d3End))
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion estimate: the ranges must be finite");
	if ((rc = checkMetric(h, m))) return rc;
	const f2* rows = nullptr;
	if ((rc = prepareRows(h, raw, rawIsDevice, m, &rows))) return rc;
	std::vector<float> d2(samples), d3(samples, 0.0f), s(samples);
	// step 1: d2 over its range with d3 = 0
	for (unsigned i = 0; i < samples; ++i) d2[i] = rangeCandidate(d2Start, d2End, i, samples);
	if ((rc = scoreCandidates(h, rows, m, d2.data(), d3.data(), samples, s.data(), nullptr, nullptr))) return rc;
	if (d2Scores) std::memcpy(d2Scores, s.data(), sizeof(float) * samples);
	const long b2 = firstMax(s);
	if (b2 < 0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion estimate: every score of the d2 range is NaN");
	const float best2 = d2[(size_t)b2];
	// step 2: d3 over its range with the best d2
	for (unsigned i = 0; i < samples; ++i) { d2[i] = best2; d3[i] = rangeCandidate(d3Start, d3End, i, samples); }
	if ((rc = scoreCandidates(h, rows, m, d2.data(), d3.data(), samples, s.data(), nullptr, nullptr))) return rc;
	if (d3Scores) std::memcpy(d3Scores, s.data(), sizeof(float) * samples);
	const long b3 = firstMax(s);
	if (b3 < 0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion estimate: every score of the d3 range is NaN");
	*bestD2 = best2;
	*bestD3 = d3[(size_t)b3];
	return OCTPIPE_OK;
}

int octpipe_debug_dispersion_metrics(octpipe_t* h, const void* raw, int rawIsDevice, const OctPipeDispersionMetric* m, const float* d2, const float* d3,
                                     unsigned candidates, float* metrics, float* scores, double* sweepKernelMs) {
	if (!metrics && !scores) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion metrics: no output");
	std::vector<float> own;
	if (!scores) { own.resize(candidates ? candidates : 1); scores = own.data(); }
	return scoresEntry(h, raw, rawIsDevice, m, d2, d3, candidates, scores, metrics, sweepKernelMs);
}

int octpipe_debug_dispersion_phasors(octpipe_t* h, float d0, float d1, const float* d2, const float* d3, unsigned candidates, float* theta,
                                     float* phasorsComplex) {
	int rc = enterCall(h, "dispersion phasors", checkLength);
	if (rc) return rc;
	if (!d2 || !d3 || !phasorsComplex || candidates == 0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "dispersion phasors: null argument or no candidates");
	if ((rc = launchPhasors(h, d0, d1, d2, d3, candidates, theta != nullptr))) return rc;
	const size_t n = (size_t)candidates * (size_t)h->N;
	if ((rc = downloadSync(h, phasorsComplex, h->sweep.p[SweepScratch::PHASOR], sizeof(f2) * n))) return rc;
	if (theta && (rc = downloadSync(h, theta, h->sweep.p[SweepScratch::THETA], sizeof(float) * n))) return rc;
	return OCTPIPE_OK;
}

}  // extern "C"
