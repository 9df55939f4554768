// pipe_phase.hip -- phase extraction / k-linearisation calibration (include/octpipe.h "phase extraction"; reference docs:
// docs/docs/plugin-phaseextraction.md).
//
//   octpipe_phase_accumulate       oct_phase_accumulate_kernel (phase_extract.h): exact int64 column sums of the selected A-scans of
//                                  one raw buffer; a host buffer is staged row range by row range, only the selected rows travel
//   octpipe_phase_mean             the sums over the A-scan count, on the host
//   octpipe_extract_resample_curve oct_phase_extract_kernel<LOG2N> (one wave) on the mean, then the cubic fit on the host in float64
// Everything runs on the handle's compute stream behind what is already enqueued there, and touches nothing the processing chain
// reads or writes.  The accumulator and the scratch belong to the handle (PhaseState, released in octpipe_destroy).
#include <algorithm>

#include "pipe_internal.h"
#include "phase_extract.h"
#include "phase_stage.h"

namespace octimpl {

namespace {

constexpr size_t kStageBytes = 64ull << 20;  // host rows staged per copy
constexpr uint64_t kMaxAscans = 1ull << 31;   // |sample| < 2^32, so 2^31 A-scans keep every column sum below 2^63

template <int F> hipError_t launchAccF(bool vec, dim3 grid, const oct::PhaseAccArgs& a, hipStream_t s) {
	if (vec) hipLaunchKernelGGL((oct::oct_phase_accumulate_kernel<F, true>), grid, dim3(oct::PHASE_THREADS), 0, s, a);
	else hipLaunchKernelGGL((oct::oct_phase_accumulate_kernel<F, false>), grid, dim3(oct::PHASE_THREADS), 0, s, a);
	return hipGetLastError();
}

// rows [firstRow, firstRow + rows) of the buffer at d_raw (device) into the accumulator
int launchAccumulate(octpipe* h, const void* d_raw, size_t firstRow, unsigned rows) {
	const int fmt = oct::ph_format(h->sampleFormat, h->acq.bitDepth);
	const bool packed = oct::format_packed(fmt);
	const unsigned N = (unsigned)h->N;
	const size_t rowBytes = rawBytes(h) / ((size_t)h->A * (size_t)h->B);
	const uintptr_t base = reinterpret_cast<uintptr_t>(d_raw);
	// the vector form: whole loads per row, every load aligned (16 bytes; packed: 12-byte loads of dword alignment, N % 8 == 0)
	const bool vec = packed ? (N % 8 == 0 && base % 4 == 0) : (rowBytes % 16 == 0 && base % 16 == 0);
	oct::PhaseAccArgs a{};
	a.raw = d_raw;
	a.acc = h->phaseState.as<unsigned long long>(PhaseState::ACC);
	a.firstRow = firstRow;
	a.rows = rows;
	a.N = N;
	a.chunks = vec ? N / oct::format_vector(fmt) : N;
	a.rowsPerPass = a.chunks <= (unsigned)oct::PHASE_THREADS ? (unsigned)oct::PHASE_THREADS / a.chunks : 1u;
	a.colBlocks = a.rowsPerPass > 1 ? 1u : (a.chunks + oct::PHASE_THREADS - 1) / oct::PHASE_THREADS;
	a.bitshift = h->params.bitshift ? 1 : 0;
	// enough workgroups to fill every CU (8 per CU), each with at least PHASE_UNROLL rows per lane
	int dev = 0, cus = 0;
	HIP_TRY(hipGetDevice(&dev));
	HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
	const size_t passes = ((size_t)rows + a.rowsPerPass - 1) / a.rowsPerPass;
	size_t groups = std::max<size_t>(1, (size_t)cus * 8 / a.colBlocks);
	groups = std::min(groups, std::max<size_t>(1, passes / oct::PHASE_UNROLL));
	a.rowGroups = (unsigned)groups;
	const dim3 grid((unsigned)(groups * a.colBlocks));
	// (a value that names none of the other seven runs as PH_I32)
	const hipError_t e = oct::with_format<oct::PH_COUNT>(fmt >= 0 && fmt < oct::PH_I32 ? fmt : oct::PH_I32, hipErrorInvalidValue,
	                                                     [&](auto F) { return launchAccF<F()>(vec, grid, a, h->stream); });
	HIP_TRY(e);
	return OCTPIPE_OK;
}

int ensureAccumulator(octpipe* h) {
	PhaseState& s = h->phaseState;
	if (s.p[PhaseState::ACC]) return OCTPIPE_OK;
	int rc = grow(h, s, PhaseState::ACC, sizeof(int64_t) * (size_t)h->N);
	if (rc) return rc;
	HIP_TRY(hipMemsetAsync(s.p[PhaseState::ACC], 0, sizeof(int64_t) * (size_t)h->N, h->stream));
	s.count = 0;
	return OCTPIPE_OK;
}

int accumulateEntry(octpipe* h, const void* raw, int rawIsDevice, uint32_t firstAscan, uint32_t ascanCount, double* kernelMs) {
	int rc = enterCall(h, "phase accumulate");
	if (rc) return rc;
	if (!raw) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase accumulate: raw is NULL");
	const uint64_t lines = (uint64_t)h->A * (uint64_t)h->B;
	if (ascanCount < 1 || (uint64_t)firstAscan + (uint64_t)ascanCount > lines)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase accumulate: need ascanCount >= 1 and firstAscan + ascanCount <= A*B = " + std::to_string(lines));
	if ((rc = ensureAccumulator(h))) return rc;
	PhaseState& s = h->phaseState;
	if (s.count + ascanCount >= kMaxAscans)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase accumulate: ascanCount would take the accumulated A-scan count to 2^31 (" + std::to_string(s.count) +
		                                              " accumulated); call octpipe_phase_reset");
	StreamTimer timer(kernelMs != nullptr, "phase accumulate");
	if ((rc = timer.begin(h->stream))) return rc;
	if (rawIsDevice) {
		if ((rc = launchAccumulate(h, raw, firstAscan, ascanCount))) return rc;
	} else {
		// only the selected rows cross the bus, in slices of the staging buffer (stream order keeps a slice's copy behind the
		// kernel that read the previous one).  Packed 12-bit rows of odd length start inside a byte triple on every odd row:
		// phase_stage.h cuts the slices at even rows and has the kernel skip a leading row
		const int fmt = oct::ph_format(h->sampleFormat, h->acq.bitDepth);
		const bool packed = oct::format_packed(fmt);
		const size_t N = (size_t)h->N, elem = oct::format_elem_bytes(fmt);
		const oct::PhaseStagePlan plan = oct::phase_stage_plan(packed, N, elem, firstAscan, ascanCount, kStageBytes);
		if ((rc = grow(h, s, PhaseState::STAGE, plan.stageBytes))) return rc;
		for (size_t i = 0; i < plan.slices; ++i) {
			const oct::PhaseStageSlice sl = oct::phase_stage_slice(plan, packed, N, elem, firstAscan, ascanCount, i);
			const hipError_t e = hipMemcpyAsync(s.p[PhaseState::STAGE], static_cast<const char*>(raw) + sl.srcByte, sl.bytes, hipMemcpyHostToDevice, h->stream);
			if (e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, std::string("phase accumulate: ") + hipGetErrorString(e));
			if ((rc = launchAccumulate(h, s.p[PhaseState::STAGE], sl.firstRow, (unsigned)sl.rows))) return rc;
		}
	}
	if ((rc = timer.end(h->stream))) return rc;
	hipError_t e = hipStreamSynchronize(h->stream);
	if (e == hipSuccess) e = timer.elapsedMs(kernelMs);
	if (e != hipSuccess) return fail(OCTPIPE_ERR_DEVICE, std::string("phase accumulate: ") + hipGetErrorString(e));
	s.count += ascanCount;
	return OCTPIPE_OK;
}

int hostMean(octpipe* h, std::vector<float>& mean, uint64_t* ascans) {
	PhaseState& s = h->phaseState;
	if (!s.p[PhaseState::ACC] || s.count == 0) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase mean: no A-scans accumulated");
	std::vector<int64_t> sums((size_t)h->N);
	int rc = downloadSync(h, sums.data(), s.p[PhaseState::ACC], sizeof(int64_t) * sums.size());
	if (rc) return rc;
	// uint32 samples under bitshift decode to v * 2^-32: their integer is v, the scale comes here
	const bool u32 = h->sampleFormat == OCTPIPE_FORMAT_AUTO && h->acq.bitDepth > 16;
	const double scale = (u32 && h->params.bitshift) ? 1.0 / 4294967296.0 : 1.0;
	mean.resize(sums.size());
	for (size_t n = 0; n < sums.size(); ++n) mean[n] = (float)(((double)sums[n] / (double)s.count) * scale);
	if (ascans) *ascans = s.count;
	return OCTPIPE_OK;
}

// least squares of curve[j], j in [a, b], on {1, t, t^2, t^3}, t = j / (N - 1).  Solved on {1, s, s^2, s^3} with
// s = (j - (a + b) / 2) / ((b - a) / 2) in [-1, 1], where the normal equations are well conditioned whatever the width of [a, b] --
// in powers of t their condition grows like ((N - 1) / (b - a))^6, and with a short [a, b] next to N - 1 no digit of c0..c3 was left --
// by Gaussian elimination with partial pivoting, then expanded into powers of t (s = alpha t + beta).  In long double (80 bits on
// x86-64; where it is float64 the result is float64's): the expansion multiplies the s-coefficients by up to alpha^3.
void fitCubic(const float* curve, int N, int a, int b, float* coeffs) {
	typedef long double real;
	const real mid = 0.5L * ((real)a + (real)b), half = 0.5L * (real)(b - a);
	real A[4][5] = {};
	for (int j = a; j <= b; ++j) {
		const real t = ((real)j - mid) / half;
		const real p[4] = {1.0L, t, t * t, t * t * t};
		for (int r = 0; r < 4; ++r) {
			for (int c = 0; c < 4; ++c) A[r][c] += p[r] * p[c];
			A[r][4] += p[r] * (real)curve[j];
		}
	}
	for (int c = 0; c < 4; ++c) {
		int piv = c;
		for (int r = c + 1; r < 4; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
		if (piv != c) for (int k = 0; k < 5; ++k) std::swap(A[c][k], A[piv][k]);
		for (int r = c + 1; r < 4; ++r) {
			const real f = A[r][c] / A[c][c];
			for (int k = c; k < 5; ++k) A[r][k] -= f * A[c][k];
		}
	}
	real x[4];
	for (int r = 3; r >= 0; --r) {
		real v = A[r][4];
		for (int k = r + 1; k < 4; ++k) v -= A[r][k] * x[k];
		x[r] = v / A[r][r];
	}
	// sum_k x[k] (alpha t + beta)^k in powers of t
	const real alpha = (real)(N - 1) / half, beta = -mid / half;
	const real binom[4][4] = {{1, 0, 0, 0}, {1, 1, 0, 0}, {1, 2, 1, 0}, {1, 3, 3, 1}};
	real ap[4] = {1, alpha, alpha * alpha, alpha * alpha * alpha}, bp[4] = {1, beta, beta * beta, beta * beta * beta};
	real out[4] = {};
	for (int k = 0; k < 4; ++k)
		for (int i = 0; i <= k; ++i) out[i] += x[k] * binom[k][i] * ap[i] * bp[k - i];
	for (int k = 0; k < 4; ++k) coeffs[k] = (float)out[k];
}

int extractEntry(octpipe* h, const float* meanIn, const OctPipePhaseExtraction* x, float* spectrum, float* envelope, float* phase, float* curve,
                 float* coeffs) {
	int rc = enterCall(h, "phase extraction");
	if (rc) return rc;
	const int N = h->N;
	if (N < 256 || N > 4096 || (N & (N - 1)) || h->bluestein)
		return fail(OCTPIPE_ERR_UNSUPPORTED, "phase extraction supports samplesPerLine = 256, 512, 1024, 2048 and 4096 (got " + std::to_string(N) + ")");
	if (!x) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase extraction: x is NULL");
	if (!curve) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase extraction: curve is NULL");
	if (x->peakStart < 2) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase extraction: peakStart must be >= 2");
	if (x->peakEnd < x->peakStart + 2 || x->peakEnd > (uint32_t)(N / 2 - 1))
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase extraction: peakEnd must lie in [peakStart + 2, N/2 - 1 = " + std::to_string(N / 2 - 1) + "]");
	if ((uint64_t)x->ignoreFirst + (uint64_t)x->ignoreLast + 9 > (uint64_t)N)
		return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase extraction: ignoreFirst / ignoreLast leave fewer than 9 samples (b - a >= 8 with a = ignoreFirst, b = N-1-ignoreLast)");
	std::vector<float> mean;
	if (meanIn) {
		mean.assign(meanIn, meanIn + N);
		for (int n = 0; n < N; ++n)
			if (!std::isfinite(mean[(size_t)n])) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase extraction: mean[" + std::to_string(n) + "] is not finite");
	} else if ((rc = hostMean(h, mean, nullptr))) {
		return rc;
	}
	const f2* tw = planTwiddles(h, &rc);
	if (rc) return rc;
	// one block of scratch: mean | spectrum | envelope | phase | curve | status
	const size_t fl = (size_t)N;
	if ((rc = grow(h, h->phaseState, PhaseState::EXTRACT, sizeof(float) * (fl * 4 + fl / 2) + 16))) return rc;
	float* d = h->phaseState.as<float>(PhaseState::EXTRACT);
	oct::PhaseExtractArgs g{};
	g.mean = d;
	g.spectrum = d + fl;
	g.envelope = d + fl + fl / 2;
	g.phase = d + 2 * fl + fl / 2;
	g.curve = d + 3 * fl + fl / 2;
	g.status = reinterpret_cast<int*>(d + 4 * fl + fl / 2);
	g.twiddle = tw;
	g.peakStart = (int)x->peakStart;
	g.peakEnd = (int)x->peakEnd;
	g.windowRaw = x->windowRaw ? 1 : 0;
	g.hannPeak = x->hannPeak ? 1 : 0;
	g.a = (int)x->ignoreFirst;
	g.b = N - 1 - (int)x->ignoreLast;
	HIP_TRY(hipMemcpyAsync(d, mean.data(), sizeof(float) * fl, hipMemcpyHostToDevice, h->stream));
	HIP_TRY(oct::launch_phase_extract(h->log2n, g, h->stream));
	std::vector<float> out(fl * 4 + 4);  // spectrum | envelope | phase | curve | status
	HIP_TRY(hipMemcpyAsync(out.data(), g.spectrum, sizeof(float) * (fl * 3 + fl / 2) + sizeof(int), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	const float* o = out.data();
	int status = 0;
	std::memcpy(&status, o + 3 * fl + fl / 2, sizeof(int));
	if (spectrum) std::memcpy(spectrum, o, sizeof(float) * (fl / 2));
	if (envelope) std::memcpy(envelope, o + fl / 2, sizeof(float) * fl);
	if (phase) std::memcpy(phase, o + fl + fl / 2, sizeof(float) * fl);
	if (status) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase extraction: no calibration signal in the selected band (the phase at b = N-1-ignoreLast is zero or not finite)");
	std::memcpy(curve, o + 2 * fl + fl / 2, sizeof(float) * fl);
	if (coeffs) fitCubic(curve, N, g.a, g.b, coeffs);
	return OCTPIPE_OK;
}

}  // namespace

}  // namespace octimpl

using namespace octimpl;

extern "C" {

int octpipe_phase_reset(octpipe_t* h) {
	int rc = enterCall(h, "phase reset");
	if (rc) return rc;
	if ((rc = ensureAccumulator(h))) return rc;
	HIP_TRY(hipMemsetAsync(h->phaseState.p[PhaseState::ACC], 0, sizeof(int64_t) * (size_t)h->N, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	h->phaseState.count = 0;
	return OCTPIPE_OK;
}

int octpipe_phase_accumulate(octpipe_t* h, const void* raw, int rawIsDevice, uint32_t firstAscan, uint32_t ascanCount) {
	return accumulateEntry(h, raw, rawIsDevice, firstAscan, ascanCount, nullptr);
}

int octpipe_phase_mean(octpipe_t* h, float* mean, uint64_t* ascans) {
	int rc = enterCall(h, "phase mean");
	if (rc) return rc;
	if (!mean) return fail(OCTPIPE_ERR_INVALID_ARGUMENT, "phase mean: mean is NULL");
	std::vector<float> m;
	if ((rc = hostMean(h, m, ascans))) return rc;
	std::memcpy(mean, m.data(), sizeof(float) * m.size());
	return OCTPIPE_OK;
}

int octpipe_extract_resample_curve(octpipe_t* h, const float* mean, const OctPipePhaseExtraction* x, float* spectrum, float* envelope, float* phase,
                                   float* curve, float* coeffs) {
	return extractEntry(h, mean, x, spectrum, envelope, phase, curve, coeffs);
}

int octpipe_debug_phase_accumulate(octpipe_t* h, const void* raw, int rawIsDevice, uint32_t firstAscan, uint32_t ascanCount, double* kernelMs) {
	return accumulateEntry(h, raw, rawIsDevice, firstAscan, ascanCount, kernelMs);
}

}  // extern "C"
