// phase_extract_inst.hip -- instantiates the phase extraction kernel for ONE transform length
// (compiled once per OCT_LOG2N so the lengths build in parallel).
#include "phase_extract.h"
#include "launch.h"

#ifndef OCT_LOG2N
#error "compile with -DOCT_LOG2N=<8..12>"
#endif

namespace oct {

#define OCT_CAT2(a, b) a##b
#define OCT_CAT(a, b) OCT_CAT2(a, b)

hipError_t OCT_CAT(launch_phase_extract_, OCT_LOG2N)(const PhaseExtractArgs& g, hipStream_t stream) {
	constexpr int kLog2N = OCT_LOG2N;
	auto kernel = oct_phase_extract_kernel<kLog2N>;
	constexpr size_t lds = phase_extract_lds_bytes<kLog2N>();
	static_assert(lds <= 160 * 1024, "LDS budget of a CU");
	KernelLaunchInfo info;
	hipError_t e = kernel_launch_info(kernel, 64, lds, &info);  // (the opt-in above 64 KiB of dynamic LDS)
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(kernel, dim3(1), dim3(64), lds, stream, g);
	return hipGetLastError();
}

}  // namespace oct
