// dispersion_sweep_inst.hip -- instantiates the dispersion sweep kernel for ONE transform length
// (compiled once per OCT_LOG2N so the lengths build in parallel).
#include "dispersion_sweep.h"
#include "launch.h"

#ifndef OCT_LOG2N
#error "compile with -DOCT_LOG2N=<8..12>"
#endif

namespace oct {

#define OCT_CAT2(a, b) a##b
#define OCT_CAT(a, b) OCT_CAT2(a, b)

hipError_t OCT_CAT(launch_dispersion_sweep_, OCT_LOG2N)(const SweepArgs& a, hipStream_t stream) {
	constexpr int kLog2N = OCT_LOG2N;
	auto kernel = oct_dispersion_sweep_kernel<kLog2N>;
	constexpr int waves = sweep_waves<kLog2N>();
	constexpr size_t lds = sweep_lds_bytes<kLog2N>();
	static_assert(lds <= 160 * 1024, "LDS budget of a CU");
	KernelLaunchInfo info;
	hipError_t e = kernel_launch_info(kernel, waves * 64, lds, &info);
	if (e != hipSuccess) return e;
	// persistent grid: every resident workgroup loops over (candidate, A-scan) items, the twiddle table is filled once per workgroup
	const unsigned total = a.K * a.M;
	const unsigned need = (total + waves - 1) / waves;
	unsigned blocks = (unsigned)(info.numCU * info.blocksPerCU);
	if (blocks > need) blocks = need;
	if (blocks == 0) return hipSuccess;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(waves * 64), lds, stream, a);
	return hipGetLastError();
}

}  // namespace oct
