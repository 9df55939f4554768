// boundary_trace_inst.hip -- instantiates the boundary tracing kernel (boundary_trace.h): one wave or one workgroup per B-scan, the
// choices in LDS or in the handle's scratch.
#include "boundary_trace.h"

namespace oct {

// form: 1 wave / LDS, 2 wave / scratch, 3 workgroup / LDS, 4 workgroup / scratch (include/octpipe_debug.h); `bscans` B-scans from a.bFirst
hipError_t launch_boundary_trace(unsigned form, const TraceArgs& a, unsigned bscans, hipStream_t s) {
	const dim3 grid(bscans), wave(64), group((a.H + 63) / 64 * 64);
	switch (form) {
	case 1: hipLaunchKernelGGL((oct_boundary_trace_kernel<true, true>), grid, wave, 0, s, a); break;
	case 2: hipLaunchKernelGGL((oct_boundary_trace_kernel<true, false>), grid, wave, 0, s, a); break;
	case 3: hipLaunchKernelGGL((oct_boundary_trace_kernel<false, true>), grid, group, 0, s, a); break;
	case 4: hipLaunchKernelGGL((oct_boundary_trace_kernel<false, false>), grid, group, 0, s, a); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

}  // namespace oct
