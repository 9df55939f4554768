// angio_launch.h -- how the angiography kernels (angiogram.h) and their registered counterparts (repeat_register.h) are launched: the
// run-time repeat count, method and projection function to template arguments, and the grids.  A kernel family is a struct of three
// templates (AngioKernels in angiogram_inst.hip, RegisterKernels in repeat_register_inst.hip): volume<METHOD, M>(), enface<METHOD, FN, M>()
// and team<METHOD, FN, M>() return the kernel.  `n` is the AngioArgs inside the kernel's argument `a`.
#pragma once
#include <type_traits>

#include "angiogram.h"

namespace oct {

// f(integral_constant<unsigned, M>) for the run-time repeat count
template <class F>
hipError_t with_repeats(unsigned M, F f) {
	switch (M) {
	case 2: f(std::integral_constant<unsigned, 2>()); break;
	case 3: f(std::integral_constant<unsigned, 3>()); break;
	case 4: f(std::integral_constant<unsigned, 4>()); break;
	case 5: f(std::integral_constant<unsigned, 5>()); break;
	case 6: f(std::integral_constant<unsigned, 6>()); break;
	case 7: f(std::integral_constant<unsigned, 7>()); break;
	case 8: f(std::integral_constant<unsigned, 8>()); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

template <class K, int METHOD, class ARGS>
hipError_t volume_method(const AngioArgs& n, const ARGS& a, dim3 grid, dim3 block, hipStream_t s) {
	return with_repeats(n.M, [&](auto m) { hipLaunchKernelGGL((K::template volume<METHOD, decltype(m)::value>()), grid, block, 0, s, a); });
}

template <class K, int METHOD, int FN, class ARGS>
hipError_t enface_method(bool team, const AngioArgs& n, const ARGS& a, dim3 grid, dim3 block, hipStream_t s) {
	return with_repeats(n.M, [&](auto m) {
		if (team) hipLaunchKernelGGL((K::template team<METHOD, FN, decltype(m)::value>()), grid, block, 0, s, a);
		else hipLaunchKernelGGL((K::template enface<METHOD, FN, decltype(m)::value>()), grid, block, 0, s, a);
	});
}

template <class K, class ARGS>
hipError_t launch_volume(int method, const AngioArgs& n, const ARGS& a, hipStream_t s) {
	const unsigned rowsPerGroup = ANGIO_ROWS * (SURF_THREADS / 64);
	const dim3 grid((n.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
	switch (method) {
	case 0: return volume_method<K, 0>(n, a, grid, block, s);
	case 1: return volume_method<K, 1>(n, a, grid, block, s);
	case 2: return volume_method<K, 2>(n, a, grid, block, s);
	default: return hipErrorInvalidValue;
	}
}

// team: four A-scans per wave (thickness <= ANGIO_TEAM_BINS), else one
template <class K, class ARGS>
hipError_t launch_enface(int method, int function, bool team, const AngioEnfaceArgs& e, const ARGS& a, hipStream_t s) {
	if (team && e.thickness > ANGIO_TEAM_BINS) return hipErrorInvalidValue;
	const unsigned rowsPerGroup = (SURF_THREADS / 64) * (team ? 64 / ANGIO_TEAM_LANES : 1);
	const dim3 grid((e.n.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
	switch (method * 2 + (function != 0)) {
	case 0: return enface_method<K, 0, 0>(team, e.n, a, grid, block, s);
	case 1: return enface_method<K, 0, 1>(team, e.n, a, grid, block, s);
	case 2: return enface_method<K, 1, 0>(team, e.n, a, grid, block, s);
	case 3: return enface_method<K, 1, 1>(team, e.n, a, grid, block, s);
	case 4: return enface_method<K, 2, 0>(team, e.n, a, grid, block, s);
	case 5: return enface_method<K, 2, 1>(team, e.n, a, grid, block, s);
	default: return hipErrorInvalidValue;
	}
}

}  // namespace oct
