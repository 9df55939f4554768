// angiogram_inst.hip -- instantiates the angiography kernels (angiogram.h) for every repeat count 2 ... 8: the volume kernel per method,
// both forms of the en face kernel per method and projection function.
#include "angiogram.h"

namespace oct {

namespace {

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

template <int METHOD>
hipError_t volume_method(const AngioVolumeArgs& a, dim3 grid, dim3 block, hipStream_t s) {
	return with_repeats(a.n.M, [&](auto m) { hipLaunchKernelGGL((oct_angio_volume_kernel<METHOD, decltype(m)::value>), grid, block, 0, s, a); });
}

template <int METHOD, int FN>
hipError_t enface_method(bool team, const AngioEnfaceArgs& a, dim3 grid, dim3 block, hipStream_t s) {
	return with_repeats(a.n.M, [&](auto m) {
		if (team) hipLaunchKernelGGL((oct_angio_enface_team_kernel<METHOD, FN, decltype(m)::value>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((oct_angio_enface_kernel<METHOD, FN, decltype(m)::value>), grid, block, 0, s, a);
	});
}

}  // namespace

hipError_t launch_angio_volume(int method, const AngioVolumeArgs& a, hipStream_t s) {
	const unsigned rowsPerGroup = ANGIO_ROWS * (SURF_THREADS / 64);
	const dim3 grid((a.n.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
	switch (method) {
	case 0: return volume_method<0>(a, grid, block, s);
	case 1: return volume_method<1>(a, grid, block, s);
	case 2: return volume_method<2>(a, grid, block, s);
	default: return hipErrorInvalidValue;
	}
}

// team: four A-scans per wave (a.thickness <= ANGIO_TEAM_BINS), else one
hipError_t launch_angio_enface(int method, int function, bool team, const AngioEnfaceArgs& a, hipStream_t s) {
	if (team && a.thickness > ANGIO_TEAM_BINS) return hipErrorInvalidValue;
	const unsigned rowsPerGroup = (SURF_THREADS / 64) * (team ? 64 / ANGIO_TEAM_LANES : 1);
	const dim3 grid((a.n.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
	switch (method * 2 + (function != 0)) {
	case 0: return enface_method<0, 0>(team, a, grid, block, s);
	case 1: return enface_method<0, 1>(team, a, grid, block, s);
	case 2: return enface_method<1, 0>(team, a, grid, block, s);
	case 3: return enface_method<1, 1>(team, a, grid, block, s);
	case 4: return enface_method<2, 0>(team, a, grid, block, s);
	case 5: return enface_method<2, 1>(team, a, grid, block, s);
	default: return hipErrorInvalidValue;
	}
}

}  // namespace oct
