// repeat_register_inst.hip -- instantiates the repeat registration kernels (repeat_register.h): the shift search from the source rows and
// from the chunk partials, and for every repeat count 2 ... 8 the registered volume kernel per method and both forms of the registered en
// face kernel per method and projection function.
#include "repeat_register.h"

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
hipError_t volume_method(const RegVolumeArgs& a, dim3 grid, dim3 block, hipStream_t s) {
	return with_repeats(a.v.n.M, [&](auto m) { hipLaunchKernelGGL((oct_register_volume_kernel<METHOD, decltype(m)::value>), grid, block, 0, s, a); });
}

template <int METHOD, int FN>
hipError_t enface_method(bool team, const RegEnfaceArgs& a, dim3 grid, dim3 block, hipStream_t s) {
	return with_repeats(a.e.n.M, [&](auto m) {
		if (team) hipLaunchKernelGGL((oct_register_enface_team_kernel<METHOD, FN, decltype(m)::value>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((oct_register_enface_kernel<METHOD, FN, decltype(m)::value>), grid, block, 0, s, a);
	});
}

template <bool FROM_PARTIALS>
hipError_t search(const RegSearchArgs& a, hipStream_t s) {
	const size_t lds = reg_search_lds(a.M, a.k.cnt, a.R);
	auto kernel = oct_register_search_kernel<FROM_PARTIALS>;
	if (lds > (64u << 10)) {  // the opt-in to more than 64 KiB of dynamic LDS (per kernel and device)
		const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kernel, dim3(a.pCount * a.Qp), dim3(a.k.G >= REG_SEARCH_WIDE_G ? REG_SEARCH_THREADS : 64u), lds, s, a);
	return hipGetLastError();
}

}  // namespace

// the shifts of the positions [a.pFirst, a.pFirst + a.pCount): one workgroup per (position, group)
hipError_t launch_register_search(bool fromPartials, const RegSearchArgs& a, hipStream_t s) {
	if (a.M < ANGIO_MIN_REPEATS || a.M > ANGIO_MAX_REPEATS || a.R < 1 || a.R > REG_MAX_SHIFT || a.k.cnt < 2 * a.R + 1 || a.k.cnt > PEAK_MAX_SAMPLES)
		return hipErrorInvalidValue;
	return fromPartials ? search<true>(a, s) : search<false>(a, s);
}

hipError_t launch_register_volume(int method, const RegVolumeArgs& a, hipStream_t s) {
	const unsigned rowsPerGroup = ANGIO_ROWS * (SURF_THREADS / 64);
	const dim3 grid((a.v.n.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
	switch (method) {
	case 0: return volume_method<0>(a, grid, block, s);
	case 1: return volume_method<1>(a, grid, block, s);
	case 2: return volume_method<2>(a, grid, block, s);
	default: return hipErrorInvalidValue;
	}
}

// team: four A-scans per wave (a.e.thickness <= ANGIO_TEAM_BINS), else one
hipError_t launch_register_enface(int method, int function, bool team, const RegEnfaceArgs& a, hipStream_t s) {
	if (team && a.e.thickness > ANGIO_TEAM_BINS) return hipErrorInvalidValue;
	const unsigned rowsPerGroup = (SURF_THREADS / 64) * (team ? 64 / ANGIO_TEAM_LANES : 1);
	const dim3 grid((a.e.n.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
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
