// repeat_register_inst.hip -- instantiates the repeat registration kernels (repeat_register.h): the shift search from the source rows and
// from the chunk partials, and for every repeat count 2 ... 8 the registered volume kernel per method and both forms of the registered en
// face kernel per method and projection function (the launch templates: angio_launch.h).
#include "angio_launch.h"
#include "repeat_register.h"

namespace oct {

namespace {

struct RegisterKernels {
	template <int METHOD, unsigned M> static constexpr auto volume() { return oct_register_volume_kernel<METHOD, M>; }
	template <int METHOD, int FN, unsigned M> static constexpr auto enface() { return oct_register_enface_kernel<METHOD, FN, M>; }
	template <int METHOD, int FN, unsigned M> static constexpr auto team() { return oct_register_enface_team_kernel<METHOD, FN, M>; }
};

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

hipError_t launch_register_volume(int method, const RegVolumeArgs& a, hipStream_t s) { return launch_volume<RegisterKernels>(method, a.v.n, a, s); }

hipError_t launch_register_enface(int method, int function, bool team, const RegEnfaceArgs& a, hipStream_t s) {
	return launch_enface<RegisterKernels>(method, function, team, a.e, a, s);
}

}  // namespace oct
