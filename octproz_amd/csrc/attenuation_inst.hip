// attenuation_inst.hip -- instantiates the attenuation kernels (attenuation.h): the volume kernel per scale, with and without a gain table,
// writing mu32 or the float64 sums; the en face kernel per scale, gain and projection function.  The run-time scale, gain and function become
// template arguments here.
#include <type_traits>

#include "attenuation.h"

namespace oct {

namespace {

// f(integral_constant<int, SCALE>, bool_constant<GAIN>)
template <class F>
hipError_t with_scale_and_gain(int scale, bool gain, F f) {
	switch (scale * 2 + (gain ? 1 : 0)) {
	case 0: f(std::integral_constant<int, 0>(), std::false_type()); break;
	case 1: f(std::integral_constant<int, 0>(), std::true_type()); break;
	case 2: f(std::integral_constant<int, 1>(), std::false_type()); break;
	case 3: f(std::integral_constant<int, 1>(), std::true_type()); break;
	case 4: f(std::integral_constant<int, 2>(), std::false_type()); break;
	case 5: f(std::integral_constant<int, 2>(), std::true_type()); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

}  // namespace

hipError_t launch_atten_volume(int scale, bool sums, const AttenVolumeArgs& a, hipStream_t s) {
	const unsigned rowsPerGroup = ATT_ROWS * (SURF_THREADS / 64);
	const dim3 grid((a.n.g.rCount + rowsPerGroup - 1) / rowsPerGroup), block(SURF_THREADS);
	return with_scale_and_gain(scale, a.n.gain != nullptr, [&](auto sc, auto gn) {
		constexpr int SCALE = decltype(sc)::value;
		constexpr bool GAIN = decltype(gn)::value;
		if (sums) hipLaunchKernelGGL((oct_atten_volume_kernel<SCALE, GAIN, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((oct_atten_volume_kernel<SCALE, GAIN, false>), grid, block, 0, s, a);
	});
}

// a workgroup is four waves while their pieces of LDS (a.cap floats each) fit a quarter of the thickest slab's each, else one wave
hipError_t launch_atten_enface(int scale, int function, const AttenEnfaceArgs& a, hipStream_t s) {
	const size_t waveBytes = sizeof(float) * (size_t)a.cap;
	if (a.cap < 1 || waveBytes > ATT_LDS_WAVE_BYTES) return hipErrorInvalidValue;
	const unsigned waves = waveBytes * 4 <= ATT_LDS_WAVE_BYTES ? SURF_THREADS / 64 : 1;
	const dim3 grid((a.n.g.rCount + waves - 1) / waves), block(64 * waves);
	const size_t lds = waveBytes * waves;
	return with_scale_and_gain(scale, a.n.gain != nullptr, [&](auto sc, auto gn) {
		constexpr int SCALE = decltype(sc)::value;
		constexpr bool GAIN = decltype(gn)::value;
		if (function) hipLaunchKernelGGL((oct_atten_enface_kernel<SCALE, GAIN, 1>), grid, block, lds, s, a);
		else hipLaunchKernelGGL((oct_atten_enface_kernel<SCALE, GAIN, 0>), grid, block, lds, s, a);
	});
}

}  // namespace oct
