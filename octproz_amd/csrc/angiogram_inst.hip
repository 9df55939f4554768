// angiogram_inst.hip -- instantiates the angiography kernels (angiogram.h) for every repeat count 2 ... 8: the volume kernel per method,
// both forms of the en face kernel per method and projection function.
#include "angio_launch.h"

namespace oct {

namespace {

struct AngioKernels {
	template <int METHOD, unsigned M> static constexpr auto volume() { return oct_angio_volume_kernel<METHOD, M>; }
	template <int METHOD, int FN, unsigned M> static constexpr auto enface() { return oct_angio_enface_kernel<METHOD, FN, M>; }
	template <int METHOD, int FN, unsigned M> static constexpr auto team() { return oct_angio_enface_team_kernel<METHOD, FN, M>; }
};

}  // namespace

hipError_t launch_angio_volume(int method, const AngioVolumeArgs& a, hipStream_t s) { return launch_volume<AngioKernels>(method, a.n, a, s); }

hipError_t launch_angio_enface(int method, int function, bool team, const AngioEnfaceArgs& a, hipStream_t s) {
	return launch_enface<AngioKernels>(method, function, team, a, a, s);
}

}  // namespace oct
