// conv2d<> 128 -> 128 behind a layer that computed and stored only three of its four 32-channel groups (layer 0 of a net whose layer 1
// reads at most 96 channels: sicn_live.h, k_rgb.hip k_l0<4, 3>): the wide persistent conv of k_mfma16x.hip with the K walk over the
// groups 0, 1, 2 — a tile of 40 passes = 75 real K steps and 5 zero steps in place of 50 passes, and no request for the plane nobody
// wrote (conv_walk.hpp: the schedule, its compile-time check, and the argument for the zero steps).  The same accumulator columns as
// the four-group kernels: 3 and 5 with the register map of k_mfma16x_live.hip (fragments in AGPRs, every column in VGPRs), 8 with
// k_conv_x's (JV = 7: fragments in VGPRs) for a call that ends or is tapped at the layer.  The weight stream is the four-group one of
// the input-permuted handle, read through a descriptor of 80 steps (sicn_live.h: walk_groups).
#include "k_mfma16x_body.hpp"

namespace sicn {
namespace xw {

template <bool NT, int JV, int NJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_conv_g3(SICN_WIDE_KERNEL_ARGS)
{
    conv_x_body<NT, JV, NJ, 3>(SICN_WIDE_KERNEL_PASS);
}

}  // namespace xw

const void *wide_g3_kernel(bool nt, int columns)
{
    using namespace xw;
    switch (columns) {
    case 3: return nt ? (const void *)&k_conv_g3<true, 0, 3> : (const void *)&k_conv_g3<false, 0, 3>;
    case 5: return nt ? (const void *)&k_conv_g3<true, 0, 5> : (const void *)&k_conv_g3<false, 0, 5>;
    case 8: return nt ? (const void *)&k_conv_g3<true, JV_CONV, 8> : (const void *)&k_conv_g3<false, JV_CONV, 8>;
    }
    return nullptr;
}

}  // namespace sicn
