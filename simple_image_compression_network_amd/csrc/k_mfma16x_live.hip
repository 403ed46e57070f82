// conv2d<> / deconv522<> 128 -> 128 where the next layer reads fewer than 128 of the channels: the wide persistent kernels of
// k_mfma16x.hip with NJ < 8 accumulator columns.  The net's live-channel plan (sicn_live.h) permutes the layer's weight rows and bias
// so that the channels somebody reads fill columns 0 .. NJ - 1; columns NJ .. 7 do not exist here: no accumulators, no weight-fragment
// reads, no MFMAs, no packs.  Everything else is the same walk — the plane refresh schedule, the pair buffers, the weight ring (which
// still carries all 128 rows of a K step: NJ x 512 of its 4096 bytes are read) and the stores of a hand-over: 16 B per lane and channel
// half, the bytes at absent columns' positions being whatever the registers hold — except that a half without any column (channels
// 64 .. 127 with 3 columns) is not stored at all: those bytes of the tensor keep what the workspace held.  Either way the consumer's
// weights there are zero.
// Register map, both kernels: operand fragments in AGPRs (128), every column and its bias in VGPRs (JV = 0): NJ x 36 = 180 / 108
// registers, and the hand-over packs each of them in place — no v_accvgpr_read at all.
#include "k_mfma16x_body.hpp"

namespace sicn {
namespace xw {

template <bool NT, int NJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_conv_live(SICN_WIDE_KERNEL_ARGS)
{
    conv_x_body<NT, 0, NJ, 4>(SICN_WIDE_KERNEL_PASS);
}
template <bool NT, int NJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_deconv_live(SICN_WIDE_KERNEL_ARGS)
{
    deconv_x_body<NT, 0, NJ>(SICN_WIDE_KERNEL_PASS);
}

}  // namespace xw

const void *wide_live_kernel(int transposed, bool nt, int columns)
{
    using namespace xw;
    switch (columns) {
#define SICN_LIVE(NJ) \
    case NJ: \
        return transposed ? (nt ? (const void *)&k_deconv_live<true, NJ> : (const void *)&k_deconv_live<false, NJ>) \
                          : (nt ? (const void *)&k_conv_live<true, NJ> : (const void *)&k_conv_live<false, NJ>);
        SICN_LIVE(3)
        SICN_LIVE(5)
#undef SICN_LIVE
    }
    return nullptr;
}

}  // namespace sicn
