// conv2d<> / deconv522<> at ANY served channel width on v_mfma_i32_16x16x64_i8: the channel counts are run-time arguments.
// These kernels take the layers the specialised families do not (any_supported below; the reference net's own shapes never come
// here).  A served path, not a tuned one: plain HIP with the MFMA builtin, no software-pipelined patch, no persistent form.
//
//   conv   : out[y][x][o] = act((sum in[2y+ky-2][2x+kx-2][c] W[o][ky][kx][c] + b[o]) mod 256)
//   deconv : out[y][x][o] = act((sum Up[y+ky-2][x+kx-2][c] W[o][ky][kx][c] + b[o]) mod 256), Up[2i][2j] = in[i][j], zero elsewhere
// (the closed forms of k_generic.hip).  Only the low byte of the sum survives, so the uint8 input bytes go through the signed MFMA
// as they are: reading x >= 128 as x - 256 moves the sum by a multiple of 256.
//
// Decomposition.  The M grid is the output pixels (conv) or the INPUT pixels (deconv, 4-phase sub-pixel form: phase (qy, qx) =
// the outputs (2i + qy, 2j + qx), with the 9 / 6 / 6 / 4 taps whose parity matches; the inserted zeros are never touched).
// One workgroup of 4 waves = one 16 x 16 tile of M positions x one block of 64 output channels (blockIdx.y) of one image
// (blockIdx.z) and, for the deconv, one phase (the low two bits of blockIdx.x).  Wave wv owns tile rows 4 wv .. 4 wv + 3, one
// 16-position column tile per row: 4 x 4 MFMA tiles of 16 channels x 16 positions, 64 accumulator registers, whatever OFM_CH is.
//
// K walk: 64-channel chunks outside, the taps inside, so the LDS need does not depend on IFM_CH.  For each chunk the halo patch
// of the tile sits in LDS as 64 bytes per pixel: zeros for pixels outside the image and for channels >= IFM_CH (an odd multiple
// of 32 channels, or the 3 of an RGB input, leaves the rest of the last K step zero on both operands).
//   conv  : 35 x 35 input pixels in the four parity planes (row & 1, column & 1), so that the 16 positions of a column tile read
//           16 consecutive patch pixels for every tap (stride-2 positions would hit every other one): 1225 pixels = 78400 B
//   deconv: 18 x 18 input pixels, one plane: 20736 B
// The patch is single-buffered (stage, barrier, 25 / 9 / 6 / 4 taps, barrier); two conv workgroups fit a CU's 160 KiB and cover
// each other's staging.  Inside a chunk the operands of tap t + 1 are requested before the MFMAs of tap t.
//
// B operand (positions): lane (col = lane & 15, g = lane >> 4) reads bytes 16 g .. 16 g + 15 of patch pixel (row, col) + tap.
// A operand (weights): the image pack_any() builds at upload, [block][tap][chunk][tile j][row 16][64 B].  Row rho of tile j of
// block J holds channel 64 J + 16 (rho >> 2) + 4 j + (rho & 3): C/D row 4 g + r of tile j is then channel 64 J + 16 g + 4 j + r,
// i.e. a lane's 16 accumulators are 16 CONSECUTIVE channels of one pixel and the epilogue stores 16 bytes straight from registers.
// An RGB output (OFM_CH = 3) uses one tile with the rows in natural order (NT = 1) and byte stores of the 3 real channels.
#include "k_any_body.hpp"

namespace sicn {

// The tile body (patch staging, tap walk, epilogue) is any_tile() in k_any_body.hpp, shared with the ragged kernels (k_ragged.hip).
template <bool DECONV, int NT>
__global__ __launch_bounds__(256) void k_any(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int8_t *__restrict__ wimg,
                                             const int8_t *__restrict__ bias, int IW, int IH, int C, int OW, int OH, int O, int tiles_x,
                                             uint32_t floor2)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int item = (int)blockIdx.x, qy = 0, qx = 0;
    if (DECONV) {
        qy = (item >> 1) & 1;
        qx = item & 1;
        item >>= 2;
    }
    const int ty = item / tiles_x, tx = item - ty * tiles_x;
    const int img = blockIdx.z;
    any_tile<DECONV, NT>(in + (size_t)img * IH * IW * C, out + (size_t)img * OH * OW * O, wimg, bias, IW, IH, C, OW, OH, O, ty * ANY_T,
                         tx * ANY_T, qy, qx, (int)blockIdx.y, floor2, smem);
}

// ---- which shapes these kernels take.  Which layers come here is the order of the family list (sicn_abi.hip): the specialised
// ---- families stand before this one, so the reference shapes never do
//   tier A: IFM_CH % 32 == 0 and OFM_CH % 16 == 0, both <= 1024
//   tier B: the RGB ends — conv 3 -> N (N % 16 == 0), deconv N -> 3 (N % 32 == 0)
// Small and ragged shapes stay on k_generic, the independent second implementation.
bool any_supported(int cin, int cout, int transposed)
{
    if (cin > ANY_MAX_CH || cout > ANY_MAX_CH) return false;
    if (cin % 32 == 0 && cout % 16 == 0) return true;
    if (!transposed && cin == 3 && cout % 16 == 0) return true;
    if (transposed && cin % 32 == 0 && cout == 3) return true;
    return false;
}

static int any_tiles_per_block(int cout) { return cout == 3 ? 1 : 4; }

size_t any_bytes(int cin, int cout)
{
    return (size_t)((cout + 63) / 64) * 25 * ((cin + 63) / 64) * any_tiles_per_block(cout) * 1024;
}

// w_okc [cout][25 * cin] -> [block][tap ky * 5 + kx][chunk][tile][row 16][64 B], zero for channels past either count.
// Placed on a 256-byte boundary: the time of these loops on the host was seen to move by a third with the address the linker gave the
// function (profiles/ragged_owned_tables.txt, section 6), and a ragged net made per call runs them once per layer.
__attribute__((aligned(256))) void pack_any(const int8_t *w_okc, int cin, int cout, int8_t *dst)
{
    const int nblk = (cout + 63) / 64, nchunk = (cin + 63) / 64, nt = any_tiles_per_block(cout), kk = 25 * cin;
    for (int J = 0; J < nblk; J++)
        for (int t = 0; t < 25; t++)
            for (int n = 0; n < nchunk; n++)
                for (int j = 0; j < nt; j++)
                    for (int rho = 0; rho < 16; rho++) {
                        const int o = nt == 4 ? 64 * J + 16 * (rho >> 2) + 4 * j + (rho & 3) : rho;
                        int8_t *row = dst + (((((size_t)J * 25 + t) * nchunk + n) * nt + j) * 16 + rho) * 64;
                        for (int b = 0; b < 64; b++) {
                            const int c = n * 64 + b;
                            row[b] = (o < cout && c < cin) ? w_okc[(size_t)o * kk + t * cin + c] : 0;
                        }
                    }
}

template <bool DECONV, int NT>
static hipError_t launch_any_as(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, hipStream_t stream, const AnyPlan &p,
                                uint32_t floor2)
{
    const size_t lds = any_lds_bytes(DECONV);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)k_any<DECONV, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_any<DECONV, NT>), dim3(p.grid_x, p.grid_y, p.grid_z), dim3(256), lds, stream, in, out, w.d_w_any, w.d_bias, g.IW,
                       g.IH, g.CIN, g.OW, g.OH, g.COUT, p.tiles_x, floor2);
    return hipGetLastError();
}

hipError_t launch_any(const LayerGeom &g, const sicn_weights &w, const uint8_t *in, uint8_t *out, int n_images, hipStream_t stream,
                      bool relu)
{
    if ((size_t)g.IH * g.IW * g.CIN >= (size_t)OOB) return hipErrorInvalidValue;    // 31-bit offsets inside an image
    if ((size_t)g.OH * g.OW * g.COUT >= (size_t)OOB) return hipErrorInvalidValue;
    if (!any_supported(g.CIN, g.COUT, g.transposed) || !w.d_w_any) return hipErrorInvalidValue;
    const AnyPlan p = plan_any(g.transposed ? g.IW : g.OW, g.transposed ? g.IH : g.OH, g.COUT, g.transposed, n_images);
    if (!p.grid_x) return hipErrorInvalidValue;
    const uint32_t floor2 = relu ? ACT_FLOOR_RELU : ACT_FLOOR_RAW;
    if (g.transposed)
        return g.COUT == 3 ? launch_any_as<true, 1>(g, w, in, out, stream, p, floor2)
                           : launch_any_as<true, 4>(g, w, in, out, stream, p, floor2);
    return launch_any_as<false, 4>(g, w, in, out, stream, p, floor2);
}

}  // namespace sicn
