// Device-side helpers shared by the MFMA kernels (k_mfma16*.hip, k_rgb.hip, k_l0g.hip, k_gdn.hip).
#pragma once
#include "conv_walk.hpp"
#include "sicn_internal.h"
#include "sicn_plan.h"

namespace sicn {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

#define LDS_PTR(p) ((__attribute__((address_space(3))) void *)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void *)(p))

constexpr int PAD16 = 24;                     // zero tiles behind a 16x16x64 weight stream (pack_mfma16_stream): room for the prefetch
constexpr uint32_t OOB = 0x80000000u;         // beyond any image: the buffer range check returns 0

template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void block_barrier()
{
    // LDS-DMA results are ordered for readers by the issuing wave's vmcnt + this barrier; a
    // __syncthreads() here would add a full vmcnt(0) and drain the weight prefetch.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// relu7((v) mod 256) for four accumulators, packed little-endian into one dword — 5 VALU ops:
// the low byte of each accumulator is moved to the HIGH byte of a 16-bit lane (v_perm_b32), so the
// byte's sign is the lane's sign and v_pk_max_i16(x, 0) is the ReLU; a last v_perm_b32 gathers the
// four high bytes.
typedef short v2s __attribute__((ext_vector_type(2)));
// `floor2`: the two 16-bit lanes the bytes are max'ed against: 0 = the reference's ReLU; ACT_FLOOR_RAW (-32768 in
// both lanes) makes the max an identity, i.e. the lane BEFORE the ReLU (input of the GDN extension) — same instructions.
constexpr uint32_t ACT_FLOOR_RELU = 0u, ACT_FLOOR_RAW = 0x80008000u;
// the same kernel argument carries one more flag in a bit that is 0 in both floors: store the output non-temporal
constexpr uint32_t ACT_NT_STORE = 1u, ACT_FLOOR_MASK = 0x80008000u;
constexpr int NT_MIN_MB = 128;
// outputs that cannot stay in L2 / Infinity Cache anyway (>= 128 MiB per launch) bypass them
__host__ inline bool nt_store_wanted(size_t out_bytes) { return out_bytes >= ((size_t)NT_MIN_MB << 20); }
__device__ __forceinline__ uint32_t pack4_relu7(int a, int b, int c, int d, uint32_t floor2 = ACT_FLOOR_RELU)
{
    const uint32_t ab = __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x040c000cu);  // [0, a.b0, 0, b.b0]
    const uint32_t cd = __builtin_amdgcn_perm((uint32_t)d, (uint32_t)c, 0x040c000cu);
    const v2s z = __builtin_bit_cast(v2s, floor2);
    const v2s mab = __builtin_elementwise_max(__builtin_bit_cast(v2s, ab), z);
    const v2s mcd = __builtin_elementwise_max(__builtin_bit_cast(v2s, cd), z);
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, mcd), __builtin_bit_cast(uint32_t, mab), 0x07050301u);
}

// Tensor layouts.
//   LAYOUT_NHWC  : [H][W][C]                 the ABI layout = the reference's stream bytes
//   LAYOUT_GROUP : [C/32][H][W][32]          internal, between two layers of a chain: every 32-channel
//                  group is its own plane, so a kernel that walks K group by group touches each
//                  128-byte line once and a lane-per-pixel epilogue stores 1 KiB per wave instruction
//   LAYOUT_PHASE : [y&1][x&1][C/32][H/2][W/2][32]   GROUP split by pixel parity: what a deconv
//                  phase (py,px) produces is then CONTIGUOUS (its outputs are the pixels of one
//                  parity), instead of 32-byte pieces at a 64-byte stride
constexpr int LAYOUT_NHWC = 0, LAYOUT_GROUP = 1, LAYOUT_PHASE = 2;

// The layouts as strides (wave-uniform): byte offset of channel group g of pixel (y, x) in an image of W x H pixels, C channels
//   offset = ((y>>sh)*row + (x>>sh))*pix + g*grp + ((y&sh)*2 + (x&sh))*ph          (no branches)
struct TensorMap {
    uint32_t sh, row, pix, grp, ph;
};
__device__ __forceinline__ TensorMap tensor_map(int layout, int C, int W, int H)
{
    if (layout == LAYOUT_NHWC) return TensorMap{0u, (uint32_t)W, (uint32_t)C, 32u, 0u};
    if (layout == LAYOUT_GROUP) return TensorMap{0u, (uint32_t)W, 32u, (uint32_t)(W * H) * 32u, 0u};
    const uint32_t hw = (uint32_t)((W >> 1) * (H >> 1));
    return TensorMap{1u, (uint32_t)(W >> 1), 32u, hw * 32u, (uint32_t)(C >> 5) * hw * 32u};
}
__device__ __forceinline__ uint32_t tensor_offset(const TensorMap &t, int y, int x, uint32_t g)
{
    return (((uint32_t)y >> t.sh) * t.row + ((uint32_t)x >> t.sh)) * t.pix + g * t.grp +
           (((uint32_t)y & t.sh) * 2u + ((uint32_t)x & t.sh)) * t.ph;
}

// Tile geometry of the 16x16x64 kernels: TILE_Y x TX positions (TX = 32, or 16 for the layers whose
// accumulators / patch allow only one 8 x 32 workgroup per CU), sub-patch of (TILE_Y+2) x (TX+2)
// positions x 32 B, padded to SLOTS pieces per wave so that every wave issues the same number.
template <int TX>
struct Geo {
    static constexpr int PX = TX + 2;                              // patch row pitch in positions
    static constexpr int PIX = PATCH_Y * PX;                       // 340 / 180 positions
    static constexpr int SLOTS = (PIX * KSTEP + 4095) / 4096;      // LDS-DMA pieces per wave per sub-patch: 3 / 2
    static constexpr int ALLOC = SLOTS * 4 * 1024;                 // 12288 / 8192
    static constexpr int XT = TX / 16;                             // 16-position column tiles per row
    static constexpr int NC = 2 * XT;                              // column tiles per wave (2 rows)
};

// Patch position and validity of this lane's 16 bytes of LDS-DMA piece `k` of a sub-patch: position p = k*32 + lane/2 of
// the window whose origin is (Yb, Xb) in "patch coordinates"; patch coordinate (ty,tx) maps to input pixel
// (s*(Yb+ty)+ay, s*(Xb+tx)+ax).  Unswizzled image, channel group 0; group g is `+ g * tm.grp`.
struct PieceSrc {
    uint32_t off;   // byte offset of channel group 0 (meaningless if !ok)
    bool ok;
};
template <int TX>
__device__ __forceinline__ PieceSrc piece_src(const TensorMap &tm, int k, int lane, int Yb, int Xb, int s, int ay, int ax,
                                              int IW, int IH)
{
    const int p = k * 32 + (lane >> 1);
    const int ty = p / Geo<TX>::PX, tx = p - ty * Geo<TX>::PX;
    const int iy = s * (Yb + ty) + ay, ix = s * (Xb + tx) + ax;
    PieceSrc r;
    r.ok = p < Geo<TX>::PIX && iy >= 0 && iy < IH && ix >= 0 && ix < IW;
    r.off = tensor_offset(tm, iy, ix, 0u) + (uint32_t)(lane & 1) * 16u;
    return r;
}

// one LDS-DMA piece (1 KiB) of sub-patch `sub` (sub-patches are ALLOC bytes apart)
template <int ALLOC>
__device__ __forceinline__ void load_piece(uint8_t *patch, const uint8_t *in_img, int in_img_bytes, int sub,
                                           int k, uint32_t off)
{
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)in_img, 0, in_img_bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(patch + sub * ALLOC + k * 1024), 16, off, 0, 0, 0);
}

// XCD-aware work mapping.  Workgroups of a 1-D grid are dealt to the 8 XCDs round-robin (linear id % 8)
// and each XCD has its own L2, so neighbouring tiles / strips (which share halo pixels and the 128-byte
// lines at their common edge) should run on the SAME XCD at about the same time: XCD x works through
// the contiguous range [x * per, (x+1) * per) of the logical work list.  Returns the logical index of
// this workgroup, or -1 if it has none (the grid is padded to a multiple of 8).
// n_xcd is a kernel argument: the launcher takes it from the device (sicn_plan.h, chip_geom()); host and device only have to agree.
__device__ __forceinline__ int xcd_logical_index(int n_items, int n_xcd)
{
    const int per = (n_items + n_xcd - 1) / n_xcd;
    const int l = (int)blockIdx.x, idx = (l % n_xcd) * per + l / n_xcd;
    return (l / n_xcd < per && idx < n_items) ? idx : -1;
}

// (the conv tap order, conv_tap: conv_walk.hpp)

}  // namespace sicn
