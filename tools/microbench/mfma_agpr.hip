// Microbenchmark (round 2): the one-wave-per-SIMD, 128 x 128-per-wave tile again — but with the accumulators PINNED in
// AGPRs (inline-asm MFMA with a tied "+a" operand: hipcc's own allocation shuffled them through 908 v_accvgpr moves per
// 128 MFMAs in mfma_bigtile.hip) and the next pass's fragment reads interleaved by hand, one ds_read_b128 per 4 MFMAs.
//   A: 2 workgroups x 4 waves per CU, 64 x 128 per wave, 12 reads / 32 MFMAs            (what k_mfma16 does today)
//   C: 2 workgroups x 2 waves per CU (1 wave per SIMD), 128 x 128 per wave, 16 reads / 64 MFMAs, double-buffered fragments
//   D: as C, with a workgroup barrier per pass (the kernels need one to publish the next weight tiles)
//   E: as D, with the register files' roles SWAPPED: the fragments are read by asm ds_read_b128 straight into AGPRs ("=a") and the
//      MFMAs take A and B from there ("a"); 6 of the 8 accumulator columns (j >= 2) are tied "+v" and live in VGPRs, where a VALU
//      pack could read them without v_accvgpr_read (what k_mfma16x.hip's hand-over wants)
//   F: as E, with only 4 of the 8 columns in VGPRs: the most accumulators the AGPRs can keep next to the fragments (128 + 128 of
//      256; "all accumulators in AGPRs, only the fragments moved" would need 384 and cannot be built).  D -> F -> E is the trend
//      from no AGPR operands / one D file to AGPR operands / mostly-VGPR D.
//   G: the control for E / F: D's register map (fragments in VGPRs, all accumulators in AGPRs) in E's code — asm reads and one
//      hand-written lgkmcnt(0) per pass, as the kernels have them, where C / D leave the reads and their waits to hipcc.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>
typedef int v4i __attribute__((ext_vector_type(4)));

#define MFMA(acc, A, B) asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(acc) : "v"(A), "v"(B))

__global__ __launch_bounds__(256, 2) void k_small(const int *__restrict__ src, int *__restrict__ out, int iters)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    for (int i = threadIdx.x; i < 16384; i += 256) ((int *)smem)[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v4i acc[4][8];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 8; j++) acc[i][j] = v4i{0, 0, 0, 0};
    for (int it = 0; it < iters; it++) {
        const unsigned char *base = smem + ((it * 8192 + w * 1024) & 0xFFFF);
        v4i pf[4], wf[8];
        for (int i = 0; i < 4; i++) pf[i] = *(const v4i *)(base + ((i * 1024 + lane * 16) & 0x3FFF));
        for (int j = 0; j < 8; j++) wf[j] = *(const v4i *)(smem + 32768 + ((it * 8192 + j * 1024 + lane * 16) & 0x7FFF));
        for (int j = 0; j < 8; j++) for (int i = 0; i < 4; i++)
            acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[j], pf[i], acc[i][j], 0, 0, 0);
    }
    int s = 0;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 8; j++) for (int r = 0; r < 4; r++) s += acc[i][j][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

// one pass: 64 MFMAs on (pc, wc) while the 16 fragments of the next pass are read into (pn, wn), one read per 4 MFMAs
template <bool BAR>
__device__ __forceinline__ void pass(v4i (&acc)[8][8], const v4i (&pc)[8], const v4i (&wc)[8], v4i (&pn)[8], v4i (&wn)[8],
                                     const unsigned char *smem, int it, int w, int lane)
{
    const unsigned char *pb = smem + ((it * 8192 + w * 1024) & 0xFFFF) + lane * 16;
    const unsigned char *wb = smem + 32768 + ((it * 8192) & 0x3FFF) + lane * 16;
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            MFMA(acc[i][j], wc[j], pc[i]);
            if ((i & 3) == 3) {
                const int r = j * 2 + (i >> 2);            // 0..15: pixel fragments first, then weight fragments
                if (r < 8) pn[r] = *(const v4i *)(pb + r * 1024);
                else wn[r - 8] = *(const v4i *)(wb + (r - 8) * 1024);
            }
        }
    }
    if (BAR) __builtin_amdgcn_s_barrier();
}

template <bool BAR>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_agpr(const int *__restrict__ src, int *__restrict__ out, int iters)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    for (int i = threadIdx.x; i < 16384; i += 128) ((int *)smem)[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v4i acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) acc[i][j] = v4i{0, 0, 0, 0};
    v4i pa[8], wa[8], pb[8], wb[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        pa[i] = *(const v4i *)(smem + w * 1024 + lane * 16 + i * 1024);
        wa[i] = *(const v4i *)(smem + 32768 + lane * 16 + i * 1024);
    }
    for (int it = 0; it < iters; it += 2) {
        pass<BAR>(acc, pa, wa, pb, wb, smem, it + 1, w, lane);
        pass<BAR>(acc, pb, wb, pa, wa, smem, it + 2, w, lane);
    }
    asm volatile("s_nop 15\n s_nop 15" ::: "memory");
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) s += acc[i][j][r];
    out[blockIdx.x * 128 + threadIdx.x] = s;
}

// ---- E / F ------------------------------------------------------------------------------------------------------------------
#define MFMA_AA(acc, A, B) asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(acc) : "a"(A), "a"(B))
#define MFMA_VA(acc, A, B) asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(acc) : "a"(A), "a"(B))
#define MFMA_AV(acc, A, B) asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(acc) : "v"(A), "v"(B))

template <int OFF, bool AG>   // AG: into AGPRs
__device__ __forceinline__ v4i lds_read_a(unsigned addr)
{
    v4i v;
    if constexpr (AG)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=a"(v) : "v"(addr), "n"(OFF));
    else
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}

// accumulator columns j >= JV live in VGPRs; AG: fragments in AGPRs (AG = false needs JV = 8: 128 + 256 registers)
template <int JV, bool AG>
__device__ __forceinline__ void pass_rf(v4i (&acc)[8][8], const v4i (&pc)[8], const v4i (&wc)[8], v4i (&pn)[8], v4i (&wn)[8], unsigned lds0,
                                        int it, int w, int lane)
{
    const unsigned pb = lds0 + ((it * 8192 + w * 1024) & 0xFFFF) + lane * 16;
    const unsigned wb = lds0 + 32768 + ((it * 8192) & 0x3FFF) + lane * 16;
    auto rd = [&](auto r_tag) {
        constexpr int R = decltype(r_tag)::value;
        if constexpr (R < 8)
            pn[R] = lds_read_a<R * 1024, AG>(pb);
        else
            wn[R - 8] = lds_read_a<(R - 8) * 1024, AG>(wb);
    };
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if constexpr (!AG)
                MFMA_AV(acc[i][j], wc[j], pc[i]);
            else if (j < JV)
                MFMA_AA(acc[i][j], wc[j], pc[i]);
            else
                MFMA_VA(acc[i][j], wc[j], pc[i]);
            if ((i & 3) == 3) {
                switch (j * 2 + (i >> 2)) {
#define RD(R) case R: rd(std::integral_constant<int, R>{}); break;
                    RD(0) RD(1) RD(2) RD(3) RD(4) RD(5) RD(6) RD(7) RD(8) RD(9) RD(10) RD(11) RD(12) RD(13) RD(14) RD(15)
#undef RD
                }
            }
        }
    }
    // the reads are asm statements: the wait that covers them is written by hand (as in the kernels: lgkmcnt(0) + barrier per pass)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

template <int JV, bool AG>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_regfile(const int *__restrict__ src, int *__restrict__ out, int iters)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    for (int i = threadIdx.x; i < 16384; i += 128) ((int *)smem)[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) void *)smem);
    v4i acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            acc[i][j] = v4i{0, 0, 0, 0};
            if (j < JV)
                asm volatile("" : "+a"(acc[i][j]));
            else
                asm volatile("" : "+v"(acc[i][j]));
        }
    v4i pa[8], wa[8], pb[8], wb[8];
    {
        const unsigned p0 = lds0 + w * 1024 + lane * 16, w0 = lds0 + 32768 + lane * 16;
#define RD(R) pa[R] = lds_read_a<R * 1024, AG>(p0); wa[R] = lds_read_a<R * 1024, AG>(w0);
        RD(0) RD(1) RD(2) RD(3) RD(4) RD(5) RD(6) RD(7)
#undef RD
        asm volatile("s_waitcnt lgkmcnt(0)\n s_nop 3" ::: "memory");   // the reads; v_mov / v_accvgpr_write -> asm MFMA reading it as SrcC
    }
    for (int it = 0; it < iters; it += 2) {
        pass_rf<JV, AG>(acc, pa, wa, pb, wb, lds0, it + 1, w, lane);
        pass_rf<JV, AG>(acc, pb, wb, pa, wa, lds0, it + 2, w, lane);
    }
    asm volatile("s_nop 15\n s_nop 15" ::: "memory");
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) s += acc[i][j][r];
    out[blockIdx.x * 128 + threadIdx.x] = s;
}

int main()
{
    const int iters = 4000;
    std::vector<int> h(16384);
    srand(1);
    for (auto &v : h) v = rand() ^ (rand() << 16);
    int *src, *out;
    hipMalloc(&src, 65536);
    hipMalloc(&out, 4096 * 256 * 4);
    hipMemcpy(src, h.data(), 65536, hipMemcpyHostToDevice);
    hipFuncSetAttribute((const void *)k_small, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipFuncSetAttribute((const void *)k_agpr<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipFuncSetAttribute((const void *)k_agpr<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipFuncSetAttribute((const void *)k_regfile<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipFuncSetAttribute((const void *)k_regfile<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipFuncSetAttribute((const void *)k_regfile<8, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    const char *names[6] = {"A 2 waves/SIMD  64x128, 12 reads/32 MFMA", "C 1 wave/SIMD  128x128 AGPR, 16 reads/64 MFMA", "D = C + barrier per pass",
                            "E = D, fragments in AGPRs, 6 of 8 accumulator columns in VGPRs", "F = D, fragments in AGPRs, 4 of 8 accumulator columns in VGPRs",
                            "G = D's register map, asm reads + one lgkmcnt(0) per pass as in E / F"};
    for (int round = 0; round < 4; round++)
        for (int v = 0; v < 6; v++) {
            const int blocks = 2048;   // A: 2048 x 4 waves x 32 tiles; C/D: 2048 x 2 waves x 64 tiles: same total work
            hipEventRecord(a);
            if (v == 0) hipLaunchKernelGGL(k_small, dim3(blocks), dim3(256), 65536, 0, src, out, iters);
            else if (v == 1) hipLaunchKernelGGL(k_agpr<false>, dim3(blocks), dim3(128), 65536, 0, src, out, iters);
            else if (v == 2) hipLaunchKernelGGL(k_agpr<true>, dim3(blocks), dim3(128), 65536, 0, src, out, iters);
            else if (v == 3) hipLaunchKernelGGL((k_regfile<2, true>), dim3(blocks), dim3(128), 65536, 0, src, out, iters);
            else if (v == 4) hipLaunchKernelGGL((k_regfile<4, true>), dim3(blocks), dim3(128), 65536, 0, src, out, iters);
            else hipLaunchKernelGGL((k_regfile<8, false>), dim3(blocks), dim3(128), 65536, 0, src, out, iters);
            hipEventRecord(b);
            hipEventSynchronize(b);
            float ms;
            hipEventElapsedTime(&ms, a, b);
            const double ops = 2.0 * blocks * (v ? 2 : 4) * (double)iters * (v ? 64 : 32) * 16 * 16 * 64;
            printf("round %d %s: %.3f ms  %.1f TOP/s\n", round, names[v], ms, ops / ms / 1e9);
        }
    return 0;
}
