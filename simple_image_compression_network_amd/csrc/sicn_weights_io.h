// Weight ingestion shared by the layer chains (sicn_abi.hip) and ConvLayer_Batch (sicn_convlayer.hip).  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sicn {

// FixedPointWeights (weights.hpp:110-150): w_okc[o = nf*PE + pe][k = sf*SIMD + s] = sign-extended element s (w_bit bits) of
// m_weights[pe][nf*SF + sf], words of word_bytes little-endian bytes, `tiles` words per PE; kk = K*K*IFM_CH values per output
// channel, k = (ky*K + kx)*IFM_CH + c (slidingwindow.h:1304-1325, cross-checked by conv3_nonsquare_tb.cpp:546-571).
inline void decode_finn_tiles(const void *m_weights, int word_bytes, int w_bit, int simd, int pe_n, int tiles, int kk, int cout, int8_t *w_okc)
{
    const uint8_t *raw = (const uint8_t *)m_weights;
    const int sf_n = kk / simd, nf_n = cout / pe_n;
    for (int pe = 0; pe < pe_n; pe++)
        for (int nf = 0; nf < nf_n; nf++)
            for (int sf = 0; sf < sf_n; sf++) {
                const size_t idx = (size_t)pe * tiles + (size_t)nf * sf_n + sf;
                uint64_t word = 0;
                for (int b = 0; b < word_bytes; b++) word |= (uint64_t)raw[idx * word_bytes + b] << (8 * b);
                for (int s = 0; s < simd; s++) {
                    int v = (int)((word >> (w_bit * s)) & ((1u << w_bit) - 1));
                    if (v >> (w_bit - 1)) v -= 1 << w_bit;
                    w_okc[(size_t)(nf * pe_n + pe) * kk + sf * simd + s] = (int8_t)v;
                }
            }
}

// hipMalloc + copy of `bytes` host bytes; *dev stays nullptr when the allocation fails, and the owner frees it otherwise
template <class T>
bool upload(const void *host, size_t bytes, T **dev)
{
    if (hipMalloc((void **)dev, bytes) != hipSuccess) { *dev = nullptr; return false; }
    return hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

}  // namespace sicn
