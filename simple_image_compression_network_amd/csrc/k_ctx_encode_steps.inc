// rANS-WC encoder, the text of one workgroup: group `grp` of CTX_WPB streams of ONE image, anchors and non-anchors numbered through.
// Included into the body of k_ctx_encode (sicn_codec_ctx.inc) and of k_ragged_ctx_encode (k_ragged_ctx.hip), which define before it
//   const uint8_t *lat, *scale;  const uint32_t *tfc, *trcp;  uint8_t *scratch;  uint32_t *lens   this image's arrays (k_ctx_body.hpp)
//   CtxGeom g;  uint32_t grp
// (checked below: a missing or mistyped name does not compile).  The text declares __shared__ arrays and RETURNS from the kernel (a
// wave without a stream), so nothing may follow the #include.
// Text and not a function, unlike the other stages: handed to a function, CtxGeom is loaded whole at the kernel's entry instead of
// field by field where it is used, and k_ctx_encode moved from 66 to 64 SGPRs, k_ctx_decode from 86 to 84 VGPRs.  Included, the
// uniform kernels' instructions are the ones they had when this text stood in them (profiles/ragged_ctx_resource_usage.txt).
    static_assert(ctx_names<decltype(lat), const uint8_t *> && ctx_names<decltype(scale), const uint8_t *> &&
                  ctx_names<decltype(tfc), const uint32_t *> && ctx_names<decltype(trcp), const uint32_t *> &&
                  ctx_names<decltype(scratch), uint8_t *> && ctx_names<decltype(lens), uint32_t *> && ctx_names<decltype(g), CtxGeom> &&
                  ctx_names<decltype(grp), uint32_t>, "k_ctx_encode_steps.inc: the including kernel declares the names listed above");
    __shared__ uint32_t fc[NCLS * 128], rcp[NCLS * 128];
    __shared__ __attribute__((aligned(16))) uint16_t words_all[CTX_WPB][RING_WORDS];   // one ring per wave, see ransw_encode_body
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, st = grp * CTX_WPB + wv;
    for (uint32_t i = threadIdx.x; i < NCLS * 128; i += 64 * CTX_WPB) { fc[i] = tfc[i]; rcp[i] = trcp[i]; }
    __syncthreads();
    if (st >= g.nst[0] + g.nst[1]) return;   // (no block barrier below this line)
    uint16_t *words = words_all[wv];
    const int set = st >= g.nst[0];
    const uint32_t q0 = set ? st - g.nst[0] : st;
    const uint32_t begin = q0 * WSS, cnt = min(WSS, g.nsym[set] - begin), blocks = (cnt + 255) / 256;
    uint16_t *dst = (uint16_t *)(scratch + (size_t)st * WCAP);
    uint32_t pos = WCAP / 2, top = WCAP / 2, x = RANSW_L;
    const unsigned long long below = (1ull << lane) - 1;
    auto load = [&](uint32_t q, uint32_t &sym4, uint32_t &cls4) {   // C % 4 == 0: a lane's 4 symbols are 4 channels of one pixel
        const uint32_t j = q * 256 + lane * 4;
        sym4 = cls4 = 0;
        if (j >= cnt) return;
        const uint32_t e = begin + j, px = e / g.C, ch = e - px * g.C;
        uint32_t y, xx;
        ctx_pixel(set, px, g.W, y, xx);
        const uint32_t off = (y * g.W + xx) * g.C + ch;
        sym4 = *reinterpret_cast<const uint32_t *>(lat + off);
        cls4 = ctx_class4(set, lat, scale, g.W, g.H, g.C, y, xx, off);
    };
    uint32_t nsym = 0, ncls = 0;
    if (blocks) load(blocks - 1, nsym, ncls);
    for (uint32_t q = blocks; q-- > 0;) {
        const uint32_t sym4 = nsym, cls4 = ncls;
        if (q) load(q - 1, nsym, ncls);
#pragma unroll
        for (int k = 3; k >= 0; k--) {
            const bool active0 = q * 256 + lane * 4 + k < cnt;
            const uint32_t idx = ((cls4 >> (8 * k)) & 15u) * 128 + ((sym4 >> (8 * k)) & 127u);
            const uint32_t t = fc[idx], c = t >> 16;
            uint32_t f = t & 0xFFFFu;
            const bool active = active0 && f != 0;      // f == 0 only for input the statistics stage rejected
            f = active ? f : 1u;
            const bool emit = active && (unsigned long long)x >= ((unsigned long long)f << 20);
            const unsigned long long mask = __ballot(emit);
            pos -= (uint32_t)__popcll(mask);
            if (emit) {
                words[(pos + (uint32_t)__popcll(mask & below)) & (RING_WORDS - 1)] = (uint16_t)x;
                x >>= 16;
            }
            if (active) {
                uint32_t r;
                const uint32_t qq = ransw_div(x, f, rcp[idx], r);
                x = (qq << PROB_BITS) + r + c;
            }
        }
        if (top - pos > RING_WORDS - 4 * 64 - 128) {
            wave_lds_sync();
            ring_flush(words, dst, pos, top, lane);
            wave_lds_sync();
            top = pos;
        }
    }
    pos -= 128;
    words[(pos + 2 * lane) & (RING_WORDS - 1)] = (uint16_t)x;
    words[(pos + 2 * lane + 1) & (RING_WORDS - 1)] = (uint16_t)(x >> 16);
    wave_lds_sync();
    ring_flush(words, dst, pos, top, lane);
    if (lane == 0) lens[st] = (WCAP / 2 - pos) * 2;
