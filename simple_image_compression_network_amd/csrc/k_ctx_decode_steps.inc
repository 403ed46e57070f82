// rANS-WC decoder, the text of one workgroup: group `grp` of CTX_WPB_DEC streams of set `set` (0 = anchors) of ONE image.
// Included into the body of k_ctx_decode (sicn_codec_ctx.inc) and of k_ragged_ctx_decode (k_ragged_ctx.hip), which define before it
//   const uint8_t *payload (the container's bytes behind its length table), *scale, *tst;  const uint32_t *tfc, *offsets;
//   uint8_t *lat;  uint32_t *meta                                                             this image's arrays (k_ctx_body.hpp)
//   CtxGeom g;  int set;  uint32_t grp
// (checked below).  It declares __shared__ arrays and RETURNS from the kernel, so nothing may follow the #include.
// Text and not a function: see k_ctx_encode_steps.inc.
    static_assert(ctx_names<decltype(payload), const uint8_t *> && ctx_names<decltype(scale), const uint8_t *> &&
                  ctx_names<decltype(tst), const uint8_t *> && ctx_names<decltype(tfc), const uint32_t *> &&
                  ctx_names<decltype(offsets), const uint32_t *> && ctx_names<decltype(lat), uint8_t *> && ctx_names<decltype(meta), uint32_t *> &&
                  ctx_names<decltype(g), CtxGeom> && ctx_names<decltype(set), int> && ctx_names<decltype(grp), uint32_t>,
                  "k_ctx_decode_steps.inc: the including kernel declares the names listed above");
    __shared__ uint32_t fc[NCLS * 128];
    __shared__ __attribute__((aligned(16))) uint8_t stb[NCLS * 4096];
    __shared__ __attribute__((aligned(16))) uint16_t words_all[CTX_WPB_DEC][RING_WORDS];   // one ring per wave, see ransw_decode_body
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, sidx = grp * CTX_WPB_DEC + wv, st = sidx + (set ? g.nst[0] : 0);
    {
        const uint4 *b = reinterpret_cast<const uint4 *>(tst);   // the workspace block is 16-byte aligned (ctx_carve)
        for (uint32_t i = threadIdx.x; i < NCLS * 128; i += 64 * CTX_WPB_DEC) fc[i] = tfc[i];
        for (uint32_t i = threadIdx.x; i < NCLS * 256; i += 64 * CTX_WPB_DEC) reinterpret_cast<uint4 *>(stb)[i] = b[i];
    }
    __syncthreads();
    if (sidx >= g.nst[set]) return;   // (no block barrier below this line)
    uint16_t *words = words_all[wv];
    const uint32_t begin = sidx * WSS, cnt = min(WSS, g.nsym[set] - begin), blocks = (cnt + 255) / 256;
    const uint32_t off = offsets[st], len = offsets[st + 1] - off, payload_bytes = meta[1];
    if (len < 256 || (len & 1) || (off & 1) || len > WCAP || (unsigned long long)off + len > payload_bytes) {
        if (lane == 0) atomicOr(&meta[3], 1u);
        return;
    }
    const uint32_t nwords = len / 2;
    const uint16_t *src = (const uint16_t *)(payload + off);
    uint32_t loaded = ring_fill(words, src, 0, min(nwords, RING_WORDS), lane);
    wave_lds_sync();
    uint32_t x = words[2 * lane] | ((uint32_t)words[2 * lane + 1] << 16), wpos = 128;
    const unsigned long long below = (1ull << lane) - 1;
    bool bad = false;
    // the classes of a block come from global memory (the scale map and, for the non-anchors, the four anchor neighbours the
    // previous launch decoded): requested ONE BLOCK AHEAD.  Round 3 fetched them at the top of the block they were needed in —
    // with ~6 streams per CU in flight (a set of a 4K latent has 190 streams) that latency, 64 times per stream, was half of
    // the kernel.
    auto locate = [&](uint32_t q, uint32_t &o, uint32_t &cls4) -> bool {
        const uint32_t j = q * 256 + lane * 4;
        o = cls4 = 0;
        if (j >= cnt) return false;      // cnt is a multiple of 4
        const uint32_t e = begin + j, px = e / g.C, ch = e - px * g.C;
        uint32_t y, xx;
        ctx_pixel(set, px, g.W, y, xx);
        o = (y * g.W + xx) * g.C + ch;
        cls4 = ctx_class4(set, lat, scale, g.W, g.H, g.C, y, xx, o);
        return true;
    };
    uint32_t o_next = 0, cls_next = 0;
    bool mine_next = blocks ? locate(0, o_next, cls_next) : false;
    for (uint32_t q = 0; q < blocks; q++) {
        if (loaded < nwords && loaded - min(wpos, loaded) < 4 * 64) {
            wave_lds_sync();
            loaded = ring_fill(words, src, loaded, min(nwords, wpos + RING_WORDS), lane);
            wave_lds_sync();
        }
        const bool mine = mine_next;
        const uint32_t cls4 = cls_next, o = o_next;
        mine_next = q + 1 < blocks ? locate(q + 1, o_next, cls_next) : false;
        uint32_t out4 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (mine) {
                const uint32_t base = ((cls4 >> (8 * k)) & 15u) * 128, v = x & 4095u;
                const uint32_t sy = stb[(base << 5) + v] & 127u;   // (a slot no symbol covers holds anything: caught by the range test)
                const uint32_t t = fc[base + sy], f = t & 0xFFFFu;
                bad |= f == 0 || v < (t >> 16) || v >= (t >> 16) + f;   // a class without a table, or a hole in it
                out4 |= sy << (8 * k);
                x = f * (x >> PROB_BITS) + v - (t >> 16);
            }
            const bool need = mine && x < RANSW_L;
            const unsigned long long mask = __ballot(need);
            if (need) {
                const uint32_t idx = wpos + (uint32_t)__popcll(mask & below);
                if (idx < loaded)
                    x = (x << 16) | words[idx & (RING_WORDS - 1)];
                else
                    bad = true;
            }
            wpos += (uint32_t)__popcll(mask);
        }
        if (mine) *reinterpret_cast<uint32_t *>(lat + o) = out4;
    }
    if (bad || x != RANSW_L || wpos != nwords) atomicOr(&meta[3], 1u);
