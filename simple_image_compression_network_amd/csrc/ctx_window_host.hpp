// The arithmetic of include/sicn_ragged_ctx_window.h on the host: which streams of the two checkerboard sets of a mode-4 container a
// window of latent rows needs, and the band of whole latent rows they fill.  Plain C++ without HIP, so that it also compiles into a
// stand-alone program (tests/cpp/ctx_window_plan_check.cpp runs it under the host sanitizers).  k_ragged_ctx.hip wraps it in the
// extern "C" entry points.  Under hipcc the plan of one image is __host__ __device__ (SICN_HD, k_ragged_common.hpp): the moving ROI
// decode (ctx_roi_move_host.hpp, k_ragged_ctx_roi_move.hip) evaluates it on the device from a position read there, by this one
// statement of the rule.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sicn.h"
#include "../../include/sicn_ragged_ctx_window.h"
#include "window_host.hpp"

namespace sicn_ctx_window {

constexpr uint64_t WSS = 16384;                      // the default length of a mode-4 stream (SICN_CODEC_WSTREAM_SYMBOLS)
constexpr uint64_t MAX_SYMBOLS = 0x7F000000ull;      // the coder's limit on one image (sicn_ragged_ctx_layout)

using sicn_window::a16;
constexpr uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
constexpr uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
constexpr uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// an admissible stream length (header dword 9): a power of two, 1024 .. 16384
constexpr bool length_ok(uint64_t S) { return S >= 1024 && S <= WSS && (S & (S - 1)) == 0; }

// The plan of one image: rows [r0, r0 + rh) of a [H][W][C] latent.  Every quantity is 64-bit: with W H C <= MAX_SYMBOLS no product
// below can wrap.  S: the image's stream length.
SICN_HD inline int plan_of_sl(uint32_t W, uint32_t H, uint32_t C, uint32_t S_, uint32_t r0_, uint32_t rh, uint64_t band_offset,
                              sicn_ragged_ctx_window_image *out)
{
    const uint64_t positions = (uint64_t)W * H, S = S_;
    if (positions == 0 || C == 0 || (C & 3) || !length_ok(S)) return SICN_EINVAL;
    if (positions > MAX_SYMBOLS || positions * C > MAX_SYMBOLS) return SICN_EINVAL;
    if (rh < 1 || r0_ >= H || rh > H - r0_) return SICN_EINVAL;
    if (!out) return SICN_EINVAL;
    const uint64_t r0 = r0_, r1 = r0 + rh, R = (uint64_t)W * C;
    const uint64_t a = (W + 1ull) / 2, b = W / 2ull;
    const uint64_t nsym[2] = {((H / 2ull) * W + ((H & 1) ? a : 0)) * C, ((H / 2ull) * W + ((H & 1) ? b : 0)) * C};
    // row pairs the streams [s0, s1) of a set touch
    auto pairs = [&](int set, uint64_t s0, uint64_t s1, uint64_t *p0, uint64_t *p1) {
        *p0 = s0 * S / R;
        *p1 = ceil_div(min64(nsym[set], s1 * S), R);
    };
    // non-anchor streams: the row pairs that hold the wanted rows
    uint64_t N0 = 0, N1 = 0, P0 = 0, P1 = 0;
    const uint64_t lo = (r0 >> 1) * R, hi = min64(nsym[1], ((r1 + 1) >> 1) * R);
    const bool others = hi > lo;
    uint64_t A0 = r0, A1 = r1;
    if (others) {
        N0 = lo / S;
        N1 = ceil_div(hi, S);
        pairs(1, N0, N1, &P0, &P1);
        // anchor rows: the wanted ones and every neighbour of every non-anchor the selected streams hold
        A0 = min64(r0, P0 ? 2 * P0 - 1 : 0);
        A1 = min64(H, max64(r1, 2 * P1 + 1));
    }
    const uint64_t M0 = (A0 >> 1) * R / S, M1 = ceil_div(min64(nsym[0], ((A1 + 1) >> 1) * R), S);
    uint64_t Q0, Q1;
    pairs(0, M0, M1, &Q0, &Q1);
    const uint64_t B0 = 2 * (others ? min64(P0, Q0) : Q0), B1 = min64(H, 2 * (others ? max64(P1, Q1) : Q1));
    out->band_offset = band_offset;
    out->band_bytes = (uint32_t)((B1 - B0) * R);
    out->band_row0 = (uint32_t)B0;
    out->band_rows = (uint32_t)(B1 - B0);
    out->first_stream[0] = (uint32_t)M0;
    out->end_stream[0] = (uint32_t)M1;
    out->first_stream[1] = (uint32_t)N0;
    out->end_stream[1] = (uint32_t)N1;
    out->symbols = (uint32_t)((min64(nsym[0], M1 * S) - M0 * S) + (others ? min64(nsym[1], N1 * S) - N0 * S : 0));
    return SICN_OK;
}

inline int plan_of(uint32_t W, uint32_t H, uint32_t C, uint32_t r0, uint32_t rh, uint64_t band_offset, sicn_ragged_ctx_window_image *out)
{
    return plan_of_sl(W, H, C, (uint32_t)WSS, r0, rh, band_offset, out);
}

// images_or_null: [n_images].  *band_total: bytes of the band tensor; streams_or_null[2]: the selected streams of all images, per set.
// stream_symbols_or_null: [n_images], NULL = 16384 for every image.
inline int window_layout_sl(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *stream_symbols_or_null,
                            const uint32_t *r0, const uint32_t *rh, int n_images, sicn_ragged_ctx_window_image *images_or_null,
                            uint64_t *band_total, uint64_t *streams_or_null)
{
    if (!lat_w || !lat_h || !r0 || !rh || n_images < 1) return SICN_EINVAL;
    uint64_t at = 0, sel[2] = {0, 0};
    for (int i = 0; i < n_images; i++) {
        sicn_ragged_ctx_window_image im;
        if (int rc = plan_of_sl(lat_w[i], lat_h[i], lat_c, stream_symbols_or_null ? stream_symbols_or_null[i] : (uint32_t)WSS, r0[i], rh[i], at, &im))
            return rc;
        if (images_or_null) images_or_null[i] = im;
        at += a16(im.band_bytes);
        for (int s = 0; s < 2; s++) sel[s] += im.end_stream[s] - im.first_stream[s];
    }
    if (band_total) *band_total = at;
    if (streams_or_null) { streams_or_null[0] = sel[0]; streams_or_null[1] = sel[1]; }
    return SICN_OK;
}
inline int window_layout(const uint32_t *lat_w, const uint32_t *lat_h, uint32_t lat_c, const uint32_t *r0, const uint32_t *rh, int n_images,
                         sicn_ragged_ctx_window_image *images_or_null, uint64_t *band_total, uint64_t *streams_or_null)
{
    return window_layout_sl(lat_w, lat_h, lat_c, nullptr, r0, rh, n_images, images_or_null, band_total, streams_or_null);
}

}  // namespace sicn_ctx_window
