// libsicn.so — C ABI (include/sicn.h): descriptor validation, weight ingestion from the
// reference's FixedPointWeights tile format, kernel dispatch, layer chains with caller-provided
// workspace, per-layer hipEvent timing.  Host code only; kernels live in k_*.hip.
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "conv_walk.hpp"
#include "sicn_gdn_internal.h"
#include "sicn_internal.h"
#include "sicn_live.h"
#include "sicn_weights_io.h"

using namespace sicn;

// ---- options: no mutable process-wide state. The environment is read exactly once (thread-safe static
// ---- initialisation at first use, in practice at load) into an immutable default; everything else
// ---- travels by value in sicn_options.
namespace sicn {
static int env_int(const char *name)
{
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : 0;
}
// Every field of sicn_options that is checked, in struct order: its environment variable (library defaults; nullptr = none) and its
// admissible values.  default_options ignores an inadmissible variable, loudly; resolve_options refuses an inadmissible field.
template <int32_t... V> static bool one_of(int32_t v) { return ((v == V) || ...); }
template <int32_t LO, int32_t HI> static bool within(int32_t v) { return v >= LO && v <= HI; }
struct OptionField { int32_t sicn_options::*member; const char *env; bool (*admissible)(int32_t); };
static const OptionField OPTION_FIELDS[] = {
    {&sicn_options::force_generic, "SICN_FORCE_GENERIC", within<INT32_MIN, INT32_MAX>},
    {&sicn_options::mfma_shape, "SICN_MFMA_SHAPE", one_of<0, 16>},
    {&sicn_options::tile_x, "SICN_TILE_X", one_of<0, 16, 32>},
    {&sicn_options::strip_chunks, "SICN_STRIP_CHUNKS", within<0, INT32_MAX>},
    {&sicn_options::no_phase_layout, "SICN_NO_PHASE_LAYOUT", within<0, 2>},
    {&sicn_options::split_n, "SICN_SPLIT_N", within<0, 4>},
    {&sicn_options::wave_tile, "SICN_WAVE_TILE", one_of<0, 64, 128>},
    {&sicn_options::prefetch, "SICN_PREFETCH", within<0, 3>},
    {&sicn_options::persistent_grid, nullptr, within<0, INT32_MAX>},
    // the forms that took split_k > 1, l7_loader / l0_form / gdn_fuse = 2 and mfma_shape = 32 were removed (include/sicn.h)
    {&sicn_options::split_k, "SICN_SPLIT_K", within<0, 1>},
    {&sicn_options::l7_loader, "SICN_L7_LOADER", within<0, 1>},
    {&sicn_options::l0_form, "SICN_L0_FORM", within<0, 1>},
    {&sicn_options::gdn_fuse, "SICN_GDN_FUSE", within<0, 1>},
};
const sicn_options &default_options()
{
    static const sicn_options o = [] {
        sicn_options d;
        std::memset(&d, 0, sizeof d);
        d.struct_bytes = (int32_t)sizeof(sicn_options);
        for (const OptionField &f : OPTION_FIELDS) {
            if (!f.env) continue;
            int32_t &v = d.*f.member;
            v = env_int(f.env);
            if (f.admissible(v)) continue;
            fprintf(stderr, "libsicn: ignoring out-of-range %s=%d\n", f.env, (int)v);
            v = 0;
        }
        d.force_generic = d.force_generic != 0;
        return d;
    }();
    return o;
}
// Geometry of the current device, read once per device ordinal from hipDeviceProp_t (immutable afterwards).  The code objects in
// this library are gfx950 only: any other architecture is SICN_ENODEV here, with one line on stderr, instead of a failed code
// object load at the first launch (the reference's error path is exit(-1), bnn-library.h:55).  SICN_N_CU (read at load) overrides
// the CU count: what the launch planning of a 128-CU partition does on a whole chip (tests/test_partition_plans.py runs the suite's
// plan-dependent tests that way; sicn_debug_chip shows the count in force).
int chip_geom(ChipGeom *out)
{
    constexpr int MAX_DEV = 64;
    struct Entry { std::once_flag once; int rc = SICN_ENODEV; ChipGeom geom{1, 1}; };
    static Entry table[MAX_DEV];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return SICN_ENODEV;
    Entry &e = table[dev];
    std::call_once(e.once, [&] {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return;
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            fprintf(stderr, "libsicn: device %d is %s; this library holds gfx950 (MI355X) kernels only\n", dev, prop.gcnArchName);
            return;
        }
        static const int forced_cu = env_int("SICN_N_CU");
        e.geom = chip_from_cus(forced_cu > 0 ? forced_cu : prop.multiProcessorCount);
        e.rc = SICN_OK;
    });
    if (e.rc == SICN_OK && out) *out = e.geom;
    return e.rc;
}

const DebugEnv &debug_env()
{
    static const DebugEnv d{env_int("SICN_NO_DEAL")};
    return d;
}
}  // namespace sicn

// a caller's options -> a validated copy (NULL = defaults; a shorter struct from an older build is zero-extended)
static int resolve_options(const sicn_options *in, sicn_options *out)
{
    *out = default_options();
    if (!in) return SICN_OK;
    if (in->struct_bytes < 8 || in->struct_bytes > (int32_t)sizeof(sicn_options)) return SICN_EINVAL;
    sicn_options o;
    std::memset(&o, 0, sizeof o);
    std::memcpy(&o, in, (size_t)in->struct_bytes);
    o.struct_bytes = (int32_t)sizeof(sicn_options);
    for (const OptionField &f : OPTION_FIELDS)
        if (!f.admissible(o.*f.member)) return SICN_EINVAL;
    *out = o;
    return SICN_OK;
}

extern "C" void sicn_options_init(sicn_options *opt)
{
    if (opt) *opt = default_options();
}

// 0.2: sicn_options.split_k (a reserved slot), sicn_net_workspace_bytes grows by the K-split scratch, sicn_codec_info is 44 bytes
// (stream_symbols), SICN_ENODEV for a device that is not gfx950
// 0.3: GDN / IGDN specification version 2 (include/sicn_gdn.h): the activation's BYTES change, sicn_gdn_selftest_roots_narrow is gone
// 0.4: sicn_convlayer_kernel_for; ConvLayer_Batch serves every descriptor (sub-byte lanes, any channel count) on the MFMA kernel
// 0.5: conv2d<> / deconv522<> at other channel widths run on the channel-generic MFMA kernels ("mfma_conv_any" / "mfma_deconv_any",
// kinds 5 / 6) instead of k_generic: same bytes, another kernel for valid descriptors
// 0.6: ragged batches (include/sicn_ragged.h, k_ragged.hip): images of different sizes through one launch per layer
// 0.7: ragged latent coder (include/sicn_ragged_codec.h, k_ragged_codec.hip).  Still 0.7 (no symbol, struct or byte changed): the
// synchronous rANS-W calls are the asynchronous pair with one image, so sicn_codec_workspace_bytes(SICN_CODEC_RANSW, n) also holds
// that pair's status words (it grew by less than 1 KiB) and sicn_codec_decode needs sicn_codec_batch_workspace_bytes_sl(n, 1, length)
extern "C" int sicn_version(void) { return 1000 * 0 + 17; }
extern "C" int sicn_gdn_spec_version(void) { return 2; }

extern "C" int sicn_has_alt_kernels(void) { return 0; }   // kept for callers that probe it: the alternate kernel build is gone

extern "C" const char *sicn_strerror(int code)
{
    switch (code) {
    case SICN_OK: return "ok";
    case SICN_EINVAL: return "invalid descriptor or argument";
    case SICN_ENOMEM: return "out of memory";
    case SICN_ENODEV: return "no gfx950 device, or HIP runtime error";
    case SICN_ENOSPC: return "workspace too small";
    default: return "unknown error";
    }
}

// Shape preconditions of the reference, checked up front instead of CASSERT_DATAFLOW/exit(-1):
// slidingwindow.h:1259 (IFM_CH % SIMD), mvau.hpp:101-105 (folds), conv_nonsquare_top.cpp:94-95 and
// :246-259 (output dims), config_nonsquare.h (K=5, S=2, P=2, 8/8/4 bit).
static int validate_weights_fields(const sicn_layer_desc *d)
{
    if (!d) return SICN_EINVAL;
    if (d->IFM_CH <= 0 || d->OFM_CH <= 0 || d->SIMD <= 0 || d->PE <= 0) return SICN_EINVAL;
    if (d->SIMD > 16) return SICN_EINVAL;  // SIMD*4 bits must fit a 64-bit word
    if (d->IFM_CH % d->SIMD || d->OFM_CH % d->PE) return SICN_EINVAL;
    if ((long long)d->W_TILES != (long long)(d->OFM_CH / d->PE) * (25LL * d->IFM_CH / d->SIMD)) return SICN_EINVAL;
    if (d->transposed != 0 && d->transposed != 1) return SICN_EINVAL;
    return SICN_OK;
}

extern "C" int sicn_validate_desc(const sicn_layer_desc *d)
{
    int rc = validate_weights_fields(d);
    if (rc) return rc;
    if (d->K != 5 || d->S != 2 || d->P != 2) return SICN_EINVAL;
    if (d->IN_BIT != 8 || d->OUT_BIT != 8 || d->W_BIT != 4) return SICN_EINVAL;
    if (d->IFM_ROW <= 0 || d->IFM_COL <= 0) return SICN_EINVAL;
    if (d->IFM_ROW > (1 << 20) || d->IFM_COL > (1 << 20)) return SICN_EINVAL;
    if (d->transposed) {
        if (d->OFM_ROW != 2 * d->IFM_ROW || d->OFM_COL != 2 * d->IFM_COL) return SICN_EINVAL;
    } else if (d->OFM_ROW != (d->IFM_ROW + 1) / 2 || d->OFM_COL != (d->IFM_COL + 1) / 2)
        return SICN_EINVAL;
    return SICN_OK;
}

// ---- kernel families ------------------------------------------------------------------------------
// Everything the host layer knows about a kernel family is one row of FAMILIES.  The rows are in PRIORITY order: a layer runs on the
// first family that serves its shape, and the last row serves every shape.  A new family is a new row (and its launcher).
namespace {
enum : unsigned { GROUP = 1u << 1, PHASE = 1u << 2 };   // bit l = internal layout l of k_common.hpp (NHWC, layout 0, is everybody's)

struct LaunchArgs {
    const LayerGeom &g;
    const sicn_weights &w;
    const uint8_t *in;
    uint8_t *out;
    int n_images;
    hipStream_t stream;
    const sicn_options &o;
    const ChipGeom &chip;
    const sicn_gdn *gdn;       // the layer's activation, nullptr = the reference's ReLU
    unsigned long long *deal;
    const live::Step &step;    // the layouts, and what of its channels the layer computes and reads in this call (sicn_live.h)
};

struct Family {
    KernelKind kind;           // ABI: out[2] of sicn_debug_plan
    const char *name;          // ABI: sicn_kernel_for
    int transposed;            // the direction it serves; -1: both
    bool (*shape)(int cin, int cout, int transposed);
    unsigned reads, writes;    // the internal layouts its kernels take and produce
    bool rgb_sink;             // no_phase_layout = 2 keeps the PHASE layout away from its input
    bool pre_relu;             // can store the lane before the ReLU (a layer with a GDN on a family that cannot runs on the last row)
    // packs and uploads the weight images it reads besides d_w_okc and the bias (the shape is in w); may throw std::bad_alloc
    bool (*upload_images)(const int8_t *w_okc, sicn_weights &w);
    // *act_done = true: the kernel applied a.gdn itself
    hipError_t (*launch)(const LaunchArgs &a, bool *act_done);
    void (*plan)(const LayerGeom &g, int n_images, const sicn_options &o, const ChipGeom &chip, int32_t out[12]);   // out[3..11] of sicn_debug_plan
};

template <class Pack>
bool upload_image(size_t bytes, int8_t **dev, Pack pack)
{
    std::vector<int8_t> s(bytes);
    pack(s.data());
    return upload(s.data(), s.size(), dev);
}

// layer 0 (k_rgb.hip k_l0, k_l0g.hip)
bool l0_shape(int cin, int cout, int) { return cin == 3 && cout == 128; }
bool l0_images(const int8_t *k, sicn_weights &w)
{
    return upload_image(l0_bytes(w.cout), &w.d_w_l0, [&](int8_t *s) { pack_l0(k, w.cout, s); }) &&
           upload_image(l0g_bytes(), &w.d_w_l0g, [&](int8_t *s) { pack_l0g(k, s); });   // the kernel that applies a GDN before its store
}
hipError_t l0_launch(const LaunchArgs &a, bool *act_done)
{
    // layer 0 + activation in one kernel: the pre-activation tensor never reaches HBM
    if (a.gdn && a.o.gdn_fuse != 1 && a.w.d_w_l0g && a.gdn->d_gamma_mfma) {
        *act_done = true;
        return launch_l0_gdn(a.g, a.w, *a.gdn, a.in, a.out, a.n_images, a.stream, a.step.out_layout, a.o, a.chip);
    }
    return launch_l0(a.g, a.w, a.in, a.out, a.n_images, a.stream, a.step.out_layout, a.o, a.chip, a.gdn == nullptr, a.step.groups);
}
void l0_plan(const LayerGeom &g, int n_images, const sicn_options &o, const ChipGeom &chip, int32_t out[12])
{
    const L0Plan p = plan_l0(g.OW, g.OH, n_images, false, o.strip_chunks, chip);
    out[7] = p.tiles_x; out[8] = p.y_chunks; out[9] = n_images; out[10] = p.y_chunks; out[11] = p.ty_per;
}

// layer 7 (k_rgb.hip k_l7)
bool l7_shape(int cin, int cout, int) { return cin == 128 && cout == 3; }
bool l7_images(const int8_t *k, sicn_weights &w)
{
    return upload_image(l7_bytes(w.cin), &w.d_w_l7, [&](int8_t *s) { pack_l7(k, w.cin, s); }) &&
           upload_image(l7_half_bytes(), &w.d_w_l7_half, [&](int8_t *s) { pack_l7_half(k, s); });   // the form that reads one channel half
}
hipError_t l7_launch(const LaunchArgs &a, bool *)
{
    return launch_l7(a.g, a.w, a.in, a.out, a.n_images, a.stream, a.step.in_layout, a.o, a.chip, a.step.halves);
}
void l7_plan(const LayerGeom &g, int n_images, const sicn_options &o, const ChipGeom &chip, int32_t out[12])
{
    const L7Plan p = plan_l7(g.IW, g.IH, n_images, o.strip_chunks, chip);
    out[7] = (int)p.grid_x; out[8] = 1; out[9] = 1; out[10] = p.y_chunks;
}

// the 128 / 192-channel implicit-GEMM kernels (k_mfma16.hip: pipelined k_mfma16p.hip, wide persistent k_mfma16x.hip)
bool mfma_images(const int8_t *k, sicn_weights &w)
{
    bool ok = upload_image(mfma16_stream_bytes(w.cin, w.cout), &w.d_w_mfma16,
                           [&](int8_t *s) { pack_mfma16_stream(k, w.cin, w.cout, w.transposed, s); });
    if (ok && w.transposed && mfma16x_deconv_stream_bytes(w.cin, w.cout))   // the wide persistent deconv walks the taps in its own order
        ok = upload_image(mfma16x_deconv_stream_bytes(w.cin, w.cout), &w.d_w_mfma16x,
                          [&](int8_t *s) { pack_mfma16x_deconv_stream(k, w.cin, w.cout, s); });
    return ok;
}
hipError_t mfma_launch(const LaunchArgs &a, bool *)
{
    return launch_mfma16(a.g, a.w, a.in, a.out, a.n_images, a.stream, a.step.in_layout, a.step.out_layout, a.o, a.chip, a.gdn == nullptr,
                         a.deal, a.step.cols, a.step.walk_groups);
}
void mfma_plan(const LayerGeom &g, int n_images, const sicn_options &o, const ChipGeom &chip, int32_t out[12])
{
    const MfmaPlan p = plan_mfma(g, n_images, o, chip);
    out[3] = p.family; out[4] = p.tile_x; out[5] = p.split_n; out[6] = 1;   // out[6]: the K split, removed in 0.3.x
    out[7] = (int)p.grid_x; out[8] = (int)p.grid_y; out[9] = (int)p.grid_z;
    out[10] = p.deal;
}

// every other width the matrix cores can take (k_mfma16c.hip), NHWC in and out
bool any_images(const int8_t *k, sicn_weights &w)
{
    return upload_image(any_bytes(w.cin, w.cout), &w.d_w_any, [&](int8_t *s) { pack_any(k, w.cin, w.cout, s); });
}
hipError_t any_launch(const LaunchArgs &a, bool *) { return launch_any(a.g, a.w, a.in, a.out, a.n_images, a.stream, a.gdn == nullptr); }
void any_plan(const LayerGeom &g, int n_images, const sicn_options &, const ChipGeom &, int32_t out[12])
{
    const AnyPlan p = plan_any(g.transposed ? g.IW : g.OW, g.transposed ? g.IH : g.OH, g.COUT, g.transposed, n_images);
    out[4] = p.tile; out[7] = (int)p.grid_x; out[8] = (int)p.grid_y; out[9] = (int)p.grid_z;
}

// the shape-agnostic kernel (k_generic.hip): small and ragged shapes, force_generic, and the independent second implementation
bool every_shape(int, int, int) { return true; }
hipError_t generic_launch(const LaunchArgs &a, bool *) { return launch_generic(a.g, a.w, a.in, a.out, a.n_images, a.stream, a.gdn == nullptr); }

const Family FAMILIES[] = {
    // kind, name, direction, shape | reads, writes, rgb_sink, pre_relu | images, launch, plan
    {KK_L0_RGB, "l0_rgb", 0, l0_shape, 0, GROUP, false, true, l0_images, l0_launch, l0_plan},
    {KK_L7_RGB, "l7_rgb", 1, l7_shape, GROUP | PHASE, 0, true, false, l7_images, l7_launch, l7_plan},
    {KK_MFMA_CONV, "mfma_conv", 0, mfma_supported, GROUP, GROUP, false, true, mfma_images, mfma_launch, mfma_plan},
    // the deconv's outputs come one pixel parity at a time
    {KK_MFMA_DECONV, "mfma_deconv", 1, mfma_supported, GROUP | PHASE, GROUP | PHASE, false, true, mfma_images, mfma_launch, mfma_plan},
    {KK_MFMA_CONV_ANY, "mfma_conv_any", 0, any_supported, 0, 0, false, true, any_images, any_launch, any_plan},
    {KK_MFMA_DECONV_ANY, "mfma_deconv_any", 1, any_supported, 0, 0, false, true, any_images, any_launch, any_plan},
    {KK_GENERIC, "generic", -1, every_shape, 0, 0, false, true, nullptr, generic_launch, nullptr},
};
const Family &GENERIC = FAMILIES[sizeof FAMILIES / sizeof *FAMILIES - 1];

const Family &pick_family(const sicn_layer_desc &d, const sicn_options &o)
{
    if (o.force_generic) return GENERIC;
    for (const Family &f : FAMILIES)
        if ((f.transposed < 0 || f.transposed == d.transposed) && f.shape(d.IFM_CH, d.OFM_CH, d.transposed)) return f;
    return GENERIC;
}
// the family a layer of a chain runs on, given its activation
const Family &layer_family(const sicn_layer_desc &d, const sicn_options &o, bool has_gdn)
{
    const Family &f = pick_family(d, o);
    return (has_gdn && !f.pre_relu) ? GENERIC : f;
}
}  // namespace

extern "C" const char *sicn_kernel_for(const sicn_layer_desc *d)
{
    return sicn_validate_desc(d) ? "invalid" : pick_family(*d, default_options()).name;
}

// ---- weights ----------------------------------------------------------------------------------
extern "C" void sicn_weights_free(sicn_weights *w)
{
    if (!w) return;
    if (w->d_w_okc) (void)hipFree(w->d_w_okc);
    if (w->d_bias) (void)hipFree(w->d_bias);
    if (w->d_w_mfma16) (void)hipFree(w->d_w_mfma16);
    if (w->d_w_mfma16x) (void)hipFree(w->d_w_mfma16x);
    if (w->d_w_l0) (void)hipFree(w->d_w_l0);
    if (w->d_w_l0g) (void)hipFree(w->d_w_l0g);
    if (w->d_w_l7) (void)hipFree(w->d_w_l7);
    if (w->d_w_l7_half) (void)hipFree(w->d_w_l7_half);
    if (w->d_w_any) (void)hipFree(w->d_w_any);
    delete w;
}

// a handle from decoded weights ([cout][25 cin]) and cout bias bytes: what sicn_weights_from_finn_tiles makes of its tiles, and what a
// net makes of the permuted copies of its live-channel plan (sicn_live.h).  The handle keeps the host copies and never changes.
static int weights_from_okc(int cin, int cout, int transposed, std::vector<int8_t> w_okc, const int8_t *bias, sicn_weights **out)
{
    sicn_weights *w = new (std::nothrow) sicn_weights();
    if (!w) return SICN_ENOMEM;
    w->cin = cin;
    w->cout = cout;
    w->transposed = transposed;
    bool ok = upload(w_okc.data(), w_okc.size(), &w->d_w_okc);
    // d_w_okc and the bias always (force_generic, and a layer whose family cannot store the lane before the ReLU, run on them);
    // besides them the images of the family the shape runs on
    try {
        // bias, padded to a multiple of 16 bytes so kernels may read it with 16-byte loads
        std::vector<int8_t> b(((size_t)cout + 15) / 16 * 16 + 16, 0);
        for (int i = 0; i < cout; i++) b[i] = bias[i];
        ok = ok && upload(b.data(), b.size(), &w->d_bias);
        sicn_layer_desc d{};
        d.IFM_CH = cin;
        d.OFM_CH = cout;
        d.transposed = transposed;
        const Family &f = pick_family(d, sicn_options{});
        if (ok && f.upload_images) ok = f.upload_images(w_okc.data(), *w);
        w->h_bias.assign(bias, bias + cout);
        w->h_w_okc = std::move(w_okc);
    } catch (const std::bad_alloc &) { ok = false; }
    if (!ok) {
        sicn_weights_free(w);
        return SICN_ENOMEM;
    }
    *out = w;
    return SICN_OK;
}

extern "C" int sicn_weights_from_finn_tiles(const sicn_layer_desc *d, const void *m_weights, int word_bytes,
                                            const int8_t *bias, sicn_weights **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    int rc = validate_weights_fields(d);
    if (rc || !m_weights || !bias) return SICN_EINVAL;
    if (chip_geom(nullptr) != SICN_OK) return SICN_ENODEV;   // no device, or not a gfx950 one: refuse before anything is uploaded
    if (word_bytes != 1 && word_bytes != 2 && word_bytes != 4 && word_bytes != 8) return SICN_EINVAL;
    if (d->SIMD * 4 > word_bytes * 8) return SICN_EINVAL;
    const int cin = d->IFM_CH, cout = d->OFM_CH, kk = 25 * cin;
    std::vector<int8_t> w_okc;
    try {
        w_okc.resize((size_t)cout * kk);
    } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
    decode_finn_tiles(m_weights, word_bytes, 4, d->SIMD, d->PE, d->W_TILES, kk, cout, w_okc.data());
    return weights_from_okc(cin, cout, d->transposed, std::move(w_okc), bias, out);
}

// ---- single layers ------------------------------------------------------------------------------
// Layout of the tensor between layer `p` (producer) and layer `c` (consumer) of a chain: the best
// one both kernels implement (k_common.hpp).  0 = NHWC, 1 = GROUP, 2 = PHASE.
static int link_layout(const Family &fp, const Family &fc, const sicn_options &o)
{
    const unsigned common = fp.writes & fc.reads;
    // experiments: no_phase_layout 1 = never, 2 = not towards the RGB layer
    const bool phase_ok = o.no_phase_layout == 0 || (o.no_phase_layout == 2 && !fc.rgb_sink);
    if ((common & PHASE) && phase_ok) return 2;
    if (common & GROUP) return 1;
    return 0;
}

// gdn != nullptr: the layer stores its lanes BEFORE the sign-bit ReLU and the GDN / IGDN kernel then rewrites them in
// place, in whatever layout the layer wrote (include/sicn_gdn.h; extension beyond the reference).  deal: the layer's tile-deal
// words in the workspace of a chain (launch_mfma16), or nullptr.  step: what a net's call plan makes of the layer (sicn_live.h); a
// layer run alone takes the default, everything whole and NHWC.
static int run_layer(const sicn_layer_desc *d, const sicn_weights *w, const uint8_t *in, uint8_t *out, int n_images, hipStream_t stream,
                     int want_transposed, const sicn_options &o, const sicn_gdn *gdn, const live::Step &step, unsigned long long *deal)
{
    int rc = sicn_validate_desc(d);
    if (rc) return rc;
    if (!w || !in || !out || n_images < 0) return SICN_EINVAL;
    if (want_transposed >= 0 && d->transposed != want_transposed) return SICN_EINVAL;
    if (w->cin != d->IFM_CH || w->cout != d->OFM_CH || w->transposed != d->transposed) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    if (n_images > 65535) return SICN_EINVAL;
    if (gdn && gdn->channels != d->OFM_CH) return SICN_EINVAL;
    const LayerGeom g = geom_of(*d);
    ChipGeom chip;
    if ((rc = chip_geom(&chip)) != SICN_OK) return rc;   // no device, or not a gfx950 one
    bool act_done = false;
    const LaunchArgs args{g, *w, in, out, n_images, stream, o, chip, gdn, deal, step};
    hipError_t e = layer_family(*d, o, gdn != nullptr).launch(args, &act_done);
    if (act_done) gdn = nullptr;
    if (e == hipSuccess && gdn) e = launch_gdn(*gdn, out, step.out_layout, d->OFM_ROW, d->OFM_COL, n_images, stream);
    if (e == hipErrorInvalidValue) return SICN_EINVAL;
    return e == hipSuccess ? SICN_OK : SICN_ENODEV;
}

extern "C" int sicn_conv2d(const sicn_layer_desc *d, const sicn_weights *w, const uint8_t *in, uint8_t *out,
                           int n_images, void *hip_stream)
{
    return run_layer(d, w, in, out, n_images, (hipStream_t)hip_stream, 0, default_options(), nullptr, live::Step{}, nullptr);
}

extern "C" int sicn_conv2d_opt(const sicn_layer_desc *d, const sicn_weights *w, const uint8_t *in, uint8_t *out,
                               int n_images, const sicn_options *opt, void *hip_stream)
{
    sicn_options o;
    int rc = resolve_options(opt, &o);
    return rc ? rc : run_layer(d, w, in, out, n_images, (hipStream_t)hip_stream, 0, o, nullptr, live::Step{}, nullptr);
}

extern "C" int sicn_deconv522(const sicn_layer_desc *d, const sicn_weights *w, const uint8_t *in,
                              uint8_t *out, int n_images, void *hip_stream)
{
    return run_layer(d, w, in, out, n_images, (hipStream_t)hip_stream, 1, default_options(), nullptr, live::Step{}, nullptr);
}

extern "C" int sicn_deconv522_opt(const sicn_layer_desc *d, const sicn_weights *w, const uint8_t *in, uint8_t *out,
                                  int n_images, const sicn_options *opt, void *hip_stream)
{
    sicn_options o;
    int rc = resolve_options(opt, &o);
    return rc ? rc : run_layer(d, w, in, out, n_images, (hipStream_t)hip_stream, 1, o, nullptr, live::Step{}, nullptr);
}

// ---- layer chains ---------------------------------------------------------------------------------
constexpr int MAX_LAYERS = 64;   // of a net (sicn_net_create_gdn): a call's facts and steps are arrays on the stack

struct sicn_net {
    std::vector<sicn_layer_desc> descs;
    std::vector<const sicn_weights *> weights;
    std::vector<const sicn_gdn *> gdn;         // per layer, nullptr = the reference's ReLU
    sicn_options opt;                          // fixed at creation
    // the live-channel plan (sicn_live.h): per layer what the next layer reads of it, and the handles of the permuted copies of its
    // weights — derived[l][2 in + out], in / out = 1: the input channels arrive / the output channels leave in the order of the
    // producing layer's plan ([0] stays nullptr: weights[l] itself).  Made at creation, owned by the net, never changed.
    std::vector<live::Layer> live;
    std::vector<std::array<sicn_weights *, 4>> derived;
    // profiling: the only state a launch changes.  One flat ring of event pairs; a forward call reserves the
    // slots of its layers with one atomic fetch_add, so calls on several streams / threads never share a slot.
    static constexpr int EV_RING = 8192;
    mutable std::atomic<bool> profile{false};
    mutable std::atomic<int> ev_next{0};       // slots handed out since the last reset (may run past EV_RING)
    std::vector<hipEvent_t> ev_begin, ev_end;  // [EV_RING], created by sicn_net_profile
    mutable std::unique_ptr<std::atomic<int>[]> ev_layer;   // [EV_RING] layer recorded in the slot (release on write, acquire on read:
                                                            // sicn_net_layer_ms may run beside forward calls on other threads)
};

static size_t out_bytes(const sicn_layer_desc &d) { return (size_t)d.OFM_COL * d.OFM_ROW * d.OFM_CH; }
static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

extern "C" int sicn_net_create(const sicn_layer_desc *descs, sicn_weights *const *weights, int n_layers,
                               sicn_net **out)
{
    return sicn_net_create_opt(descs, weights, n_layers, nullptr, out);
}

extern "C" int sicn_net_create_opt(const sicn_layer_desc *descs, sicn_weights *const *weights, int n_layers,
                                   const sicn_options *opt, sicn_net **out)
{
    return sicn_net_create_gdn(descs, weights, nullptr, n_layers, opt, out);
}

// The live-channel tables of a new net and the permuted copies of the weights they call for.  Layer l may skip accumulator columns
// (live[l].nj < 8) when it is a 128 -> 128 layer without a GDN whose consumer has enough all-zero input channels, and a whole
// 32-channel group (live[l].ng < 4) when it is a 3 -> 128 layer without a GDN whose consumer reads at most 96 channels; whether it
// does is decided per call (sicn_net_forward).  May throw std::bad_alloc.
static int make_live_plan(sicn_net *net)
{
    const size_t n = net->descs.size();
    net->live.assign(n, live::Layer{});
    net->derived.assign(n, std::array<sicn_weights *, 4>{});
    for (size_t l = 0; l < n; l++) {
        live::Layer &L = net->live[l];
        const sicn_weights &w = *net->weights[l];
        L.cin = w.cin;
        L.cout = w.cout;
        L.gdn = net->gdn[l] != nullptr;
        if (!w.h_w_okc.empty()) L.in_mask = live::live_inputs(w.h_w_okc.data(), w.cin, w.cout);
    }
    live::make_tables(net->live, net->opt.force_generic != 0);
    for (size_t l = 0; l < n; l++) {
        const sicn_weights &w = *net->weights[l];
        for (int v = 1; v < 4; v++) {
            const bool in_p = (v & 2) != 0, out_p = (v & 1) != 0;
            // a layer has a p where it may skip columns (a wide layer) or a group (layer 0's family): sicn_live.h
            if ((in_p && !(l > 0 && !net->live[l - 1].p.empty())) || (out_p && net->live[l].p.empty())) continue;
            std::vector<int8_t> okc = w.h_w_okc, bias = w.h_bias;
            if (in_p) {
                std::vector<int8_t> t(okc.size());
                live::permute_inputs(okc.data(), w.cout, net->live[l - 1].p, t.data());
                okc.swap(t);
                // behind a producer that stores three groups the wide conv walks three (sicn_live.h: walk_groups) and takes the
                // steps 75 .. 79 of this copy's stream for zero tiles: no weight on an input position in the fourth group
                if (net->live[l - 1].ng < live::GROUPS && w.cin == live::CH &&
                    !conv_inputs_zero_from(okc.data(), w.cin, w.cout, net->live[l - 1].ng * live::GROUP_CH))
                    return SICN_EINVAL;
            }
            if (out_p) {
                std::vector<int8_t> t(okc.size());
                live::permute_outputs(okc.data(), w.h_bias.data(), w.cin, net->live[l].p, t.data(), bias.data());
                okc.swap(t);
            }
            if (int rc = weights_from_okc(w.cin, w.cout, w.transposed, std::move(okc), bias.data(), &net->derived[l][(size_t)v])) return rc;
        }
    }
    return SICN_OK;
}

extern "C" int sicn_net_create_gdn(const sicn_layer_desc *descs, sicn_weights *const *weights, const sicn_gdn *const *gdn,
                                   int n_layers, const sicn_options *opt, sicn_net **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (!descs || !weights || n_layers <= 0 || n_layers > MAX_LAYERS) return SICN_EINVAL;
    sicn_options o;
    if (int rc = resolve_options(opt, &o)) return rc;
    for (int i = 0; i < n_layers; i++) {
        int rc = sicn_validate_desc(&descs[i]);
        if (rc) return rc;
        const sicn_weights *w = weights[i];
        if (!w || w->cin != descs[i].IFM_CH || w->cout != descs[i].OFM_CH || w->transposed != descs[i].transposed)
            return SICN_EINVAL;
        if (i > 0 && (descs[i].IFM_CH != descs[i - 1].OFM_CH || descs[i].IFM_ROW != descs[i - 1].OFM_ROW ||
                      descs[i].IFM_COL != descs[i - 1].OFM_COL))
            return SICN_EINVAL;
        if (gdn && gdn[i] && gdn[i]->channels != descs[i].OFM_CH) return SICN_EINVAL;
    }
    sicn_net *net = new (std::nothrow) sicn_net();
    if (!net) return SICN_ENOMEM;
    try {
        net->descs.assign(descs, descs + n_layers);
        net->weights.assign(weights, weights + n_layers);
        net->gdn.assign((size_t)n_layers, nullptr);
        if (gdn) net->gdn.assign(gdn, gdn + n_layers);
        net->opt = o;
        if (int rc = make_live_plan(net)) {
            sicn_net_free(net);
            return rc;
        }
    } catch (const std::exception &) {
        sicn_net_free(net);
        return SICN_ENOMEM;
    }
    *out = net;
    return SICN_OK;
}

extern "C" void sicn_net_free(sicn_net *net)
{
    if (!net) return;
    for (auto &v : net->derived)
        for (sicn_weights *w : v) sicn_weights_free(w);
    for (hipEvent_t e : net->ev_begin) (void)hipEventDestroy(e);
    for (hipEvent_t e : net->ev_end) (void)hipEventDestroy(e);
    delete net;
}

// Two ping-pong buffers, each large enough for the largest intermediate activation.
static size_t pingpong_slot_bytes(const sicn_net *net, int n_images)
{
    size_t mx = 0;
    for (size_t i = 0; i + 1 < net->descs.size(); i++) mx = mx > out_bytes(net->descs[i]) ? mx : out_bytes(net->descs[i]);
    return align256(mx * (size_t)n_images);
}

// round 5: the wide persistent kernels' tile deal (k_mfma16x.hip: DealX) — DEAL_WORDS zeroed words per layer, behind the ping-pong buffers
static size_t deal_bytes(const sicn_net *net) { return align256(net->descs.size() * (size_t)DEAL_WORDS * sizeof(unsigned long long)); }

extern "C" size_t sicn_net_workspace_bytes(const sicn_net *net, int n_images)
{
    if (!net || n_images <= 0) return 0;
    return 2 * pingpong_slot_bytes(net, n_images) + deal_bytes(net);
}

// What the host layer knows of every layer of the net for a call of n_images on this chip (sicn_live.h).  chip == nullptr: nothing that
// depends on the chip is asked, no layer counts as wide or dealing.
static void call_facts(const sicn_net *net, int n_images, const ChipGeom *chip, live::CallFacts *out)
{
    const int n_layers = (int)net->descs.size();
    const Family *fam[MAX_LAYERS];
    for (int l = 0; l < n_layers; l++) fam[l] = &layer_family(net->descs[l], net->opt, net->gdn[l] != nullptr);
    for (int l = 0; l < n_layers; l++) {
        const LayerGeom g = geom_of(net->descs[l]);
        live::CallFacts &f = out[l] = live::CallFacts{};
        f.transposed = g.transposed != 0;
        f.l7 = fam[l]->kind == KK_L7_RGB;
        f.link_layout = l + 1 < n_layers ? link_layout(*fam[l], *fam[l + 1], net->opt) : 0;
        // no family with pre_relu == false is an MFMA family (FAMILIES): pick_family and layer_family agree on every layer asked here
        if (chip && (fam[l]->kind == KK_MFMA_CONV || fam[l]->kind == KK_MFMA_DECONV) && wide_supported(g)) {
            const MfmaPlan p = plan_mfma(g, n_images, net->opt, *chip);   // only the 128 -> 128 shape has a family 2 and a deal
            f.wide = p.family == 2;
            f.deals = p.deal != 0;
        }
    }
}

// What a call would do, for tests: the plan sicn_net_forward executes, made the way it makes it.  need_chip = false: what is asked for
// does not depend on the chip, and the call succeeds without one.
static int debug_call_plan(const sicn_net *net, int first, int last, int tap_layer, int n_images, bool args_ok, bool need_chip, live::Step *steps)
{
    if (!net || !args_ok || n_images <= 0) return SICN_EINVAL;
    const int n_layers = (int)net->descs.size();
    if (first < 0 || last >= n_layers || first > last) return SICN_EINVAL;
    ChipGeom chip;
    if (need_chip)
        if (int rc = chip_geom(&chip)) return rc;
    live::CallFacts facts[MAX_LAYERS];
    call_facts(net, n_images, need_chip ? &chip : nullptr, facts);
    live::plan_call(net->live, facts, n_layers, first, last, tap_layer, steps);
    return SICN_OK;
}

// per layer of the net the columns computed (8 outside [first, last]) and the output channels that the call's next layer reads
extern "C" int sicn_debug_net_columns(const sicn_net *net, int first, int last, int tap_layer, int n_images, int32_t *columns,
                                      int32_t *live_outputs)
{
    live::Step steps[MAX_LAYERS];
    if (int rc = debug_call_plan(net, first, last, tap_layer, n_images, columns && live_outputs, true, steps)) return rc;
    for (size_t l = 0; l < net->descs.size(); l++) {
        columns[l] = steps[l].cols;
        live_outputs[l] = steps[l].live_out;
    }
    return SICN_OK;
}

// per layer of the net the 64-channel halves of its input that it reads
extern "C" int sicn_debug_net_input_halves(const sicn_net *net, int first, int last, int tap_layer, int n_images, int32_t *halves)
{
    live::Step steps[MAX_LAYERS];
    if (int rc = debug_call_plan(net, first, last, tap_layer, n_images, halves != nullptr, true, steps)) return rc;
    for (size_t l = 0; l < net->descs.size(); l++) halves[l] = steps[l].halves;
    return SICN_OK;
}

// per layer of the net the 32-channel groups it computes and stores, and the groups the layer that wrote its input computed (4 outside
// [first, last] and for the first layer of the call)
extern "C" int sicn_debug_net_groups(const sicn_net *net, int first, int last, int tap_layer, int n_images, int32_t *groups_out,
                                     int32_t *groups_in)
{
    live::Step steps[MAX_LAYERS];
    if (int rc = debug_call_plan(net, first, last, tap_layer, n_images, groups_out && groups_in, false, steps)) return rc;
    for (size_t l = 0; l < net->descs.size(); l++) {
        groups_out[l] = steps[l].groups;
        groups_in[l] = steps[l].groups_in;
    }
    return SICN_OK;
}

// per layer of the net the 32-channel groups of its input that its K walk covers — 3 for a conv on the wide family behind a layer that
// stored three groups in this call (live::walk_groups), 4 for every other launch and outside [first, last]
extern "C" int sicn_debug_net_walk_groups(const sicn_net *net, int first, int last, int tap_layer, int n_images, int32_t *walk_groups)
{
    live::Step steps[MAX_LAYERS];
    if (int rc = debug_call_plan(net, first, last, tap_layer, n_images, walk_groups != nullptr, true, steps)) return rc;
    for (size_t l = 0; l < net->descs.size(); l++) walk_groups[l] = steps[l].walk_groups;
    return SICN_OK;
}

extern "C" int sicn_net_forward(const sicn_net *net, int first, int last, const uint8_t *in, uint8_t *out,
                                int tap_layer, uint8_t *tap_out, int n_images, void *workspace,
                                size_t workspace_bytes, void *hip_stream)
{
    if (!net || !in || !out || n_images < 0) return SICN_EINVAL;
    const int n_layers = (int)net->descs.size();
    if (first < 0 || last >= n_layers || first > last) return SICN_EINVAL;
    if (tap_layer >= 0 && (tap_layer < first || tap_layer > last || !tap_out)) return SICN_EINVAL;
    if (n_images == 0) return SICN_OK;
    const size_t slot = pingpong_slot_bytes(net, n_images);
    if (last > first && (!workspace || workspace_bytes < 2 * slot)) return SICN_ENOSPC;
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *pp[2] = {(uint8_t *)workspace, (uint8_t *)workspace + slot};
    unsigned long long *deal_base = nullptr;   // the tile-deal words of this call's layers, zeroed below (a smaller / absent workspace: static deal)
    ChipGeom chip;
    if (int rc = chip_geom(&chip)) return rc;
    // the plan of this call (sicn_live.h): per layer the layouts, the columns and groups it computes (a layer on the wide family only the
    // columns the next layer reads, layer 0's family only the groups), the copy of its weights, and what it reads of its input
    live::CallFacts facts[MAX_LAYERS];
    live::Step steps[MAX_LAYERS];
    call_facts(net, n_images, &chip, facts);
    live::plan_call(net->live, facts, n_layers, first, last, tap_layer, steps);
    {
        // does a layer of this call deal tiles dynamically?  (small inputs never do: no zeroing launch in front of them)
        bool any_deal = false;
        for (int l = first; l <= last; l++) any_deal |= facts[l].deals;
        if (any_deal && workspace && workspace_bytes >= 2 * slot + deal_bytes(net) && !debug_env().no_deal) {
            deal_base = (unsigned long long *)((uint8_t *)workspace + 2 * slot);
            // zeroed once per forward pass, by a kernel; every layer of the call gets its own DEAL_WORDS
            if (launch_zero_words(deal_base, deal_bytes(net) / sizeof(unsigned long long), stream) != hipSuccess) return SICN_ENODEV;
        }
    }
    const uint8_t *cur = in;
    // profiling: reserve this call's event slots (one per layer) in one atomic step
    int slot0 = -1;
    if (net->profile.load(std::memory_order_acquire)) {
        const int need = last - first + 1;
        const int at = net->ev_next.fetch_add(need, std::memory_order_relaxed);
        if (at + need <= sicn_net::EV_RING) slot0 = at;   // ring full: this call is not timed
    }
    for (int l = first; l <= last; l++) {
        const live::Step &step = steps[l];
        const sicn_weights *wl = step.variant ? net->derived[l][(size_t)step.variant] : net->weights[l];
        if (!wl) return SICN_EINVAL;
        // a tapped layer (the latent) is written straight into the caller's buffer and the next layer reads it there: no copy
        // (round 3 copied it device-to-device behind the layer: 4.8 us per forward pass on small inputs, 15 us on 8 x 4K)
        uint8_t *dst = (l == last) ? out : (l == tap_layer ? tap_out : pp[(l - first) & 1]);
        const int ev = slot0 >= 0 ? slot0 + (l - first) : -1;
        if (ev >= 0) {
            net->ev_layer[ev].store(-1, std::memory_order_relaxed);   // becomes l once both events are recorded
            if (hipEventRecord(net->ev_begin[ev], stream) != hipSuccess) return SICN_ENODEV;
        }
        int rc = run_layer(&net->descs[l], wl, cur, dst, n_images, stream, -1, net->opt, net->gdn[l], step,
                           deal_base ? deal_base + (size_t)l * DEAL_WORDS : nullptr);
        if (rc) return rc;
        if (ev >= 0) {
            if (hipEventRecord(net->ev_end[ev], stream) != hipSuccess) return SICN_ENODEV;
            net->ev_layer[ev].store(l, std::memory_order_release);
        }
        if (l == tap_layer && tap_out != dst) {
            if (hipMemcpyAsync(tap_out, dst, out_bytes(net->descs[l]) * (size_t)n_images, hipMemcpyDeviceToDevice,
                               stream) != hipSuccess)
                return SICN_ENODEV;
        }
        cur = dst;
    }
    return SICN_OK;
}

extern "C" int sicn_eight_layers_net(const sicn_net *net, const uint8_t *in, uint8_t *out, uint8_t *latent,
                                     int n_images, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!net) return SICN_EINVAL;
    const int n = (int)net->descs.size();
    const int tap = latent ? 3 : -1;
    if (latent && n < 4) return SICN_EINVAL;
    return sicn_net_forward(net, 0, n - 1, in, out, tap, latent, n_images, workspace, workspace_bytes, hip_stream);
}

extern "C" int sicn_net_profile(sicn_net *net, int enable)
{
    if (!net) return SICN_EINVAL;
    if (enable && net->ev_begin.empty()) {
        const size_t n = (size_t)sicn_net::EV_RING;
        std::vector<hipEvent_t> a, b;
        try {
            a.reserve(n);
            b.reserve(n);
            net->ev_layer.reset(new std::atomic<int>[n]);
            for (size_t i = 0; i < n; i++) net->ev_layer[i].store(-1, std::memory_order_relaxed);
        } catch (const std::bad_alloc &) { return SICN_ENOMEM; }
        bool ok = true;
        for (size_t i = 0; i < n && ok; i++) {
            hipEvent_t e;
            if ((ok = hipEventCreate(&e) == hipSuccess)) a.push_back(e);
            if (ok && (ok = hipEventCreate(&e) == hipSuccess)) b.push_back(e);
        }
        if (!ok) {   // all or nothing: a half-made ring would be indexed out of range later
            for (hipEvent_t e : a) (void)hipEventDestroy(e);
            for (hipEvent_t e : b) (void)hipEventDestroy(e);
            return SICN_ENODEV;
        }
        net->ev_begin.swap(a);
        net->ev_end.swap(b);
    }
    net->profile.store(enable != 0, std::memory_order_release);
    return SICN_OK;
}

extern "C" int sicn_net_layer_ms(sicn_net *net, int reset, float *ms_sum, int *launches)
{
    if (!net || !ms_sum || !launches) return SICN_EINVAL;
    const size_t n_layers = net->descs.size();
    for (size_t l = 0; l < n_layers; l++) {
        ms_sum[l] = 0.f;
        launches[l] = 0;
    }
    int used = net->ev_next.load(std::memory_order_acquire);
    if (used > sicn_net::EV_RING) used = sicn_net::EV_RING;
    if (net->ev_begin.empty()) used = 0;
    for (int i = 0; i < used; i++) {
        const int l = net->ev_layer[i].load(std::memory_order_acquire);
        if (l < 0 || (size_t)l >= n_layers) continue;   // reserved by a call that failed before recording
        if (hipEventSynchronize(net->ev_end[i]) != hipSuccess) return SICN_ENODEV;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, net->ev_begin[i], net->ev_end[i]) != hipSuccess) return SICN_ENODEV;
        ms_sum[l] += ms;
        launches[l]++;
    }
    if (reset) {
        for (int i = 0; i < used; i++) net->ev_layer[i].store(-1, std::memory_order_relaxed);
        net->ev_next.store(0, std::memory_order_release);
    }
    return SICN_OK;
}

// ---- crop of NHWC batches (one launch; see k_crop_nhwc) -----------------------------------------------------------------------------
extern "C" int sicn_crop_nhwc(const uint8_t *src, uint8_t *dst, int n_images, int src_h, int src_w, int h, int w, int channels,
                              void *hip_stream)
{
    if (n_images < 0 || h < 0 || w < 0 || channels <= 0 || h > src_h || w > src_w) return SICN_EINVAL;
    if ((size_t)n_images * h * w && (!src || !dst)) return SICN_EINVAL;
    if (chip_geom(nullptr) != SICN_OK) return SICN_ENODEV;
    const hipError_t e = launch_crop_nhwc(src, dst, n_images, src_h, src_w, h, w, channels, (hipStream_t)hip_stream);
    return e == hipSuccess ? SICN_OK : SICN_ENODEV;
}

// ---- launch planning, inspectable without a GPU (tests/test_abi_load.py): what would this layer launch on a chip of n_cu CUs? ----
extern "C" int sicn_debug_plan(const sicn_layer_desc *d, int n_images, const sicn_options *opt, int n_cu, int32_t out[12])
{
    sicn_options o;
    if (int rc = resolve_options(opt, &o)) return rc;
    if (int rc = sicn_validate_desc(d)) return rc;
    if (!out || n_images <= 0 || n_cu <= 0) return SICN_EINVAL;
    const ChipGeom chip = chip_from_cus(n_cu);
    const LayerGeom g = geom_of(*d);
    for (int i = 0; i < 12; i++) out[i] = 0;
    out[0] = chip.n_cu;
    out[1] = chip.n_xcd;
    const Family &f = pick_family(*d, o);
    out[2] = (int)f.kind;
    if (f.plan) f.plan(g, n_images, o, chip, out);
    return SICN_OK;
}
// the chip the launchers plan with on the current device (the device's own CU count, or SICN_N_CU): what a test that forces a count asserts first
extern "C" int sicn_debug_chip(int32_t out[2])
{
    if (!out) return SICN_EINVAL;
    ChipGeom chip;
    if (int rc = chip_geom(&chip)) return rc;
    out[0] = chip.n_cu;
    out[1] = chip.n_xcd;
    return SICN_OK;
}
// host mirror of the kernels' XCD-aware work list: the item of workgroup `block`, or -1 (a bijection for every XCD count)
extern "C" long long sicn_debug_xcd_item(long long block, long long n_items, int n_xcd)
{
    return n_xcd > 0 ? (long long)xcd_item_of((long)block, (long)n_items, n_xcd) : -1;
}

// ---- GDN / IGDN activation objects (include/sicn_gdn.h; extension beyond the reference) ------------------------
extern "C" void sicn_gdn_free(sicn_gdn *g)
{
    if (!g) return;
    if (g->d_beta) (void)hipFree(g->d_beta);
    if (g->d_beta_mfma) (void)hipFree(g->d_beta_mfma);
    if (g->d_gamma) (void)hipFree(g->d_gamma);
    if (g->d_gamma_mfma) (void)hipFree(g->d_gamma_mfma);
    delete g;
}

extern "C" long long sicn_gdn_selftest_roots(int inverse, uint32_t n_begin, unsigned long long count)
{
    if ((inverse != 0 && inverse != 1) || (unsigned long long)n_begin + count > (1ull << 31)) return SICN_EINVAL;
    unsigned long long bad = 0;
    if (sicn::gdn_selftest_roots(inverse, n_begin, count, &bad) != hipSuccess) return SICN_ENODEV;
    return (long long)bad;
}

extern "C" int sicn_gdn_create(int channels, int inverse, int shift, const uint32_t *beta, const uint8_t *gamma, sicn_gdn **out)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    if (channels <= 0 || channels > 1024 || (inverse != 0 && inverse != 1) || shift < 1 || shift > 24 || !beta || !gamma)
        return SICN_EINVAL;
    for (int i = 0; i < channels; i++) {
        if (beta[i] < 1 || beta[i] > 65535) return SICN_EINVAL;
        for (int j = 0; j < channels; j++)
            if (gamma[(size_t)i * channels + j] > 127) return SICN_EINVAL;
    }
    sicn_gdn *g = new (std::nothrow) sicn_gdn();
    if (!g) return SICN_ENOMEM;
    // kc = 2^s (1 + b 2^-16), s = 16 - shift / 8 - shift, b = 5 / 33 (oracle/sicn_gdn_oracle.c): 17 significant bits, exact in binary32
    *g = sicn_gdn{channels, inverse, shift, std::ldexp((float)(65536 + (inverse ? 33 : 5)), (inverse ? 8 : 16) - shift - 16), nullptr, nullptr, nullptr, nullptr};
    bool ok = upload(beta, (size_t)channels * 4, &g->d_beta) &&
              upload(gamma, (size_t)channels * channels, &g->d_gamma);
    if (ok && (channels == 128 || channels == 192)) {
        try {
            std::vector<int8_t> img((size_t)channels * channels);
            pack_gdn_gamma(gamma, channels, img.data());
            std::vector<uint32_t> beta_mfma((size_t)channels);   // the low digit of x^2 goes through the MFMA as lo - 128
            for (int i = 0; i < channels; i++) {
                uint32_t row = 0;
                for (int j = 0; j < channels; j++) row += gamma[(size_t)i * channels + j];
                beta_mfma[(size_t)i] = beta[i] + 128u * row;
            }
            ok = upload(img.data(), img.size(), &g->d_gamma_mfma) && upload(beta_mfma.data(), beta_mfma.size() * 4, &g->d_beta_mfma);
        } catch (const std::bad_alloc &) { ok = false; }
    }
    if (!ok) {
        sicn_gdn_free(g);
        return SICN_ENOMEM;
    }
    *out = g;
    return SICN_OK;
}

namespace sicn {
int gdn_apply_lanes(const sicn_gdn &g, uint8_t *lanes, long long n_positions, hipStream_t stream)
{
    // chunks of < 2 GiB (the kernel addresses a chunk through one buffer descriptor with 31-bit offsets)
    const long long chunk = ((1LL << 31) - 4096) / g.channels;
    for (long long p = 0; p < n_positions; p += chunk) {
        const long long n = n_positions - p < chunk ? n_positions - p : chunk;
        hipError_t e = launch_gdn(g, lanes + (size_t)p * g.channels, 0 /* NHWC */, (int)n, 1, 1, stream);
        if (e == hipErrorInvalidValue) return SICN_EINVAL;
        if (e != hipSuccess) return SICN_ENODEV;
    }
    return SICN_OK;
}
}  // namespace sicn

extern "C" int sicn_gdn_apply(const sicn_gdn *g, uint8_t *lanes, long long n_positions, void *hip_stream)
{
    if (!g || n_positions < 0 || (n_positions && !lanes)) return SICN_EINVAL;
    return gdn_apply_lanes(*g, lanes, n_positions, (hipStream_t)hip_stream);
}

extern "C" int sicn_conv2d_gdn(const sicn_layer_desc *d, const sicn_weights *w, const sicn_gdn *gdn, const uint8_t *in,
                               uint8_t *out, int n_images, const sicn_options *opt, void *hip_stream)
{
    sicn_options o;
    int rc = resolve_options(opt, &o);
    return rc ? rc : run_layer(d, w, in, out, n_images, (hipStream_t)hip_stream, 0, o, gdn, live::Step{}, nullptr);
}

extern "C" int sicn_deconv522_gdn(const sicn_layer_desc *d, const sicn_weights *w, const sicn_gdn *gdn, const uint8_t *in,
                                  uint8_t *out, int n_images, const sicn_options *opt, void *hip_stream)
{
    sicn_options o;
    int rc = resolve_options(opt, &o);
    return rc ? rc : run_layer(d, w, in, out, n_images, (hipStream_t)hip_stream, 1, o, gdn, live::Step{}, nullptr);
}
