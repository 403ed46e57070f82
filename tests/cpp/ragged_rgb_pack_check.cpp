// Stand-alone check of csrc/ragged_rgb_host.hpp (the K packing and the weight images of a ragged net's packed RGB ends) for builds
// with the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all ragged_rgb_pack_check.cpp -o ragged_rgb_pack_check
// It packs random weights over the full nibble range, walks K on the CPU exactly as the header says the kernels do — the RGBX patch
// with arbitrary NON-ZERO bytes in the X byte and in every slot that only zero weights meet, K steps, rows — and compares the low
// byte of every accumulator with the direct closed form written out below.  A single wrong weight byte in a real slot must change
// some output, or the check could not see a mis-packing.  Every image and weight buffer is a heap block of EXACTLY its length.
// Exit status 0 and one line "ragged_rgb_pack_check ok: <n> checks" when everything held.  No device, no library.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "../../simple_image_compression_network_amd/csrc/ragged_rgb_host.hpp"

namespace {

using namespace sicn;

long long checks = 0;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        checks++;                                                                     \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

template <class T>
std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

std::mt19937 rng(20260115u);
int nibble() { return (int)(rng() % 16u) - 8; }
uint8_t junk() { return (uint8_t)(1u + rng() % 255u); }       // never 0

// ---- conv 3 -> N ------------------------------------------------------------------------------------------------------------------
// the closed form: out[y][x][o] = (sum in[2y + ky - 2][2x + kx - 2][c] W[o][ky][kx][c] + b[o]) mod 256
std::unique_ptr<uint8_t[]> conv_direct(const uint8_t *in, int W, int H, const int8_t *w, const int8_t *b, int N)
{
    const int OW = (W + 1) / 2, OH = (H + 1) / 2;
    auto out = exact<uint8_t>((size_t)OH * OW * N);
    for (int y = 0; y < OH; y++)
        for (int x = 0; x < OW; x++)
            for (int o = 0; o < N; o++) {
                int acc = b[o];
                for (int ky = 0; ky < 5; ky++)
                    for (int kx = 0; kx < 5; kx++) {
                        const int iy = 2 * y + ky - 2, ix = 2 * x + kx - 2;
                        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                        for (int c = 0; c < 3; c++) acc += (int)in[((size_t)iy * W + ix) * 3 + c] * w[(size_t)o * 75 + (ky * 5 + kx) * 3 + c];
                    }
                out[((size_t)y * OW + x) * N + o] = (uint8_t)acc;
            }
    return out;
}

// the kernel's walk over the packed image `img`: tiles of 16 x 16 positions, a 36 x 40 RGBX patch each, 3 K steps of 64 bytes
std::unique_ptr<uint8_t[]> conv_walk(const uint8_t *in, int W, int H, const int8_t *img, const int8_t *b, int N)
{
    const int OW = (W + 1) / 2, OH = (H + 1) / 2, nblk = (N + 63) / 64;
    constexpr int ROWS = 36, PX = 40;
    auto out = exact<uint8_t>((size_t)OH * OW * N);
    auto patch = exact<uint8_t>((size_t)ROWS * PX * 4);
    for (int y0 = 0; y0 < OH; y0 += 16)
        for (int x0 = 0; x0 < OW; x0 += 16) {
            for (int r = 0; r < ROWS; r++)
                for (int p = 0; p < PX; p++) {
                    uint8_t *d = &patch[((size_t)r * PX + p) * 4];
                    const int iy = 2 * y0 - 2 + r, ix = 2 * x0 - 2 + p;
                    const bool met_by_real_weights = r < 35 && p < 35;
                    for (int c = 0; c < 3; c++)
                        d[c] = !met_by_real_weights ? junk() : (iy >= 0 && iy < H && ix >= 0 && ix < W) ? in[((size_t)iy * W + ix) * 3 + c] : 0;
                    d[3] = junk();
                }
            for (int ly = 0; ly < 16 && y0 + ly < OH; ly++)
                for (int lx = 0; lx < 16 && x0 + lx < OW; lx++)
                    for (int J = 0; J < nblk; J++)
                        for (int j = 0; j < 4; j++)
                            for (int rho = 0; rho < 16; rho++) {
                                const int o = rgb_conv_channel(J, j, rho);
                                if (o >= N) continue;
                                int acc = b[o];
                                for (int s = 0; s < RGB_CONV_KSTEPS; s++) {
                                    const int8_t *row = img + ((((size_t)J * RGB_CONV_KSTEPS + s) * 4 + j) * 16 + rho) * 64;
                                    for (int k = 0; k < 64; k++) {
                                        // lane (col, g) reads bytes 16 g .. of pixels 2 lx + 4 (g & 1) .. of patch row 2 ly + 2 s + (g >> 1)
                                        const int g = k >> 4, pr = 2 * ly + 2 * s + (g >> 1), off = 8 * lx + 16 * (g & 1) + (k & 15);
                                        acc += (int)(int8_t)patch[(size_t)pr * PX * 4 + off] * row[k];
                                    }
                                }
                                out[((size_t)(y0 + ly) * OW + x0 + lx) * N + o] = (uint8_t)acc;
                            }
        }
    return out;
}

struct ConvCase {
    int W, H, N;
    std::unique_ptr<uint8_t[]> in, ref;
    std::unique_ptr<int8_t[]> w, b, img;
    size_t out_bytes;
};

ConvCase conv_case(int W, int H, int N)
{
    ConvCase c{W, H, N, exact<uint8_t>((size_t)H * W * 3), nullptr, exact<int8_t>((size_t)N * 75), exact<int8_t>((size_t)N),
               exact<int8_t>(rgb_conv_bytes(N)), (size_t)((H + 1) / 2) * ((W + 1) / 2) * N};
    for (size_t i = 0; i < (size_t)H * W * 3; i++) c.in[i] = (uint8_t)(rng() & 255u);
    for (size_t i = 0; i < (size_t)N * 75; i++) c.w[i] = (int8_t)nibble();
    for (int i = 0; i < N; i++) c.b[i] = (int8_t)((int)(rng() & 255u) - 128);
    pack_rgb_conv(c.w.get(), N, c.img.get());
    c.ref = conv_direct(c.in.get(), W, H, c.w.get(), c.b.get(), N);
    return c;
}

bool same(const uint8_t *a, const uint8_t *b, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

void conv_checks()
{
    // the row order is pack_any's: C/D row 4 g + r of tile j is channel 64 J + 16 g + 4 j + r
    for (int J = 0; J < 16; J++)
        for (int j = 0; j < 4; j++)
            for (int g = 0; g < 4; g++)
                for (int r = 0; r < 4; r++) EXPECT(rgb_conv_channel(J, j, 4 * g + r) == 64 * J + 16 * g + 4 * j + r);
    // every (ky, kx, c) sits in exactly one byte of one K step
    int seen[5][5][3] = {};
    for (int s = 0; s < RGB_CONV_KSTEPS; s++)
        for (int k = 0; k < 64; k++) {
            const RgbConvSlot t = rgb_conv_slot(s, k);
            if (t.real) seen[t.ky][t.kx][t.c]++;
        }
    for (int ky = 0; ky < 5; ky++)
        for (int kx = 0; kx < 5; kx++)
            for (int c = 0; c < 3; c++) EXPECT(seen[ky][kx][c] == 1);
    for (int N : {16, 80, 128})
        for (int size = 0; size < 2; size++) {
            ConvCase c = conv_case(size ? 33 : 5, size ? 31 : 3, N);
            EXPECT(rgb_conv_bytes(N) == (size_t)((N + 63) / 64) * 12288);
            auto got = conv_walk(c.in.get(), c.W, c.H, c.img.get(), c.b.get(), N);
            EXPECT(same(got.get(), c.ref.get(), c.out_bytes));
            // slots that are not real, and rows of channels past N, are zero
            for (size_t i = 0; i < rgb_conv_bytes(N); i++) {
                const int k = (int)(i & 63), rho = (int)(i >> 6) & 15, j = (int)(i >> 10) & 3, s = (int)((i >> 12) % 3), J = (int)((i >> 12) / 3);
                if (!rgb_conv_slot(s, k).real || rgb_conv_channel(J, j, rho) >= N) EXPECT(c.img[i] == 0);
            }
        }
    // one wrong byte in a real slot of a real channel is seen, whichever slot it is
    ConvCase c = conv_case(5, 3, 16);
    int tried = 0;
    for (size_t i = 0; i < rgb_conv_bytes(16); i++) {
        const int k = (int)(i & 63), rho = (int)(i >> 6) & 15, j = (int)(i >> 10) & 3, s = (int)(i >> 12);
        if (!rgb_conv_slot(s, k).real || rgb_conv_channel(0, j, rho) >= 16) continue;
        c.img[i] = (int8_t)(c.img[i] + 1);
        auto got = conv_walk(c.in.get(), c.W, c.H, c.img.get(), c.b.get(), 16);
        EXPECT(!same(got.get(), c.ref.get(), c.out_bytes));
        c.img[i] = (int8_t)(c.img[i] - 1);
        tried++;
    }
    EXPECT(tried == 16 * 75);
}

// ---- deconv N -> 3 ----------------------------------------------------------------------------------------------------------------
// the closed form: out[y][x][o] = (sum Up[y + ky - 2][x + kx - 2][c] W[o][ky][kx][c] + b[o]) mod 256, Up[2 i][2 j] = in[i][j], 0 elsewhere
std::unique_ptr<uint8_t[]> deconv_direct(const uint8_t *in, int W, int H, int C, const int8_t *w, const int8_t *b)
{
    const int OW = 2 * W, OH = 2 * H;
    auto out = exact<uint8_t>((size_t)OH * OW * 3);
    for (int y = 0; y < OH; y++)
        for (int x = 0; x < OW; x++)
            for (int o = 0; o < 3; o++) {
                int acc = b[o];
                for (int ky = 0; ky < 5; ky++)
                    for (int kx = 0; kx < 5; kx++) {
                        const int uy = y + ky - 2, ux = x + kx - 2;
                        if (uy < 0 || ux < 0 || (uy & 1) || (ux & 1) || uy / 2 >= H || ux / 2 >= W) continue;
                        const uint8_t *p = in + ((size_t)(uy / 2) * W + ux / 2) * C;
                        for (int c = 0; c < C; c++) acc += (int)p[c] * w[(size_t)o * 25 * C + (size_t)(ky * 5 + kx) * C + c];
                    }
                out[((size_t)y * OW + x) * 3 + o] = (uint8_t)acc;
            }
    return out;
}

// the kernel's walk: tiles of 16 x 16 INPUT positions, an 18 x 18 x 64 patch per chunk, nine offsets, 16 rows = 4 phases x (3 + 1)
std::unique_ptr<uint8_t[]> deconv_walk(const uint8_t *in, int W, int H, int C, const int8_t *img, const int8_t *b, bool *row3_zero)
{
    const int OW = 2 * W, OH = 2 * H, nchunk = (C + 63) / 64;
    auto out = exact<uint8_t>((size_t)OH * OW * 3);
    auto patch = exact<uint8_t>((size_t)nchunk * 18 * 18 * 64);
    *row3_zero = true;
    for (int y0 = 0; y0 < H; y0 += 16)
        for (int x0 = 0; x0 < W; x0 += 16) {
            for (int n = 0; n < nchunk; n++)
                for (int pr = 0; pr < 18; pr++)
                    for (int pc = 0; pc < 18; pc++)
                        for (int k = 0; k < 64; k++) {
                            const int iy = y0 - 1 + pr, ix = x0 - 1 + pc, ch = n * 64 + k;
                            patch[(((size_t)n * 18 + pr) * 18 + pc) * 64 + k] =
                                ch >= C ? junk() : (iy >= 0 && iy < H && ix >= 0 && ix < W) ? in[((size_t)iy * W + ix) * C + ch] : 0;
                        }
            for (int ly = 0; ly < 16 && y0 + ly < H; ly++)
                for (int lx = 0; lx < 16 && x0 + lx < W; lx++)
                    for (int rho = 0; rho < 16; rho++) {
                        const int phase = rho >> 2, c = rho & 3;
                        int acc = c < 3 ? b[c] : 0;
                        for (int t = 0; t < RGB_DECONV_OFFSETS; t++)
                            for (int n = 0; n < nchunk; n++) {
                                const int8_t *row = img + (((size_t)t * nchunk + n) * 16 + rho) * 64;
                                const uint8_t *px = &patch[(((size_t)n * 18 + ly + t / 3) * 18 + lx + t % 3) * 64];
                                for (int k = 0; k < 64; k++) acc += (int)(int8_t)px[k] * row[k];
                            }
                        if (c == 3) {
                            if (acc != 0) *row3_zero = false;
                            continue;
                        }
                        // lane (col, g) holds rows 4 g .. 4 g + 3: phase g -> output pixel (2 my + (g >> 1), 2 mx + (g & 1))
                        out[((size_t)(2 * (y0 + ly) + (phase >> 1)) * OW + 2 * (x0 + lx) + (phase & 1)) * 3 + c] = (uint8_t)acc;
                    }
        }
    return out;
}

struct DeconvCase {
    int W, H, C;
    std::unique_ptr<uint8_t[]> in, ref;
    std::unique_ptr<int8_t[]> w, b, img;
    size_t out_bytes;
};

DeconvCase deconv_case(int W, int H, int C)
{
    DeconvCase c{W, H, C, exact<uint8_t>((size_t)H * W * C), nullptr, exact<int8_t>((size_t)75 * C), exact<int8_t>(3),
                 exact<int8_t>(rgb_deconv_bytes(C)), (size_t)4 * H * W * 3};
    for (size_t i = 0; i < (size_t)H * W * C; i++) c.in[i] = (uint8_t)(rng() & 255u);
    for (size_t i = 0; i < (size_t)75 * C; i++) c.w[i] = (int8_t)nibble();
    for (int i = 0; i < 3; i++) c.b[i] = (int8_t)((int)(rng() & 255u) - 128);
    pack_rgb_deconv(c.w.get(), C, c.img.get());
    c.ref = deconv_direct(c.in.get(), W, H, C, c.w.get(), c.b.get());
    return c;
}

void deconv_checks()
{
    // every (phase, c, ky, kx) with ky = qy mod 2, kx = qx mod 2 sits in exactly one (offset, row); 9 + 6 + 6 + 4 taps per channel
    int seen[3][5][5] = {};
    for (int t = 0; t < RGB_DECONV_OFFSETS; t++)
        for (int rho = 0; rho < 16; rho++) {
            const RgbDeconvRow r = rgb_deconv_row(t, rho);
            EXPECT(r.phase == rho >> 2 && r.c == (rho & 3));
            if (!r.real) continue;
            EXPECT(r.ky >= 0 && r.ky < 5 && r.kx >= 0 && r.kx < 5 && (r.ky & 1) == (r.phase >> 1) && (r.kx & 1) == (r.phase & 1));
            seen[r.c][r.ky][r.kx]++;
        }
    for (int c = 0; c < 3; c++)
        for (int ky = 0; ky < 5; ky++)
            for (int kx = 0; kx < 5; kx++) EXPECT(seen[c][ky][kx] == 1);
    for (int C : {32, 96, 128})
        for (int size = 0; size < 2; size++) {
            DeconvCase c = deconv_case(size ? 17 : 3, size ? 18 : 5, C);
            EXPECT(rgb_deconv_bytes(C) == (size_t)9 * ((C + 63) / 64) * 1024);
            bool row3_zero = false;
            auto got = deconv_walk(c.in.get(), c.W, c.H, C, c.img.get(), c.b.get(), &row3_zero);
            EXPECT(same(got.get(), c.ref.get(), c.out_bytes));
            EXPECT(row3_zero);
            const int nchunk = (C + 63) / 64;
            for (size_t i = 0; i < rgb_deconv_bytes(C); i++) {
                const int k = (int)(i & 63), rho = (int)(i >> 6) & 15, n = (int)((i >> 10) % nchunk), t = (int)((i >> 10) / nchunk);
                if (!rgb_deconv_row(t, rho).real || n * 64 + k >= C) EXPECT(c.img[i] == 0);
            }
        }
    // one wrong byte in a real slot is seen: every real (offset, row), a few channels each
    DeconvCase c = deconv_case(3, 5, 32);
    int tried = 0;
    bool z;
    for (size_t i = 0; i < rgb_deconv_bytes(32); i++) {
        const int k = (int)(i & 63), rho = (int)(i >> 6) & 15, t = (int)(i >> 10);
        if (!rgb_deconv_row(t, rho).real || k >= 32 || k % 5 != (int)(i >> 6) % 5) continue;
        c.img[i] = (int8_t)(c.img[i] + 1);
        auto got = deconv_walk(c.in.get(), c.W, c.H, 32, c.img.get(), c.b.get(), &z);
        EXPECT(!same(got.get(), c.ref.get(), c.out_bytes));
        c.img[i] = (int8_t)(c.img[i] - 1);
        tried++;
    }
    EXPECT(tried >= 75 * 6);
}

}  // namespace

int main()
{
    conv_checks();
    deconv_checks();
    std::printf("ragged_rgb_pack_check ok: %lld checks\n", checks);
    return 0;
}
