// Stand-alone check of csrc/conv_pack.cpp on the CPU (tests/test_conv_pack_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it).  For seeded weights it walks every (class, row, k) of every weight copy:
//   position  the element sits where conv_pack.h says, in both orders, for 1 and 4 parity classes (the index is restated here)
//   bf16x3    the three bf16 terms sum back to the fp32 weight exactly
//   fp16x2    hi + lo, scaled back by 2^-q[row], is within the bound tests/test_h2_model_cpu.py asserts for this split
//             (h2_model.split_error_bound with top_exp = 15, restated in split_bound below), the row's largest in [2^14, 2^15)
//   slack     K padding, row padding to 128 and the two K steps behind the last class are zero; no vector is longer than documented
// and every granule of the tap table against the formula of conv_pack.h, padded and slack entries carrying the out-of-range mark.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "conv_pack.h"

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (++failures <= 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                         \
    } while (0)

static unsigned rng_state = 20261021u;
static float rnd()      // weights spread over 24 octaves, both signs, no zeros
{
    rng_state = rng_state * 1664525u + 1013904223u;
    const float m = 1.0f + (float)(rng_state >> 9) / (float)(1 << 23);
    rng_state = rng_state * 1664525u + 1013904223u;
    return std::ldexp((rng_state & 1) ? m : -m, -(int)((rng_state >> 8) % 24));
}

static float bf16_value(uint16_t t) { uint32_t u = (uint32_t)t << 16; float f; memcpy(&f, &u, 4); return f; }
static double half_value(uint16_t h) { _Float16 v; memcpy(&v, &h, 2); return (double)v; }

// tests/h2_model.py split_error_bound(m, top_exp=15): |hi + lo - v| / |v| for a scaled v in [2^(e-1), 2^e)
static double split_bound(double v)
{
    int e;
    std::frexp(std::fabs(v), &e);
    const double v_min = std::ldexp(1.0, e - 1);
    return v_min < std::ldexp(1.0, -24) ? 1.0 : std::fmax(std::ldexp(1.0, -23), std::ldexp(1.0, -25) / v_min);
}

// conv_pack.h, restated: [class][K step][row][32] and [class][K step][half step][row][16]
static size_t index_of(ConvOrder order, int rows, int K_pad, int c, int n, int k)
{
    const size_t steps = K_pad / 32, step = k / 32;
    if (order == CONV_ORDER_STEP) return ((c * steps + step) * rows + n) * 32 + k % 32;
    return (((c * steps + step) * 2 + k % 32 / 16) * rows + n) * 16 + k % 16;
}

struct Shape { const char* name; int cin, cout, kh, kw, deconv; };

static void check_weights(const Shape& s)
{
    const int cin_pad = (s.cin + 3) / 4 * 4, classes = s.deconv ? 4 : 1, taps = s.deconv ? 4 : s.kh * s.kw;
    const int rows = ((s.cout + 3) / 4 * 4 + 127) / 128 * 128, K_pad = (taps * cin_pad + 31) / 32 * 32;
    std::vector<float> w((size_t)s.cin * s.cout * s.kh * s.kw), packed;
    for (float& v : w) v = rnd();
    // ---- [class][rows][K_pad] --------------------------------------------------------------------------------------------------
    if (s.deconv) pack_deconv2x_w(w.data(), s.cin, s.cout, cin_pad, rows, K_pad, packed);
    else pack_conv_w(w.data(), s.cout, s.cin, s.kh, s.kw, cin_pad, rows, K_pad, packed);
    CHECK(packed.size() == (size_t)classes * rows * K_pad, "%s: %zu packed floats", s.name, packed.size());
    for (int c = 0; c < classes; ++c)
        for (int n = 0; n < rows; ++n)
            for (int k = 0; k < K_pad; ++k) {
                const int tap = k / cin_pad, ci = k % cin_pad;
                float want = 0.f;
                if (n < s.cout && tap < taps && ci < s.cin) {
                    if (s.deconv) {      // class (py, px), tap (ty, tx): ky = 3 - py - 2 ty, kx = 3 - px - 2 tx; weights (Cin, Cout, 4, 4)
                        const int ky = 3 - c / 2 - 2 * (tap / 2), kx = 3 - c % 2 - 2 * (tap % 2);
                        want = w[(((size_t)ci * s.cout + n) * 4 + ky) * 4 + kx];
                    } else {
                        want = w[(((size_t)n * s.cin + ci) * s.kh + tap / s.kw) * s.kw + tap % s.kw];
                    }
                }
                CHECK(packed[((size_t)c * rows + n) * K_pad + k] == want, "%s: packed class %d row %d k %d", s.name, c, n, k);
            }
    // ---- the planes --------------------------------------------------------------------------------------------------------------
    const size_t body = (size_t)classes * rows * K_pad, plane = body + 2 * (size_t)rows * 32;
    CHECK(conv_plane_elems(classes, rows, K_pad) == plane, "%s: plane size", s.name);
    std::vector<uint16_t> b3[2], h2;
    std::vector<int> q;
    std::vector<_Float16> half(packed.size()), f16r;
    for (size_t i = 0; i < packed.size(); ++i) half[i] = (_Float16)packed[i];
    pack_bf16x3(packed, classes, rows, K_pad, CONV_ORDER_STEP, b3[0]);
    pack_bf16x3(packed, classes, rows, K_pad, CONV_ORDER_FRAG, b3[1]);
    pack_f16r(half, classes, rows, K_pad, f16r);
    pack_h2r(packed, classes, rows, K_pad, h2, q);
    CHECK(b3[0].size() == 3 * plane && b3[1].size() == 3 * plane && f16r.size() == plane && h2.size() == 2 * plane && q.size() == (size_t)rows,
          "%s: sizes of the copies", s.name);
    if (failures) return;
    std::vector<double> top(rows, 0.0);      // the row's largest scaled weight, over all classes
    for (int c = 0; c < classes; ++c)
        for (int n = 0; n < rows; ++n)
            for (int k = 0; k < K_pad; ++k) {
                const float v = packed[((size_t)c * rows + n) * K_pad + k];
                for (int o = 0; o < 2; ++o) {
                    const ConvOrder order = o ? CONV_ORDER_FRAG : CONV_ORDER_STEP;
                    const size_t at = index_of(order, rows, K_pad, c, n, k);
                    CHECK(at < body && at == conv_plane_index(order, rows, K_pad, c, n, k), "%s: index class %d row %d k %d order %d", s.name, c, n, k, o);
                    const double sum = (double)bf16_value(b3[o][at]) + (double)bf16_value(b3[o][plane + at]) + (double)bf16_value(b3[o][2 * plane + at]);
                    CHECK(sum == (double)v, "%s: bf16x3 class %d row %d k %d order %d: %.9g for %.9g", s.name, c, n, k, o, sum, (double)v);
                }
                const size_t at = index_of(CONV_ORDER_FRAG, rows, K_pad, c, n, k);
                CHECK(!memcmp(&f16r[at], &half[((size_t)c * rows + n) * K_pad + k], 2), "%s: f16 fragment class %d row %d k %d", s.name, c, n, k);
                const double scaled = std::ldexp((double)v, q[n]), got = half_value(h2[at]) + half_value(h2[plane + at]);
                CHECK(std::fabs(got - scaled) <= split_bound(scaled) * std::fabs(scaled),
                      "%s: fp16x2 class %d row %d k %d: %.17g for %.17g", s.name, c, n, k, got, scaled);
                top[n] = std::fmax(top[n], std::fabs(scaled));
            }
    for (int n = 0; n < rows; ++n)
        CHECK(n < s.cout ? top[n] >= 16384.0 && top[n] < 32768.0 : (top[n] == 0.0 && q[n] == 0), "%s: row %d: largest scaled weight %g, q %d", s.name, n, top[n], q[n]);
    for (size_t i = body; i < plane; ++i) {      // the two K steps of slack
        bool zero = !memcmp(&f16r[i], "\0", 2) && h2[i] == 0 && h2[plane + i] == 0;
        for (int o = 0; o < 2; ++o) zero = zero && b3[o][i] == 0 && b3[o][plane + i] == 0 && b3[o][2 * plane + i] == 0;
        CHECK(zero, "%s: slack element %zu", s.name, i - body);
    }
}

static void check_taps(const Shape& s, int dil, int esize)
{
    const int Cin = (s.cin + 3) / 4 * 4, classes = s.deconv ? 4 : 1, kh = s.deconv ? 2 : s.kh, kw = s.deconv ? 2 : s.kw;
    const int K_pad = (kh * kw * Cin + 31) / 32 * 32, W = 11, xCs = Cin + 8, G = K_pad / 4;
    std::vector<int> tab;
    conv_tap_table(classes, K_pad, Cin, kh, kw, dil, dil, W, xCs, esize, tab);
    CHECK(tab.size() == (size_t)classes * (G + CONV_TAP_SLACK) * 4, "%s: %zu words of tap table", s.name, tab.size());
    if (failures) return;
    for (int c = 0; c < classes; ++c)
        for (int g = 0; g < G + CONV_TAP_SLACK; ++g) {
            const int* t = &tab[((size_t)c * (G + CONV_TAP_SLACK) + g) * 4];
            const int tap = 4 * g / Cin, ci = 4 * g % Cin, ky = tap / kw, kx = tap % kw;
            if (g >= G || tap >= kh * kw)
                CHECK(t[0] == CONV_TAP_OUT && t[0] + 64 < 0 && !t[1] && !t[2] && !t[3], "%s: granule %d of class %d is not marked out of range", s.name, g, c);
            else
                CHECK(t[0] == ky * dil && t[1] == kx * dil && t[2] == ((ky * dil * W + kx * dil) * xCs + ci) * esize && !t[3],
                      "%s: granule %d of class %d (dilation %d): %d %d %d %d", s.name, g, c, dil, t[0], t[1], t[2], t[3]);
        }
}

int main()
{
    const Shape shapes[] = {
        {"cin12 cout5 1x3", 12, 5, 1, 3, 0},          // K 36 in 64, cin_pad == Cin, rows 128
        {"cin3 cout136 3x3", 3, 136, 3, 3, 0},        // Cin padded to 4: K 36 in 64, rows 256
        {"deconv cin12 cout5", 12, 5, 4, 4, 1},       // four classes, K 48 in 64
        {"deconv cin3 cout136", 3, 136, 4, 4, 1},     // four classes, K 16 in 32, rows 256
    };
    for (const Shape& s : shapes) {
        check_weights(s);
        check_taps(s, 1, 4);
        check_taps(s, 2, 4);
        check_taps(s, 2, 2);      // a half view
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("conv_pack: ok\n");
    return 0;
}
