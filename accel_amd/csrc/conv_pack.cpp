// Host side of a convolution's parameter block (conv_pack.h): weight repacking, the tap table, the epilogue constants.
#include "conv_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>

void pack_conv_w(const float* w, int Cout, int Cin, int kh, int kw, int cin_pad, int rows, int K_pad, std::vector<float>& out)
{
    out.assign((size_t)rows * K_pad, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx)
                    out[(size_t)co * K_pad + (size_t)(ky * kw + kx) * cin_pad + ci] =
                        w[(((size_t)co * Cin + ci) * kh + ky) * kw + kx];
}

void pack_deconv2x_w(const float* w, int Cin, int Cout, int cin_pad, int rows, int K_pad, std::vector<float>& out)
{
    out.assign((size_t)4 * rows * K_pad, 0.f);
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            float* base = out.data() + (size_t)(py * 2 + px) * rows * K_pad;
            for (int co = 0; co < Cout; ++co)
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx) {
                        const int ky = 3 - py - 2 * ty, kx = 3 - px - 2 * tx;
                        for (int ci = 0; ci < Cin; ++ci)
                            base[(size_t)co * K_pad + (size_t)(ty * 2 + tx) * cin_pad + ci] =
                                w[(((size_t)ci * Cout + co) * 4 + ky) * 4 + kx];
                    }
        }
}

// f(index into [class][rows][K_pad], index into the plane) for every (class, row, k)
template <class F>
static void for_each_weight(int classes, int rows, int K_pad, ConvOrder order, F f)
{
    for (int c = 0; c < classes; ++c)
        for (int n = 0; n < rows; ++n)
            for (int k = 0; k < K_pad; ++k) f(((size_t)c * rows + n) * K_pad + k, conv_plane_index(order, rows, K_pad, c, n, k));
}

void bf16_split3(float v, uint16_t t[3])
{
    float r = v;
    for (int pl = 0; pl < 3; ++pl) {
        uint32_t u; memcpy(&u, &r, 4);
        u &= 0xFFFF0000u;
        t[pl] = (uint16_t)(u >> 16);
        float top; memcpy(&top, &u, 4);
        r -= top;
    }
}

void pack_bf16x3(const std::vector<float>& packed, int classes, int rows, int K_pad, ConvOrder order, std::vector<uint16_t>& out)
{
    const size_t plane = conv_plane_elems(classes, rows, K_pad);
    out.assign(3 * plane, 0);
    for_each_weight(classes, rows, K_pad, order, [&](size_t src, size_t dst) {
        uint16_t t[3];
        bf16_split3(packed[src], t);
        for (int pl = 0; pl < 3; ++pl) out[pl * plane + dst] = t[pl];
    });
}

void pack_f16r(const std::vector<_Float16>& half, int classes, int rows, int K_pad, std::vector<_Float16>& out)
{
    out.assign(conv_plane_elems(classes, rows, K_pad), (_Float16)0.f);
    for_each_weight(classes, rows, K_pad, CONV_ORDER_FRAG, [&](size_t src, size_t dst) { out[dst] = half[src]; });
}

void pack_h2r(const std::vector<float>& packed, int classes, int rows, int K_pad, std::vector<uint16_t>& out, std::vector<int>& qexp)
{
    const size_t plane = conv_plane_elems(classes, rows, K_pad);
    out.assign(2 * plane, 0);
    qexp.assign(rows, 0);
    for (int n = 0; n < rows; ++n) {
        float amax = 0.f;
        for (int c = 0; c < classes; ++c)
            for (int k = 0; k < K_pad; ++k) amax = std::max(amax, std::fabs(packed[((size_t)c * rows + n) * K_pad + k]));
        if (amax > 0.f && std::isfinite(amax)) { int e; std::frexp(amax, &e); qexp[n] = 15 - e; }
    }
    for (int c = 0; c < classes; ++c)      // (loops of its own: through for_each_weight this one measured a third slower)
        for (int n = 0; n < rows; ++n)
            for (int k = 0; k < K_pad; ++k) {
                const float v = std::ldexp(packed[((size_t)c * rows + n) * K_pad + k], qexp[n]);
                const size_t dst = conv_plane_index(CONV_ORDER_FRAG, rows, K_pad, c, n, k);
                const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
                memcpy(&out[dst], &hi, 2);
                memcpy(&out[plane + dst], &lo, 2);
            }
}

void conv_tap_table(int classes, int K_pad, int Cin, int kh, int kw, int dh, int dw, int W, int xCs, int esize, std::vector<int>& tab)
{
    const int G = K_pad / 4, slack = CONV_TAP_SLACK;
    tab.assign((size_t)classes * (G + slack) * 4, 0);
    for (int cls = 0; cls < classes; ++cls)
        for (int g = 0; g < G + slack; ++g) {
            const int k = g * 4, tap = k / Cin, ci = k % Cin;
            const int ky = tap / kw, kx = tap % kw;
            int* t = &tab[((size_t)cls * (G + slack) + g) * 4];
            if (g >= G || tap >= kh * kw) { t[0] = CONV_TAP_OUT; continue; }
            t[0] = ky * dh; t[1] = kx * dw;
            t[2] = ((ky * dh * W + kx * dw) * xCs + ci) * esize;
        }
}

void bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C,
             std::vector<float>& scale, std::vector<float>& shift)
{
    scale.assign(C, 0.f); shift.assign(C, 0.f);
    for (int c = 0; c < C; ++c) {
        const float gg = gamma ? gamma[c] : 1.0f;
        const float sd = sqrtf(var[c] + eps);
        scale[c] = gg / sd;
        shift[c] = beta[c] - (gg * mean[c]) / sd;
    }
}

void conv_fold_epilogue(int rows, int cout, const std::vector<float>* bn_scale, const std::vector<float>* bn_shift, const float* bias,
                        const float* mul, std::vector<float>& scale, std::vector<float>& shift)
{
    scale.assign(rows, 0.f); shift.assign(rows, 0.f);
    for (int i = 0; i < cout; ++i) scale[i] = 1.f;
    if (bn_scale)
        for (int i = 0; i < cout; ++i) { scale[i] = (*bn_scale)[i]; shift[i] = (*bn_shift)[i]; }
    if (bias)
        for (int i = 0; i < cout; ++i) shift[i] += bias[i] * scale[i];
    if (mul)
        for (int i = 0; i < cout; ++i) { scale[i] *= *mul; shift[i] *= *mul; }
}

void conv_fold_epilogue2(int rows, int cout, const float* bias2, const std::vector<float>* bn_scale, const std::vector<float>* bn_shift,
                         std::vector<float>& scale2, std::vector<float>& shift2)
{
    scale2.assign(rows, 0.f); shift2.assign(rows, 0.f);
    for (int i = 0; i < cout; ++i) {
        scale2[i] = bias2 ? 1.f : (*bn_scale)[i];
        shift2[i] = bias2 ? bias2[i] : (*bn_shift)[i];
    }
}

void conv_h2_scale(const std::vector<float>& scale, const std::vector<int>& q, int n, int k, std::vector<float>& out)
{
    out.assign(scale.size(), 0.f);
    for (int i = 0; i < (int)scale.size() && i < n; ++i) out[i] = std::ldexp(scale[i], k - q[i]);
}
