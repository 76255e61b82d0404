// The bilinear interpolation of the scores to a source pixel, as scores_labels.hip and the interpolated form of confidence.hip both compute it:
// the taps, their loads and the blend, the restatement of accel_amd/utils/image.py interpolation_taps / labels_interpolated_host bit for bit.
//
// Taps, in integer arithmetic (source row y of h rows over a region of out_h rows; columns alike with w, out_w):
//     num = clamp((2 * y + 1) * out_h - h, 0, 2 * h * (out_h - 1))           (< 2^31: sizes are at most 32768)
//     y0  = num / (2 * h);   y1 = min(y0 + 1, out_h - 1);   fy = double(num - 2 * h * y0) / double(2 * h)        ONE IEEE division
// which is the half-pixel-centre coordinate (y + 0.5) * out_h / h - 0.5 clamped to the region: the inverse of the resize the frame went
// through on the way in (frames_resample.h).  Taps never leave the valid region: the padding is never read.
// Blend, in float64, each operation rounded on its own (no fma), in the order of frames::blend; a<row><col> the fp32 taps as doubles:
//     gx = 1 - fx;  gy = 1 - fy;  top = a00 * gx + a01 * fx;  bot = a10 * gx + a11 * fx;  v = top * gy + bot * fy
// At h x w == out_h x out_w, fx = fy = 0 and v is the stored score.  Scores are assumed FINITE: inf * 0 arises in the blend.
#pragma once
#include <hip/hip_runtime.h>

namespace interp {

struct Tap { int i0, i1; double f; };

// the two taps and the weight of the second for output index i of `dst` over a region of `src`
__device__ __forceinline__ Tap tap(int i, int dst, int src)
{
    const int two = 2 * dst;
    const int num = min(max((2 * i + 1) * src - dst, 0), two * (src - 1));
    Tap t;
    t.i0 = num / two;
    t.i1 = min(t.i0 + 1, src - 1);
    t.f = (double)(num - two * t.i0) / (double)two;
    return t;
}

// the four taps of one class plane: rows r0 and r1 of the frame's first plane, the plane `at` floats further on, columns x0 and x1
struct Taps { float a00, a01, a10, a11; };

__device__ __forceinline__ Taps load_taps(const float* r0, const float* r1, size_t at, int x0, int x1)
{
    Taps t;
    t.a00 = r0[at + x0]; t.a01 = r0[at + x1]; t.a10 = r1[at + x0]; t.a11 = r1[at + x1];
    return t;
}

// the weights of a pixel, and the seven-operation blend of one class's four taps under them
struct Weights {
    double fx, fy, gx, gy;
    __device__ __forceinline__ Weights(const Tap ty, const Tap tx)
    {
#pragma clang fp contract(off)
        fx = tx.f; fy = ty.f; gx = 1.0 - fx; gy = 1.0 - fy;
    }
};

__device__ __forceinline__ double blend(const Taps t, const Weights w)
{
#pragma clang fp contract(off)
    const double t0 = (double)t.a00 * w.gx, t1 = (double)t.a01 * w.fx;
    const double top = t0 + t1;
    const double b0 = (double)t.a10 * w.gx, b1 = (double)t.a11 * w.fx;
    const double bot = b0 + b1;
    const double u0 = top * w.gy, u1 = bot * w.fy;
    return u0 + u1;
}

}  // namespace interp
