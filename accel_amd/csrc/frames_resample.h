// The float64 arithmetic of accel_amd/utils/image.py that the frame kernels (frames_u8.hip, frames_yuv.h) restate bit for bit: where the four
// taps of _resize_bilinear lie, how they are blended, and how a grey level becomes the centred fp32 value.  Every operation is an IEEE double
// operation rounded on its own (hipcc contracts a*b + c into an fma in device code by default; numpy does not).
#pragma once
#include <hip/hip_runtime.h>

namespace frames {

struct Means { double b, g, r; };

struct Taps { int x0, x1, y0, y1; double fx, fy; };

// the taps of output pixel (x, y): source coordinate (dst + 0.5) * step - 0.5 clamped to the h x w image
__device__ __forceinline__ Taps taps(int h, int w, int x, int y, double step)
{
#pragma clang fp contract(off)
    double sy = ((double)y + 0.5) * step - 0.5;
    double sx = ((double)x + 0.5) * step - 0.5;
    sy = fmin(fmax(sy, 0.0), (double)(h - 1));
    sx = fmin(fmax(sx, 0.0), (double)(w - 1));
    Taps t;
    t.y0 = (int)floor(sy); t.x0 = (int)floor(sx);
    t.y1 = min(t.y0 + 1, h - 1); t.x1 = min(t.x0 + 1, w - 1);
    t.fy = sy - (double)t.y0; t.fx = sx - (double)t.x0;
    return t;
}

// one grey level of the resized image from its four taps (a<row><column>): numpy's order of operations, rint, clamp to [0, 255]
__device__ __forceinline__ int blend(double a00, double a01, double a10, double a11, const Taps& t)
{
#pragma clang fp contract(off)
    const double gx = 1.0 - t.fx, gy = 1.0 - t.fy;
    const double t0 = a00 * gx, t1 = a01 * t.fx;
    const double top = t0 + t1;
    const double b0 = a10 * gx, b1 = a11 * t.fx;
    const double bot = b0 + b1;
    const double u0 = top * gy, u1 = bot * t.fy;
    const double v = fmin(fmax(rint(u0 + u1), 0.0), 255.0);
    return (int)v;
}

__device__ __forceinline__ float centred(int grey, double mean)
{
    return (float)((double)grey - mean);       // exact difference (both are doubles with few bits), one rounding to fp32
}

}  // namespace frames
