// The taps of a bilinear interpolation of the scores to a source pixel, as scores_labels.hip and scores_confidence.hip both compute them: the
// restatement of accel_amd/utils/image.py interpolation_taps, bit for bit.
//
// Taps, in integer arithmetic (source row y of h rows over a region of out_h rows; columns alike with w, out_w):
//     num = clamp((2 * y + 1) * out_h - h, 0, 2 * h * (out_h - 1))           (< 2^31: sizes are at most 32768)
//     y0  = num / (2 * h);   y1 = min(y0 + 1, out_h - 1);   fy = double(num - 2 * h * y0) / double(2 * h)        ONE IEEE division
// which is the half-pixel-centre coordinate (y + 0.5) * out_h / h - 0.5 clamped to the region: the inverse of the resize the frame went
// through on the way in (frames_resample.h).  Taps never leave the valid region: the padding is never read.
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

}  // namespace interp
