// The nearest geometry of finished frames, as results_u8.hip, labels_summary.hip, overlay_yuv.hip and the nearest form of confidence.hip all
// compute it.  The valid (unpadded) region of a map is out_h x out_w in its top-left corner, the source frame is h x w, and source pixel (y, x)
// takes map pixel
//     (min(y * out_h / h, out_h - 1), min(x * out_w / w, out_w - 1))            (integer division)
// which is dataset/cityscape._nearest_resize (the rule of the reference's evaluator, lib/dataset/cityscape.py:227) applied to the cropped region.
// Products of two sizes stay below 2^31: sizes are at most 32768 (checked by the callers, accel_io.cpp results_args).
// And the alignment predicate the launchers of these files and of scores_labels.hip choose their vector paths by.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nearest {

// the map column of source column x and the exact stepping to the columns after it: a thread that owns a few consecutive pixels of one row pays
// one division, then advances by out_w / w with the remainder carried (Bresenham)
struct Column {
    int sx, rem, qw, rw, w, last;
    __device__ __forceinline__ Column(int x, int out_w, int w_) : w(w_), last(out_w - 1)
    {
        const unsigned p = (unsigned)x * (unsigned)out_w;
        sx = (int)(p / (unsigned)w_);
        rem = (int)(p - (unsigned)sx * (unsigned)w_);
        qw = out_w / w_;
        rw = out_w - qw * w_;
    }
    __device__ __forceinline__ int col() const { return min(sx, last); }
    __device__ __forceinline__ void next()
    {
        sx += qw; rem += rw;
        if (rem >= w) { rem -= w; ++sx; }
    }
};

__device__ __forceinline__ int source_row(int y, int out_h, int h)
{
    return min((int)((unsigned)y * (unsigned)out_h / (unsigned)h), out_h - 1);
}

inline bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace nearest
