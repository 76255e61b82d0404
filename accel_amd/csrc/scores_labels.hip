// Labels at the source frame's size from bilinearly INTERPOLATED scores: the scores tensor (n x NCLS x H x W fp32, NCHW, the layout of
// `logits`) is read where it lies, every class plane is interpolated to the source pixel and the argmax is taken there -- the usual practice
// of semantic segmentation, where results_u8.hip copies the finished label of the nearest map pixel.  A byte per source pixel is written.
//
// The geometry vocabulary is that of results_u8.hip and confidence.hip: one valid region out_h x out_w in the top-left corner of the H x W
// map, one source size h x w.  The arithmetic restates accel_amd/utils/image.py labels_interpolated_host bit for bit.
//
// Taps, their loads and the blend: scores_interp.h (integer taps clamped to the valid region -- the padding is never read -- one IEEE division
// per weight, a float64 blend with each operation rounded on its own), shared with the interpolated form of confidence.hip.
// Label: the first k with the largest v_k (ascending scan, strict >): the tie rule of `labels`.
// At h x w == out_h x out_w, fx = fy = 0 and v_k is the stored score: the result is the crop of `labels`.
// Scores are assumed FINITE: a pixel with a non-finite tap is unspecified (inf * 0 arises in the blend).
//
// V = 1: one source pixel per thread; consecutive lanes take consecutive x of one row, so the taps of a wavefront are contiguous runs of
// each class plane (overlapping when the map is scaled up: served by the caches).  All NCLS x 4 tap loads are issued before the compare
// chain.  V = 4: the identity geometry with widths, pitches and addresses allowing (the launcher checks): one 16-byte load per class plane,
// an fp32 compare chain (the blend is the identity there) and one dword store of four labels.
// Grid-stride loop, no LDS, no atomics.  blockIdx.z is the frame.  The kernel only READS the scores.
#include "kernels.h"
#include "labels_nearest.h"
#include "scores_interp.h"
#include <stdint.h>

namespace {

using nearest::aligned;

template <int NCLS, int V>
__global__ __launch_bounds__(256) void scores_labels_kernel(const float* __restrict__ scores, int H, int W, int out_h, int out_w, int h, int w,
                                                            unsigned char* __restrict__ dst, size_t dst_pitch)
{
    const int z = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const float* img = scores + (size_t)z * NCLS * plane;
    const int QW = w / V;                          // V = 4: w % 4 == 0
    const long units = (long)QW * h;

    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
        const int y = (int)(u / QW), x0 = (int)(u - (long)y * QW) * V;
        unsigned char* out = dst + ((size_t)z * h + y) * dst_pitch + x0;
        if (V == 4) {
            const float* p = img + (size_t)y * W + x0;
            float4 t[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) t[k] = *reinterpret_cast<const float4*>(p + (size_t)k * plane);
            unsigned lab[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned best = 0;
                float bv = j == 0 ? t[0].x : j == 1 ? t[0].y : j == 2 ? t[0].z : t[0].w;
#pragma unroll
                for (int k = 1; k < NCLS; ++k) {
                    const float v = j == 0 ? t[k].x : j == 1 ? t[k].y : j == 2 ? t[k].z : t[k].w;
                    if (v > bv) { bv = v; best = (unsigned)k; }
                }
                lab[j] = best;
            }
            *reinterpret_cast<uint32_t*>(out) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
        } else {
            const interp::Tap ty = interp::tap(y, h, out_h), tx = interp::tap(x0, w, out_w);
            const float* r0 = img + (size_t)ty.i0 * W;
            const float* r1 = img + (size_t)ty.i1 * W;
            interp::Taps a[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) a[k] = interp::load_taps(r0, r1, (size_t)k * plane, tx.i0, tx.i1);
            const interp::Weights wt(ty, tx);
            unsigned best = 0;
            double bv = 0.0;
#pragma unroll
            for (int k = 0; k < NCLS; ++k) {
                const double v = interp::blend(a[k], wt);
                if (k == 0 || v > bv) { bv = v; best = (unsigned)k; }
            }
            out[0] = (unsigned char)best;
        }
    }
}

template <int NCLS>
hipError_t launch_ncls(const float* scores, int n, int H, int W, int out_h, int out_w, int h, int w, unsigned char* dst, size_t dst_pitch, hipStream_t st)
{
    const bool vec = h == out_h && w == out_w && w % 4 == 0 && W % 4 == 0 && aligned(scores, 16) && dst_pitch % 4 == 0 && aligned(dst, 4);
    const long units = (long)(vec ? w / 4 : w) * h;
    // enough blocks per frame to fill the chip; the grid-stride loop takes the rest
    long blocks = (units + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks, 1, (unsigned)n);
    if (vec) hipLaunchKernelGGL((scores_labels_kernel<NCLS, 4>), grid, dim3(256), 0, st, scores, H, W, out_h, out_w, h, w, dst, dst_pitch);
    else hipLaunchKernelGGL((scores_labels_kernel<NCLS, 1>), grid, dim3(256), 0, st, scores, H, W, out_h, out_w, h, w, dst, dst_pitch);
    return hipGetLastError();
}

}  // namespace

// The callers (accel_io.cpp scores_labels_args) have checked: 1 <= n <= 32768, h, w >= 1, 1 <= out_h <= H, 1 <= out_w <= W <= 32768, h, w <= 32768,
// ncls in {2, 19, 21}, dst_pitch >= w.  Reads of `scores` stay inside out_h x out_w of each of the n * ncls planes (both taps of a row and of a
// column are clamped into the region), writes inside the first w bytes of each of the n * h rows of dst.
hipError_t launch_scores_labels(const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, unsigned char* dst, size_t dst_pitch,
                                hipStream_t st)
{
    switch (ncls) {
    case 2: return launch_ncls<2>(scores, n, H, W, out_h, out_w, h, w, dst, dst_pitch, st);
    case 19: return launch_ncls<19>(scores, n, H, W, out_h, out_w, h, w, dst, dst_pitch, st);
    case 21: return launch_ncls<21>(scores, n, H, W, out_h, out_w, h, w, dst, dst_pitch, st);
    }
    return hipErrorInvalidValue;
}
