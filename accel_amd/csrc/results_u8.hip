// The output side of a frame on the GPU: the `labels` map (n x H x W uint8, written by score_tail_kernel) taken back to the SOURCE frame's
// size and finished there -- as labels, as a confusion matrix against ground truth, or as a colour image.
//
// One geometry for the three kernels.  The valid (unpadded) region of a label map is out_h x out_w in its top-left corner; the source
// frame is h x w; source pixel (y, x) takes
//     labels[min(y * out_h / h, out_h - 1)][min(x * out_w / w, out_w - 1)]            (integer division)
// which is dataset/cityscape._nearest_resize (the rule of the reference's evaluator, lib/dataset/cityscape.py:227) applied to the
// cropped region, and the crop itself when h x w == out_h x out_w (IDENT: dword or wider loads and stores where widths, pitches and
// addresses allow).  A thread owns a few consecutive pixels of one row, so the column index costs one division per thread: it advances by
// out_w / w with the remainder carried (Bresenham).  Everything is integer arithmetic on bytes: every result has one correct value.
// Bandwidth kernels: bytes in + bytes out.  They only READ `labels`.
#include "kernels.h"
#include "labels_nearest.h"
#include <stdint.h>

namespace {

using nearest::Column;
using nearest::source_row;
using nearest::aligned;

// ---- labels at the source size -------------------------------------------------------------------------------------------------------
// A thread takes V consecutive pixels of one destination row.  IDENT with V = 16 / 4: one uint4 / dword load and store (the launcher has
// checked w % V == 0 and the alignment of both rows); IDENT with V = 1: bytes.  Not IDENT: V = 4 gathered bytes, stored as one dword when
// VST (w % 4 == 0, aligned destination rows), else byte by byte with a tail.
template <int V, bool IDENT, bool VST>
__global__ __launch_bounds__(256) void labels_source_kernel(const unsigned char* __restrict__ labels, int H, int W, int out_h, int out_w, int h, int w,
                                                            unsigned char* __restrict__ dst, size_t dst_pitch)
{
    const int QW = (w + V - 1) / V;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * h) return;
    const int y = (int)(q / QW), x0 = (int)(q - (long)y * QW) * V;
    const unsigned char* row = labels + (size_t)blockIdx.z * H * W + (size_t)(IDENT ? y : source_row(y, out_h, h)) * W;
    unsigned char* out = dst + ((size_t)blockIdx.z * h + y) * dst_pitch + x0;
    if (IDENT) {
        if (V == 16) *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(row + x0);
        else if (V == 4) *reinterpret_cast<uint32_t*>(out) = *reinterpret_cast<const uint32_t*>(row + x0);
        else out[0] = row[x0];
    } else {
        Column c(x0, out_w, w);
        unsigned v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { v[k] = row[c.col()]; c.next(); }      // (columns past w - 1 are clamped into the row: read, not stored)
        if (VST && V == 4) {
            *reinterpret_cast<uint32_t*>(out) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (x0 + k < w) out[k] = (unsigned char)v[k];
        }
    }
}

// ---- confusion matrix ----------------------------------------------------------------------------------------------------------------
// hist[gt * ncls + pred] += 1 for every source pixel with gt < ncls and pred < ncls (demo.fast_hist: rows ground truth, columns prediction;
// 255 and every other id >= ncls are ignored).  A segmentation map is long runs of ONE (gt, pred) pair, so the counts are aggregated
// before they meet an atomic:
//   1. a thread walks units of 16 consecutive pixels of a row (grid stride) and counts the run of its current key in a register; only a
//      change of key sends the finished run to LDS
//   2. at the end the wavefront looks at the leader's key: when every lane holds that key -- the realistic case -- the counts are summed
//      across the wave and ONE lane adds them; otherwise each lane adds its own
//   3. a block-private LDS table of 32-bit bins (a block sees fewer than 2^32 pixels: the launcher sizes the grid for it)
//   4. one 64-bit device-scope atomic add per non-zero bin per block into the persistent accumulator
// Integer sums: the result does not depend on the order of arrival.
// GV: the ground-truth rows allow uint4 loads (pitch % 16 == 0, 16-byte aligned base); PV: IDENT and the label rows do (W % 16 == 0,
// aligned base).  Units that cross the end of a row, and everything else, go byte by byte.
template <bool IDENT, bool GV, bool PV>
__global__ __launch_bounds__(256) void labels_hist_kernel(const unsigned char* __restrict__ labels, int H, int W, int out_h, int out_w,
                                                          const unsigned char* __restrict__ gt, int n, int h, int w, size_t gt_pitch, int ncls,
                                                          unsigned long long* __restrict__ hist)
{
    __shared__ unsigned bins[32 * 32];
    const int nb = ncls * ncls;
    for (int i = threadIdx.x; i < nb; i += 256) bins[i] = 0;
    __syncthreads();

    const unsigned uncls = (unsigned)ncls;
    unsigned key = 0, cnt = 0;
    auto feed = [&](unsigned g, unsigned p) {
        if (g < uncls && p < uncls) {
            const unsigned k = g * uncls + p;
            if (k == key) {
                ++cnt;
            } else {
                if (cnt) atomicAdd(&bins[key], cnt);
                key = k; cnt = 1;
            }
        }
    };

    const int UW = (w + 15) >> 4;
    const long per_image = (long)UW * h, units = per_image * n;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
        const int z = (int)(u / per_image);
        const int r = (int)(u - (long)z * per_image);
        const int y = r / UW, x0 = (r - y * UW) << 4;
        const unsigned char* g = gt + ((size_t)z * h + y) * gt_pitch + x0;
        const unsigned char* row = labels + (size_t)z * H * W + (size_t)(IDENT ? y : source_row(y, out_h, h)) * W;
        const bool full = x0 + 16 <= w;
        if (GV && full && (!IDENT || PV)) {
            const uint4 gv = *reinterpret_cast<const uint4*>(g);
            const unsigned gw[4] = {gv.x, gv.y, gv.z, gv.w};
            if (IDENT) {
                const uint4 pv = *reinterpret_cast<const uint4*>(row + x0);
                const unsigned pw[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) feed((gw[k >> 2] >> (8 * (k & 3))) & 255u, (pw[k >> 2] >> (8 * (k & 3))) & 255u);
            } else {
                Column c(x0, out_w, w);
#pragma unroll
                for (int k = 0; k < 16; ++k) { feed((gw[k >> 2] >> (8 * (k & 3))) & 255u, row[c.col()]); c.next(); }
            }
        } else {
            Column c(x0, out_w, w);
            const int m = min(16, w - x0);
            for (int k = 0; k < m; ++k) { feed(g[k], IDENT ? row[x0 + k] : row[c.col()]); c.next(); }
        }
    }

    // the run every lane still holds: one add for the wavefront when it is the same run in all of them
    const unsigned lk = __builtin_amdgcn_readfirstlane(key);
    if (!cnt) key = lk;       // a lane that counted nothing agrees with anyone
    if (__all(key == lk)) {
        unsigned s = cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&bins[lk], s);
    } else if (cnt) {
        atomicAdd(&bins[key], cnt);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        const unsigned v = bins[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

// ---- colour image ----------------------------------------------------------------------------------------------------------------------
// out = palette[label] (256 x 3 RGB, passed BY VALUE: 768 bytes of kernel argument, no allocation, ordered with the stream for free),
// written in B, G, R order (what the frames are) or R, G, B (what PIL wants).  With a frame (h x w x 3 BGR, pitched) every channel is
// (alpha * colour + (256 - alpha) * frame + 128) >> 8.  The block packs the table into LDS once (one entry per thread, already in the
// output's channel order); a thread takes 4 consecutive pixels = 12 bytes = three dwords when VEC (w % 4 == 0, destination and frame rows
// 4-byte aligned).
struct Palette { unsigned char rgb[768]; };

template <bool IDENT, bool VEC, bool BLEND>
__global__ __launch_bounds__(256) void labels_colour_kernel(const unsigned char* __restrict__ labels, int H, int W, int out_h, int out_w, int h, int w,
                                                            const Palette pal, int rgb_order, const unsigned char* __restrict__ frame,
                                                            size_t frame_pitch, int alpha, unsigned char* __restrict__ dst, size_t dst_pitch, int label_dword)
{
    __shared__ unsigned table[256];
    {
        const unsigned r = pal.rgb[3 * threadIdx.x], g = pal.rgb[3 * threadIdx.x + 1], b = pal.rgb[3 * threadIdx.x + 2];
        table[threadIdx.x] = rgb_order ? (r | (g << 8) | (b << 16)) : (b | (g << 8) | (r << 16));
    }
    __syncthreads();
    const int QW = (w + 3) >> 2;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * h) return;
    const int y = (int)(q / QW), x0 = (int)(q - (long)y * QW) * 4;
    const unsigned char* row = labels + (size_t)blockIdx.z * H * W + (size_t)(IDENT ? y : source_row(y, out_h, h)) * W;
    unsigned char* out = dst + ((size_t)blockIdx.z * h + y) * dst_pitch + 3 * (size_t)x0;
    const unsigned char* fr = BLEND ? frame + ((size_t)blockIdx.z * h + y) * frame_pitch + 3 * (size_t)x0 : nullptr;
    unsigned char o[12];
    Column c(x0, out_w, w);
    // IDENT, w % 4 == 0 and 4-byte aligned label rows (label_dword, uniform): the four labels are one dword
    const uint32_t four = IDENT && label_dword ? *reinterpret_cast<const uint32_t*>(row + x0) : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned lab = !IDENT ? row[c.col()] : label_dword ? (four >> (8 * k)) & 255u : row[min(x0 + k, w - 1)];
        const unsigned v = table[lab];
        c.next();
        o[3 * k] = (unsigned char)(v & 255u); o[3 * k + 1] = (unsigned char)((v >> 8) & 255u); o[3 * k + 2] = (unsigned char)((v >> 16) & 255u);
    }
    if (BLEND) {
        unsigned char f[12];
        if (VEC) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(fr);
            const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int k = 0; k < 12; ++k) f[k] = (unsigned char)((d[k >> 2] >> (8 * (k & 3))) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) f[k] = x0 + k / 3 < w ? fr[k] : (unsigned char)0;
        }
        const unsigned a = (unsigned)alpha, ia = 256u - a;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const unsigned fv = f[3 * k + (rgb_order ? 2 - ch : ch)];       // the frame is B, G, R
                o[3 * k + ch] = (unsigned char)((a * o[3 * k + ch] + ia * fv + 128u) >> 8);
            }
    }
    if (VEC) {
        uint32_t* p = reinterpret_cast<uint32_t*>(out);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            p[j] = (uint32_t)o[4 * j] | ((uint32_t)o[4 * j + 1] << 8) | ((uint32_t)o[4 * j + 2] << 16) | ((uint32_t)o[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (x0 + k / 3 < w) out[k] = o[k];
    }
}

}  // namespace

// The callers (accel_io.cpp results_args) have checked: n, h, w >= 1, 1 <= out_h <= H, 1 <= out_w <= W <= 32768, h, w <= 32768, pitches >= a row.
// Reads of `labels` stay inside out_h x out_w of each of the n maps (row and column indices are clamped), reads of gt / frame and writes of dst
// inside w (3 * w) bytes of each of the n * h rows.
hipError_t launch_labels_source(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, int h, int w, unsigned char* dst, size_t dst_pitch,
                                hipStream_t st)
{
#define SRC_LAUNCH(V, IDENT, VST)                                                                                                            \
    hipLaunchKernelGGL((labels_source_kernel<V, IDENT, VST>), dim3((unsigned)(((long)((w + V - 1) / V) * h + 255) / 256), 1, (unsigned)n), \
                       dim3(256), 0, st, labels, H, W, out_h, out_w, h, w, dst, dst_pitch)
    if (h == out_h && w == out_w) {
        if (w % 16 == 0 && W % 16 == 0 && dst_pitch % 16 == 0 && aligned(labels, 16) && aligned(dst, 16)) SRC_LAUNCH(16, true, true);
        else if (w % 4 == 0 && W % 4 == 0 && dst_pitch % 4 == 0 && aligned(labels, 4) && aligned(dst, 4)) SRC_LAUNCH(4, true, true);
        else SRC_LAUNCH(1, true, false);
    } else if (w % 4 == 0 && dst_pitch % 4 == 0 && aligned(dst, 4)) {
        SRC_LAUNCH(4, false, true);
    } else {
        SRC_LAUNCH(4, false, false);
    }
#undef SRC_LAUNCH
    return hipGetLastError();
}

hipError_t launch_labels_hist(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, const unsigned char* gt, int h, int w, size_t gt_pitch,
                              int ncls, unsigned long long* hist, hipStream_t st)
{
    const long units = (long)((w + 15) / 16) * h * n;
    // enough blocks to fill the chip several times over, few enough that the 64-bit atomics of their epilogues stay a footnote; and never
    // 2^32 pixels in one block (32-bit LDS bins)
    long blocks = (units + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const long pixels = (long)n * h * w, floor_blocks = pixels / (1L << 31) + 1;
    if (blocks < floor_blocks) blocks = floor_blocks;
    const bool ident = h == out_h && w == out_w;
    const bool gv = gt_pitch % 16 == 0 && aligned(gt, 16);
    const bool pv = ident && W % 16 == 0 && aligned(labels, 16);
#define HIST_LAUNCH(IDENT, GV, PV)                                                                                                       \
    hipLaunchKernelGGL((labels_hist_kernel<IDENT, GV, PV>), dim3((unsigned)blocks), dim3(256), 0, st, labels, H, W, out_h, out_w, gt, n, h, w, \
                       gt_pitch, ncls, hist)
    if (ident && gv && pv) HIST_LAUNCH(true, true, true);
    else if (ident) HIST_LAUNCH(true, false, false);
    else if (gv) HIST_LAUNCH(false, true, false);
    else HIST_LAUNCH(false, false, false);
#undef HIST_LAUNCH
    return hipGetLastError();
}

hipError_t launch_labels_colour(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, int h, int w, const unsigned char* palette_rgb,
                                int rgb_order, const unsigned char* frame, size_t frame_pitch, int alpha, unsigned char* dst, size_t dst_pitch, hipStream_t st)
{
    Palette pal;
    for (int i = 0; i < 768; ++i) pal.rgb[i] = palette_rgb[i];
    const bool blend = frame != nullptr && alpha < 256;
    const bool ident = h == out_h && w == out_w;
    const bool vec = w % 4 == 0 && dst_pitch % 4 == 0 && aligned(dst, 4) && (!blend || (frame_pitch % 4 == 0 && aligned(frame, 4)));
    const int label_dword = ident && w % 4 == 0 && W % 4 == 0 && aligned(labels, 4);
    const dim3 grid((unsigned)(((long)((w + 3) / 4) * h + 255) / 256), 1, (unsigned)n);
#define COL_LAUNCH(IDENT, VEC, BLEND)                                                                                                  \
    hipLaunchKernelGGL((labels_colour_kernel<IDENT, VEC, BLEND>), grid, dim3(256), 0, st, labels, H, W, out_h, out_w, h, w, pal, rgb_order, \
                       frame, frame_pitch, alpha, dst, dst_pitch, label_dword)
    if (ident) {
        if (vec) { if (blend) COL_LAUNCH(true, true, true); else COL_LAUNCH(true, true, false); }
        else { if (blend) COL_LAUNCH(true, false, true); else COL_LAUNCH(true, false, false); }
    } else {
        if (vec) { if (blend) COL_LAUNCH(false, true, true); else COL_LAUNCH(false, true, false); }
        else { if (blend) COL_LAUNCH(false, false, true); else COL_LAUNCH(false, false, false); }
    }
#undef COL_LAUNCH
    return hipGetLastError();
}
