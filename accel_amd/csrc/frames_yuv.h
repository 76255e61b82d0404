// What every route from YUV video frames shares: the formats and their layout, the colour rule, and the three kernel shapes -- frames -> the fp32
// image tensor the plans read (`data` / `data_key`) in one kernel (colour conversion, resize, mean subtraction, padding), and frames -> packed
// BGR bytes -- each written once over a SAMPLE SOURCE.  Only a source knows where the samples of a format lie and how chroma reaches a luma
// pixel; the sources are frames_yuv.hip (replicated chroma) and frames_sited.hip (interpolated chroma siting).  overlay_yuv.hip takes the
// formats, the layout and the patch shape from here.
//
// One frame (frame i starts at i * frame_bytes; bytes in the gaps -- between rows, between the planes, after a frame -- are never read):
//   I420   h rows of w luma bytes `pitch` apart from byte 0; at `u_offset` the Cb plane and at `v_offset` the Cr plane, each h/2 rows of w/2
//          bytes `pitch_c` apart.  h, w even.  (YV12: v_offset < u_offset.)
//   NV12   the same luma plane; at `u_offset` h/2 rows of w/2 (Cb, Cr) byte pairs, `pitch` apart as well (pitch_c = v_offset = 0).  h, w even.
//   P010   NV12's shape in little-endian 16-bit words: h rows of w luma words, at `u_offset` h/2 rows of w/2 (Cb, Cr) word pairs.  The sample is
//          word >> 6: the low six bits are never looked at.  h, w even; every word is 2-byte aligned.
//   YUY2   h rows `pitch` apart of w/2 quads Y0 Cb Y1 Cr.  w even.
//
// Restates accel_amd/utils/image.py bit for bit: transform(resize(yuv_to_bgr_host(frame, siting = s))) as fp32 (nv12_to_bgr_host for NV12).
//   colour      with c = Y - yoff, d = Cb - mid, e = Cr - mid in int32 and arithmetic right shifts
//                   R = clip((ky*c + krv*e         + half) >> shift, 0, 255)
//                   G = clip((ky*c - kgu*d - kgv*e + half) >> shift, 0, 255)
//                   B = clip((ky*c + kbu*d         + half) >> shift, 0, 255)
//               8-bit formats: mid = 128, shift = 16, (yoff, ky, krv, kgu, kgv, kbu) = nv12_coefficients; |accumulator| <= 3.6e7
//               P010: mid = 512, shift = 18, 4 * yoff and the other five of yuv10_coefficients; |accumulator| < 1.5e8
//               (both tables: frames_yuv.hip); half = 1 << (shift - 1)
//   interior    step == 1: those bytes; else each of the four taps of _resize_bilinear is converted to B, G, R bytes first and the float64
//               blend of frames_resample.h runs on them, as frames_u8.hip runs it on BGR bytes
//   value       fp32(double(grey) - mean[c]) in plane 2 - c; padding fp32(0 - mean[c])
// Bandwidth kernels, store-bound: 12 bytes written per pixel; 1.5 (I420, NV12), 2 (YUY2) or 3 (P010) read.  No range slot: the tensor is read by
// prep_rgb / prep_flow, which raise the slots of what they write.
#pragma once
#include "kernels.h"
#include "frames_resample.h"
#include <stdint.h>

namespace yuv {

using frames::Means;
using frames::centred;

enum { I420 = 0, P010 = 1, YUY2 = 2, NV12 = 3 };      // accel_yuv_layout.format (include/accel_hip.h)

struct Coef { int yoff, ky, krv, kgu, kgv, kbu; };      // yoff in the units of the samples (4 x the table's for P010)

struct Layout { size_t pitch, pitch_c, u_offset, v_offset, frame_bytes; };

// rows of the patch a thread of the step-1 kernel, of the byte converter and of the overlay owns: chroma is shared by two rows, or by none
template <int F> struct Patch { static constexpr int ROWS = F == YUY2 ? 1 : 2; };

// one pixel as B | G << 8 | R << 16
template <int F>
__device__ __forceinline__ uint32_t to_bgr(int Y, int cb, int cr, const Coef& k)
{
    constexpr int shift = F == P010 ? 18 : 16, mid = F == P010 ? 512 : 128;
    const int c = k.ky * (Y - k.yoff) + (1 << (shift - 1)), d = cb - mid, e = cr - mid;
    const int r = min(max((c + k.krv * e) >> shift, 0), 255);
    const int g = min(max((c - k.kgu * d - k.kgv * e) >> shift, 0), 255);
    const int b = min(max((c + k.kbu * d) >> shift, 0), 255);
    return (uint32_t)b | (uint32_t)g << 8 | (uint32_t)r << 16;
}

// a 10-bit sample: every word of a P010 frame is 2-byte aligned (accel_io.cpp yuv_layout_args)
__device__ __forceinline__ int word10(const unsigned char* p)
{
    return *reinterpret_cast<const uint16_t*>(p) >> 6;
}

inline bool coefficients(const YuvLayout& y, Coef& k)
{
    const int32_t* c = y.format == P010 ? yuv10_coefficients(y.colour) : nv12_coefficients(y.colour);
    if (!c) return false;
    k = {y.format == P010 ? 4 * c[0] : c[0], c[1], c[2], c[3], c[4], c[5]};
    return true;
}

// ---- the three kernel shapes over a sample source Src, which supplies ---------------------------------------------------------------------
//   ROWS                                            the rows of its patch (Patch<F>::ROWS)
//   patch<WIDE>(img, l, h, w, x0, y, k, px)         the 4-pixel x ROWS-row patch at (x0, y) -- x0 a multiple of 4, y a multiple of ROWS -- as
//                                                   B | G << 8 | R << 16 per pixel; pixels outside the h x w frame are left alone.  WIDE: the
//                                                   layout and the source address allow the source's wide loads of a whole patch (its
//                                                   predicate, handed to the launch functions below); a patch the frame's edge cuts (2 columns:
//                                                   w is even), and every patch without WIDE, is gathered sample by sample
//   pixel(img, l, h, w, x, y, k)                    pixel (x, y) of a frame, x < w and y < h, in the same form

// step == 1: a thread produces a 4-pixel x ROWS-row patch of the padded H x W tensor.  VST: W % 4 == 0 and a 16-byte aligned destination --
// three float4 stores per row; otherwise scalar stores with a row tail.
template <class Src, bool WIDE, bool VST>
__global__ __launch_bounds__(256) void frames_copy_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, Layout l, Coef k,
                                                          int H, int W, Means mean)
{
    constexpr int ROWS = Src::ROWS;
    const int QW = (W + 3) >> 2, QH = (H + ROWS - 1) / ROWS;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * QH) return;
    const int y = (int)(q / QW) * ROWS, x0 = (int)(q % QW) * 4;
    const unsigned char* img = src + (size_t)blockIdx.z * l.frame_bytes;
    const size_t plane = (size_t)H * W;
    const uint32_t none = 1u << 24;       // outside the frame: padding
    uint32_t px[ROWS][4];
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) px[j][i] = none;
    Src::template patch<WIDE>(img, l, h, w, x0, y, k, px);
    const float pad_b = centred(0, mean.b), pad_g = centred(0, mean.g), pad_r = centred(0, mean.r);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        if (y + j >= H) break;
        float vb[4], vg[4], vr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t p = px[j][i];
            const bool in = p != none;
            vb[i] = in ? centred(p & 255u, mean.b) : pad_b;
            vg[i] = in ? centred((p >> 8) & 255u, mean.g) : pad_g;
            vr[i] = in ? centred((p >> 16) & 255u, mean.r) : pad_r;
        }
        float* out = dst + (size_t)blockIdx.z * 3 * plane + (size_t)(y + j) * W + x0;
        if (VST) {
            *reinterpret_cast<float4*>(out) = make_float4(vr[0], vr[1], vr[2], vr[3]);
            *reinterpret_cast<float4*>(out + plane) = make_float4(vg[0], vg[1], vg[2], vg[3]);
            *reinterpret_cast<float4*>(out + 2 * plane) = make_float4(vb[0], vb[1], vb[2], vb[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < W) { out[i] = vr[i]; out[plane + i] = vg[i]; out[2 * plane + i] = vb[i]; }
        }
    }
}

// step != 1: a gather, one output pixel per thread; the four taps are converted to B, G, R bytes, then blended per channel
template <class Src>
__global__ __launch_bounds__(256) void frames_resample_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, Layout l,
                                                              Coef k, int out_h, int out_w, double step, int H, int W, Means mean)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const unsigned char* img = src + (size_t)blockIdx.z * l.frame_bytes;
    float* out = dst + (size_t)blockIdx.z * 3 * H * W + i;
    const size_t plane = (size_t)H * W;
    int b = 0, g = 0, r = 0;
    if (y < out_h && x < out_w) {
        const frames::Taps t = frames::taps(h, w, x, y, step);
        const uint32_t p00 = Src::pixel(img, l, h, w, t.x0, t.y0, k), p01 = Src::pixel(img, l, h, w, t.x1, t.y0, k);
        const uint32_t p10 = Src::pixel(img, l, h, w, t.x0, t.y1, k), p11 = Src::pixel(img, l, h, w, t.x1, t.y1, k);
        b = frames::blend((double)(p00 & 255u), (double)(p01 & 255u), (double)(p10 & 255u), (double)(p11 & 255u), t);
        g = frames::blend((double)((p00 >> 8) & 255u), (double)((p01 >> 8) & 255u), (double)((p10 >> 8) & 255u), (double)((p11 >> 8) & 255u), t);
        r = frames::blend((double)(p00 >> 16), (double)(p01 >> 16), (double)(p10 >> 16), (double)(p11 >> 16), t);
    }
    out[0] = centred(r, mean.r);
    out[plane] = centred(g, mean.g);
    out[2 * plane] = centred(b, mean.b);
}

// -> packed BGR bytes, a 4 x ROWS patch per thread.  VST: out_pitch % 4 == 0 and a 4-byte aligned destination -- the 12 bytes of a whole patch
// row are three dwords (B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3); otherwise byte stores.  Bytes between the rows of the destination are not written.
template <class Src, bool WIDE, bool VST>
__global__ __launch_bounds__(256) void to_bgr_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h, int w, Layout l,
                                                     Coef k, size_t out_pitch)
{
    constexpr int ROWS = Src::ROWS;
    const int QW = (w + 3) >> 2, QH = h / ROWS;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * QH) return;
    const int y = (int)(q / QW) * ROWS, x0 = (int)(q % QW) * 4;
    const unsigned char* img = src + (size_t)blockIdx.z * l.frame_bytes;
    uint32_t px[ROWS][4] = {};
    Src::template patch<WIDE>(img, l, h, w, x0, y, k, px);
    const int cols = min(4, w - x0);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        unsigned char* out = dst + ((size_t)blockIdx.z * h + y + j) * out_pitch + 3 * (size_t)x0;
        const uint32_t* p = px[j];
        if (VST && cols == 4) {
            uint32_t* o = reinterpret_cast<uint32_t*>(out);
            o[0] = p[0] | p[1] << 24;
            o[1] = p[1] >> 8 | p[2] << 16;
            o[2] = p[2] >> 16 | p[3] << 8;
        } else {
            for (int i = 0; i < cols; ++i) {
                out[3 * i] = (unsigned char)(p[i] & 255u);
                out[3 * i + 1] = (unsigned char)((p[i] >> 8) & 255u);
                out[3 * i + 2] = (unsigned char)(p[i] >> 16);
            }
        }
    }
}

// ---- the launch functions: `wide` is the source's predicate -- whether every whole patch of every frame may be read with its wide loads ------
typedef bool (*WidePredicate)(const unsigned char* src, const YuvLayout& y);

// n frames in device memory -> n x 3 x H x W fp32 planar RGB.  The caller has checked the layout and the geometry (accel_io.cpp frame_yuv_args):
// the format, the parity of h and w, the pitches, the plane offsets, frame_bytes >= the frame's extent, the 2-byte alignment of P010, colour in
// 0 .. 3, out_h <= H, out_w <= W, and step == 1 only with out_h == h, out_w == w.  Reads stay inside the planes of every frame (every chroma
// index and the resampling coordinates are clamped), writes inside H x W.
template <class Src>
hipError_t launch_frames(WidePredicate wide_loads, const unsigned char* src, int n, const YuvLayout& y, const double* means_bgr, int out_h, int out_w,
                         double step, int H, int W, float* dst, hipStream_t st)
{
    Coef k;
    if (!coefficients(y, k)) return hipErrorInvalidValue;
    const Layout l = {y.pitch, y.pitch_c, y.u_offset, y.v_offset, y.frame_bytes};
    const Means mean = {means_bgr[0], means_bgr[1], means_bgr[2]};
    const int h = y.h, w = y.w;
    if (step == 1.0 && out_h == h && out_w == w) {
        constexpr int ROWS = Src::ROWS;
        const bool wide = wide_loads(src, y);
        const bool vst = W % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
        const long patches = (long)((W + 3) / 4) * ((H + ROWS - 1) / ROWS);
        const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
        if (wide && vst) hipLaunchKernelGGL((frames_copy_kernel<Src, true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (vst) hipLaunchKernelGGL((frames_copy_kernel<Src, false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (wide) hipLaunchKernelGGL((frames_copy_kernel<Src, true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else hipLaunchKernelGGL((frames_copy_kernel<Src, false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
    } else {
        const long pixels = (long)H * W;
        hipLaunchKernelGGL(frames_resample_kernel<Src>, dim3((unsigned)((pixels + 255) / 256), 1, (unsigned)n), dim3(256), 0, st,
                           src, dst, h, w, l, k, out_h, out_w, step, H, W, mean);
    }
    return hipGetLastError();
}

// n frames in device memory -> n x h x w x 3 BGR bytes, rows `out_pitch` bytes apart (>= 3 * w), h * out_pitch from frame to frame
template <class Src>
hipError_t launch_to_bgr(WidePredicate wide_loads, const unsigned char* src, int n, const YuvLayout& y, unsigned char* dst, size_t out_pitch,
                         hipStream_t st)
{
    Coef k;
    if (!coefficients(y, k)) return hipErrorInvalidValue;
    const Layout l = {y.pitch, y.pitch_c, y.u_offset, y.v_offset, y.frame_bytes};
    const int h = y.h, w = y.w;
    const bool wide = wide_loads(src, y);
    const bool vst = out_pitch % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    const long patches = (long)((w + 3) / 4) * (h / Src::ROWS);
    const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
    if (wide && vst) hipLaunchKernelGGL((to_bgr_kernel<Src, true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (vst) hipLaunchKernelGGL((to_bgr_kernel<Src, false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (wide) hipLaunchKernelGGL((to_bgr_kernel<Src, true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else hipLaunchKernelGGL((to_bgr_kernel<Src, false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    return hipGetLastError();
}

// the replicated sources of formats 0 .. 3 (frames_yuv.hip), which launch_frames_yuv / launch_yuv_to_bgr (frames_sited.hip) call for siting 0
hipError_t frames_replicated(const unsigned char* src, int n, const YuvLayout& y, const double* means_bgr, int out_h, int out_w, double step,
                             int H, int W, float* dst, hipStream_t st);
hipError_t replicated_to_bgr(const unsigned char* src, int n, const YuvLayout& y, unsigned char* dst, size_t out_pitch, hipStream_t st);

}  // namespace yuv
