// uint8 video frames -> the fp32 image tensor the plans read (`data` / `data_key`): resize, mean subtraction and padding on the GPU.
//
// Restates accel_amd/utils/image.py (resize + transform, the project's statement of lib/utils/image.py:194-235 of the reference) per
// output pixel, bit for bit:
//   interior (y < out_h, x < out_w)   grey level = the source byte when step == 1, else the bilinear sample of _resize_bilinear:
//                                     float64, separately rounded operations in numpy's order, rint, clamp to [0, 255] -- the host
//                                     path resizes a uint8 image to a uint8 image, so the intermediate rounding is part of the contract
//   value stored in plane 2 - c       fp32(double(grey) - mean[c]) for source channel c in B, G, R order: ONE rounding, from float64
//                                     (an fp32 subtraction differs from it at a quarter to a half of the 256 grey levels)
//   padding                           fp32(0 - mean[c]): resize pads with zeros BEFORE transform removes the mean
// A bandwidth kernel: 3 bytes read and 12 written per pixel.  No range slot: the tensor is read by prep_rgb / prep_flow, which raise
// the slots of what they write.
#include "kernels.h"
#include "frames_resample.h"
#include <stdint.h>

namespace {

using frames::Means;
using frames::centred;

// One grey level of the resized image: _resize_bilinear of utils/image.py for channel c of output pixel (x, y), whose taps are `t`
// (frames_resample.h holds the arithmetic, shared with frames_yuv.h).
__device__ __forceinline__ int resample(const unsigned char* __restrict__ img, size_t pitch, const frames::Taps& t, int c)
{
    const unsigned char* r0 = img + (size_t)t.y0 * pitch + c;
    const unsigned char* r1 = img + (size_t)t.y1 * pitch + c;
    return frames::blend((double)r0[3 * t.x0], (double)r0[3 * t.x1], (double)r1[3 * t.x0], (double)r1[3 * t.x1], t);
}

// step == 1: a thread takes 4 consecutive pixels of a row.  FAST: w % 4 == 0, pitch % 4 == 0 and a 4-byte aligned source -- the 12
// source bytes are three dwords; VST: W % 4 == 0 and a 16-byte aligned destination -- one float4 store per plane.
template <bool FAST, bool VST>
__global__ __launch_bounds__(256) void frames_u8_copy_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, size_t pitch,
                                                             int H, int W, Means mean)
{
    const int QW = (W + 3) >> 2;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * H) return;
    const int y = (int)(q / QW), x0 = (int)(q - (long)y * QW) * 4;
    const unsigned char* img = src + (size_t)blockIdx.z * h * pitch;
    float* out = dst + (size_t)blockIdx.z * 3 * H * W + (size_t)y * W + x0;
    const size_t plane = (size_t)H * W;
    const float pad_b = centred(0, mean.b), pad_g = centred(0, mean.g), pad_r = centred(0, mean.r);
    float vb[4], vg[4], vr[4];
    if (FAST && y < h && x0 + 3 < w) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(img + (size_t)y * pitch + 3 * (size_t)x0);
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];      // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        vb[0] = centred(d0 & 255u, mean.b);         vg[0] = centred((d0 >> 8) & 255u, mean.g);  vr[0] = centred((d0 >> 16) & 255u, mean.r);
        vb[1] = centred(d0 >> 24, mean.b);          vg[1] = centred(d1 & 255u, mean.g);         vr[1] = centred((d1 >> 8) & 255u, mean.r);
        vb[2] = centred((d1 >> 16) & 255u, mean.b); vg[2] = centred(d1 >> 24, mean.g);          vr[2] = centred(d2 & 255u, mean.r);
        vb[3] = centred((d2 >> 8) & 255u, mean.b);  vg[3] = centred((d2 >> 16) & 255u, mean.g); vr[3] = centred(d2 >> 24, mean.r);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k;
            if (y < h && x < w) {
                const unsigned char* p = img + (size_t)y * pitch + 3 * (size_t)x;
                vb[k] = centred(p[0], mean.b); vg[k] = centred(p[1], mean.g); vr[k] = centred(p[2], mean.r);
            } else {
                vb[k] = pad_b; vg[k] = pad_g; vr[k] = pad_r;
            }
        }
    }
    if (VST) {
        *reinterpret_cast<float4*>(out) = make_float4(vr[0], vr[1], vr[2], vr[3]);
        *reinterpret_cast<float4*>(out + plane) = make_float4(vg[0], vg[1], vg[2], vg[3]);
        *reinterpret_cast<float4*>(out + 2 * plane) = make_float4(vb[0], vb[1], vb[2], vb[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < W) { out[k] = vr[k]; out[plane + k] = vg[k]; out[2 * plane + k] = vb[k]; }
    }
}

// step != 1: a gather, one output pixel per thread
__global__ __launch_bounds__(256) void frames_u8_resample_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, size_t pitch,
                                                                 int out_h, int out_w, double step, int H, int W, Means mean)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const unsigned char* img = src + (size_t)blockIdx.z * h * pitch;
    float* out = dst + (size_t)blockIdx.z * 3 * H * W + i;
    const size_t plane = (size_t)H * W;
    int b = 0, g = 0, r = 0;
    if (y < out_h && x < out_w) {
        const frames::Taps t = frames::taps(h, w, x, y, step);
        b = resample(img, pitch, t, 0);
        g = resample(img, pitch, t, 1);
        r = resample(img, pitch, t, 2);
    }
    out[0] = centred(r, mean.r);
    out[plane] = centred(g, mean.g);
    out[2 * plane] = centred(b, mean.b);
}

}  // namespace

// n frames of h x w x 3 uint8 BGR, `pitch` bytes per row, h * pitch bytes per frame -> n x 3 x H x W fp32 planar RGB.  The caller has
// checked the geometry (accel_io.cpp frame_u8_args): out_h <= H, out_w <= W, pitch >= 3 * w, and step == 1 only with out_h == h,
// out_w == w.  Reads stay inside h x w (the resampling coordinates are clamped), writes inside H x W.
hipError_t launch_frames_u8(const unsigned char* src, int n, int h, int w, size_t pitch, const double* means_bgr, int out_h, int out_w, double step,
                            int H, int W, float* dst, hipStream_t st)
{
    const Means mean = {means_bgr[0], means_bgr[1], means_bgr[2]};
    if (step == 1.0 && out_h == h && out_w == w) {
        const bool fast = w % 4 == 0 && pitch % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0;
        const bool vst = W % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
        const long quads = (long)((W + 3) / 4) * H;
        const dim3 grid((unsigned)((quads + 255) / 256), 1, (unsigned)n);
        if (fast && vst) hipLaunchKernelGGL((frames_u8_copy_kernel<true, true>), grid, dim3(256), 0, st, src, dst, h, w, pitch, H, W, mean);
        else if (vst) hipLaunchKernelGGL((frames_u8_copy_kernel<false, true>), grid, dim3(256), 0, st, src, dst, h, w, pitch, H, W, mean);
        else hipLaunchKernelGGL((frames_u8_copy_kernel<false, false>), grid, dim3(256), 0, st, src, dst, h, w, pitch, H, W, mean);
    } else {
        const long pixels = (long)H * W;
        hipLaunchKernelGGL(frames_u8_resample_kernel, dim3((unsigned)((pixels + 255) / 256), 1, (unsigned)n), dim3(256), 0, st,
                           src, dst, h, w, pitch, out_h, out_w, step, H, W, mean);
    }
    return hipGetLastError();
}
