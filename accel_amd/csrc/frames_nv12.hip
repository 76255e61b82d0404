// NV12 video frames -- what a hardware or software decoder hands out -- -> the fp32 image tensor the plans read (`data` / `data_key`), in one
// kernel: colour conversion, resize, mean subtraction and padding.  And -> packed BGR bytes, for viewers and for the finishing kernels.
//
// One frame: h rows of w luma bytes, `pitch` bytes apart, from byte 0; at byte `uv_offset` h/2 rows of w/2 (Cb, Cr) byte pairs at the same pitch;
// frame i starts at i * frame_bytes.  h and w are even.  Bytes in the gaps (between rows, between the planes, after a frame) are never read.
//
// Restates accel_amd/utils/image.py bit for bit: transform(resize(nv12_to_bgr_host(frame))) as fp32.
//   colour      pixel (x, y) takes Y at (x, y) and Cb, Cr at (x >> 1, y >> 1) (replicated chroma); with c = Y - yoff, d = Cb - 128, e = Cr - 128
//               in int32 and arithmetic right shifts
//                   R = clip((ky*c + krv*e         + 32768) >> 16, 0, 255)
//                   G = clip((ky*c - kgu*d - kgv*e + 32768) >> 16, 0, 255)
//                   B = clip((ky*c + kbu*d         + 32768) >> 16, 0, 255)
//               (yoff, ky, krv, kgu, kgv, kbu) = round(65536 x the standard's value) for BT.601 / BT.709, limited / full range: NV12_COEF below,
//               held to image.nv12_coefficients by the CPU suite.  |accumulator| <= 3.6e7.
//   interior    step == 1: those bytes; else each of the four taps of _resize_bilinear is converted to B, G, R bytes first and the float64
//               blend of frames_resample.h runs on them, as frames_u8.hip runs it on BGR bytes
//   value       fp32(double(grey) - mean[c]) in plane 2 - c; padding fp32(0 - mean[c])
// Bandwidth kernels: 1.5 bytes read and 12 written per pixel.  No range slot: the tensor is read by prep_rgb / prep_flow, which raise the
// slots of what they write.
#include "kernels.h"
#include "frames_resample.h"
#include <stdint.h>

namespace {

using frames::Means;
using frames::centred;

struct Coef { int yoff, ky, krv, kgu, kgv, kbu; };

//                                 yoff  ky     krv     kgu    kgv    kbu
const int32_t NV12_COEF[4][6] = {{16, 76309, 104597, 25675, 53279, 132201},      // 0  BT.601 limited range
                                 {0,  65536, 91881,  22553, 46802, 116130},      // 1  BT.601 full range
                                 {16, 76309, 117489, 13975, 34925, 138438},      // 2  BT.709 limited range
                                 {0,  65536, 103206, 12276, 30679, 121609}};     // 3  BT.709 full range

struct Layout { size_t pitch, uv_offset, frame_bytes; };

// one pixel as B | G << 8 | R << 16
__device__ __forceinline__ uint32_t to_bgr(int Y, int cb, int cr, const Coef& k)
{
    const int c = k.ky * (Y - k.yoff) + 32768, d = cb - 128, e = cr - 128;
    const int r = min(max((c + k.krv * e) >> 16, 0), 255);
    const int g = min(max((c - k.kgu * d - k.kgv * e) >> 16, 0), 255);
    const int b = min(max((c + k.kbu * d) >> 16, 0), 255);
    return (uint32_t)b | (uint32_t)g << 8 | (uint32_t)r << 16;
}

__device__ __forceinline__ uint32_t pixel_bgr(const unsigned char* __restrict__ img, const Layout& l, int x, int y, const Coef& k)
{
    const unsigned char* uv = img + l.uv_offset + (size_t)(y >> 1) * l.pitch + (x & ~1);
    return to_bgr(img[(size_t)y * l.pitch + x], uv[0], uv[1], k);
}

// The 4-pixel x 2-row patch at (x0, y) -- x0 a multiple of 4, y even -- as B | G << 8 | R << 16 per pixel; pixels outside the h x w frame are
// left alone.  h and w are even, so both rows, and both pixels of a chroma pair, are inside or outside together.  DW: pitch, uv_offset,
// frame_bytes and the source address are multiples of 4 -- a whole patch is two luma dwords and one chroma dword (Cb0 Cr0 Cb1 Cr1), each chroma
// byte read once; a patch the frame's edge cuts, and every patch without DW, is gathered from bytes into the same three dwords.
template <bool DW>
__device__ __forceinline__ void patch_bgr(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x0, int y, const Coef& k, uint32_t (&px)[2][4])
{
    if (y >= h || x0 >= w) return;
    const unsigned char* y0 = img + (size_t)y * l.pitch + x0;
    const unsigned char* y1 = y0 + l.pitch;
    const unsigned char* uv = img + l.uv_offset + (size_t)(y >> 1) * l.pitch + x0;
    uint32_t l0 = 0, l1 = 0, c = 0;
    const int cols = min(4, w - x0);      // 4 or 2
    if (DW && cols == 4) {
        l0 = *reinterpret_cast<const uint32_t*>(y0);
        l1 = *reinterpret_cast<const uint32_t*>(y1);
        c = *reinterpret_cast<const uint32_t*>(uv);
    } else {
        for (int i = 0; i < cols; ++i) {
            l0 |= (uint32_t)y0[i] << (8 * i);
            l1 |= (uint32_t)y1[i] << (8 * i);
            c |= (uint32_t)uv[i] << (8 * i);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < cols) {
            const int cb = (c >> (16 * (i >> 1))) & 255u, cr = (c >> (16 * (i >> 1) + 8)) & 255u;
            px[0][i] = to_bgr((l0 >> (8 * i)) & 255u, cb, cr, k);
            px[1][i] = to_bgr((l1 >> (8 * i)) & 255u, cb, cr, k);
        }
    }
}

// step == 1: a thread produces a 4-pixel x 2-row patch of the padded H x W tensor.  VST: W % 4 == 0 and a 16-byte aligned destination -- six
// float4 stores; otherwise scalar stores with a row tail.
template <bool DW, bool VST>
__global__ __launch_bounds__(256) void frames_nv12_copy_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, Layout l,
                                                               Coef k, int H, int W, Means mean)
{
    const int QW = (W + 3) >> 2, QH = (H + 1) >> 1;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * QH) return;
    const int y = (int)(q / QW) * 2, x0 = (int)(q % QW) * 4;
    const unsigned char* img = src + (size_t)blockIdx.z * l.frame_bytes;
    const size_t plane = (size_t)H * W;
    const uint32_t none = 1u << 24;       // outside the frame: padding
    uint32_t px[2][4] = {{none, none, none, none}, {none, none, none, none}};
    patch_bgr<DW>(img, l, h, w, x0, y, k, px);
    const float pad_b = centred(0, mean.b), pad_g = centred(0, mean.g), pad_r = centred(0, mean.r);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
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
__global__ __launch_bounds__(256) void frames_nv12_resample_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, Layout l,
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
        const uint32_t p00 = pixel_bgr(img, l, t.x0, t.y0, k), p01 = pixel_bgr(img, l, t.x1, t.y0, k);
        const uint32_t p10 = pixel_bgr(img, l, t.x0, t.y1, k), p11 = pixel_bgr(img, l, t.x1, t.y1, k);
        b = frames::blend((double)(p00 & 255u), (double)(p01 & 255u), (double)(p10 & 255u), (double)(p11 & 255u), t);
        g = frames::blend((double)((p00 >> 8) & 255u), (double)((p01 >> 8) & 255u), (double)((p10 >> 8) & 255u), (double)((p11 >> 8) & 255u), t);
        r = frames::blend((double)(p00 >> 16), (double)(p01 >> 16), (double)(p10 >> 16), (double)(p11 >> 16), t);
    }
    out[0] = centred(r, mean.r);
    out[plane] = centred(g, mean.g);
    out[2 * plane] = centred(b, mean.b);
}

// NV12 -> packed BGR bytes, a 4 x 2 patch per thread.  VST: out_pitch % 4 == 0 and a 4-byte aligned destination -- the 12 bytes of a whole patch
// row are three dwords (B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3); otherwise byte stores.  Bytes between the rows of the destination are not written.
template <bool DW, bool VST>
__global__ __launch_bounds__(256) void nv12_to_bgr_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h, int w, Layout l,
                                                          Coef k, size_t out_pitch)
{
    const int QW = (w + 3) >> 2, QH = h >> 1;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * QH) return;
    const int y = (int)(q / QW) * 2, x0 = (int)(q % QW) * 4;
    const unsigned char* img = src + (size_t)blockIdx.z * l.frame_bytes;
    uint32_t px[2][4] = {};
    patch_bgr<DW>(img, l, h, w, x0, y, k, px);
    const int cols = min(4, w - x0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
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

bool dwords(const unsigned char* src, size_t pitch, size_t uv_offset, size_t frame_bytes)
{
    return pitch % 4 == 0 && uv_offset % 4 == 0 && frame_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0;
}

}  // namespace

const int32_t* nv12_coefficients(int colour)
{
    return colour >= 0 && colour < 4 ? NV12_COEF[colour] : nullptr;
}

// n NV12 frames in device memory -> n x 3 x H x W fp32 planar RGB.  The caller has checked the layout and the geometry (accel_io.cpp
// frame_nv12_args): h, w even, pitch >= w, uv_offset >= h * pitch, frame_bytes >= uv_offset + (h / 2) * pitch, colour in 0 .. 3, out_h <= H,
// out_w <= W, and step == 1 only with out_h == h, out_w == w.  Reads stay inside the two planes of every frame (the resampling coordinates
// are clamped), writes inside H x W.  A width with w % 4 == 2 keeps the dword loads: only the patch the frame's edge cuts reads bytes.
hipError_t launch_frames_nv12(const unsigned char* src, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                              const double* means_bgr, int out_h, int out_w, double step, int H, int W, float* dst, hipStream_t st)
{
    const int32_t* c = nv12_coefficients(colour);
    if (!c) return hipErrorInvalidValue;
    const Coef k = {c[0], c[1], c[2], c[3], c[4], c[5]};
    const Layout l = {pitch, uv_offset, frame_bytes};
    const Means mean = {means_bgr[0], means_bgr[1], means_bgr[2]};
    if (step == 1.0 && out_h == h && out_w == w) {
        const bool dw = dwords(src, pitch, uv_offset, frame_bytes);
        const bool vst = W % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
        const long patches = (long)((W + 3) / 4) * ((H + 1) / 2);
        const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
        if (dw && vst) hipLaunchKernelGGL((frames_nv12_copy_kernel<true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (vst) hipLaunchKernelGGL((frames_nv12_copy_kernel<false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (dw) hipLaunchKernelGGL((frames_nv12_copy_kernel<true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else hipLaunchKernelGGL((frames_nv12_copy_kernel<false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
    } else {
        const long pixels = (long)H * W;
        hipLaunchKernelGGL(frames_nv12_resample_kernel, dim3((unsigned)((pixels + 255) / 256), 1, (unsigned)n), dim3(256), 0, st,
                           src, dst, h, w, l, k, out_h, out_w, step, H, W, mean);
    }
    return hipGetLastError();
}

// n NV12 frames in device memory -> n x h x w x 3 BGR bytes, rows `out_pitch` bytes apart (>= 3 * w), h * out_pitch from frame to frame
hipError_t launch_nv12_to_bgr(const unsigned char* src, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                              unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    const int32_t* c = nv12_coefficients(colour);
    if (!c) return hipErrorInvalidValue;
    const Coef k = {c[0], c[1], c[2], c[3], c[4], c[5]};
    const Layout l = {pitch, uv_offset, frame_bytes};
    const bool dw = dwords(src, pitch, uv_offset, frame_bytes);
    const bool vst = out_pitch % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    const long patches = (long)((w + 3) / 4) * (h / 2);
    const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
    if (dw && vst) hipLaunchKernelGGL((nv12_to_bgr_kernel<true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (vst) hipLaunchKernelGGL((nv12_to_bgr_kernel<false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (dw) hipLaunchKernelGGL((nv12_to_bgr_kernel<true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else hipLaunchKernelGGL((nv12_to_bgr_kernel<false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    return hipGetLastError();
}
