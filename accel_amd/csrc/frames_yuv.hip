// I420, P010 and YUY2 video frames -- what a software decoder, a 10-bit hardware decoder and a capture card hand out -- -> the fp32 image tensor
// the plans read (`data` / `data_key`), in one kernel: colour conversion, resize, mean subtraction and padding.  And -> packed BGR bytes.  The
// three kernel shapes of frames_nv12.hip, templated on the format; only the sample fetchers know a layout.
//
// One frame (frame i starts at i * frame_bytes; bytes in the gaps -- between rows, between the planes, after a frame -- are never read):
//   I420   h rows of w luma bytes `pitch` apart from byte 0; at `u_offset` the Cb plane and at `v_offset` the Cr plane, each h/2 rows of w/2
//          bytes `pitch_c` apart.  Pixel (x, y) takes chroma at (x >> 1, y >> 1).  h, w even.  (YV12: v_offset < u_offset.)
//   YUY2   h rows `pitch` apart of w/2 quads Y0 Cb Y1 Cr.  Pixel (x, y) takes the chroma of quad x >> 1 of its own row.  w even.
//   P010   NV12's shape in little-endian 16-bit words: h rows of w luma words, at `u_offset` h/2 rows of w/2 (Cb, Cr) word pairs, `pitch` bytes
//          apart in both planes.  The sample is word >> 6: the low six bits are never looked at.  h, w even; every word is 2-byte aligned.
//
// Restates accel_amd/utils/image.py bit for bit: transform(resize(yuv_to_bgr_host(frame))) as fp32.
//   colour      8-bit formats: the rule and the six integers of frames_nv12.hip, with c = Y - yoff, d = Cb - 128, e = Cr - 128
//                   R = clip((ky*c + krv*e + 32768) >> 16, 0, 255), G and B alike
//               P010: c = Y10 - 4 * yoff, d = Cb10 - 512, e = Cr10 - 512
//                   R = clip((ky*c + krv*e + (1 << 17)) >> 18, 0, 255), G and B alike
//               with the same five integers for the limited-range modes (the 10-bit signal is 4 times the 8-bit one) and
//               round(65536 x value x 1020 / 1023) for the full-range ones: YUV10_COEF below, held to image.yuv10_coefficients by the CPU
//               suite.  int32 and arithmetic right shifts; |accumulator| < 1.5e8.
//   interior    step == 1: those bytes; else each of the four taps of _resize_bilinear is converted to B, G, R bytes first and the float64
//               blend of frames_resample.h runs on them
//   value       fp32(double(grey) - mean[c]) in plane 2 - c; padding fp32(0 - mean[c])
// Bandwidth kernels, store-bound: 12 bytes written per pixel; 1.5 (I420), 2 (YUY2) or 3 (P010) read.  No range slot, as for the other frame routes.
#include "kernels.h"
#include "frames_resample.h"
#include <stdint.h>

namespace {

using frames::Means;
using frames::centred;

enum { I420 = 0, P010 = 1, YUY2 = 2 };

struct Coef { int yoff, ky, krv, kgu, kgv, kbu; };      // yoff in the units of the samples (4 x the table's for P010)

//                                  yoff  ky     krv     kgu    kgv    kbu
const int32_t YUV10_COEF[4][6] = {{16, 76309, 104597, 25675, 53279, 132201},      // 0  BT.601 limited range: the 8-bit integers
                                  {0,  65344, 91612,  22487, 46664, 115789},      // 1  BT.601 full range: x 1020 / 1023
                                  {16, 76309, 117489, 13975, 34925, 138438},      // 2  BT.709 limited range: the 8-bit integers
                                  {0,  65344, 102903, 12240, 30589, 121252}};    // 3  BT.709 full range: x 1020 / 1023

struct Layout { size_t pitch, pitch_c, u_offset, v_offset, frame_bytes; };

// rows of the patch a thread of the step-1 kernel and of the byte converter produces: chroma is shared by two rows, or by none
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

// a 10-bit sample: every word of a P010 frame is 2-byte aligned (accel_io.cpp frame_yuv_args)
__device__ __forceinline__ int word10(const unsigned char* p)
{
    return *reinterpret_cast<const uint16_t*>(p) >> 6;
}

// ---- the sample fetchers: pixel (x, y) of a frame, x < w and y < h --------------------------------------------------------------------------
template <int F>
__device__ __forceinline__ uint32_t pixel_bgr(const unsigned char* __restrict__ img, const Layout& l, int x, int y, const Coef& k)
{
    if (F == I420) {
        const size_t c = (size_t)(y >> 1) * l.pitch_c + (x >> 1);
        return to_bgr<F>(img[(size_t)y * l.pitch + x], img[l.u_offset + c], img[l.v_offset + c], k);
    } else if (F == YUY2) {
        const unsigned char* row = img + (size_t)y * l.pitch;
        const unsigned char* quad = row + 4 * (size_t)(x >> 1);
        return to_bgr<F>(row[2 * (size_t)x], quad[1], quad[3], k);
    } else {
        const unsigned char* uv = img + l.u_offset + (size_t)(y >> 1) * l.pitch + 4 * (size_t)(x >> 1);
        return to_bgr<F>(word10(img + (size_t)y * l.pitch + 2 * (size_t)x), word10(uv), word10(uv + 2), k);
    }
}

// The 4-pixel x ROWS-row patch at (x0, y) -- x0 a multiple of 4, y a multiple of ROWS -- as B | G << 8 | R << 16 per pixel; pixels outside the
// h x w frame are left alone.  w is even (and h where ROWS == 2), so the rows of a patch, and both pixels of a chroma pair, are inside or outside
// together.  WIDE: the layout and the source address allow the wide loads of a whole patch (wide_loads below) --
//   I420   two luma dwords and one 16-bit load from each chroma plane
//   YUY2   two dwords (Y0 Cb0 Y1 Cr0 | Y2 Cb1 Y3 Cr1)
//   P010   two 8-byte luma loads and one 8-byte chroma load (Cb0 Cr0 Cb1 Cr1)
// a patch the frame's edge cuts (2 columns), and every patch without WIDE, is gathered sample by sample.
template <int F, bool WIDE>
__device__ __forceinline__ void patch_bgr(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x0, int y, const Coef& k,
                                          uint32_t (&px)[Patch<F>::ROWS][4])
{
    constexpr int ROWS = Patch<F>::ROWS;
    if (y >= h || x0 >= w) return;
    const int cols = min(4, w - x0);      // 4 or 2
    int Y[ROWS][4] = {}, cb[2] = {}, cr[2] = {};
    if (F == I420) {
        const unsigned char* y0 = img + (size_t)y * l.pitch + x0;
        const size_t c = (size_t)(y >> 1) * l.pitch_c + (x0 >> 1);
        const unsigned char* u = img + l.u_offset + c;
        const unsigned char* v = img + l.v_offset + c;
        if (WIDE && cols == 4) {
            const uint32_t uu = *reinterpret_cast<const uint16_t*>(u), vv = *reinterpret_cast<const uint16_t*>(v);
            cb[0] = uu & 255u; cb[1] = uu >> 8; cr[0] = vv & 255u; cr[1] = vv >> 8;
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                const uint32_t d = *reinterpret_cast<const uint32_t*>(y0 + j * l.pitch);
#pragma unroll
                for (int i = 0; i < 4; ++i) Y[j][i] = (d >> (8 * i)) & 255u;
            }
        } else {
            for (int i = 0; i < cols / 2; ++i) { cb[i] = u[i]; cr[i] = v[i]; }
            for (int j = 0; j < ROWS; ++j)
                for (int i = 0; i < cols; ++i) Y[j][i] = y0[j * l.pitch + i];
        }
    } else if (F == YUY2) {
        const unsigned char* row = img + (size_t)y * l.pitch + 2 * (size_t)x0;
        if (WIDE && cols == 4) {
            const uint32_t q0 = reinterpret_cast<const uint32_t*>(row)[0], q1 = reinterpret_cast<const uint32_t*>(row)[1];
            Y[0][0] = q0 & 255u; cb[0] = (q0 >> 8) & 255u; Y[0][1] = (q0 >> 16) & 255u; cr[0] = q0 >> 24;
            Y[0][2] = q1 & 255u; cb[1] = (q1 >> 8) & 255u; Y[0][3] = (q1 >> 16) & 255u; cr[1] = q1 >> 24;
        } else {
            for (int i = 0; i < cols / 2; ++i) {
                Y[0][2 * i] = row[4 * i]; cb[i] = row[4 * i + 1]; Y[0][2 * i + 1] = row[4 * i + 2]; cr[i] = row[4 * i + 3];
            }
        }
    } else {
        const unsigned char* y0 = img + (size_t)y * l.pitch + 2 * (size_t)x0;
        const unsigned char* uv = img + l.u_offset + (size_t)(y >> 1) * l.pitch + 2 * (size_t)x0;
        if (WIDE && cols == 4) {
            const uint2 c = *reinterpret_cast<const uint2*>(uv);
            cb[0] = (c.x & 0xffffu) >> 6; cr[0] = c.x >> 22; cb[1] = (c.y & 0xffffu) >> 6; cr[1] = c.y >> 22;
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                const uint2 d = *reinterpret_cast<const uint2*>(y0 + j * l.pitch);
                Y[j][0] = (d.x & 0xffffu) >> 6; Y[j][1] = d.x >> 22; Y[j][2] = (d.y & 0xffffu) >> 6; Y[j][3] = d.y >> 22;
            }
        } else {
            for (int i = 0; i < cols / 2; ++i) { cb[i] = word10(uv + 4 * i); cr[i] = word10(uv + 4 * i + 2); }
            for (int j = 0; j < ROWS; ++j)
                for (int i = 0; i < cols; ++i) Y[j][i] = word10(y0 + j * l.pitch + 2 * i);
        }
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cols) px[j][i] = to_bgr<F>(Y[j][i], cb[i >> 1], cr[i >> 1], k);
}

// step == 1: a thread produces a 4-pixel x ROWS-row patch of the padded H x W tensor.  VST: W % 4 == 0 and a 16-byte aligned destination --
// three float4 stores per row; otherwise scalar stores with a row tail.
template <int F, bool WIDE, bool VST>
__global__ __launch_bounds__(256) void frames_yuv_copy_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, Layout l,
                                                              Coef k, int H, int W, Means mean)
{
    constexpr int ROWS = Patch<F>::ROWS;
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
    patch_bgr<F, WIDE>(img, l, h, w, x0, y, k, px);
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
template <int F>
__global__ __launch_bounds__(256) void frames_yuv_resample_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, Layout l,
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
        const uint32_t p00 = pixel_bgr<F>(img, l, t.x0, t.y0, k), p01 = pixel_bgr<F>(img, l, t.x1, t.y0, k);
        const uint32_t p10 = pixel_bgr<F>(img, l, t.x0, t.y1, k), p11 = pixel_bgr<F>(img, l, t.x1, t.y1, k);
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
template <int F, bool WIDE, bool VST>
__global__ __launch_bounds__(256) void yuv_to_bgr_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h, int w, Layout l,
                                                         Coef k, size_t out_pitch)
{
    constexpr int ROWS = Patch<F>::ROWS;
    const int QW = (w + 3) >> 2, QH = h / ROWS;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * QH) return;
    const int y = (int)(q / QW) * ROWS, x0 = (int)(q % QW) * 4;
    const unsigned char* img = src + (size_t)blockIdx.z * l.frame_bytes;
    uint32_t px[ROWS][4] = {};
    patch_bgr<F, WIDE>(img, l, h, w, x0, y, k, px);
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

// whether every whole patch of every frame may be read with the wide loads of patch_bgr: x0 is a multiple of 4, so what has to be aligned is
// the start of every row of every plane of every frame
bool wide_loads(const unsigned char* src, const YuvLayout& y)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    switch (y.format) {
    case I420: return (a | y.pitch | y.frame_bytes) % 4 == 0 && (y.pitch_c | y.u_offset | y.v_offset) % 2 == 0;
    case YUY2: return (a | y.pitch | y.frame_bytes) % 4 == 0;
    default:   return (a | y.pitch | y.frame_bytes | y.u_offset) % 8 == 0;
    }
}

bool coefficients(const YuvLayout& y, Coef& k)
{
    const int32_t* c = y.format == P010 ? yuv10_coefficients(y.colour) : nv12_coefficients(y.colour);
    if (!c) return false;
    k = {y.format == P010 ? 4 * c[0] : c[0], c[1], c[2], c[3], c[4], c[5]};
    return true;
}

template <int F>
hipError_t frames_yuv(const unsigned char* src, int n, const YuvLayout& y, const double* means_bgr, int out_h, int out_w, double step, int H, int W,
                      float* dst, hipStream_t st)
{
    Coef k;
    if (!coefficients(y, k)) return hipErrorInvalidValue;
    const Layout l = {y.pitch, y.pitch_c, y.u_offset, y.v_offset, y.frame_bytes};
    const Means mean = {means_bgr[0], means_bgr[1], means_bgr[2]};
    const int h = y.h, w = y.w;
    if (step == 1.0 && out_h == h && out_w == w) {
        constexpr int ROWS = Patch<F>::ROWS;
        const bool wide = wide_loads(src, y);
        const bool vst = W % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
        const long patches = (long)((W + 3) / 4) * ((H + ROWS - 1) / ROWS);
        const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
        if (wide && vst) hipLaunchKernelGGL((frames_yuv_copy_kernel<F, true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (vst) hipLaunchKernelGGL((frames_yuv_copy_kernel<F, false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (wide) hipLaunchKernelGGL((frames_yuv_copy_kernel<F, true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else hipLaunchKernelGGL((frames_yuv_copy_kernel<F, false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
    } else {
        const long pixels = (long)H * W;
        hipLaunchKernelGGL(frames_yuv_resample_kernel<F>, dim3((unsigned)((pixels + 255) / 256), 1, (unsigned)n), dim3(256), 0, st,
                           src, dst, h, w, l, k, out_h, out_w, step, H, W, mean);
    }
    return hipGetLastError();
}

template <int F>
hipError_t yuv_to_bgr(const unsigned char* src, int n, const YuvLayout& y, unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    Coef k;
    if (!coefficients(y, k)) return hipErrorInvalidValue;
    const Layout l = {y.pitch, y.pitch_c, y.u_offset, y.v_offset, y.frame_bytes};
    const int h = y.h, w = y.w;
    const bool wide = wide_loads(src, y);
    const bool vst = out_pitch % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    const long patches = (long)((w + 3) / 4) * (h / Patch<F>::ROWS);
    const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
    if (wide && vst) hipLaunchKernelGGL((yuv_to_bgr_kernel<F, true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (vst) hipLaunchKernelGGL((yuv_to_bgr_kernel<F, false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (wide) hipLaunchKernelGGL((yuv_to_bgr_kernel<F, true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else hipLaunchKernelGGL((yuv_to_bgr_kernel<F, false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    return hipGetLastError();
}

}  // namespace

const int32_t* yuv10_coefficients(int colour)
{
    return colour >= 0 && colour < 4 ? YUV10_COEF[colour] : nullptr;
}

// n frames in device memory -> n x 3 x H x W fp32 planar RGB.  The caller has checked the layout and the geometry (accel_io.cpp frame_yuv_args):
// the format, the parity of h and w, the pitches, the plane offsets, frame_bytes >= the frame's extent, the 2-byte alignment of P010, colour in
// 0 .. 3, out_h <= H, out_w <= W, and step == 1 only with out_h == h, out_w == w.  Reads stay inside the planes of every frame (the resampling
// coordinates are clamped), writes inside H x W.
hipError_t launch_frames_yuv(const unsigned char* src, int n, const YuvLayout& y, const double* means_bgr, int out_h, int out_w, double step,
                             int H, int W, float* dst, hipStream_t st)
{
    switch (y.format) {
    case I420: return frames_yuv<I420>(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    case P010: return frames_yuv<P010>(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    case YUY2: return frames_yuv<YUY2>(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    }
    return hipErrorInvalidValue;
}

// n frames in device memory -> n x h x w x 3 BGR bytes, rows `out_pitch` bytes apart (>= 3 * w), h * out_pitch from frame to frame
hipError_t launch_yuv_to_bgr(const unsigned char* src, int n, const YuvLayout& y, unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    switch (y.format) {
    case I420: return yuv_to_bgr<I420>(src, n, y, dst, out_pitch, st);
    case P010: return yuv_to_bgr<P010>(src, n, y, dst, out_pitch, st);
    case YUY2: return yuv_to_bgr<YUY2>(src, n, y, dst, out_pitch, st);
    }
    return hipErrorInvalidValue;
}
