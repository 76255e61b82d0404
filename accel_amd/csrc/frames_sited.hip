// I420, P010, YUY2 and NV12 video frames with interpolated chroma siting -> the fp32 image tensor the plans read, and -> packed BGR bytes: the
// three kernel shapes of frames_yuv.hip, templated on the format and on the siting.  Where frames_nv12.hip and frames_yuv.hip hand every luma
// pixel the chroma sample of its 2 x 2 block (of its pair, for YUY2), these kernels interpolate Cb and Cr to the luma pixel first, as the siting
// of the source says, and feed the result to the same colour rule.
//
// Formats: 0 I420, 1 P010, 2 YUY2 as in frames_yuv.hip; 3 NV12 -- h rows of w luma bytes `pitch` apart from byte 0 and, at `u_offset`, h/2 rows
// of w/2 (Cb, Cr) byte pairs at the same pitch (pitch_c = v_offset = 0).
//
// Restates accel_amd/utils/image.py bit for bit: transform(resize(yuv_to_bgr_host(frame, siting = s))) as fp32 (nv12_to_bgr_host for format 3).
//   chroma      planes of cw = w/2 columns and ch = h/2 rows (ch = h and no vertical step for YUY2).  For luma pixel (x, y), k = x >> 1 and
//               j = y >> 1; each axis takes two neighbouring samples with weights that sum to 4:
//                   co-sited (sample k lies on luma 2k)         even coordinate: (k: 4)            odd: (k: 2, k+1: 2)
//                   centred  (sample k lies on luma 2k + 0.5)   even coordinate: (k-1: 1, k: 3)    odd: (k: 3, k+1: 1)
//               indices clamped to [0, cw-1] and [0, ch-1], and C = (sum_rows sum_cols wy wx c[row][col] + 8) >> 4 for Cb and Cr alike: one
//               rounding, none between the axes.  P010: on the 10-bit word >> 6 samples.
//   siting      1 left: horizontal co-sited, vertical centred;  2 centre: both centred;  3 topleft: both co-sited.  (0, replicated chroma, is
//               dispatched to the launchers of frames_nv12.hip and frames_yuv.hip: those kernels, bit for bit.)  Interlaced siting is not offered.
//   colour      C enters the rule of frames_yuv.hip (to_bgr) where the replicated sample enters it there; the six integers come from the tables
//               of frames_nv12.hip and frames_yuv.hip (nv12_coefficients, yuv10_coefficients)
//   interior    step == 1: those bytes; else each of the four taps of _resize_bilinear is converted to B, G, R bytes with sited chroma first and
//               the float64 blend of frames_resample.h runs on them
//   value       fp32(double(grey) - mean[c]) in plane 2 - c; padding fp32(0 - mean[c])
// Bandwidth kernels, store-bound like their replicated twins: the same bytes cross HBM; the neighbouring chroma samples (up to 4 columns x 3 rows
// around a patch) are clamped scalar loads that other threads of the block have brought into L1/L2.  No range slot, as for the other frame routes.
#include "kernels.h"
#include "frames_resample.h"
#include <stdint.h>

namespace {

using frames::Means;
using frames::centred;

enum { I420 = 0, P010 = 1, YUY2 = 2, NV12 = 3 };
enum { COSITED = 0, CENTRED = 1, NOSTEP = 2 };      // how an axis interpolates

struct Coef { int yoff, ky, krv, kgu, kgv, kbu; };      // yoff in the units of the samples (4 x the table's for P010)

struct Layout { size_t pitch, pitch_c, u_offset, v_offset, frame_bytes; };

// siting S (1 .. 3) of format F -> the modes of its two axes
template <int F, int S> struct Axes {
    static constexpr int H = S == 2 ? CENTRED : COSITED;
    static constexpr int V = F == YUY2 ? NOSTEP : (S == 3 ? COSITED : CENTRED);
};

// rows of the patch a thread of the step-1 kernel and of the byte converter produces: chroma is shared by two rows, or by none
template <int F> struct Patch { static constexpr int ROWS = F == YUY2 ? 1 : 2; };

// one pixel as B | G << 8 | R << 16: the rule of frames_yuv.hip
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

// a 10-bit sample: every word of a P010 frame is 2-byte aligned (accel_io.cpp frame_yuv_sited_args)
__device__ __forceinline__ int word10(const unsigned char* p)
{
    return *reinterpret_cast<const uint16_t*>(p) >> 6;
}

// ---- the sample fetchers --------------------------------------------------------------------------------------------------------------------
// luma of pixel (x, y), x < w and y < h
template <int F>
__device__ __forceinline__ int luma_at(const unsigned char* __restrict__ img, const Layout& l, int x, int y)
{
    const unsigned char* row = img + (size_t)y * l.pitch;
    if (F == P010) return word10(row + 2 * (size_t)x);
    return row[F == YUY2 ? 2 * (size_t)x : (size_t)x];
}

// chroma sample (col, row) of the planes, col < cw and row < ch
template <int F>
__device__ __forceinline__ void chroma_at(const unsigned char* __restrict__ img, const Layout& l, int col, int row, int& cb, int& cr)
{
    if (F == I420) {
        const size_t c = (size_t)row * l.pitch_c + col;
        cb = img[l.u_offset + c]; cr = img[l.v_offset + c];
    } else if (F == YUY2) {
        const unsigned char* quad = img + (size_t)row * l.pitch + 4 * (size_t)col;
        cb = quad[1]; cr = quad[3];
    } else if (F == NV12) {
        const unsigned char* uv = img + l.u_offset + (size_t)row * l.pitch + 2 * (size_t)col;
        cb = uv[0]; cr = uv[1];
    } else {
        const unsigned char* uv = img + l.u_offset + (size_t)row * l.pitch + 4 * (size_t)col;
        cb = word10(uv); cr = word10(uv + 2);
    }
}

// the two taps of luma coordinate x on an axis of mode M: indices i0, i1 (not clamped yet) and weights w0, w1 that sum to 4
template <int M>
__device__ __forceinline__ void axis_taps(int x, int& i0, int& w0, int& i1, int& w1)
{
    const int k = x >> 1, odd = x & 1;
    if (M == NOSTEP) { i0 = i1 = x; w0 = 4; w1 = 0; }
    else if (M == COSITED) { i0 = k; i1 = k + odd; w0 = odd ? 2 : 4; w1 = odd ? 2 : 0; }
    else { i0 = k - 1 + odd; i1 = k + odd; w0 = odd ? 3 : 1; w1 = odd ? 1 : 3; }
}

// pixel (x, y) of a frame, x < w and y < h, with sited chroma: up to 2 x 2 chroma samples
template <int F, int S>
__device__ __forceinline__ uint32_t pixel_bgr(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x, int y, const Coef& k)
{
    const int cw = w >> 1, ch = F == YUY2 ? h : h >> 1;
    int c0, c1, wx0, wx1, r0, r1, wy0, wy1;
    axis_taps<Axes<F, S>::H>(x, c0, wx0, c1, wx1);
    axis_taps<Axes<F, S>::V>(y, r0, wy0, r1, wy1);
    c0 = min(max(c0, 0), cw - 1); c1 = min(max(c1, 0), cw - 1);
    r0 = min(max(r0, 0), ch - 1); r1 = min(max(r1, 0), ch - 1);
    int b00, b01, b10, b11, e00, e01, e10, e11;
    chroma_at<F>(img, l, c0, r0, b00, e00); chroma_at<F>(img, l, c1, r0, b01, e01);
    chroma_at<F>(img, l, c0, r1, b10, e10); chroma_at<F>(img, l, c1, r1, b11, e11);
    const int cb = (wy0 * (wx0 * b00 + wx1 * b01) + wy1 * (wx0 * b10 + wx1 * b11) + 8) >> 4;
    const int cr = (wy0 * (wx0 * e00 + wx1 * e01) + wy1 * (wx0 * e10 + wx1 * e11) + 8) >> 4;
    return to_bgr<F>(luma_at<F>(img, l, x, y), cb, cr, k);
}

// The 4-pixel x ROWS-row patch at (x0, y) -- x0 a multiple of 4, y a multiple of ROWS -- as B | G << 8 | R << 16 per pixel; pixels outside the
// h x w frame are left alone.  w is even (and h where ROWS == 2), so the rows of a patch are inside or outside together.  WIDE: the layout and
// the source address allow the wide luma loads of a whole patch (wide_loads below): a dword per row (I420, NV12), two dwords (YUY2), 8 bytes
// (P010); a patch the frame's edge cuts (2 columns), and every patch without WIDE, gathers its luma sample by sample.  The chroma a patch needs
// is the table of columns (x0 >> 1) - 1 .. (x0 >> 1) + 2 and rows (y >> 1) - 1 .. (y >> 1) + 1, each index clamped to the plane: a centred axis
// uses all of it, a co-sited one neither the first column nor the first row, YUY2 its own row alone.
template <int F, int S, bool WIDE>
__device__ __forceinline__ void patch_bgr(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x0, int y, const Coef& k,
                                          uint32_t (&px)[Patch<F>::ROWS][4])
{
    constexpr int ROWS = Patch<F>::ROWS, HM = Axes<F, S>::H, VM = Axes<F, S>::V;
    if (y >= h || x0 >= w) return;
    const int cols = min(4, w - x0);      // 4 or 2
    const int cw = w >> 1, ch = F == YUY2 ? h : h >> 1;
    int Y[ROWS][4] = {};
    if (WIDE && cols == 4) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const unsigned char* row = img + (size_t)(y + j) * l.pitch;
            if (F == I420 || F == NV12) {
                const uint32_t d = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
                for (int i = 0; i < 4; ++i) Y[j][i] = (d >> (8 * i)) & 255u;
            } else if (F == YUY2) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(row + 2 * (size_t)x0);      // Y0 Cb0 Y1 Cr0 | Y2 Cb1 Y3 Cr1
                const uint32_t q0 = q[0], q1 = q[1];
                Y[j][0] = q0 & 255u; Y[j][1] = (q0 >> 16) & 255u; Y[j][2] = q1 & 255u; Y[j][3] = (q1 >> 16) & 255u;
            } else {
                const uint2 d = *reinterpret_cast<const uint2*>(row + 2 * (size_t)x0);
                Y[j][0] = (d.x & 0xffffu) >> 6; Y[j][1] = d.x >> 22; Y[j][2] = (d.y & 0xffffu) >> 6; Y[j][3] = d.y >> 22;
            }
        }
    } else {
        for (int j = 0; j < ROWS; ++j)
            for (int i = 0; i < cols; ++i) Y[j][i] = luma_at<F>(img, l, x0 + i, y + j);
    }
    // the chroma table: TR rows x 4 columns, row r of the table is chroma row (y >> 1) - 1 + r (YUY2: row y), column t is (x0 >> 1) - 1 + t
    constexpr int TR = VM == NOSTEP ? 1 : 3;
    constexpr int R0 = VM == CENTRED ? 0 : (VM == COSITED ? 1 : 0), T0 = HM == CENTRED ? 0 : 1;      // the first row and column in use
    int cb[TR][4] = {}, cr[TR][4] = {};
#pragma unroll
    for (int r = R0; r < TR; ++r) {
        const int row = VM == NOSTEP ? y : min(max((y >> 1) - 1 + r, 0), ch - 1);
#pragma unroll
        for (int t = T0; t < 4; ++t) {
            const int col = min(max((x0 >> 1) - 1 + t, 0), cw - 1);
            chroma_at<F>(img, l, col, row, cb[r][t], cr[r][t]);
        }
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        // the rows of the table pixel row y + j blends (y is even where there is a vertical step: j is the parity)
        const int ra = VM == NOSTEP ? 0 : (VM == COSITED ? 1 : j), rb = VM == NOSTEP ? 0 : 1 + j;
        const int wya = VM == NOSTEP ? 4 : (VM == COSITED ? (j ? 2 : 4) : (j ? 3 : 1)), wyb = 4 - wya;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // the columns of the table pixel x0 + i blends (x0 is a multiple of 4: i & 1 is the parity, 1 + (i >> 1) its own sample)
            const int odd = i & 1, own = 1 + (i >> 1);
            const int ta = HM == COSITED ? own : own - 1 + odd, tb = own + odd;
            const int wxa = HM == COSITED ? (odd ? 2 : 4) : (odd ? 3 : 1), wxb = 4 - wxa;
            const int u = (wya * (wxa * cb[ra][ta] + wxb * cb[ra][tb]) + wyb * (wxa * cb[rb][ta] + wxb * cb[rb][tb]) + 8) >> 4;
            const int v = (wya * (wxa * cr[ra][ta] + wxb * cr[ra][tb]) + wyb * (wxa * cr[rb][ta] + wxb * cr[rb][tb]) + 8) >> 4;
            if (i < cols) px[j][i] = to_bgr<F>(Y[j][i], u, v, k);
        }
    }
}

// step == 1: a thread produces a 4-pixel x ROWS-row patch of the padded H x W tensor.  VST: W % 4 == 0 and a 16-byte aligned destination --
// three float4 stores per row; otherwise scalar stores with a row tail.
template <int F, int S, bool WIDE, bool VST>
__global__ __launch_bounds__(256) void frames_sited_copy_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w, Layout l,
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
    patch_bgr<F, S, WIDE>(img, l, h, w, x0, y, k, px);
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

// step != 1: a gather, one output pixel per thread; the four taps are converted to B, G, R bytes with sited chroma, then blended per channel
template <int F, int S>
__global__ __launch_bounds__(256) void frames_sited_resample_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int h, int w,
                                                                    Layout l, Coef k, int out_h, int out_w, double step, int H, int W, Means mean)
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
        const uint32_t p00 = pixel_bgr<F, S>(img, l, h, w, t.x0, t.y0, k), p01 = pixel_bgr<F, S>(img, l, h, w, t.x1, t.y0, k);
        const uint32_t p10 = pixel_bgr<F, S>(img, l, h, w, t.x0, t.y1, k), p11 = pixel_bgr<F, S>(img, l, h, w, t.x1, t.y1, k);
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
template <int F, int S, bool WIDE, bool VST>
__global__ __launch_bounds__(256) void sited_to_bgr_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h, int w, Layout l,
                                                           Coef k, size_t out_pitch)
{
    constexpr int ROWS = Patch<F>::ROWS;
    const int QW = (w + 3) >> 2, QH = h / ROWS;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * QH) return;
    const int y = (int)(q / QW) * ROWS, x0 = (int)(q % QW) * 4;
    const unsigned char* img = src + (size_t)blockIdx.z * l.frame_bytes;
    uint32_t px[ROWS][4] = {};
    patch_bgr<F, S, WIDE>(img, l, h, w, x0, y, k, px);
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

// whether the luma of every whole patch of every frame may be read with the wide loads of patch_bgr: x0 is a multiple of 4, so what has to be
// aligned is the start of every luma row of every frame (chroma is read sample by sample)
bool wide_loads(const unsigned char* src, const YuvLayout& y)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    return (a | y.pitch | y.frame_bytes) % (y.format == P010 ? 8 : 4) == 0;
}

bool coefficients(const YuvLayout& y, Coef& k)
{
    const int32_t* c = y.format == P010 ? yuv10_coefficients(y.colour) : nv12_coefficients(y.colour);
    if (!c) return false;
    k = {y.format == P010 ? 4 * c[0] : c[0], c[1], c[2], c[3], c[4], c[5]};
    return true;
}

template <int F, int S>
hipError_t frames_sited(const unsigned char* src, int n, const YuvLayout& y, const double* means_bgr, int out_h, int out_w, double step, int H, int W,
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
        if (wide && vst) hipLaunchKernelGGL((frames_sited_copy_kernel<F, S, true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (vst) hipLaunchKernelGGL((frames_sited_copy_kernel<F, S, false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else if (wide) hipLaunchKernelGGL((frames_sited_copy_kernel<F, S, true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
        else hipLaunchKernelGGL((frames_sited_copy_kernel<F, S, false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, H, W, mean);
    } else {
        const long pixels = (long)H * W;
        hipLaunchKernelGGL((frames_sited_resample_kernel<F, S>), dim3((unsigned)((pixels + 255) / 256), 1, (unsigned)n), dim3(256), 0, st,
                           src, dst, h, w, l, k, out_h, out_w, step, H, W, mean);
    }
    return hipGetLastError();
}

template <int F, int S>
hipError_t sited_to_bgr(const unsigned char* src, int n, const YuvLayout& y, unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    Coef k;
    if (!coefficients(y, k)) return hipErrorInvalidValue;
    const Layout l = {y.pitch, y.pitch_c, y.u_offset, y.v_offset, y.frame_bytes};
    const int h = y.h, w = y.w;
    const bool wide = wide_loads(src, y);
    const bool vst = out_pitch % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    const long patches = (long)((w + 3) / 4) * (h / Patch<F>::ROWS);
    const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
    if (wide && vst) hipLaunchKernelGGL((sited_to_bgr_kernel<F, S, true, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (vst) hipLaunchKernelGGL((sited_to_bgr_kernel<F, S, false, true>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else if (wide) hipLaunchKernelGGL((sited_to_bgr_kernel<F, S, true, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    else hipLaunchKernelGGL((sited_to_bgr_kernel<F, S, false, false>), grid, dim3(256), 0, st, src, dst, h, w, l, k, out_pitch);
    return hipGetLastError();
}

template <int F>
hipError_t frames_sited_of(int siting, const unsigned char* src, int n, const YuvLayout& y, const double* means_bgr, int out_h, int out_w, double step,
                           int H, int W, float* dst, hipStream_t st)
{
    switch (siting) {
    case 1: return frames_sited<F, 1>(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    case 2: return frames_sited<F, 2>(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    case 3: return frames_sited<F, F == YUY2 ? 1 : 3>(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);      // YUY2: left and topleft coincide
    }
    return hipErrorInvalidValue;
}

template <int F>
hipError_t sited_to_bgr_of(int siting, const unsigned char* src, int n, const YuvLayout& y, unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    switch (siting) {
    case 1: return sited_to_bgr<F, 1>(src, n, y, dst, out_pitch, st);
    case 2: return sited_to_bgr<F, 2>(src, n, y, dst, out_pitch, st);
    case 3: return sited_to_bgr<F, F == YUY2 ? 1 : 3>(src, n, y, dst, out_pitch, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace

// n frames in device memory -> n x 3 x H x W fp32 planar RGB, chroma sited as `siting` says.  The caller has checked the layout and the geometry
// (accel_io.cpp frame_yuv_sited_args): what launch_frames_yuv asks for, format in 0 .. 3 with NV12's fields for 3, siting in 0 .. 3.  Siting 0
// is the replicated kernel of the format, launched by its own launcher.  Reads stay inside the planes of every frame (every chroma index and the
// resampling coordinates are clamped), writes inside H x W.
hipError_t launch_frames_yuv_sited(const unsigned char* src, int n, const YuvLayout& y, int siting, const double* means_bgr, int out_h, int out_w,
                                   double step, int H, int W, float* dst, hipStream_t st)
{
    if (siting == 0)
        return y.format == NV12 ? launch_frames_nv12(src, n, y.h, y.w, y.pitch, y.u_offset, y.frame_bytes, y.colour, means_bgr, out_h, out_w, step,
                                                     H, W, dst, st)
                                : launch_frames_yuv(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    switch (y.format) {
    case I420: return frames_sited_of<I420>(siting, src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    case P010: return frames_sited_of<P010>(siting, src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    case YUY2: return frames_sited_of<YUY2>(siting, src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    case NV12: return frames_sited_of<NV12>(siting, src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    }
    return hipErrorInvalidValue;
}

// n frames in device memory -> n x h x w x 3 BGR bytes, rows `out_pitch` bytes apart (>= 3 * w), h * out_pitch from frame to frame
hipError_t launch_yuv_to_bgr_sited(const unsigned char* src, int n, const YuvLayout& y, int siting, unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    if (siting == 0)
        return y.format == NV12 ? launch_nv12_to_bgr(src, n, y.h, y.w, y.pitch, y.u_offset, y.frame_bytes, y.colour, dst, out_pitch, st)
                                : launch_yuv_to_bgr(src, n, y, dst, out_pitch, st);
    switch (y.format) {
    case I420: return sited_to_bgr_of<I420>(siting, src, n, y, dst, out_pitch, st);
    case P010: return sited_to_bgr_of<P010>(siting, src, n, y, dst, out_pitch, st);
    case YUY2: return sited_to_bgr_of<YUY2>(siting, src, n, y, dst, out_pitch, st);
    case NV12: return sited_to_bgr_of<NV12>(siting, src, n, y, dst, out_pitch, st);
    }
    return hipErrorInvalidValue;
}
