// The label map blended over a video frame IN THE FRAME'S OWN FORMAT AND LAYOUT -- I420 / YV12, P010, YUY2 or NV12 in, the same bytes out: what
// an encoder, a compositor or a capture-card output takes, without a trip through BGR.  One kernel shape, templated on the format; the kernel
// knows no colour standard: the palette arrives as a table of (Y, Cb, Cr) per label (utils/image.py palette_ycbcr), in the units of the samples.
//
// Restates accel_amd/utils/image.py overlay_yuv_host bit for bit.  a = alpha in 0 .. 256, T the table, L(x, y) the label of source pixel (x, y)
// -- labels[min(y * out_h / h, out_h - 1)][min(x * out_w / w, out_w - 1)], the geometry of results_u8.hip:
//   luma            Y'  = (a * T[L(x, y)].Y + (256 - a) * Y + 128) >> 8
//   4:2:0 chroma    Cb' = (a * S + (256 - a) * 4 * Cb + 512) >> 10, S = the sum of T[L].Cb over the 2 x 2 luma pixels of the sample; Cr alike
//   4:2:2 chroma    Cb' = (a * S2 + (256 - a) * 2 * Cb + 256) >> 9, S2 over the two pixels of the quad (YUY2)
//   P010            the operands are word >> 6, the stored word is sample << 6 (its low six bits are zero)
// One rounding per sample and no clip: a convex combination stays inside the range of its operands.  uint32 throughout (<= 256 * 4 * 1023 + 512).
// The overlay's chroma is the block mean of the palette colours whatever the siting of the frame's samples, which are blended where they are.
//
// A thread owns the 4-pixel x ROWS patch of frames_yuv.h -- whole 2 x 2 (YUY2: 1 x 2) blocks -- reads all its samples, then stores them: no
// thread reads a sample another writes, so dst == frame (in place on a decoder's surface) is allowed and the two pointers carry no __restrict__.
// Bytes that are not samples (between rows, between planes, after a frame) are neither read nor written.
// A bandwidth kernel: about 1 label byte + the frame's bytes in, the frame's bytes out.
#include "frames_yuv.h"
#include "labels_nearest.h"

namespace {

using namespace yuv;      // the formats, Layout, Patch, word10

struct TableYcc { uint16_t ycc[768]; };       // passed BY VALUE: 1536 bytes of kernel argument, no allocation, ordered with the stream for free

using nearest::Column;
using nearest::source_row;

__device__ __forceinline__ void store10(unsigned char* p, unsigned v) { *reinterpret_cast<uint16_t*>(p) = (uint16_t)(v << 6); }

// WIDE: the layout, the source and the destination address allow the wide accesses of a whole patch (wide_access below) --
//   I420   two luma dwords and one 16-bit access in each chroma plane
//   NV12   two luma dwords and one chroma dword (Cb0 Cr0 Cb1 Cr1)
//   YUY2   two dwords (Y0 Cb0 Y1 Cr0 | Y2 Cb1 Y3 Cr1)
//   P010   two 8-byte luma accesses and one 8-byte chroma access
// a patch the frame's edge cuts (2 columns), and every patch without WIDE, goes sample by sample.  IDENT: h x w == out_h x out_w, the labels
// of a patch row are one dword when label_dword (uniform: W % 4 == 0, 4-byte aligned maps).
template <int F, bool IDENT, bool WIDE>
__global__ __launch_bounds__(256) void overlay_yuv_kernel(const unsigned char* __restrict__ labels, int H, int W, int out_h, int out_w, int h, int w,
                                                          Layout l, const TableYcc pal, int alpha, const unsigned char* frame, unsigned char* dst,
                                                          int label_dword)
{
    constexpr int ROWS = Patch<F>::ROWS;
    __shared__ unsigned table[256];       // Y | Cb << 10 | Cr << 20: a triple fits one dword at 8 and at 10 bits
    table[threadIdx.x] = (unsigned)pal.ycc[3 * threadIdx.x] | (unsigned)pal.ycc[3 * threadIdx.x + 1] << 10 | (unsigned)pal.ycc[3 * threadIdx.x + 2] << 20;
    __syncthreads();
    const int QW = (w + 3) >> 2, QH = h / ROWS;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)QW * QH) return;
    const int y = (int)(q / QW) * ROWS, x0 = (int)(q % QW) * 4;
    const int cols = min(4, w - x0);      // 4 or 2: w is even
    const bool whole = WIDE && cols == 4;

    // ---- the table entries of the patch's pixels (columns past w - 1 are clamped into the row: read, not used)
    unsigned t[ROWS][4];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const unsigned char* row = labels + (size_t)blockIdx.z * H * W + (size_t)(IDENT ? y + j : source_row(y + j, out_h, h)) * W;
        if (IDENT) {
            if (label_dword && cols == 4) {
                const uint32_t four = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
                for (int i = 0; i < 4; ++i) t[j][i] = table[(four >> (8 * i)) & 255u];
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) t[j][i] = table[row[min(x0 + i, w - 1)]];
            }
        } else {
            Column c(x0, out_w, w);
#pragma unroll
            for (int i = 0; i < 4; ++i) { t[j][i] = table[row[c.col()]]; c.next(); }
        }
    }

    // ---- the patch's samples
    const unsigned char* img = frame + (size_t)blockIdx.z * l.frame_bytes;
    unsigned char* out = dst + (size_t)blockIdx.z * l.frame_bytes;
    unsigned Y[ROWS][4] = {}, cb[2] = {}, cr[2] = {};
    size_t o_y, o_u, o_v = 0;             // byte offsets of the patch in the luma plane and in the chroma plane(s)
    if (F == I420) {
        o_y = (size_t)y * l.pitch + x0;
        const size_t c = (size_t)(y >> 1) * l.pitch_c + (x0 >> 1);
        o_u = l.u_offset + c; o_v = l.v_offset + c;
        if (whole) {
            const uint32_t uu = *reinterpret_cast<const uint16_t*>(img + o_u), vv = *reinterpret_cast<const uint16_t*>(img + o_v);
            cb[0] = uu & 255u; cb[1] = uu >> 8; cr[0] = vv & 255u; cr[1] = vv >> 8;
        } else {
            for (int i = 0; i < cols / 2; ++i) { cb[i] = img[o_u + i]; cr[i] = img[o_v + i]; }
        }
    } else if (F == NV12) {
        o_y = (size_t)y * l.pitch + x0;
        o_u = l.u_offset + (size_t)(y >> 1) * l.pitch + x0;
        if (whole) {
            const uint32_t c = *reinterpret_cast<const uint32_t*>(img + o_u);
            cb[0] = c & 255u; cr[0] = (c >> 8) & 255u; cb[1] = (c >> 16) & 255u; cr[1] = c >> 24;
        } else {
            for (int i = 0; i < cols / 2; ++i) { cb[i] = img[o_u + 2 * i]; cr[i] = img[o_u + 2 * i + 1]; }
        }
    } else if (F == YUY2) {
        o_y = o_u = (size_t)y * l.pitch + 2 * (size_t)x0;
        if (whole) {
            const uint32_t q0 = reinterpret_cast<const uint32_t*>(img + o_y)[0], q1 = reinterpret_cast<const uint32_t*>(img + o_y)[1];
            Y[0][0] = q0 & 255u; cb[0] = (q0 >> 8) & 255u; Y[0][1] = (q0 >> 16) & 255u; cr[0] = q0 >> 24;
            Y[0][2] = q1 & 255u; cb[1] = (q1 >> 8) & 255u; Y[0][3] = (q1 >> 16) & 255u; cr[1] = q1 >> 24;
        } else {
            for (int i = 0; i < cols / 2; ++i) {
                const unsigned char* p = img + o_y + 4 * i;
                Y[0][2 * i] = p[0]; cb[i] = p[1]; Y[0][2 * i + 1] = p[2]; cr[i] = p[3];
            }
        }
    } else {
        o_y = (size_t)y * l.pitch + 2 * (size_t)x0;
        o_u = l.u_offset + (size_t)(y >> 1) * l.pitch + 2 * (size_t)x0;
        if (whole) {
            const uint2 c = *reinterpret_cast<const uint2*>(img + o_u);
            cb[0] = (c.x & 0xffffu) >> 6; cr[0] = c.x >> 22; cb[1] = (c.y & 0xffffu) >> 6; cr[1] = c.y >> 22;
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                const uint2 d = *reinterpret_cast<const uint2*>(img + o_y + j * l.pitch);
                Y[j][0] = (d.x & 0xffffu) >> 6; Y[j][1] = d.x >> 22; Y[j][2] = (d.y & 0xffffu) >> 6; Y[j][3] = d.y >> 22;
            }
        } else {
            for (int i = 0; i < cols / 2; ++i) { cb[i] = word10(img + o_u + 4 * i); cr[i] = word10(img + o_u + 4 * i + 2); }
            for (int j = 0; j < ROWS; ++j)
                for (int i = 0; i < cols; ++i) Y[j][i] = word10(img + o_y + j * l.pitch + 2 * i);
        }
    }
    if (F == I420 || F == NV12) {
        if (whole) {
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                const uint32_t d = *reinterpret_cast<const uint32_t*>(img + o_y + j * l.pitch);
#pragma unroll
                for (int i = 0; i < 4; ++i) Y[j][i] = (d >> (8 * i)) & 255u;
            }
        } else {
            for (int j = 0; j < ROWS; ++j)
                for (int i = 0; i < cols; ++i) Y[j][i] = img[o_y + j * l.pitch + i];
        }
    }

    // ---- the blend: one rounding per sample
    const unsigned a = (unsigned)alpha, ia = 256u - a;
    constexpr unsigned CSH = F == YUY2 ? 9 : 10, CN = F == YUY2 ? 2 : 4, M10 = 1023u;
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) Y[j][i] = (a * (t[j][i] & M10) + ia * Y[j][i] + 128u) >> 8;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        unsigned su = 0, sv = 0;
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
#pragma unroll
            for (int i = 2 * p; i < 2 * p + 2; ++i) { su += (t[j][i] >> 10) & M10; sv += t[j][i] >> 20; }
        cb[p] = (a * su + ia * CN * cb[p] + (1u << (CSH - 1))) >> CSH;
        cr[p] = (a * sv + ia * CN * cr[p] + (1u << (CSH - 1))) >> CSH;
    }

    // ---- every load of this thread is done: the stores (in place: the bytes just read)
    if (F == I420) {
        if (whole) {
            *reinterpret_cast<uint16_t*>(out + o_u) = (uint16_t)(cb[0] | cb[1] << 8);
            *reinterpret_cast<uint16_t*>(out + o_v) = (uint16_t)(cr[0] | cr[1] << 8);
        } else {
            for (int i = 0; i < cols / 2; ++i) { out[o_u + i] = (unsigned char)cb[i]; out[o_v + i] = (unsigned char)cr[i]; }
        }
    } else if (F == NV12) {
        if (whole) {
            *reinterpret_cast<uint32_t*>(out + o_u) = cb[0] | cr[0] << 8 | cb[1] << 16 | cr[1] << 24;
        } else {
            for (int i = 0; i < cols / 2; ++i) { out[o_u + 2 * i] = (unsigned char)cb[i]; out[o_u + 2 * i + 1] = (unsigned char)cr[i]; }
        }
    } else if (F == YUY2) {
        if (whole) {
            uint32_t* o = reinterpret_cast<uint32_t*>(out + o_y);
            o[0] = Y[0][0] | cb[0] << 8 | Y[0][1] << 16 | cr[0] << 24;
            o[1] = Y[0][2] | cb[1] << 8 | Y[0][3] << 16 | cr[1] << 24;
        } else {
            for (int i = 0; i < cols / 2; ++i) {
                unsigned char* p = out + o_y + 4 * i;
                p[0] = (unsigned char)Y[0][2 * i]; p[1] = (unsigned char)cb[i]; p[2] = (unsigned char)Y[0][2 * i + 1]; p[3] = (unsigned char)cr[i];
            }
        }
    } else {
        if (whole) {
            *reinterpret_cast<uint2*>(out + o_u) = make_uint2(cb[0] << 6 | cr[0] << 22, cb[1] << 6 | cr[1] << 22);
#pragma unroll
            for (int j = 0; j < ROWS; ++j)
                *reinterpret_cast<uint2*>(out + o_y + j * l.pitch) = make_uint2(Y[j][0] << 6 | Y[j][1] << 22, Y[j][2] << 6 | Y[j][3] << 22);
        } else {
            for (int i = 0; i < cols / 2; ++i) { store10(out + o_u + 4 * i, cb[i]); store10(out + o_u + 4 * i + 2, cr[i]); }
            for (int j = 0; j < ROWS; ++j)
                for (int i = 0; i < cols; ++i) store10(out + o_y + j * l.pitch + 2 * i, Y[j][i]);
        }
    }
    if (F == I420 || F == NV12) {
        if (whole) {
#pragma unroll
            for (int j = 0; j < ROWS; ++j)
                *reinterpret_cast<uint32_t*>(out + o_y + j * l.pitch) = Y[j][0] | Y[j][1] << 8 | Y[j][2] << 16 | Y[j][3] << 24;
        } else {
            for (int j = 0; j < ROWS; ++j)
                for (int i = 0; i < cols; ++i) out[o_y + j * l.pitch + i] = (unsigned char)Y[j][i];
        }
    }
}

// whether every whole patch of every frame may be read at `p` with the wide accesses above: x0 is a multiple of 4, so what has to be aligned
// is the start of every row of every plane of every frame (the conditions of frames_yuv.hip wide_loads; NV12's chroma dword like I420's luma)
bool wide_access(const unsigned char* p, const YuvLayout& y)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    switch (y.format) {
    case I420: return (a | y.pitch | y.frame_bytes) % 4 == 0 && (y.pitch_c | y.u_offset | y.v_offset) % 2 == 0;
    case YUY2: return (a | y.pitch | y.frame_bytes) % 4 == 0;
    case NV12: return (a | y.pitch | y.frame_bytes | y.u_offset) % 4 == 0;
    default:   return (a | y.pitch | y.frame_bytes | y.u_offset) % 8 == 0;
    }
}

template <int F>
hipError_t overlay_yuv(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, const YuvLayout& y, const TableYcc& pal, int alpha,
                       const unsigned char* frame, unsigned char* dst, hipStream_t st)
{
    const Layout l = {y.pitch, F == NV12 ? y.pitch : y.pitch_c, y.u_offset, y.v_offset, y.frame_bytes};
    const int h = y.h, w = y.w;
    const bool ident = h == out_h && w == out_w;
    const bool wide = wide_access(frame, y) && wide_access(dst, y);
    const int label_dword = ident && W % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 4 == 0;
    const long patches = (long)((w + 3) / 4) * (h / Patch<F>::ROWS);
    const dim3 grid((unsigned)((patches + 255) / 256), 1, (unsigned)n);
#define OVL_LAUNCH(IDENT, WIDE)                                                                                                             \
    hipLaunchKernelGGL((overlay_yuv_kernel<F, IDENT, WIDE>), grid, dim3(256), 0, st, labels, H, W, out_h, out_w, h, w, l, pal, alpha, frame, dst, \
                       label_dword)
    if (ident) { if (wide) OVL_LAUNCH(true, true); else OVL_LAUNCH(true, false); }
    else { if (wide) OVL_LAUNCH(false, true); else OVL_LAUNCH(false, false); }
#undef OVL_LAUNCH
    return hipGetLastError();
}

}  // namespace

// n label maps of H x W bytes (valid region out_h x out_w, top left) blended with weight alpha / 256 over n frames laid out as `y` says (format 3:
// NV12, interleaved 8-bit chroma at u_offset, rows `pitch` apart; y.colour is not looked at) into `dst`, which has the same layout and may be
// `frame` itself.  palette_ycc: 768 host words, (Y, Cb, Cr) per label in the units of the samples.  The caller (accel_io.cpp overlay_args) has
// checked the layout, the geometry, alpha, the table's range, P010's 2-byte alignment of both addresses, and that the two buffers are equal or
// disjoint.  Reads of `labels` stay inside out_h x out_w of each map; reads of `frame` and writes of `dst` inside the samples of each frame.
hipError_t launch_overlay_yuv(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, const YuvLayout& y, const uint16_t* palette_ycc,
                              int alpha, const unsigned char* frame, unsigned char* dst, hipStream_t st)
{
    TableYcc pal;
    for (int i = 0; i < 768; ++i) pal.ycc[i] = palette_ycc[i];
    switch (y.format) {
    case I420: return overlay_yuv<I420>(labels, n, H, W, out_h, out_w, y, pal, alpha, frame, dst, st);
    case P010: return overlay_yuv<P010>(labels, n, H, W, out_h, out_w, y, pal, alpha, frame, dst, st);
    case YUY2: return overlay_yuv<YUY2>(labels, n, H, W, out_h, out_w, y, pal, alpha, frame, dst, st);
    case NV12: return overlay_yuv<NV12>(labels, n, H, W, out_h, out_w, y, pal, alpha, frame, dst, st);
    }
    return hipErrorInvalidValue;
}
