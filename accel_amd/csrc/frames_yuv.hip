// Replicated chroma, formats 0 .. 3: every luma pixel of an I420, P010, YUY2 or NV12 frame takes the chroma sample of its 2 x 2 block (of its
// pair, for YUY2) -- pixel (x, y) takes Cb, Cr at (x >> 1, y >> 1), YUY2 those of quad x >> 1 of its own row.  The sample sources that the
// kernels of frames_yuv.h run on for siting 0, and the two tables of colour integers.
#include "frames_yuv.h"

namespace {

using namespace yuv;

// (yoff, ky, krv, kgu, kgv, kbu) = round(65536 x the standard's value) for BT.601 / BT.709, limited / full range: held to
// image.nv12_coefficients by the CPU suite
//                                 yoff  ky     krv     kgu    kgv    kbu
const int32_t NV12_COEF[4][6] = {{16, 76309, 104597, 25675, 53279, 132201},      // 0  BT.601 limited range
                                 {0,  65536, 91881,  22553, 46802, 116130},      // 1  BT.601 full range
                                 {16, 76309, 117489, 13975, 34925, 138438},      // 2  BT.709 limited range
                                 {0,  65536, 103206, 12276, 30679, 121609}};     // 3  BT.709 full range

// P010: the same five integers for the limited-range modes (the 10-bit signal is 4 times the 8-bit one) and round(65536 x value x 1020 / 1023)
// for the full-range ones: held to image.yuv10_coefficients by the CPU suite
//                                  yoff  ky     krv     kgu    kgv    kbu
const int32_t YUV10_COEF[4][6] = {{16, 76309, 104597, 25675, 53279, 132201},      // 0  BT.601 limited range: the 8-bit integers
                                  {0,  65344, 91612,  22487, 46664, 115789},      // 1  BT.601 full range: x 1020 / 1023
                                  {16, 76309, 117489, 13975, 34925, 138438},      // 2  BT.709 limited range: the 8-bit integers
                                  {0,  65344, 102903, 12240, 30589, 121252}};    // 3  BT.709 full range: x 1020 / 1023

// ---- I420, P010, YUY2 -------------------------------------------------------------------------------------------------------------------------
template <int F> struct Replicated {
    static constexpr int ROWS = Patch<F>::ROWS;

    static __device__ __forceinline__ uint32_t pixel(const unsigned char* __restrict__ img, const Layout& l, int, int, int x, int y, const Coef& k)
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

    // w is even (and h where ROWS == 2), so the rows of a patch, and both pixels of a chroma pair, are inside or outside together.  WIDE
    // (wide_loads below) --
    //   I420   two luma dwords and one 16-bit load from each chroma plane
    //   YUY2   two dwords (Y0 Cb0 Y1 Cr0 | Y2 Cb1 Y3 Cr1)
    //   P010   two 8-byte luma loads and one 8-byte chroma load (Cb0 Cr0 Cb1 Cr1)
    template <bool WIDE>
    static __device__ __forceinline__ void patch(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x0, int y, const Coef& k,
                                                 uint32_t (&px)[ROWS][4])
    {
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
};

// whether every whole patch of every frame may be read with the wide loads above: x0 is a multiple of 4, so what has to be aligned is the start
// of every row of every plane of every frame
bool wide_loads(const unsigned char* src, const YuvLayout& y)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    switch (y.format) {
    case I420: return (a | y.pitch | y.frame_bytes) % 4 == 0 && (y.pitch_c | y.u_offset | y.v_offset) % 2 == 0;
    case YUY2: return (a | y.pitch | y.frame_bytes) % 4 == 0;
    default:   return (a | y.pitch | y.frame_bytes | y.u_offset) % 8 == 0;
    }
}

// ---- NV12 -------------------------------------------------------------------------------------------------------------------------------------
template <> struct Replicated<NV12> {
    static constexpr int ROWS = 2;

    static __device__ __forceinline__ uint32_t pixel(const unsigned char* __restrict__ img, const Layout& l, int, int, int x, int y, const Coef& k)
    {
        const unsigned char* uv = img + l.u_offset + (size_t)(y >> 1) * l.pitch + (x & ~1);
        return to_bgr<NV12>(img[(size_t)y * l.pitch + x], uv[0], uv[1], k);
    }

    // h and w are even, so both rows, and both pixels of a chroma pair, are inside or outside together.  WIDE (dwords below): a whole patch is
    // two luma dwords and one chroma dword (Cb0 Cr0 Cb1 Cr1), each chroma byte read once; a patch the frame's edge cuts, and every patch without
    // WIDE, is gathered from bytes into the same three dwords.  A width with w % 4 == 2 keeps the dword loads: only the cut patch reads bytes.
    template <bool WIDE>
    static __device__ __forceinline__ void patch(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x0, int y, const Coef& k,
                                                 uint32_t (&px)[2][4])
    {
        if (y >= h || x0 >= w) return;
        const unsigned char* y0 = img + (size_t)y * l.pitch + x0;
        const unsigned char* y1 = y0 + l.pitch;
        const unsigned char* uv = img + l.u_offset + (size_t)(y >> 1) * l.pitch + x0;
        uint32_t l0 = 0, l1 = 0, c = 0;
        const int cols = min(4, w - x0);      // 4 or 2
        if (WIDE && cols == 4) {
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
                px[0][i] = to_bgr<NV12>((l0 >> (8 * i)) & 255u, cb, cr, k);
                px[1][i] = to_bgr<NV12>((l1 >> (8 * i)) & 255u, cb, cr, k);
            }
        }
    }
};

bool dwords(const unsigned char* src, const YuvLayout& y)
{
    return y.pitch % 4 == 0 && y.u_offset % 4 == 0 && y.frame_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0;
}

// launch(source, predicate) for the source of `format`
template <class Launch>
hipError_t with_source(int format, Launch launch)
{
    switch (format) {
    case I420: return launch(Replicated<I420>(), wide_loads);
    case P010: return launch(Replicated<P010>(), wide_loads);
    case YUY2: return launch(Replicated<YUY2>(), wide_loads);
    case NV12: return launch(Replicated<NV12>(), dwords);
    }
    return hipErrorInvalidValue;
}

}  // namespace

const int32_t* nv12_coefficients(int colour)
{
    return colour >= 0 && colour < 4 ? NV12_COEF[colour] : nullptr;
}

const int32_t* yuv10_coefficients(int colour)
{
    return colour >= 0 && colour < 4 ? YUV10_COEF[colour] : nullptr;
}

hipError_t yuv::frames_replicated(const unsigned char* src, int n, const YuvLayout& y, const double* means_bgr, int out_h, int out_w, double step,
                                  int H, int W, float* dst, hipStream_t st)
{
    return with_source(y.format, [&](auto s, WidePredicate wide) {
        return launch_frames<decltype(s)>(wide, src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    });
}

hipError_t yuv::replicated_to_bgr(const unsigned char* src, int n, const YuvLayout& y, unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    return with_source(y.format, [&](auto s, WidePredicate wide) { return launch_to_bgr<decltype(s)>(wide, src, n, y, dst, out_pitch, st); });
}
