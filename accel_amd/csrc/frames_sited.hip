// Interpolated chroma siting, formats 0 .. 3: where the sources of frames_yuv.hip hand every luma pixel the chroma sample of its block, these
// interpolate Cb and Cr to the luma pixel first, as the siting of the frame says, and feed the result to the same colour rule.  The sample
// sources that the kernels of frames_yuv.h run on for siting 1 .. 3, and the dispatch of every YUV frame route over format and siting.
//
// Restates accel_amd/utils/image.py chroma_upsample bit for bit.
//   chroma      planes of cw = w/2 columns and ch = h/2 rows (ch = h and no vertical step for YUY2).  For luma pixel (x, y), k = x >> 1 and
//               j = y >> 1; each axis takes two neighbouring samples with weights that sum to 4:
//                   co-sited (sample k lies on luma 2k)         even coordinate: (k: 4)            odd: (k: 2, k+1: 2)
//                   centred  (sample k lies on luma 2k + 0.5)   even coordinate: (k-1: 1, k: 3)    odd: (k: 3, k+1: 1)
//               indices clamped to [0, cw-1] and [0, ch-1], and C = (sum_rows sum_cols wy wx c[row][col] + 8) >> 4 for Cb and Cr alike: one
//               rounding, none between the axes.  P010: on the 10-bit word >> 6 samples.
//   siting      1 left: horizontal co-sited, vertical centred;  2 centre: both centred;  3 topleft: both co-sited.  Interlaced siting is not
//               offered.
// Store-bound like the replicated sources: the same bytes cross HBM; the neighbouring chroma samples (up to 4 columns x 3 rows around a patch)
// are clamped scalar loads that other threads of the block have brought into L1/L2.
#include "frames_yuv.h"

namespace {

using namespace yuv;

enum { COSITED = 0, CENTRED = 1, NOSTEP = 2 };      // how an axis interpolates

// siting S (1 .. 3) of format F -> the modes of its two axes
template <int F, int S> struct Axes {
    static constexpr int H = S == 2 ? CENTRED : COSITED;
    static constexpr int V = F == YUY2 ? NOSTEP : (S == 3 ? COSITED : CENTRED);
};

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

template <int F, int S> struct Sited {
    static constexpr int ROWS = Patch<F>::ROWS;

    // up to 2 x 2 chroma samples
    static __device__ __forceinline__ uint32_t pixel(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x, int y, const Coef& k)
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

    // w is even (and h where ROWS == 2), so the rows of a patch are inside or outside together.  WIDE (wide_loads below): the wide luma loads
    // of a whole patch: a dword per row (I420, NV12), two dwords (YUY2), 8 bytes (P010).  The chroma a patch needs is the table of columns
    // (x0 >> 1) - 1 .. (x0 >> 1) + 2 and rows (y >> 1) - 1 .. (y >> 1) + 1, each index clamped to the plane: a centred axis uses all of it, a
    // co-sited one neither the first column nor the first row, YUY2 its own row alone.
    template <bool WIDE>
    static __device__ __forceinline__ void patch(const unsigned char* __restrict__ img, const Layout& l, int h, int w, int x0, int y, const Coef& k,
                                                 uint32_t (&px)[ROWS][4])
    {
        constexpr int HM = Axes<F, S>::H, VM = Axes<F, S>::V;
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
};

// whether the luma of every whole patch of every frame may be read with the wide loads above: x0 is a multiple of 4, so what has to be aligned
// is the start of every luma row of every frame (chroma is read sample by sample)
bool wide_loads(const unsigned char* src, const YuvLayout& y)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    return (a | y.pitch | y.frame_bytes) % (y.format == P010 ? 8 : 4) == 0;
}

template <int F, class Launch>
hipError_t with_siting(int siting, Launch launch)
{
    switch (siting) {
    case 1: return launch(Sited<F, 1>());
    case 2: return launch(Sited<F, 2>());
    case 3: return launch(Sited<F, F == YUY2 ? 1 : 3>());      // YUY2: left and topleft coincide
    }
    return hipErrorInvalidValue;
}

// launch(source) for the source of `format` and `siting` (1 .. 3)
template <class Launch>
hipError_t with_source(int format, int siting, Launch launch)
{
    switch (format) {
    case I420: return with_siting<I420>(siting, launch);
    case P010: return with_siting<P010>(siting, launch);
    case YUY2: return with_siting<YUY2>(siting, launch);
    case NV12: return with_siting<NV12>(siting, launch);
    }
    return hipErrorInvalidValue;
}

}  // namespace

// n frames in device memory -> n x 3 x H x W fp32 planar RGB, chroma sited as `siting` says (0: replicated).  What the caller has checked, and
// what the kernels then keep to: launch_frames of frames_yuv.h.
hipError_t launch_frames_yuv(const unsigned char* src, int n, const YuvLayout& y, int siting, const double* means_bgr, int out_h, int out_w,
                             double step, int H, int W, float* dst, hipStream_t st)
{
    if (siting == 0) return yuv::frames_replicated(src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    return with_source(y.format, siting, [&](auto s) {
        return yuv::launch_frames<decltype(s)>(wide_loads, src, n, y, means_bgr, out_h, out_w, step, H, W, dst, st);
    });
}

// n frames in device memory -> n x h x w x 3 BGR bytes, rows `out_pitch` bytes apart (>= 3 * w), h * out_pitch from frame to frame
hipError_t launch_yuv_to_bgr(const unsigned char* src, int n, const YuvLayout& y, int siting, unsigned char* dst, size_t out_pitch, hipStream_t st)
{
    if (siting == 0) return yuv::replicated_to_bgr(src, n, y, dst, out_pitch, st);
    return with_source(y.format, siting, [&](auto s) { return yuv::launch_to_bgr<decltype(s)>(wide_loads, src, n, y, dst, out_pitch, st); });
}
