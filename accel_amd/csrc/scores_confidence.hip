// The confidence of INTERPOLATED scores, in one pass with their labels: the scores tensor (n x NCLS x H x W fp32, NCHW, the layout of `logits`) is
// read once where it lies, every class plane is interpolated bilinearly to the source pixel as scores_labels.hip does it, and from those values
// v_k the pixel is finished as confidence.hip finishes a stored pixel -- the largest softmax probability in 256 levels, the margin between the two
// best values, the runner-up class, a histogram of the levels per frame -- and, because it has been found on the way, as the label: the argmax
// launch_scores_labels writes.  So conf, margin and second describe the winner that label names, where confidence.hip describes the nearest map
// pixel's.  The arithmetic restates accel_amd/utils/image.py confidence_interpolated_host bit for bit up to the exp.
//
// Geometry: that of scores_labels.hip (one valid region out_h x out_w in the top-left corner of the H x W map, one source size h x w).
// Taps: scores_interp.h (integer arithmetic, clamped to the valid region -- the padding is never read -- one IEEE division per weight).
// Blend, in float64, each operation rounded on its own (no fma), in the order of scores_labels.hip; a<row><col> the fp32 taps as doubles:
//     gx = 1 - fx;  gy = 1 - fy;  top = a00 * gx + a01 * fx;  bot = a10 * gx + a11 * fx;  v_k = top * gy + bot * fy
// Scan, on the float64 v_k: label = the first maximal class, second = the first maximal class among the others,
//     margin = float(v[label] - v[second])        ONE float64 subtraction, rounded once to fp32 (0 on a tie at the top)
//     conf   = min(255, floor(256 * p)),  p = 1 / sum_k exp(v_k - v[label])       classes in ascending order, all in float64; a NaN gives 0
// PROB: the stored values are probabilities, blended the same way: conf = min(255, floor(256 * v[label])), no exponential.
// Scores are assumed FINITE: a pixel with a non-finite tap is unspecified (inf * 0 arises in the blend).
// At h x w == out_h x out_w every weight is 0 and v_k is the stored score: conf, second and hist are those of confidence.hip, the label is
// the crop of `labels`, and the margin -- the difference of two fp32 values, exact in float64 unless their exponents lie more than 29 apart --
// is its fp32 subtraction.
//
// V = 1: one source pixel per thread; consecutive lanes take consecutive x of one row.  All NCLS x 4 tap loads are issued before the arithmetic;
// the taps die as the v_k are made, and the NCLS doubles live on through the scan and the exp loop.
// V = 4: the identity geometry with widths, pitches and addresses allowing (the launcher checks): a thread owns 4 consecutive pixels, one 16-byte
// load per class plane, the same scan on the stored scores, dword / float4 stores.  (The blend's a * 1 + b * 0 turns a stored -0 into +0
// unless b is negative too; this path keeps it.  They compare equal: only the sign of a zero margin can differ, on a tie at the top between zeros.)
// Histogram: levels_hist.h, shared with confidence.hip -- runs of equal levels counted in a register, then in 256 block-private 32-bit LDS bins,
// then one 64-bit atomic per non-zero bin per block into the frame's 256 words.  blockIdx.z is the frame: a block never spans two.
// Integer sums: exact, independent of the order of arrival.  The kernel only READS the scores.
#include "kernels.h"
#include "levels_hist.h"
#include "scores_interp.h"
#include <stdint.h>

namespace {

// T = double: the interpolated values.  T = float: the stored scores of the identity geometry, which ARE the values there -- compared as floats
// (the conversion to double is exact and monotone: the same scan), widened where the arithmetic begins.
template <int NCLS, bool PROB, typename T>
__device__ __forceinline__ void finish_values(const T (&v)[NCLS], unsigned& label, unsigned& conf, float& margin, unsigned& second)
{
#pragma clang fp contract(off)
    int best = v[1] > v[0] ? 1 : 0, sec = 1 - best;
    T v1 = v[best], v2 = v[sec];
#pragma unroll
    for (int k = 2; k < NCLS; ++k) {
        const T x = v[k];
        if (x > v1) { sec = best; v2 = v1; best = k; v1 = x; }
        else if (x > v2) { sec = k; v2 = x; }
    }
    label = (unsigned)best;
    second = (unsigned)sec;
    const double top = (double)v1;
    margin = (float)(top - (double)v2);
    double scaled;
    if (PROB) {
        scaled = 256.0 * top;
    } else {
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < NCLS; ++k) sum += exp((double)v[k] - top);
        scaled = 256.0 * (1.0 / sum);
    }
    const double f = floor(scaled);
    conf = f >= 255.0 ? 255u : f > 0.0 ? (unsigned)f : 0u;      // (a NaN gives 0)
}

struct InterpOut {
    unsigned char* labels; size_t labels_pitch;
    unsigned char* conf; size_t conf_pitch;
    float* margin; size_t margin_pitch;        // bytes, a multiple of 4 (of 16 when V = 4)
    unsigned char* second; size_t second_pitch;
    unsigned long long* hist;                  // n x 256
};

template <int NCLS, int V, bool PROB>
__global__ __launch_bounds__(256) void scores_confidence_kernel(const float* __restrict__ scores, int H, int W, int out_h, int out_w, int h, int w,
                                                                InterpOut o)
{
    __shared__ unsigned bins[256];
    const bool want_hist = o.hist != nullptr;      // uniform
    if (want_hist) {
        bins[threadIdx.x] = 0;
        __syncthreads();
    }
    const int z = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const float* img = scores + (size_t)z * NCLS * plane;
    const int QW = w / V;                          // V = 4: w % 4 == 0
    const long units = (long)QW * h;
    unsigned key = 0, cnt = 0;                     // the run of equal levels this thread is in

    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
        const int y = (int)(u / QW), x0 = (int)(u - (long)y * QW) * V;
        unsigned lab[V], c[V], s[V];
        float mg[V];
        if (V == 4) {
            const float* p = img + (size_t)y * W + x0;
            float4 t[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) t[k] = *reinterpret_cast<const float4*>(p + (size_t)k * plane);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float l[NCLS];
#pragma unroll
                for (int k = 0; k < NCLS; ++k) l[k] = j == 0 ? t[k].x : j == 1 ? t[k].y : j == 2 ? t[k].z : t[k].w;
                finish_values<NCLS, PROB>(l, lab[j], c[j], mg[j], s[j]);
            }
        } else {
#pragma clang fp contract(off)
            const interp::Tap ty = interp::tap(y, h, out_h), tx = interp::tap(x0, w, out_w);
            const float* r0 = img + (size_t)ty.i0 * W;
            const float* r1 = img + (size_t)ty.i1 * W;
            float a00[NCLS], a01[NCLS], a10[NCLS], a11[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) {
                a00[k] = r0[(size_t)k * plane + tx.i0]; a01[k] = r0[(size_t)k * plane + tx.i1];
                a10[k] = r1[(size_t)k * plane + tx.i0]; a11[k] = r1[(size_t)k * plane + tx.i1];
            }
            const double fx = tx.f, fy = ty.f, gx = 1.0 - fx, gy = 1.0 - fy;
            double v[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) {
                const double t0 = (double)a00[k] * gx, t1 = (double)a01[k] * fx;
                const double top = t0 + t1;
                const double b0 = (double)a10[k] * gx, b1 = (double)a11[k] * fx;
                const double bot = b0 + b1;
                const double u0 = top * gy, u1 = bot * fy;
                v[k] = u0 + u1;
            }
            finish_values<NCLS, PROB>(v, lab[0], c[0], mg[0], s[0]);
        }
        const size_t row = (size_t)z * h + y;
        if (V == 4) {
            if (o.labels) *reinterpret_cast<uint32_t*>(o.labels + row * o.labels_pitch + x0) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            if (o.conf) *reinterpret_cast<uint32_t*>(o.conf + row * o.conf_pitch + x0) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            if (o.second) *reinterpret_cast<uint32_t*>(o.second + row * o.second_pitch + x0) = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
            if (o.margin)
                *reinterpret_cast<float4*>(reinterpret_cast<char*>(o.margin) + row * o.margin_pitch + (size_t)x0 * 4) = make_float4(mg[0], mg[1], mg[2], mg[3]);
        } else {
            if (o.labels) o.labels[row * o.labels_pitch + x0] = (unsigned char)lab[0];
            if (o.conf) o.conf[row * o.conf_pitch + x0] = (unsigned char)c[0];
            if (o.second) o.second[row * o.second_pitch + x0] = (unsigned char)s[0];
            if (o.margin) *reinterpret_cast<float*>(reinterpret_cast<char*>(o.margin) + row * o.margin_pitch + (size_t)x0 * 4) = mg[0];
        }
        if (want_hist) {
#pragma unroll
            for (int j = 0; j < V; ++j) levels::count(bins, key, cnt, c[j]);
        }
    }

    if (want_hist) levels::flush(bins, key, cnt, o.hist + (size_t)z * 256);
}

inline bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

template <int NCLS>
hipError_t launch_ncls(const float* scores, int n, int H, int W, int out_h, int out_w, int h, int w, int is_prob, const InterpOut& o, hipStream_t st)
{
    const bool vec = h == out_h && w == out_w && w % 4 == 0 && W % 4 == 0 && aligned(scores, 16) &&
                     (!o.labels || (o.labels_pitch % 4 == 0 && aligned(o.labels, 4))) && (!o.conf || (o.conf_pitch % 4 == 0 && aligned(o.conf, 4))) &&
                     (!o.second || (o.second_pitch % 4 == 0 && aligned(o.second, 4))) && (!o.margin || (o.margin_pitch % 16 == 0 && aligned(o.margin, 16)));
    const long units = (long)(vec ? w / 4 : w) * h;
    // few enough blocks per frame that the 64-bit atomics of their epilogues stay a footnote (a block sees fewer than 2^32 pixels: a frame has at
    // most 2^30); the grid-stride loop takes the rest
    long blocks = (units + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    const dim3 grid((unsigned)blocks, 1, (unsigned)n);
#define INTERP_LAUNCH(V, PROB) \
    hipLaunchKernelGGL((scores_confidence_kernel<NCLS, V, PROB>), grid, dim3(256), 0, st, scores, H, W, out_h, out_w, h, w, o)
    if (vec) { if (is_prob) INTERP_LAUNCH(4, true); else INTERP_LAUNCH(4, false); }
    else { if (is_prob) INTERP_LAUNCH(1, true); else INTERP_LAUNCH(1, false); }
#undef INTERP_LAUNCH
    return hipGetLastError();
}

}  // namespace

// The callers (accel_io.cpp confidence_args) have checked: 1 <= n <= 32768, h, w >= 1, 1 <= out_h <= H, 1 <= out_w <= W <= 32768, h, w <= 32768, ncls in
// {2, 19, 21}, pitches >= a row, margin_pitch % 4 == 0, at least one output.  Reads of `scores` stay inside out_h x out_w of each of the n * ncls planes
// (both taps of a row and of a column are clamped into the region), writes inside w (4 * w) bytes of each of the n * h rows and the n * 256 words of
// hist, which are OVERWRITTEN (zeroed here first).
hipError_t launch_scores_confidence(const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, int is_prob,
                                    unsigned char* labels, size_t labels_pitch, unsigned char* conf, size_t conf_pitch, float* margin, size_t margin_pitch,
                                    unsigned char* second, size_t second_pitch, unsigned long long* hist, hipStream_t st)
{
    if (hist) {
        const hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
    }
    const InterpOut o = {labels, labels_pitch, conf, conf_pitch, margin, margin_pitch, second, second_pitch, hist};
    switch (ncls) {
    case 2: return launch_ncls<2>(scores, n, H, W, out_h, out_w, h, w, is_prob, o, st);
    case 19: return launch_ncls<19>(scores, n, H, W, out_h, out_w, h, w, is_prob, o, st);
    case 21: return launch_ncls<21>(scores, n, H, W, out_h, out_w, h, w, is_prob, o, st);
    }
    return hipErrorInvalidValue;
}
