// How sure the network was, per source pixel: the scores tensor (n x NCLS x H x W fp32, NCHW, the layout of `logits`) read once and finished where
// it lies -- as the largest softmax probability in 256 levels, as the margin between the two best scores, as the runner-up class, as a histogram of
// the levels per frame and, in the interpolated form, as the label.  ONE kernel in two forms, which differ in where a pixel's NCLS values come from:
//   nearest        the stored scores of the map pixel results_u8.hip takes (labels_nearest.h), so every output lines up pixel for pixel with
//                  launch_labels_source: conf, margin and second describe the winner `labels` names there
//   interpolated   every class plane interpolated bilinearly to the source pixel as scores_labels.hip does it (scores_interp.h: taps clamped to the
//                  valid region, a float64 blend); the label is the argmax launch_scores_labels writes, found on the way, and conf, margin and
//                  second describe THAT winner.  Restates accel_amd/utils/image.py confidence_interpolated_host bit for bit up to the exp.
// Geometry: one valid region out_h x out_w in the top-left corner of the H x W map, one source size h x w.
//
// Arithmetic (finish_values), on the values v_k -- fp32 stored scores or float64 interpolated ones; an fp32 value is compared as it is (the
// conversion to double is exact and monotone: the same scan) and widened where the arithmetic begins:
//     label = the first maximal class (the tail's argmax), second = the first maximal class among the others
//     conf  = min(255, floor(256 * p)),  p = 1 / sum_k exp(v_k - v[label])
// with the differences, exp, the sum (classes in ascending order), the reciprocal and the scaling in float64: the byte is a function of the values
// and differs from a float64 restatement on the host only where 256 * p lies within ~1e-13 of an integer; a NaN gives 0.  Exact whatever the exp:
// m-way ties of everything (p = 1 / m), two equal classes of two (128), saturation (p = 1 -> 256 -> 255).
// PROB: the values are probabilities already (a tail lowered with softmax=1): conf = min(255, floor(256 * double(v[label]))), no exponential.
// The margin (0 on a tie at the top) is rounded by the rule of the form, a parameter of finish_values:
//     nearest        v[label] - v[second], ONE fp32 subtraction of two stored values
//     interpolated   float(double(v[label]) - double(v[second])), ONE float64 subtraction rounded once -- also where the values are stored scores
//                    (the identity geometry), whose difference is exact in float64 unless their exponents lie more than 29 apart: only there do the
//                    two rules differ
// Interpolated scores are assumed FINITE: a pixel with a non-finite tap is unspecified (inf * 0 arises in the blend).
//
// V = 1: one source pixel per thread, consecutive lanes consecutive x of one row; gathered (nearest) or all NCLS x 4 tap loads issued before the
// arithmetic (interpolated: the taps die as the v_k are made, the NCLS doubles live on through the scan and the exp loop).
// V = 4: the identity geometry with widths, pitches and addresses allowing (the launcher checks): a thread owns 4 consecutive pixels, one 16-byte
// load per class plane (coalesced along x), the scan on the stored scores -- which ARE the values of both forms there -- dword / float4 stores.
// (The blend's a * 1 + b * 0 turns a stored -0 into +0 unless b is negative too; this path keeps it.  They compare equal: only the sign of a zero
// margin can differ, on a tie at the top between zeros.)
// Histogram: levels_hist.h -- runs of equal levels counted in a register, then in 256 block-private 32-bit LDS bins, then one 64-bit atomic per
// non-zero bin per block into the frame's 256 words (as labels_hist_kernel does).  blockIdx.z is the frame: a block never spans two.
// Integer sums: exact, independent of the order of arrival.  The kernel only READS the scores.
#include "kernels.h"
#include "labels_nearest.h"
#include "levels_hist.h"
#include "scores_interp.h"
#include <stdint.h>

namespace {

// MARGIN64: the margin is the float64 difference rounded once (the interpolated form) instead of the fp32 difference (the nearest form)
template <int NCLS, bool PROB, bool MARGIN64, typename T>
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
    margin = MARGIN64 ? (float)(top - (double)v2) : (float)v1 - (float)v2;
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

template <int NCLS, int V, bool PROB, bool INTERP>
__global__ __launch_bounds__(256) void confidence_kernel(const float* __restrict__ scores, int H, int W, int out_h, int out_w, int h, int w, ConfOut o)
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
                finish_values<NCLS, PROB, INTERP>(l, lab[j], c[j], mg[j], s[j]);
            }
        } else if (INTERP) {
            const interp::Tap ty = interp::tap(y, h, out_h), tx = interp::tap(x0, w, out_w);
            const float* r0 = img + (size_t)ty.i0 * W;
            const float* r1 = img + (size_t)ty.i1 * W;
            interp::Taps a[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) a[k] = interp::load_taps(r0, r1, (size_t)k * plane, tx.i0, tx.i1);
            const interp::Weights wt(ty, tx);
            double v[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) v[k] = interp::blend(a[k], wt);
            finish_values<NCLS, PROB, true>(v, lab[0], c[0], mg[0], s[0]);
        } else {
            const float* p = img + (size_t)nearest::source_row(y, out_h, h) * W + nearest::Column(x0, out_w, w).col();
            float l[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) l[k] = p[(size_t)k * plane];
            finish_values<NCLS, PROB, false>(l, lab[0], c[0], mg[0], s[0]);
        }
        const size_t row = (size_t)z * h + y;
        if (V == 4) {
            if (INTERP && o.labels) *reinterpret_cast<uint32_t*>(o.labels + row * o.labels_pitch + x0) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            if (o.conf) *reinterpret_cast<uint32_t*>(o.conf + row * o.conf_pitch + x0) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            if (o.second) *reinterpret_cast<uint32_t*>(o.second + row * o.second_pitch + x0) = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
            if (o.margin)
                *reinterpret_cast<float4*>(reinterpret_cast<char*>(o.margin) + row * o.margin_pitch + (size_t)x0 * 4) = make_float4(mg[0], mg[1], mg[2], mg[3]);
        } else {
            if (INTERP && o.labels) o.labels[row * o.labels_pitch + x0] = (unsigned char)lab[0];
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

template <int NCLS>
hipError_t launch_ncls(const float* scores, int n, int H, int W, int out_h, int out_w, int h, int w, int is_prob, bool interp, const ConfOut& o,
                       hipStream_t st)
{
    using nearest::aligned;
    const bool vec = h == out_h && w == out_w && w % 4 == 0 && W % 4 == 0 && aligned(scores, 16) &&
                     (!o.labels || (o.labels_pitch % 4 == 0 && aligned(o.labels, 4))) && (!o.conf || (o.conf_pitch % 4 == 0 && aligned(o.conf, 4))) &&
                     (!o.second || (o.second_pitch % 4 == 0 && aligned(o.second, 4))) && (!o.margin || (o.margin_pitch % 16 == 0 && aligned(o.margin, 16)));
    const long units = (long)(vec ? w / 4 : w) * h;
    // few enough blocks per frame that the 64-bit atomics of their epilogues stay a footnote (a block sees fewer than 2^32 pixels: a frame has at
    // most 2^30); the grid-stride loop takes the rest
    long blocks = (units + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    const dim3 grid((unsigned)blocks, 1, (unsigned)n);
#define CONF_LAUNCH(V, PROB, INTERP) \
    hipLaunchKernelGGL((confidence_kernel<NCLS, V, PROB, INTERP>), grid, dim3(256), 0, st, scores, H, W, out_h, out_w, h, w, o)
#define CONF_FORM(V, PROB) do { if (interp) CONF_LAUNCH(V, PROB, true); else CONF_LAUNCH(V, PROB, false); } while (0)
    if (vec) { if (is_prob) CONF_FORM(4, true); else CONF_FORM(4, false); }
    else { if (is_prob) CONF_FORM(1, true); else CONF_FORM(1, false); }
#undef CONF_FORM
#undef CONF_LAUNCH
    return hipGetLastError();
}

}  // namespace

// The callers (accel_io.cpp confidence_args) have checked: 1 <= n <= 32768, h, w >= 1, 1 <= out_h <= H, 1 <= out_w <= W <= 32768, h, w <= 32768, ncls in
// {2, 19, 21}, pitches >= a row, margin_pitch % 4 == 0, at least one output, no labels in the nearest form.  Reads of `scores` stay inside out_h x
// out_w of each of the n * ncls planes (the nearest row and column, and both taps of a row and of a column, are clamped into the region), writes
// inside w (4 * w) bytes of each of the n * h rows and the n * 256 words of hist, which are OVERWRITTEN (zeroed here first).
hipError_t launch_confidence(const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, int is_prob, bool interp,
                             const ConfOut& o, hipStream_t st)
{
    if (o.labels && !interp) return hipErrorInvalidValue;
    if (o.hist) {
        const hipError_t e = hipMemsetAsync(o.hist, 0, (size_t)n * 256 * sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
    }
    switch (ncls) {
    case 2: return launch_ncls<2>(scores, n, H, W, out_h, out_w, h, w, is_prob, interp, o, st);
    case 19: return launch_ncls<19>(scores, n, H, W, out_h, out_w, h, w, is_prob, interp, o, st);
    case 21: return launch_ncls<21>(scores, n, H, W, out_h, out_w, h, w, is_prob, interp, o, st);
    }
    return hipErrorInvalidValue;
}
