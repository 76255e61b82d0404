// How sure the network was, per source pixel: the scores tensor (n x NCLS x H x W fp32, NCHW, the layout of `logits`) read once and
// finished where it lies -- as the largest softmax probability in 256 levels, as the margin between the two best scores, as the
// runner-up class, and as a histogram of the levels per frame.
//
// The geometry is that of results_u8.hip (one valid region out_h x out_w in the top-left corner of the H x W map, one source size
// h x w, source pixel (y, x) takes map pixel (min(y * out_h / h, out_h - 1), min(x * out_w / w, out_w - 1)) in integer division), so
// every output lines up pixel for pixel with launch_labels_source.
//
// Arithmetic.  best = the first maximal class (the tail's argmax: `labels`); second = the first maximal class among the others;
// margin = l[best] - l[second], ONE fp32 subtraction of two stored values (0 on a tie at the top).
//   conf = min(255, floor(256 * p)),  p = 1 / sum_k exp(l_k - l[best])
// with the differences, exp, the sum (classes in ascending order), the reciprocal and the scaling in float64: the byte is a function of
// the scores and differs from a float64 restatement on the host only where 256 * p lies within ~1e-13 of an integer.  Exact whatever
// the exp: m-way ties of everything (p = 1 / m), two equal classes of two (128), saturation (p = 1 -> 256 -> 255).
// PROB: the stored values are probabilities already (a tail lowered with softmax=1): conf = min(255, floor(256 * double(l[best]))),
// no exponential; margin and second as above, on the stored values.
//
// V = 4: the identity geometry with widths, pitches and addresses allowing (the launcher checks): a thread owns 4 consecutive pixels,
// one 16-byte load per class plane (coalesced along x), uchar4 / float4 stores.  V = 1: one source pixel per thread, gathered, scalar.
// Histogram: runs of equal levels are counted in a register, then in 256 block-private 32-bit LDS bins, then one 64-bit atomic per
// non-zero bin per block into the frame's 256 words (as labels_hist_kernel does).  blockIdx.z is the frame: a block never spans two.
// Integer sums: exact, independent of the order of arrival.  The kernel only READS the scores.
#include "kernels.h"
#include "levels_hist.h"
#include <stdint.h>

namespace {

template <int NCLS, bool PROB>
__device__ __forceinline__ void finish_pixel(const float (&l)[NCLS], unsigned& conf, float& margin, unsigned& second)
{
    int best = l[1] > l[0] ? 1 : 0, sec = 1 - best;
    float v1 = l[best], v2 = l[sec];
#pragma unroll
    for (int k = 2; k < NCLS; ++k) {
        const float x = l[k];
        if (x > v1) { sec = best; v2 = v1; best = k; v1 = x; }
        else if (x > v2) { sec = k; v2 = x; }
    }
    margin = v1 - v2;
    second = (unsigned)sec;
    double scaled;
    if (PROB) {
        scaled = 256.0 * (double)v1;
    } else {
        const double top = (double)v1;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < NCLS; ++k) sum += exp((double)l[k] - top);
        scaled = 256.0 * (1.0 / sum);
    }
    const double f = floor(scaled);
    conf = f >= 255.0 ? 255u : f > 0.0 ? (unsigned)f : 0u;      // (a NaN gives 0)
}

struct ConfOut {
    unsigned char* conf; size_t conf_pitch;
    float* margin; size_t margin_pitch;        // bytes, a multiple of 4 (of 16 when V = 4)
    unsigned char* second; size_t second_pitch;
    unsigned long long* hist;                  // n x 256
};

template <int NCLS, int V, bool PROB>
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
        unsigned c[V], s[V];
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
                finish_pixel<NCLS, PROB>(l, c[j], mg[j], s[j]);
            }
        } else {
            const int sy = min((int)((unsigned)y * (unsigned)out_h / (unsigned)h), out_h - 1);
            const int sx = min((int)((unsigned)x0 * (unsigned)out_w / (unsigned)w), out_w - 1);      // < 2^31: both are image sizes
            const float* p = img + (size_t)sy * W + sx;
            float l[NCLS];
#pragma unroll
            for (int k = 0; k < NCLS; ++k) l[k] = p[(size_t)k * plane];
            finish_pixel<NCLS, PROB>(l, c[0], mg[0], s[0]);
        }
        const size_t row = (size_t)z * h + y;
        if (V == 4) {
            if (o.conf) *reinterpret_cast<uint32_t*>(o.conf + row * o.conf_pitch + x0) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            if (o.second) *reinterpret_cast<uint32_t*>(o.second + row * o.second_pitch + x0) = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
            if (o.margin)
                *reinterpret_cast<float4*>(reinterpret_cast<char*>(o.margin) + row * o.margin_pitch + (size_t)x0 * 4) = make_float4(mg[0], mg[1], mg[2], mg[3]);
        } else {
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
hipError_t launch_ncls(const float* scores, int n, int H, int W, int out_h, int out_w, int h, int w, int is_prob, const ConfOut& o, hipStream_t st)
{
    const bool vec = h == out_h && w == out_w && w % 4 == 0 && W % 4 == 0 && aligned(scores, 16) &&
                     (!o.conf || (o.conf_pitch % 4 == 0 && aligned(o.conf, 4))) && (!o.second || (o.second_pitch % 4 == 0 && aligned(o.second, 4))) &&
                     (!o.margin || (o.margin_pitch % 16 == 0 && aligned(o.margin, 16)));
    const long units = (long)(vec ? w / 4 : w) * h;
    // few enough blocks per frame that the 64-bit atomics of their epilogues stay a footnote (a block sees fewer than 2^32 pixels:
    // a frame has at most 2^30)
    long blocks = (units + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    const dim3 grid((unsigned)blocks, 1, (unsigned)n);
#define CONF_LAUNCH(V, PROB) \
    hipLaunchKernelGGL((confidence_kernel<NCLS, V, PROB>), grid, dim3(256), 0, st, scores, H, W, out_h, out_w, h, w, o)
    if (vec) { if (is_prob) CONF_LAUNCH(4, true); else CONF_LAUNCH(4, false); }
    else { if (is_prob) CONF_LAUNCH(1, true); else CONF_LAUNCH(1, false); }
#undef CONF_LAUNCH
    return hipGetLastError();
}

}  // namespace

// The callers (accel_io.cpp confidence_args) have checked: n, h, w >= 1, 1 <= out_h <= H, 1 <= out_w <= W <= 32768, h, w <= 32768, ncls in
// {2, 19, 21}, pitches >= a row, margin_pitch % 4 == 0, at least one output.  Reads of `scores` stay inside out_h x out_w of each of the n * ncls
// planes, writes inside w (4 * w) bytes of each of the n * h rows and the n * 256 words of hist, which are OVERWRITTEN (zeroed here first).
hipError_t launch_confidence(const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, int is_prob, unsigned char* conf,
                             size_t conf_pitch, float* margin, size_t margin_pitch, unsigned char* second, size_t second_pitch, unsigned long long* hist,
                             hipStream_t st)
{
    if (hist) {
        const hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
    }
    const ConfOut o = {conf, conf_pitch, margin, margin_pitch, second, second_pitch, hist};
    switch (ncls) {
    case 2: return launch_ncls<2>(scores, n, H, W, out_h, out_w, h, w, is_prob, o, st);
    case 19: return launch_ncls<19>(scores, n, H, W, out_h, out_w, h, w, is_prob, o, st);
    case 21: return launch_ncls<21>(scores, n, H, W, out_h, out_w, h, w, is_prob, o, st);
    }
    return hipErrorInvalidValue;
}
