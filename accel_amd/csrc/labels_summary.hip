// What is in a finished frame, where, and did it just change: per frame and class the area, the coordinate sums and the bounding box of the label
// map at the SOURCE frame's size, and -- against the previous frame's map at that size -- the class-transition matrix.  The geometry is that of
// results_u8.hip: the valid region of a label map (n x H x W uint8) is out_h x out_w in its top-left corner, the source frame is h x w, and source
// pixel (y, x) has the label
//     L = labels[min(y * out_h / h, out_h - 1)][min(x * out_w / w, out_w - 1)]            (integer division)
// For every frame f and class k < ncls (ncls <= 32; ids >= ncls are ignored, as the confusion matrix ignores them):
//     stats[f][k] = (area, sum_x, sum_y)          uint64, over the source pixels with L == k  (up to 2^15 * 2^30: 64 bits)
//     box[f][k]   = (x0, y0, x1, y1)              int32, the inclusive extremes of those pixels; (w, h, -1, -1) for a class without one
//     trans[f][p * ncls + c]                      uint64, the source pixels with prev == p < ncls and L == c < ncls (rows: the previous frame)
// restated bit for bit by accel_amd/utils/image.py labels_summary_host.  Integer sums, minima and maxima: exact, whatever the order of arrival.
//
// One pass.  A thread walks units of 16 consecutive pixels of one row of one frame (grid stride inside the frame; blockIdx.z is the frame) and keeps
// the RUN of its current key -- the label, or the (previous, current) pair when tracking -- in registers: count, sum of x, sum of y and the four
// extremes.  A unit whose 16 bytes all equal the key (the realistic case: label maps are mostly runs) costs a handful of integer operations; only a
// change of key sends the finished run to the block's LDS tables (32-bit areas and transition bins, 64-bit coordinate sums, the extremes by atomic
// min / max).  At the end a wavefront whose lanes all hold the same key adds ONE run for all of them.  Then the block issues one 64-bit device-scope
// atomic add per non-zero sum and one atomic min / max per extreme of a touched class into the results, which the launcher has initialised (zeros
// and the identities of min and max) on the same stream.
// 32-bit run registers: the launcher sizes the grid so that a thread sees at most 65536 pixels (sum of x or y < 2^31); a block sees fewer than 2^32.
//
// Tracking: the thread that computes L for source pixel p first reads prev[p], counts the transition, then stores L to kept[p].  prev and kept may
// be the SAME map (the model's kept map, updated in place): one thread reads and writes the same bytes, in that order.  Without prev it only stores.
// VEC: the rows of prev and kept (and, at the identity geometry, of labels) allow 16-byte accesses (pitches % 16 == 0, aligned bases); units that cross
// the end of a row, and everything else, go byte by byte.  Nothing outside out_h x out_w of `labels` is read.
#include "kernels.h"
#include "labels_nearest.h"
#include <stdint.h>

namespace {

using nearest::Column;
using nearest::source_row;
using nearest::aligned;

struct SummaryMaps {
    const unsigned char* prev; size_t prev_pitch;       // n x h rows, or null: nothing to compare with
    unsigned char* kept; size_t kept_pitch;             // n x h rows, or null: the current map is not kept; may be `prev`
    unsigned long long* stats;                          // n x ncls x 3, or null
    int* box;                                           // n x ncls x 4, or null
    unsigned long long* trans;                          // n x ncls x ncls, non-null iff prev is
};

__device__ __forceinline__ unsigned byte_of(const unsigned (&w)[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }
__device__ __forceinline__ bool all_bytes(const unsigned (&w)[4], unsigned b)
{
    const unsigned r = b * 0x01010101u;
    return ((w[0] ^ r) | (w[1] ^ r) | (w[2] ^ r) | (w[3] ^ r)) == 0u;
}

constexpr unsigned NO_KEY = 0xffffffffu;

template <bool IDENT, bool VEC>
__global__ __launch_bounds__(256) void labels_summary_kernel(const unsigned char* __restrict__ labels, int H, int W, int out_h, int out_w, int h, int w,
                                                             int ncls, SummaryMaps o)
{
    __shared__ unsigned s_area[32];
    __shared__ unsigned long long s_sx[32], s_sy[32];
    __shared__ int s_box[32 * 4];
    __shared__ unsigned s_tr[32 * 32];
    const bool track = o.prev != nullptr;
    const int nb = track ? ncls * ncls : 0;
    if (threadIdx.x < 32) {
        s_area[threadIdx.x] = 0; s_sx[threadIdx.x] = 0; s_sy[threadIdx.x] = 0;
        s_box[4 * threadIdx.x] = w; s_box[4 * threadIdx.x + 1] = h; s_box[4 * threadIdx.x + 2] = -1; s_box[4 * threadIdx.x + 3] = -1;
    }
    for (int i = threadIdx.x; i < nb; i += 256) s_tr[i] = 0;
    __syncthreads();

    const unsigned uncls = (unsigned)ncls;
    // the run in registers: key = (previous << 8) | current (previous = 0 when not tracking)
    unsigned key = NO_KEY, cnt = 0, sx = 0, sy = 0;
    int bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
    auto flush = [&]() {
        const unsigned c = key & 255u, p = key >> 8;
        if (cnt && c < uncls) {
            atomicAdd(&s_area[c], cnt);
            atomicAdd(&s_sx[c], (unsigned long long)sx);
            atomicAdd(&s_sy[c], (unsigned long long)sy);
            atomicMin(&s_box[4 * c], bx0); atomicMin(&s_box[4 * c + 1], by0);
            atomicMax(&s_box[4 * c + 2], bx1); atomicMax(&s_box[4 * c + 3], by1);
            if (track && p < uncls) atomicAdd(&s_tr[p * uncls + c], cnt);
        }
    };
    // `len` pixels x .. x + len - 1 of row y, all of key k
    auto feed = [&](unsigned k, int x, int len, int y) {
        const unsigned sum_x = (unsigned)len * (unsigned)x + (unsigned)(len * (len - 1) / 2);
        if (k == key) {
            cnt += (unsigned)len; sx += sum_x; sy += (unsigned)len * (unsigned)y;
            bx0 = min(bx0, x); bx1 = max(bx1, x + len - 1); by0 = min(by0, y); by1 = max(by1, y);
        } else {
            flush();
            key = k; cnt = (unsigned)len; sx = sum_x; sy = (unsigned)len * (unsigned)y;
            bx0 = x; bx1 = x + len - 1; by0 = by1 = y;
        }
    };

    const int z = blockIdx.z;
    const int UW = (w + 15) >> 4;
    const long units = (long)UW * h;
    const unsigned char* map = labels + (size_t)z * H * W;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
        const int y = (int)(u / UW), x0 = (int)(u - (long)y * UW) << 4;
        const unsigned char* row = map + (size_t)(IDENT ? y : source_row(y, out_h, h)) * W;
        const unsigned char* pr = track ? o.prev + ((size_t)z * h + y) * o.prev_pitch + x0 : nullptr;
        unsigned char* kp = o.kept ? o.kept + ((size_t)z * h + y) * o.kept_pitch + x0 : nullptr;
        if (VEC && x0 + 16 <= w) {
            unsigned lw[4], pw[4] = {0u, 0u, 0u, 0u};
            if (IDENT) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
                lw[0] = v.x; lw[1] = v.y; lw[2] = v.z; lw[3] = v.w;
            } else {
                Column c(x0, out_w, w);
                lw[0] = lw[1] = lw[2] = lw[3] = 0u;
#pragma unroll
                for (int k = 0; k < 16; ++k) { lw[k >> 2] |= (unsigned)row[c.col()] << (8 * (k & 3)); c.next(); }
            }
            if (track) {
                const uint4 v = *reinterpret_cast<const uint4*>(pr);       // read before the store below: kept may be prev
                pw[0] = v.x; pw[1] = v.y; pw[2] = v.z; pw[3] = v.w;
            }
            if (kp) *reinterpret_cast<uint4*>(kp) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
            const unsigned l0 = lw[0] & 255u, p0 = pw[0] & 255u;
            if (all_bytes(lw, l0) && all_bytes(pw, p0)) {
                feed((p0 << 8) | l0, x0, 16, y);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) feed((byte_of(pw, k) << 8) | byte_of(lw, k), x0 + k, 1, y);
            }
        } else {
            Column c(x0, out_w, w);
            const int m = min(16, w - x0);
            for (int k = 0; k < m; ++k) {
                const unsigned l = IDENT ? row[x0 + k] : row[c.col()];
                c.next();
                const unsigned p = track ? pr[k] : 0u;                    // read before the store below: kept may be prev
                if (kp) kp[k] = (unsigned char)l;
                feed((p << 8) | l, x0 + k, 1, y);
            }
        }
    }

    // the run every lane still holds: one add for the wavefront when it is the same run in all of them
    const unsigned lk = __builtin_amdgcn_readfirstlane(key);
    if (key == NO_KEY) { key = lk; bx0 = by0 = 0x7fffffff; bx1 = by1 = -1; }       // a lane that saw nothing agrees with anyone (cnt = sx = sy = 0)
    if (lk != NO_KEY && __all(key == lk)) {
        unsigned long long a = cnt, tx = sx, ty = sy;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64); tx += __shfl_xor(tx, off, 64); ty += __shfl_xor(ty, off, 64);
            bx0 = min(bx0, __shfl_xor(bx0, off, 64)); by0 = min(by0, __shfl_xor(by0, off, 64));
            bx1 = max(bx1, __shfl_xor(bx1, off, 64)); by1 = max(by1, __shfl_xor(by1, off, 64));
        }
        const unsigned c = lk & 255u, p = lk >> 8;
        if ((threadIdx.x & 63) == 0 && c < uncls) {
            atomicAdd(&s_area[c], (unsigned)a);
            atomicAdd(&s_sx[c], tx);
            atomicAdd(&s_sy[c], ty);
            atomicMin(&s_box[4 * c], bx0); atomicMin(&s_box[4 * c + 1], by0);
            atomicMax(&s_box[4 * c + 2], bx1); atomicMax(&s_box[4 * c + 3], by1);
            if (track && p < uncls) atomicAdd(&s_tr[p * uncls + c], (unsigned)a);
        }
    } else {
        flush();
    }
    __syncthreads();

    if (threadIdx.x < ncls && s_area[threadIdx.x]) {
        const int k = threadIdx.x;
        const size_t at = (size_t)z * ncls + k;
        if (o.stats) {
            atomicAdd(&o.stats[3 * at], (unsigned long long)s_area[k]);
            if (s_sx[k]) atomicAdd(&o.stats[3 * at + 1], s_sx[k]);
            if (s_sy[k]) atomicAdd(&o.stats[3 * at + 2], s_sy[k]);
        }
        if (o.box) {
            atomicMin(&o.box[4 * at], s_box[4 * k]); atomicMin(&o.box[4 * at + 1], s_box[4 * k + 1]);
            atomicMax(&o.box[4 * at + 2], s_box[4 * k + 2]); atomicMax(&o.box[4 * at + 3], s_box[4 * k + 3]);
        }
    }
    for (int i = threadIdx.x; i < nb; i += 256) {
        const unsigned v = s_tr[i];
        if (v) atomicAdd(&o.trans[(size_t)z * nb + i], (unsigned long long)v);
    }
}

// zeros into stats and trans, the identities of min and max into box
__global__ __launch_bounds__(256) void labels_summary_init_kernel(unsigned long long* stats, long n_stats, int* box, long n_box, unsigned long long* trans,
                                                                  long n_trans, int h, int w)
{
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_stats; i += stride) stats[i] = 0ull;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_trans; i += stride) trans[i] = 0ull;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_box; i += stride) box[i] = (i & 3) == 0 ? w : (i & 3) == 1 ? h : -1;
}

}  // namespace

// The callers (accel_io.cpp summary_args) have checked: 1 <= n <= 32768, 1 <= out_h <= H <= 32768, 1 <= out_w <= W <= 32768, 1 <= h, w <= 32768,
// 1 <= ncls <= 32, pitches >= a row, at least one of stats / box / trans / kept, trans only with prev.  Reads of `labels` stay inside out_h x out_w of
// each of the n maps (row and column indices are clamped), reads of prev and writes of kept inside w bytes of each of the n * h rows; stats (n x ncls x
// 3 words), box (n x ncls x 4) and trans (n x ncls x ncls) are OVERWRITTEN (initialised here first).  prev is read only when trans is asked for.
hipError_t launch_labels_summary(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls, const unsigned char* prev,
                                 size_t prev_pitch, unsigned long long* stats, int* box, unsigned long long* trans, unsigned char* kept, size_t kept_pitch,
                                 hipStream_t st)
{
    if ((!stats && !box && !trans && !kept) || (trans && !prev)) return hipErrorInvalidValue;
    if (!trans) prev = nullptr;
    if (stats || box || trans) {
        const long ns = stats ? (long)n * ncls * 3 : 0, nx = box ? (long)n * ncls * 4 : 0, nt = trans ? (long)n * ncls * ncls : 0;
        const long most = ns > nt ? (ns > nx ? ns : nx) : (nt > nx ? nt : nx);
        long blocks = (most + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(labels_summary_init_kernel, dim3((unsigned)blocks), dim3(256), 0, st, stats, ns, box, nx, trans, nt, h, w);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // Blocks per frame.  The results of a frame are a handful of cache lines, and the epilogues' atomics on them are served one after the other:
    // measured, a launch takes about 80 .. 160 ns per block of a frame whatever the frame's size, while the body takes time in proportion to
    // units / blocks (profiles/labels_summary.md).  The sum of the two is smallest near blocks ~ sqrt(units): sqrt(units) / 4, at most one block
    // per 256 units; and never more than 65536 pixels = 4096 units in one thread (32-bit run registers)
    const long units = (long)((w + 15) / 16) * h;
    long blocks = (long)(sqrt((double)units) / 4.0);
    if (blocks > (units + 255) / 256) blocks = (units + 255) / 256;
    if (blocks < 1) blocks = 1;
    const long floor_blocks = (units + 256L * 4096 - 1) / (256L * 4096);
    if (blocks < floor_blocks) blocks = floor_blocks;
    const bool ident = h == out_h && w == out_w;
    const bool vec = (!ident || (W % 16 == 0 && aligned(labels, 16))) && (!prev || (prev_pitch % 16 == 0 && aligned(prev, 16)))
                     && (!kept || (kept_pitch % 16 == 0 && aligned(kept, 16)));
    const SummaryMaps o = {prev, prev_pitch, kept, kept_pitch, stats, box, trans};
    const dim3 grid((unsigned)blocks, 1, (unsigned)n);
#define SUM_LAUNCH(IDENT, VEC) \
    hipLaunchKernelGGL((labels_summary_kernel<IDENT, VEC>), grid, dim3(256), 0, st, labels, H, W, out_h, out_w, h, w, ncls, o)
    if (ident) { if (vec) SUM_LAUNCH(true, true); else SUM_LAUNCH(true, false); }
    else { if (vec) SUM_LAUNCH(false, true); else SUM_LAUNCH(false, false); }
#undef SUM_LAUNCH
    return hipGetLastError();
}
