// Trimap evaluation: the distance of every source pixel to the nearest boundary of the GROUND TRUTH, and the confusion matrix counted per band of
// that distance.  For a ground-truth map g (h x w uint8, rows gt_pitch apart; the frames of a batch are independent):
//     edge(y, x)  = one of the 4-neighbours of (y, x) INSIDE the frame holds another byte (raw bytes: a border to an ignored id is an edge)
//     d(y, x)     = min(cap, min over edge pixels (y', x') of max(|y - y'|, |x - x'|))            (Chebyshev; cap where there is no edge)
//     bucket(y, x) = the number of widths[i] <= d           (widths: 1 .. 4 strictly ascending values in 1 .. 16, cap = the last one)
//     hist[bucket][gt * ncls + pred] += 1 for every source pixel with gt < ncls and pred < ncls, pred by the nearest rule of labels_nearest.h
// restated by accel_amd/utils/image.py boundary_distance_host and band_hist_host.  Integer arithmetic: every result has one correct value.
//
// A block of 256 threads walks tiles of 16 x 64 source pixels of one frame (block stride over all tiles of all frames).  Per tile, with R = cap:
//   1. the ground truth of the tile and a halo of R pixels goes to LDS (48 x 96 bytes at R = 16; dwords where the rows allow it).  What lies outside
//      the frame is stored as 0 and never COMPARED: the edge step asks the coordinates, not the bytes, whether a neighbour exists
//   2. edge flags of the tile and R - 1 pixels around it, one wavefront per row, gathered with two ballots into a 96-bit mask per row
//   3. the row pass: hd(y, x) = the smallest |dx| <= R - 1 to an edge of row y, R where there is none: a find-first-set on each side of the mask
//   4. the column pass, per thread for its 4 consecutive pixels of one row: d = min(R, min over |dy| <= R - 1 of max(|dy|, hd(y + dy, x)))
// then d is stored (boundary_distance_kernel), or bucketed and counted with the prediction (labels_band_hist_kernel): runs of one (bucket, gt, pred)
// key in a register, a block-private LDS table of (K + 1) * ncls * ncls 32-bit bins, one 64-bit device-scope atomic add per non-zero bin per block --
// the scheme of labels_hist_kernel (results_u8.hip).  Every loop bound is a launch constant.
#include "kernels.h"
#include "labels_nearest.h"
#include <stdint.h>

namespace {

using nearest::Column;
using nearest::source_row;
using nearest::aligned;

constexpr int TH = 16, TW = 64;                 // the tile a block owns at a time
constexpr int HALO = 16;                        // the largest cap: the LDS arrays are laid out for it, whatever R is
constexpr int GH = TH + 2 * HALO, GW = TW + 2 * HALO;       // 48 x 96: LDS position (i, j) is frame pixel (ty0 - 16 + i, tx0 - 16 + j)

struct TileLds {
    unsigned char g[GH * GW];                   // ground truth; rows 16 - R .. 31 + R are staged
    unsigned long long mask[GH][2];             // edge flags of a row, bit j; rows and columns 17 - R .. (30 | 78) + R
    unsigned char hd[GH * TW];                  // the row pass, column j - 16; rows 17 - R .. 30 + R
};

struct Tiles {
    int tiles_x, tiles_y;
    long long total;                            // n * tiles_y * tiles_x
};

// d of the thread's four pixels (ty0 + tid / 16, tx0 + 4 * (tid % 16) + k), one per byte.  Ends with every thread past its reads of t.hd only:
// the caller puts a barrier between its own reads of t.g and the next call
__device__ __forceinline__ unsigned tile_distance(TileLds& t, const unsigned char* __restrict__ gt, size_t gt_pitch, int h, int w, int ty0, int tx0, int R,
                                                  int gt_dword)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 1. rows 16 - R .. 31 + R, all 24 dwords of each
    const int rows = TH + 2 * R;
    for (int q = tid; q < rows * (GW / 4); q += 256) {
        const int i = HALO - R + q / (GW / 4), c = q % (GW / 4);
        const int y = ty0 - HALO + i, x = tx0 - HALO + 4 * c;
        unsigned v = 0;
        if (y >= 0 && y < h) {
            const unsigned char* row = gt + (size_t)y * gt_pitch;
            if (gt_dword && x >= 0 && x + 4 <= w) {
                v = *reinterpret_cast<const uint32_t*>(row + x);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k >= 0 && x + k < w) v |= (unsigned)row[x + k] << (8 * k);
            }
        }
        *reinterpret_cast<uint32_t*>(&t.g[i * GW + 4 * c]) = v;
    }
    __syncthreads();
    // 2. one wavefront per row: lanes are columns j = lane and j = 64 + lane
    const int lo = HALO + 1 - R, hi_row = HALO + TH - 2 + R, hi_col = HALO + TW - 2 + R;
    for (int i = lo + wave; i <= hi_row; i += 4) {
        const int y = ty0 - HALO + i;
        unsigned long long m[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int j = 64 * half + lane, x = tx0 - HALO + j;
            bool e = false;
            if (j >= lo && j <= hi_col && y >= 0 && y < h && x >= 0 && x < w) {
                const unsigned char* p = &t.g[i * GW + j];
                const unsigned char c = p[0];
                e = (y > 0 && p[-GW] != c) || (y < h - 1 && p[GW] != c) || (x > 0 && p[-1] != c) || (x < w - 1 && p[1] != c);
            }
            m[half] = __ballot(e);
        }
        if (lane == 0) { t.mask[i][0] = m[0]; t.mask[i][1] = m[1]; }
    }
    __syncthreads();
    // 3. one wavefront per row: lane is tile column `lane`, bit j = lane + 16 of the mask
    const unsigned near_bits = (1u << R) - 1u;                          // |dx| <= R - 1 on the right: bit dx
    const unsigned far_bits = 0xffffu & ~((1u << (HALO - R)) - 1u);       // and on the left: bit 15 - |dx|
    for (int i = lo + wave; i <= hi_row; i += 4) {
        const unsigned long long m0 = t.mask[i][0], m1 = t.mask[i][1];
        const int j = lane + HALO;                                      // 16 .. 79
        const unsigned right = (unsigned)(j < 64 ? (m0 >> j) | (m1 << (64 - j)) : m1 >> (j - 64)) & near_bits;
        const int s = j - 15;                                           // 1 .. 64
        const unsigned left = (unsigned)(s < 64 ? (m0 >> s) | (m1 << (64 - s)) : m1) & far_bits;
        int d = R;
        if (right) d = __ffs((int)right) - 1;
        if (left) d = min(d, __clz((int)left) - 16);
        t.hd[i * TW + lane] = (unsigned char)d;
    }
    __syncthreads();
    // 4. the thread's four pixels
    const int ty = tid >> 4, tx4 = (tid & 15) << 2;
    unsigned d0 = R, d1 = R, d2 = R, d3 = R;
    for (int dy = 1 - R; dy <= R - 1; ++dy) {
        const unsigned v = *reinterpret_cast<const uint32_t*>(&t.hd[(ty + HALO + dy) * TW + tx4]);
        const unsigned a = (unsigned)(dy < 0 ? -dy : dy);
        d0 = min(d0, max(a, v & 255u));
        d1 = min(d1, max(a, (v >> 8) & 255u));
        d2 = min(d2, max(a, (v >> 16) & 255u));
        d3 = min(d3, max(a, v >> 24));
    }
    return d0 | (d1 << 8) | (d2 << 16) | (d3 << 24);
}

__device__ __forceinline__ void tile_at(const Tiles& g, long long tile, int& z, int& ty0, int& tx0)
{
    const long long per = (long long)g.tiles_x * g.tiles_y;
    z = (int)(tile / per);
    const int r = (int)(tile - (long long)z * per);
    ty0 = (r / g.tiles_x) * TH;
    tx0 = (r % g.tiles_x) * TW;
}

__global__ __launch_bounds__(256) void boundary_distance_kernel(const unsigned char* __restrict__ maps, int h, int w, size_t pitch, int R, Tiles tiles,
                                                                int src_dword, unsigned char* __restrict__ dst, size_t dst_pitch, int dst_dword)
{
    __shared__ TileLds t;
    for (long long tile = blockIdx.x; tile < tiles.total; tile += gridDim.x) {
        int z, ty0, tx0;
        tile_at(tiles, tile, z, ty0, tx0);
        const unsigned d = tile_distance(t, maps + (size_t)z * h * pitch, pitch, h, w, ty0, tx0, R, src_dword);
        const int y = ty0 + (threadIdx.x >> 4), x0 = tx0 + ((threadIdx.x & 15) << 2);
        if (y < h && x0 < w) {
            unsigned char* out = dst + ((size_t)z * h + y) * dst_pitch + x0;
            if (dst_dword && x0 + 4 <= w) {
                *reinterpret_cast<uint32_t*>(out) = d;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x0 + k < w) out[k] = (unsigned char)(d >> (8 * k));
            }
        }
        __syncthreads();        // the next tile overwrites what the slowest thread may still be reading
    }
}

// the widths, one per byte; 255 in the unused ones (no distance reaches it)
struct Widths { int n, cap; unsigned packed; };

__global__ __launch_bounds__(256) void labels_band_hist_kernel(const unsigned char* __restrict__ labels, int H, int W, int out_h, int out_w,
                                                               const unsigned char* __restrict__ gt, int h, int w, size_t gt_pitch, int ncls, Widths wd,
                                                               Tiles tiles, int gt_dword, int label_dword, unsigned long long* __restrict__ hist)
{
    __shared__ TileLds t;
    __shared__ unsigned bins[5 * 32 * 32];
    const int nb = (wd.n + 1) * ncls * ncls;
    for (int i = threadIdx.x; i < nb; i += 256) bins[i] = 0;
    // (the first barrier of tile_distance orders this with the first add)

    const unsigned uncls = (unsigned)ncls;
    const int R = wd.cap;
    const unsigned w0 = wd.packed & 255u, w1 = (wd.packed >> 8) & 255u, w2 = (wd.packed >> 16) & 255u, w3 = wd.packed >> 24;
    const bool ident = h == out_h && w == out_w;
    unsigned key = 0, cnt = 0;
    auto feed = [&](unsigned d, unsigned g, unsigned p) {
        if (g < uncls && p < uncls) {
            const unsigned b = (d >= w0 ? 1u : 0u) + (d >= w1 ? 1u : 0u) + (d >= w2 ? 1u : 0u) + (d >= w3 ? 1u : 0u);
            const unsigned k = (b * uncls + g) * uncls + p;
            if (k == key) {
                ++cnt;
            } else {
                if (cnt) atomicAdd(&bins[key], cnt);
                key = k; cnt = 1;
            }
        }
    };

    for (long long tile = blockIdx.x; tile < tiles.total; tile += gridDim.x) {
        int z, ty0, tx0;
        tile_at(tiles, tile, z, ty0, tx0);
        const unsigned d = tile_distance(t, gt + (size_t)z * h * gt_pitch, gt_pitch, h, w, ty0, tx0, R, gt_dword);
        const int ty = threadIdx.x >> 4, tx4 = (threadIdx.x & 15) << 2;
        const int y = ty0 + ty, x0 = tx0 + tx4;
        if (y < h && x0 < w) {
            const unsigned g4 = *reinterpret_cast<const uint32_t*>(&t.g[(ty + HALO) * GW + HALO + tx4]);
            const unsigned char* row = labels + (size_t)z * H * W + (size_t)(ident ? y : source_row(y, out_h, h)) * W;
            if (ident && label_dword && x0 + 4 <= w) {
                const unsigned p4 = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
                for (int k = 0; k < 4; ++k) feed((d >> (8 * k)) & 255u, (g4 >> (8 * k)) & 255u, (p4 >> (8 * k)) & 255u);
            } else {
                Column c(x0, out_w, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (x0 + k < w) feed((d >> (8 * k)) & 255u, (g4 >> (8 * k)) & 255u, ident ? row[x0 + k] : row[c.col()]);
                    c.next();
                }
            }
        }
        __syncthreads();        // the next tile overwrites t.g and t.hd
    }

    // the run every lane still holds: one add for the wavefront when it is the same run in all of them
    const unsigned lk = __builtin_amdgcn_readfirstlane(key);
    if (!cnt) key = lk;       // a lane that counted nothing agrees with anyone
    if (__all(key == lk)) {
        unsigned s = cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&bins[lk], s);
    } else if (cnt) {
        atomicAdd(&bins[key], cnt);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        const unsigned v = bins[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

// blocks for `tiles.total` tiles: enough to fill the chip a few times over, few enough that a block's table (zeroed, then scanned for its non-zero
// bins) serves many tiles; and never 2^32 pixels = 2^22 tiles in one block (32-bit LDS bins)
Tiles tiles_of(int n, int h, int w, unsigned* blocks)
{
    Tiles t;
    t.tiles_x = (w + TW - 1) / TW;
    t.tiles_y = (h + TH - 1) / TH;
    t.total = (long long)n * t.tiles_x * t.tiles_y;
    long long b = t.total < 2560 ? t.total : 2560;
    const long long floor_blocks = t.total / (1LL << 21) + 1;
    if (b < floor_blocks) b = floor_blocks;
    *blocks = (unsigned)b;
    return t;
}

}  // namespace

// The callers (accel_io.cpp band_args) have checked: 1 <= n, h, w <= 32768, pitches >= w, 1 <= cap <= 16.  Reads of `maps` and writes of `dst` stay inside w
// bytes of each of the n * h rows.
hipError_t launch_boundary_distance(const unsigned char* maps, int n, int h, int w, size_t pitch, int cap, unsigned char* dst, size_t dst_pitch, hipStream_t st)
{
    if (cap < 1 || cap > HALO) return hipErrorInvalidValue;
    unsigned blocks;
    const Tiles tiles = tiles_of(n, h, w, &blocks);
    const int src_dword = pitch % 4 == 0 && aligned(maps, 4), dst_dword = dst_pitch % 4 == 0 && aligned(dst, 4);
    hipLaunchKernelGGL(boundary_distance_kernel, dim3(blocks), dim3(256), 0, st, maps, h, w, pitch, cap, tiles, src_dword, dst, dst_pitch, dst_dword);
    return hipGetLastError();
}

// The callers have checked the geometry of launch_labels_hist, n <= 32768, and 1 <= nwidths <= 4 strictly ascending widths in 1 .. 16.  hist holds
// (nwidths + 1) * ncls * ncls words that are added to.  Reads of `labels` stay inside out_h x out_w of each map, reads of gt inside w bytes of each row.
hipError_t launch_labels_band_hist(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, const unsigned char* gt, int h, int w,
                                   size_t gt_pitch, int ncls, const int* widths, int nwidths, unsigned long long* hist, hipStream_t st)
{
    if (nwidths < 1 || nwidths > 4 || ncls < 1 || ncls > 32) return hipErrorInvalidValue;
    Widths wd = {nwidths, widths[nwidths - 1], 0xffffffffu};
    for (int i = 0; i < nwidths; ++i) {
        if (widths[i] < 1 || widths[i] > HALO || (i && widths[i] <= widths[i - 1])) return hipErrorInvalidValue;
        wd.packed = (wd.packed & ~(255u << (8 * i))) | ((unsigned)widths[i] << (8 * i));
    }
    unsigned blocks;
    const Tiles tiles = tiles_of(n, h, w, &blocks);
    const int gt_dword = gt_pitch % 4 == 0 && aligned(gt, 4);
    const int label_dword = h == out_h && w == out_w && W % 4 == 0 && aligned(labels, 4);
    hipLaunchKernelGGL(labels_band_hist_kernel, dim3(blocks), dim3(256), 0, st, labels, H, W, out_h, out_w, gt, h, w, gt_pitch, ncls, wd, tiles, gt_dword,
                       label_dword, hist);
    return hipGetLastError();
}
