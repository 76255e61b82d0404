// Objects per class: the connected components of the label map at the SOURCE frame's size.  The geometry is that of labels_summary.hip: source pixel
// (y, x) of an h x w frame has the label L = labels[min(y * out_h / h, out_h - 1)][min(x * out_w / w, out_w - 1)]; L >= ncls is background, which
// belongs to no component and separates components.  Two other pixels of one frame are joined when their labels are equal and they are 4-adjacent
// (connectivity 8: or diagonally adjacent).  Per frame f, for the components with area >= min_area in ascending order of their ANCHOR (the
// component's first pixel in raster order, the smallest y * w + x):
//     count[f]                        int32, their number -- the full number, also above max_components
//     comp[f][i]  (i < max_components) int32 x 8 = (class, area, x0, y0, x1, y1, ax, ay); -1 in the records after the last
//     sums[f][i]                      uint64 x 2 = (sum_x, sum_y) over the component's source pixels; 0 in the records after the last
//     ids[f][y][x]                    int32, the record index of the pixel's component; -1 for background, filtered and truncated components
// restated bit for bit by accel_amd/utils/image.py labels_components_host.  Integer minima, maxima and sums: exact, whatever the order of arrival.
//
// The result depends on an unbounded neighbourhood, so it takes phases, and every phase boundary is a KERNEL boundary on the one stream: no
// grid-wide barrier, no flag, no persistent block.  Scratch (the caller's): `parent` and `area`, one int32 per source pixel, and `blocks`, one
// int32 per chunk of 1024 pixels.  Linear indices y * w + x are per frame and stay below 2^30.
//   1 tiles    one block per 16 x 64 tile.  A wavefront takes one row of the tile per step: the run a pixel lies in starts at the highest set bit at or
//              below its lane in the ballot of "my left neighbour differs", so rows collapse to runs without a loop.  Then the runs of adjacent
//              rows are united in LDS (union-find, atomicMin, always towards the SMALLER index: a root is the first pixel of its set), only where
//              the edge is not implied by the edge one pixel to the left.  parent[p] = the global index of the tile-local root, -1 for
//              background; area[p] = 0.
//   2 seams    one thread per pixel of a tile's first row (the edges up, up-left, up-right) and of a tile's first column (the edges left and the
//              two diagonals across the vertical seam): the same union on `parent` with device-scope atomicMin.  Parents are read with relaxed
//              agent-scope atomic loads; an older parent than the current one is harmless, since the atomicMin returns the current one.
//   3 flatten  every pixel follows its chain to the root (the anchor, by construction) and stores it; areas are counted per run of equal roots in
//              registers, then per wavefront where all its lanes hold one root, then per block in an LDS table keyed by the root, and only then
//              added to area[root]: one global atomic per block and root, not per pixel.
//   4 count    the qualifying roots (parent[p] == p and area[p] >= min_area) per chunk of 1024 consecutive pixels -> blocks
//   5 scan     one block per frame: the exclusive scan of the frame's chunk counts in place, and count[f] = the total
//   6 slots    slot = scanned count + rank inside the chunk: anchor order and the first-max_components truncation without a sort.  The root's
//              thread stores class, area and anchor (and the anchor as the first box) and replaces area[root] by the slot, or -1.
//   7 records  every pixel looks up its root's slot: ids, and -- aggregated as in phase 3 -- the box by atomic min / max and the sums by 64-bit add.
// Deviations from a 16-byte label fetch at the identity geometry: a wavefront of phase 1 reads the 64 consecutive bytes of a tile row in one
// instruction, which is one memory transaction already; wider loads would save instructions of a phase that is bound by its LDS unions.
//
// Termination.  Every chain walk goes to a strictly smaller index and stops otherwise (the comparisons are unsigned, so a negative parent stops it
// too): at most h * w steps (phase 1: 1024).  A union repeats only after the atomicMin found the cell already lowered, and the larger of its two
// ends strictly decreases from round to round: at most h * w rounds (phase 1: 1024).  Table probes: 8.  The scan: chunks / 256 rounds.
#include "kernels.h"
#include "labels_nearest.h"
#include <stdint.h>

namespace {

using nearest::Column;
using nearest::source_row;

constexpr int TH = 16, TW = 64;             // the tile of phase 1: TW is the wavefront
constexpr int CHUNK = 1024;                 // pixels per block of phases 4 and 6
constexpr unsigned BG = 255u;               // background in LDS and registers (ncls <= 32: never a class)
constexpr int TABLE = 256, PROBES = 8;      // the per-block tables of phases 3 and 7

struct Geo { int H, W, out_h, out_w, h, w, ncls; };

template <bool IDENT>
__device__ __forceinline__ unsigned label_at(const unsigned char* map, const Geo& g, int y, int x)
{
    if ((unsigned)y >= (unsigned)g.h || (unsigned)x >= (unsigned)g.w) return BG;
    const int row = IDENT ? y : source_row(y, g.out_h, g.h);
    const int col = IDENT ? x : min((int)((unsigned)x * (unsigned)g.out_w / (unsigned)g.w), g.out_w - 1);
    const unsigned v = map[(size_t)row * g.W + col];
    return v < (unsigned)g.ncls ? v : BG;
}

// ---- union-find in LDS (phase 1) ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* par, int i)
{
    for (;;) {                                                  // i strictly decreases: at most TH * TW steps
        const int p = __hip_atomic_load(&par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((unsigned)p >= (unsigned)i) return i;
        i = p;
    }
}

__device__ __forceinline__ void lds_union(int* par, int a, int b)
{
    for (;;) {                                                  // max(a, b) strictly decreases: at most TH * TW rounds
        a = lds_find(par, a); b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if ((unsigned)old >= (unsigned)a) return;               // a was a root and now points at b
        a = old;                                                // somebody lowered it first: old < a, and old and b are still to be united
    }
}

// ---- union-find on the parent array (phase 2) --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int dev_find(int* par, int i)
{
    for (;;) {                                                  // i strictly decreases: at most h * w steps
        const int p = __hip_atomic_load(&par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)p >= (unsigned)i) return i;
        i = p;
    }
}

__device__ __forceinline__ void dev_union(int* par, int a, int b)
{
    for (;;) {                                                  // max(a, b) strictly decreases: at most h * w rounds
        a = dev_find(par, a); b = dev_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);                  // device scope; returns the current parent, whatever the loads above saw
        if ((unsigned)old >= (unsigned)a) return;
        a = old;
    }
}

// the exclusive scan of one int per thread over the 256 threads of a block; s_wave: 4 ints of LDS
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_wave, int& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (k < wv) before += s_wave[k]; total += s_wave[k]; }
    __syncthreads();
    return before + inc - v;
}

// ---- phase 1 -------------------------------------------------------------------------------------------------------------------------------------------
template <bool IDENT>
__global__ __launch_bounds__(256) void components_tiles_kernel(const unsigned char* __restrict__ labels, Geo g, int conn8, int* __restrict__ parent,
                                                               int* __restrict__ area)
{
    __shared__ int s_par[TH * TW];
    __shared__ unsigned char s_lab[TH * TW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t frame = (size_t)blockIdx.z * g.h * g.w;
    const unsigned char* map = labels + (size_t)blockIdx.z * g.H * g.W;
    const int gx = tx0 + lane, cx = min(gx, g.w - 1);
    const int col = IDENT ? cx : Column(cx, g.out_w, g.w).col();

    for (int r = 0; r < TH / 4; ++r) {
        const int ly = wv + 4 * r, gy = ty0 + ly;
        unsigned lab = BG;
        if (gx < g.w && gy < g.h) {
            const unsigned v = map[(size_t)(IDENT ? gy : source_row(gy, g.out_h, g.h)) * g.W + col];
            if (v < (unsigned)g.ncls) lab = v;
        }
        const unsigned left = __shfl_up(lab, 1, 64);
        const unsigned long long starts = __ballot(lane == 0 || left != lab);      // bit 0 is always set
        const int first = 63 - __clzll(starts & (~0ull >> (63 - lane)));
        s_lab[ly * TW + lane] = (unsigned char)lab;
        s_par[ly * TW + lane] = lab == BG ? -1 : ly * TW + first;
    }
    __syncthreads();

    // the edges to the row above.  (y, x) - (y - 1, x) is implied by the same edge one pixel to the left when both left neighbours have the label;
    // a diagonal is implied when the pixel above, or the pixel beside on the diagonal's side, has the label
    for (int r = 0; r < TH / 4; ++r) {
        const int ly = wv + 4 * r, i = ly * TW + lane;
        const unsigned lab = s_lab[i];
        if (ly == 0 || lab == BG) continue;
        const unsigned up = s_lab[i - TW];
        const unsigned left = lane > 0 ? s_lab[i - 1] : BG, ul = lane > 0 ? s_lab[i - TW - 1] : BG;
        if (up == lab) {
            if (left != lab || ul != lab) lds_union(s_par, i, i - TW);
        } else if (conn8) {
            const unsigned right = lane < TW - 1 ? s_lab[i + 1] : BG, ur = lane < TW - 1 ? s_lab[i - TW + 1] : BG;
            if (ul == lab && left != lab) lds_union(s_par, i, i - TW - 1);
            if (ur == lab && right != lab) lds_union(s_par, i, i - TW + 1);
        }
    }
    __syncthreads();

    for (int r = 0; r < TH / 4; ++r) {
        const int ly = wv + 4 * r, gy = ty0 + ly, i = ly * TW + lane;
        if (gx >= g.w || gy >= g.h) continue;
        const size_t at = frame + (size_t)gy * g.w + gx;
        int p = -1;
        if (s_lab[i] != BG) {
            const int root = lds_find(s_par, i);
            p = (ty0 + root / TW) * g.w + tx0 + root % TW;
        }
        parent[at] = p;
        area[at] = 0;
    }
}

// ---- phase 2 -------------------------------------------------------------------------------------------------------------------------------------------
template <bool IDENT>
__global__ __launch_bounds__(256) void components_seams_kernel(const unsigned char* __restrict__ labels, Geo g, int conn8, int* parent, int row_seams,
                                                               long items)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= items) return;
    const unsigned char* map = labels + (size_t)blockIdx.y * g.H * g.W;
    int* par = parent + (size_t)blockIdx.y * g.h * g.w;
    const int w = g.w;
    const long across = (long)row_seams * w;
    if (t < across) {
        // a pixel of a tile's first row: the edges up, up-left and up-right cross the horizontal seam; implied edges are left out as in phase 1
        const int y = TH * ((int)(t / w) + 1), x = (int)(t % w), p = y * w + x;
        const unsigned lab = label_at<IDENT>(map, g, y, x);
        if (lab == BG) return;
        const unsigned up = label_at<IDENT>(map, g, y - 1, x), left = label_at<IDENT>(map, g, y, x - 1), ul = label_at<IDENT>(map, g, y - 1, x - 1);
        if (up == lab) {
            if (left != lab || ul != lab) dev_union(par, p, p - w);
        } else if (conn8) {
            const unsigned right = label_at<IDENT>(map, g, y, x + 1), ur = label_at<IDENT>(map, g, y - 1, x + 1);
            if (ul == lab && left != lab) dev_union(par, p, p - w - 1);
            if (ur == lab && right != lab) dev_union(par, p, p - w + 1);
        }
    } else {
        // a pixel p of a tile's first column and its left neighbour q: the edge between them, implied by the same edge one row up when that row is
        // in the same tiles and holds the label on both sides; and the two diagonals across the vertical seam
        const long u = t - across;
        const int x = TW * ((int)(u / g.h) + 1), y = (int)(u % g.h), p = y * w + x, q = p - 1;
        const unsigned lp = label_at<IDENT>(map, g, y, x), lq = label_at<IDENT>(map, g, y, x - 1);
        const unsigned up_p = label_at<IDENT>(map, g, y - 1, x), up_q = label_at<IDENT>(map, g, y - 1, x - 1);
        if (lp != BG && lp == lq && !(y % TH != 0 && up_p == lp && up_q == lp)) dev_union(par, p, q);
        if (conn8 && y > 0) {
            if (lp != BG && up_q == lp && up_p != lp && lq != lp) dev_union(par, p, p - w - 1);
            if (lq != BG && up_p == lq && up_q != lq && lp != lq) dev_union(par, q, q - w + 1);
        }
    }
}

// ---- phases 3 and 7: a block's table of (key -> sums), filled by LDS atomics, flushed by the caller -----------------------------------------------------
// the entry of `key` (>= 0) in the table, or -1 when PROBES probes found neither it nor a free entry (the caller then goes to global memory)
__device__ __forceinline__ int table_entry(int* s_key, int key)
{
    const unsigned at = ((unsigned)key * 2654435761u) >> 24;
    for (int k = 0; k < PROBES; ++k) {
        const int e = (int)((at + k) & (TABLE - 1));
        const int old = atomicCAS(&s_key[e], -1, key);
        if (old == -1 || old == key) return e;
    }
    return -1;
}

// the key all lanes with pixels agree on, or -2: `leader` is the first lane with any
__device__ __forceinline__ int wave_key(int key, unsigned cnt, int& leader)
{
    const unsigned long long have = __ballot(cnt > 0);
    leader = have ? __ffsll((long long)have) - 1 : 0;
    const int lk = __shfl(key, leader, 64);
    return have && __all(cnt == 0 || key == lk) ? lk : -2;
}

__global__ __launch_bounds__(256) void components_flatten_kernel(int* parent, int* area, int h, int w)
{
    __shared__ int s_key[TABLE];
    __shared__ unsigned s_cnt[TABLE];
    s_key[threadIdx.x] = -1; s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int* par = parent + (size_t)blockIdx.y * h * w;
    int* ar = area + (size_t)blockIdx.y * h * w;
    const int UW = (w + 15) >> 4;
    const long units = (long)UW * h, u = (long)blockIdx.x * 256 + threadIdx.x;

    int key = -1;
    unsigned cnt = 0;
    auto flush = [&](int k, unsigned c) {
        if (k < 0 || !c) return;
        const int e = table_entry(s_key, k);
        if (e >= 0) atomicAdd(&s_cnt[e], c); else atomicAdd(&ar[k], (int)c);
    };
    if (u < units) {
        const int y = (int)(u / UW), x0 = (int)(u - (long)y * UW) << 4, m = min(16, w - x0), base = y * w + x0;
        for (int k = 0; k < m; ++k) {
            int r = par[base + k];
            if (r >= 0) {
                for (;;) {                                      // r strictly decreases: at most h * w steps
                    const int p = par[r];
                    if ((unsigned)p >= (unsigned)r) break;
                    r = p;
                }
                par[base + k] = r;          // (a concurrent reader sees the old parent or the root: both are ancestors)
            }
            if (r == key) ++cnt; else { flush(key, cnt); key = r; cnt = 1; }
        }
    }
    int leader;
    const int lk = wave_key(key, key < 0 ? 0u : cnt, leader);
    if (lk != -2) {
        unsigned a = key < 0 ? 0u : cnt;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
        if ((int)(threadIdx.x & 63) == leader) flush(lk, a);
    } else {
        flush(key, cnt);
    }
    __syncthreads();
    if (s_key[threadIdx.x] >= 0) atomicAdd(&ar[s_key[threadIdx.x]], (int)s_cnt[threadIdx.x]);
}

// ---- phases 4 .. 6 -----------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int qualifying(const int* par, const int* ar, int i, int px, int min_area) { return i < px && par[i] == i && ar[i] >= min_area; }

__global__ __launch_bounds__(256) void components_count_kernel(const int* __restrict__ parent, const int* __restrict__ area, int px, int min_area,
                                                               int* __restrict__ blocks)
{
    __shared__ int s_wave[4];
    const int* par = parent + (size_t)blockIdx.y * px;
    const int* ar = area + (size_t)blockIdx.y * px;
    const int i0 = blockIdx.x * CHUNK + threadIdx.x * 4;
    int mine = 0, total;
#pragma unroll
    for (int k = 0; k < 4; ++k) mine += qualifying(par, ar, i0 + k, px, min_area);
    block_exclusive_scan(mine, s_wave, total);
    if (threadIdx.x == 0) blocks[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void components_scan_kernel(int* __restrict__ blocks, int chunks, int* __restrict__ count)
{
    __shared__ int s_wave[4];
    int* b = blocks + (size_t)blockIdx.x * chunks;
    int carry = 0;
    for (int base = 0; base < chunks; base += 256) {             // ceil(chunks / 256) rounds
        const int i = base + threadIdx.x, v = i < chunks ? b[i] : 0;
        int total;
        const int before = block_exclusive_scan(v, s_wave, total);
        if (i < chunks) b[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

template <bool IDENT>
__global__ __launch_bounds__(256) void components_slots_kernel(const unsigned char* __restrict__ labels, Geo g, const int* __restrict__ parent, int* area,
                                                               int min_area, int max_components, const int* __restrict__ blocks, int* __restrict__ comp)
{
    __shared__ int s_wave[4];
    const int px = g.h * g.w;
    const int* par = parent + (size_t)blockIdx.y * px;
    int* ar = area + (size_t)blockIdx.y * px;
    const unsigned char* map = labels + (size_t)blockIdx.y * g.H * g.W;
    const int i0 = blockIdx.x * CHUNK + threadIdx.x * 4;
    int q[4], mine = 0, total;
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k] = qualifying(par, ar, i0 + k, px, min_area); mine += q[k]; }
    int slot = blocks[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + block_exclusive_scan(mine, s_wave, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + k;
        if (i >= px || par[i] != i) continue;                    // only roots hold an area; theirs becomes the slot
        int s = -1;
        if (q[k]) {
            if (slot < max_components) {
                s = slot;
                if (comp) {
                    const int y = i / g.w, x = i - y * g.w;
                    int* rec = comp + ((size_t)blockIdx.y * max_components + s) * 8;
                    rec[0] = (int)label_at<IDENT>(map, g, y, x); rec[1] = ar[i];
                    rec[2] = x; rec[3] = y; rec[4] = x; rec[5] = y; rec[6] = x; rec[7] = y;
                }
            }
            ++slot;
        }
        ar[i] = s;
    }
}

// ---- phase 7 -------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void components_records_kernel(const int* __restrict__ parent, const int* __restrict__ area, int h, int w,
                                                                 int max_components, int* comp, unsigned long long* sums, unsigned char* ids,
                                                                 size_t ids_pitch)
{
    __shared__ int s_key[TABLE];
    __shared__ unsigned long long s_sx[TABLE], s_sy[TABLE];
    __shared__ int s_box[TABLE * 4];
    s_key[threadIdx.x] = -1; s_sx[threadIdx.x] = 0; s_sy[threadIdx.x] = 0;
    s_box[4 * threadIdx.x] = 0x7fffffff; s_box[4 * threadIdx.x + 1] = 0x7fffffff; s_box[4 * threadIdx.x + 2] = -1; s_box[4 * threadIdx.x + 3] = -1;
    __syncthreads();
    const int* par = parent + (size_t)blockIdx.y * h * w;
    const int* ar = area + (size_t)blockIdx.y * h * w;
    int* rec = comp ? comp + (size_t)blockIdx.y * max_components * 8 : nullptr;
    unsigned long long* sm = sums ? sums + (size_t)blockIdx.y * max_components * 2 : nullptr;
    const bool records = rec || sm;
    const int UW = (w + 15) >> 4;
    const long units = (long)UW * h, u = (long)blockIdx.x * 256 + threadIdx.x;

    auto to_global = [&](int s, unsigned long long tx, unsigned long long ty, int x0, int y0, int x1, int y1) {
        if (sm) { if (tx) atomicAdd(&sm[2 * s], tx); if (ty) atomicAdd(&sm[2 * s + 1], ty); }
        if (rec) { atomicMin(&rec[8 * s + 2], x0); atomicMin(&rec[8 * s + 3], y0); atomicMax(&rec[8 * s + 4], x1); atomicMax(&rec[8 * s + 5], y1); }
    };
    auto flush = [&](int s, unsigned long long tx, unsigned long long ty, int x0, int y0, int x1, int y1) {
        if (s < 0 || !records) return;
        const int e = table_entry(s_key, s);
        if (e < 0) { to_global(s, tx, ty, x0, y0, x1, y1); return; }
        atomicAdd(&s_sx[e], tx); atomicAdd(&s_sy[e], ty);
        atomicMin(&s_box[4 * e], x0); atomicMin(&s_box[4 * e + 1], y0); atomicMax(&s_box[4 * e + 2], x1); atomicMax(&s_box[4 * e + 3], y1);
    };

    // the run in registers: slot `key`, cnt pixels from bx0 to bx1 of row y
    int key = -1, bx0 = 0x7fffffff, bx1 = -1, y = 0;
    unsigned cnt = 0, sx = 0;
    if (u < units) {
        y = (int)(u / UW);
        const int x0 = (int)(u - (long)y * UW) << 4, m = min(16, w - x0), base = y * w + x0;
        int* out = ids ? reinterpret_cast<int*>(ids + ((size_t)blockIdx.y * h + y) * ids_pitch) + x0 : nullptr;
        for (int k = 0; k < m; ++k) {
            const int r = par[base + k];
            const int s = r < 0 ? -1 : ar[r];
            if (out) out[k] = s;
            if (s == key) { ++cnt; sx += (unsigned)(x0 + k); bx1 = x0 + k; }
            else {
                if (cnt) flush(key, sx, (unsigned long long)cnt * (unsigned)y, bx0, y, bx1, y);
                key = s; cnt = 1; sx = (unsigned)(x0 + k); bx0 = bx1 = x0 + k;
            }
        }
    }
    if (!records) return;
    const unsigned mine = key < 0 ? 0u : cnt;
    int leader;
    const int lk = wave_key(key, mine, leader);
    if (lk != -2) {
        unsigned long long tx = mine ? sx : 0u, ty = (unsigned long long)mine * (unsigned)y;
        int x0 = mine ? bx0 : 0x7fffffff, x1 = mine ? bx1 : -1, y0 = mine ? y : 0x7fffffff, y1 = mine ? y : -1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            tx += __shfl_xor(tx, off, 64); ty += __shfl_xor(ty, off, 64);
            x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
            x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
        }
        if ((int)(threadIdx.x & 63) == leader) flush(lk, tx, ty, x0, y0, x1, y1);
    } else if (mine) {
        flush(key, sx, (unsigned long long)cnt * (unsigned)y, bx0, y, bx1, y);
    }
    __syncthreads();
    const int s = s_key[threadIdx.x];
    if (s >= 0) to_global(s, s_sx[threadIdx.x], s_sy[threadIdx.x], s_box[4 * threadIdx.x], s_box[4 * threadIdx.x + 1], s_box[4 * threadIdx.x + 2],
                          s_box[4 * threadIdx.x + 3]);
}

// -1 into comp, zeros into sums
__global__ __launch_bounds__(256) void components_init_kernel(int* comp, long n_comp, unsigned long long* sums, long n_sums)
{
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_comp; i += stride) comp[i] = -1;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_sums; i += stride) sums[i] = 0ull;
}

}  // namespace

size_t labels_components_chunks(int h, int w) { return ((size_t)h * w + CHUNK - 1) / CHUNK; }

// The callers (accel_io.cpp components_args) have checked: 1 <= n <= 32768, 1 <= out_h <= H <= 32768, 1 <= out_w <= W <= 32768, 1 <= h, w <= 32768,
// 1 <= ncls <= 32, connectivity 4 or 8, min_area >= 1, 1 <= max_components <= 65536, ids_pitch >= 4 * w and a multiple of 4, count non-null.
// Scratch: parent and area hold n * h * w int32 each, blocks n * labels_components_chunks(h, w).  Reads of `labels` stay inside out_h x out_w of each
// of the n maps (row and column indices are clamped); every scratch index is below n * h * w (chunks); count (n), comp (n x max_components x 8)
// and sums (n x max_components x 2) are OVERWRITTEN; ids receives w words in each of its n * h rows.
hipError_t launch_labels_components(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls, int connectivity,
                                    int min_area, int max_components, int* parent, int* area, int* blocks, int* count, int* comp,
                                    unsigned long long* sums, int* ids, size_t ids_pitch, hipStream_t st)
{
    if (!parent || !area || !blocks || !count) return hipErrorInvalidValue;
    const Geo g = {H, W, out_h, out_w, h, w, ncls};
    const bool ident = h == out_h && w == out_w;
    const int conn8 = connectivity == 8;
    const int px = h * w;
    hipError_t e;
#define CC_CHECK() do { e = hipGetLastError(); if (e != hipSuccess) return e; } while (0)
    if (comp || sums) {
        const long nc = comp ? (long)n * max_components * 8 : 0, ns = sums ? (long)n * max_components * 2 : 0;
        long blocks_i = ((nc > ns ? nc : ns) + 255) / 256;
        if (blocks_i > 1024) blocks_i = 1024;
        hipLaunchKernelGGL(components_init_kernel, dim3((unsigned)blocks_i), dim3(256), 0, st, comp, nc, sums, ns);
        CC_CHECK();
    }
    const dim3 tiles((unsigned)((w + TW - 1) / TW), (unsigned)((h + TH - 1) / TH), (unsigned)n);
    if (ident) hipLaunchKernelGGL(components_tiles_kernel<true>, tiles, dim3(256), 0, st, labels, g, conn8, parent, area);
    else hipLaunchKernelGGL(components_tiles_kernel<false>, tiles, dim3(256), 0, st, labels, g, conn8, parent, area);
    CC_CHECK();
    const int row_seams = (h - 1) / TH, col_seams = (w - 1) / TW;
    const long items = (long)row_seams * w + (long)col_seams * h;
    if (items) {
        const dim3 grid((unsigned)((items + 255) / 256), (unsigned)n);
        if (ident) hipLaunchKernelGGL(components_seams_kernel<true>, grid, dim3(256), 0, st, labels, g, conn8, parent, row_seams, items);
        else hipLaunchKernelGGL(components_seams_kernel<false>, grid, dim3(256), 0, st, labels, g, conn8, parent, row_seams, items);
        CC_CHECK();
    }
    const long units = (long)((w + 15) / 16) * h;
    const dim3 per_unit((unsigned)((units + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(components_flatten_kernel, per_unit, dim3(256), 0, st, parent, area, h, w);
    CC_CHECK();
    const int chunks = (int)labels_components_chunks(h, w);
    const dim3 per_chunk((unsigned)chunks, (unsigned)n);
    hipLaunchKernelGGL(components_count_kernel, per_chunk, dim3(256), 0, st, parent, area, px, min_area, blocks);
    CC_CHECK();
    hipLaunchKernelGGL(components_scan_kernel, dim3((unsigned)n), dim3(256), 0, st, blocks, chunks, count);
    CC_CHECK();
    if (ident) hipLaunchKernelGGL(components_slots_kernel<true>, per_chunk, dim3(256), 0, st, labels, g, parent, area, min_area, max_components, blocks, comp);
    else hipLaunchKernelGGL(components_slots_kernel<false>, per_chunk, dim3(256), 0, st, labels, g, parent, area, min_area, max_components, blocks, comp);
    CC_CHECK();
    if (comp || sums || ids) {
        hipLaunchKernelGGL(components_records_kernel, per_unit, dim3(256), 0, st, parent, area, h, w, max_components, comp, sums,
                           reinterpret_cast<unsigned char*>(ids), ids_pitch);
        CC_CHECK();
    }
#undef CC_CHECK
    return hipSuccess;
}
