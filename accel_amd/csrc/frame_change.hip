// How much a frame differs from the kept key frame, measured where every input route leaves it: the image input (n x 3 x H x W fp32, planes R, G, B,
// mean-subtracted and padded -- `data`) read once, its valid region out_h x out_w summed into a grid of cell x cell cells (the SIGNATURE) and, in
// the same launch, compared cell by cell with the signature of the key frame.  The arithmetic is integer and is restated bit for bit by
// accel_amd/utils/image.py frame_signature_host / frame_change_host:
//   q = int(rint(fmin(fmax(x, -512), 512) * 8))      fp32, round half to even; NaN -> -4096, +-inf -> +-4096
//   v = 2 qR + 5 qG + qB                             64 units per grey level
//   S = the sum of v over the valid pixels of the cell            (|S| <= 2^27: int32 never overflows)
//   d = |S - S_key|,  changed iff d > level_q * area  (int64, strict; area = the valid pixels of the cell, edge cells are smaller)
//   per frame: changed = the number of changed cells (uint32), sad = the sum of d (uint64), mask = 1 where a cell changed
//
// A block of 4 wavefronts owns one row of cells over 64 * V columns (V = 4: 256, V = 1: 64 -- whole cells for every cell size): lane l of
// every wavefront owns the columns x0 .. x0 + V - 1, wavefront r the rows r, r + 4, .. of the cell row.  So the signature words are plain stores,
// and the sums are exact whatever the order.  V = 4: one 16-byte load per plane and row where W % 4 == 0 and the base is 16-byte aligned (the
// launcher checks); a quad that straddles out_w is read pixel by pixel, so nothing outside out_h x out_w is ever read.  V = 1 covers the rest.
// changed and sad: summed over the block's cells in registers first, then one 32-bit and one 64-bit atomic per block into the frame's words,
// which the launcher has zeroed.  blockIdx.y is the row of cells, blockIdx.z the frame.  The kernel only READS the image and the key signature.
#include "kernels.h"
#include <stdint.h>

namespace {

__device__ __forceinline__ int quantise(float x)
{
    return (int)rintf(fminf(fmaxf(x, -512.0f), 512.0f) * 8.0f);
}

struct ChangeOut {
    int* sig;                        // n x gh x gw
    unsigned* changed;               // n
    unsigned long long* sad;         // n
    unsigned char* mask; size_t mask_pitch;      // n x gh rows, mask_pitch bytes apart
};

template <int V>
__global__ __launch_bounds__(256) void frame_change_kernel(const float* __restrict__ img, const int* __restrict__ sig_key, int H, int W, int out_h, int out_w,
                                                           int cell_shift, int level_q, int gh, int gw, ChangeOut o)
{
    __shared__ int sums[256 / 8];                // one word per cell of the block (V = 4, cell = 8: 32 cells)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cell = 1 << cell_shift;
    const int cy = blockIdx.y, z = blockIdx.z;
    const int x0 = ((int)blockIdx.x * 64 + lane) * V;
    if (threadIdx.x < 32) sums[threadIdx.x] = 0;
    __syncthreads();

    const size_t plane = (size_t)H * W;
    const float* frame = img + (size_t)z * 3 * plane;
    const int y_end = min((cy + 1) << cell_shift, out_h);
    int acc = 0;
    if (x0 < out_w) {
        const bool whole = V == 1 || x0 + V <= out_w;
#pragma unroll 4
        for (int y = (cy << cell_shift) + wave; y < y_end; y += 4) {
            const float* p = frame + (size_t)y * W + x0;
            if (V == 4 && whole) {
                const float4 r = *reinterpret_cast<const float4*>(p);
                const float4 g = *reinterpret_cast<const float4*>(p + plane);
                const float4 b = *reinterpret_cast<const float4*>(p + 2 * plane);
                acc += 2 * (quantise(r.x) + quantise(r.y) + quantise(r.z) + quantise(r.w));
                acc += 5 * (quantise(g.x) + quantise(g.y) + quantise(g.z) + quantise(g.w));
                acc += quantise(b.x) + quantise(b.y) + quantise(b.z) + quantise(b.w);
            } else {
                for (int j = 0; j < V && x0 + j < out_w; ++j)
                    acc += 2 * quantise(p[j]) + 5 * quantise(p[plane + j]) + quantise(p[2 * plane + j]);
            }
        }
    }
    // the lanes of one cell are cell / V neighbours of one wavefront (2 .. 64, a power of two, aligned): butterfly, then one LDS add per wavefront and cell
    const int group = cell / V;
    for (int off = group >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((lane & (group - 1)) == 0) atomicAdd(&sums[lane / group], acc);
    __syncthreads();

    if (wave != 0) return;
    const int cells = 64 * V / cell;             // of this block: <= 32
    const int cx = (int)blockIdx.x * cells + lane;
    unsigned cnt = 0;
    unsigned long long dist = 0;
    if (lane < cells && cx < gw) {
        const int s = sums[lane];
        const size_t at = ((size_t)z * gh + cy) * gw + cx;
        if (o.sig) o.sig[at] = s;
        if (sig_key) {
            const int d = abs(s - sig_key[at]);                                  // <= 2^28
            const int area = (y_end - (cy << cell_shift)) * (min((cx + 1) << cell_shift, out_w) - (cx << cell_shift));
            cnt = (long long)d > (long long)level_q * area ? 1u : 0u;
            dist = (unsigned long long)d;
            if (o.mask) o.mask[((size_t)z * gh + cy) * o.mask_pitch + cx] = (unsigned char)cnt;
        }
    }
    if (!sig_key || (!o.changed && !o.sad)) return;      // uniform
    for (int off = 16; off > 0; off >>= 1) {
        cnt += __shfl_down(cnt, off);
        dist += __shfl_down(dist, off);
    }
    if (lane == 0) {
        if (o.changed && cnt) atomicAdd(o.changed + z, cnt);
        if (o.sad && dist) atomicAdd(o.sad + z, dist);
    }
}

}  // namespace

// The callers (accel_io.cpp frame_change_args) have checked: 1 <= n <= 32768, 1 <= out_h <= H <= 32768, 1 <= out_w <= W <= 32768, cell in {8, 16, 32,
// 64}, 0 <= level_q <= 32768, at least one output, changed / sad / mask only with a key, mask_pitch >= gw.  Reads of `img` stay inside out_h x out_w of
// each of the n * 3 planes, reads of sig_key and writes of sig inside n * gh * gw words, writes of mask inside gw bytes of each of the n * gh rows;
// changed and sad (n words each) are OVERWRITTEN (zeroed here first).
hipError_t launch_frame_change(const float* img, const int* sig_key, int n, int H, int W, int out_h, int out_w, int cell, int level_q, int* sig_out,
                               unsigned* changed, unsigned long long* sad, unsigned char* mask, size_t mask_pitch, hipStream_t st)
{
    const int shift = cell == 8 ? 3 : cell == 16 ? 4 : cell == 32 ? 5 : cell == 64 ? 6 : 0;
    if (!shift || (!sig_out && !changed && !sad && !mask) || (!sig_key && (changed || sad || mask))) return hipErrorInvalidValue;
    if (changed) {
        const hipError_t e = hipMemsetAsync(changed, 0, (size_t)n * sizeof(unsigned), st);
        if (e != hipSuccess) return e;
    }
    if (sad) {
        const hipError_t e = hipMemsetAsync(sad, 0, (size_t)n * sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
    }
    const int gh = (out_h + cell - 1) >> shift, gw = (out_w + cell - 1) >> shift;
    const ChangeOut o = {sig_out, changed, sad, mask, mask_pitch};
    const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(img) % 16 == 0;
    const int reach = vec ? 256 : 64;            // columns per block
    const dim3 grid((unsigned)((out_w + reach - 1) / reach), (unsigned)gh, (unsigned)n);
    if (vec) hipLaunchKernelGGL(frame_change_kernel<4>, grid, dim3(256), 0, st, img, sig_key, H, W, out_h, out_w, shift, level_q, gh, gw, o);
    else hipLaunchKernelGGL(frame_change_kernel<1>, grid, dim3(256), 0, st, img, sig_key, H, W, out_h, out_w, shift, level_q, gh, gw, o);
    return hipGetLastError();
}
