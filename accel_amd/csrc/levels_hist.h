// The histogram of conf levels per frame, as both forms of confidence.hip count it: runs of equal levels in a register, then 256
// block-private 32-bit LDS bins, then one 64-bit atomic per non-zero bin per block into the frame's 256 words.  A block of 256 threads that never
// spans two frames; the bins are zeroed (and a barrier passed) before the first count.  Integer sums: exact, independent of the order of arrival.
#pragma once
#include <hip/hip_runtime.h>

namespace levels {

// one more pixel at level c: `key`, `cnt` are the run of equal levels this thread is in
__device__ __forceinline__ void count(unsigned* bins, unsigned& key, unsigned& cnt, unsigned c)
{
    if (c == key) {
        ++cnt;
    } else {
        if (cnt) atomicAdd(&bins[key], cnt);
        key = c; cnt = 1;
    }
}

// the end of the block's pixels: every lane's last run into the bins, the bins into the frame's 256 words `hist`.  Reached by all 256 threads
__device__ __forceinline__ void flush(unsigned* bins, unsigned key, unsigned cnt, unsigned long long* hist)
{
    // the run every lane still holds: one add for the wavefront when it is the same level in all of them (a saturated region)
    const unsigned lk = __builtin_amdgcn_readfirstlane(key);
    if (!cnt) key = lk;       // a lane that counted nothing agrees with anyone
    if (__all(key == lk)) {
        unsigned sum = cnt;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&bins[lk], sum);
    } else if (cnt) {
        atomicAdd(&bins[key], cnt);
    }
    __syncthreads();
    const unsigned v = bins[threadIdx.x];
    if (v) atomicAdd(&hist[threadIdx.x], (unsigned long long)v);
}

}  // namespace levels
