// lzani_block.h -- what the threads of one block work out together: a sum, a rank, a step of an exclusive scan.  Device
// only; included by lzani_kernels_index.h and lzani_kernels_prefilter.h (after lzani_core.h: u32, u64), and by no header
// that lzani_rtc.h embeds.  Every function here holds barriers: EVERY thread of the block calls it, the same number of
// times, from block-uniform control flow.
#pragma once

namespace lzani {

// The block sum: *s_sum += the `mine` of every thread of the block, one LDS atomic per wave that has something.
// s_sum is a __shared__ word that thread 0 cleared before a barrier that lies before this call.  Ends in a barrier:
// behind it every thread may read *s_sum.  Any block size that is a multiple of 64.
__device__ __forceinline__ void block_sum(u32 mine, u32* s_sum)
{
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(s_sum, mine);
    __syncthreads();
}

// The block rank, among the block's THREADS threads: how many threads before this one raise `flag`; total: how many in
// all.  s_w is __shared__ u32[THREADS / 64] that nothing else uses; nothing has to be cleared.  Two barriers, the second
// behind the last read of s_w: the next call may follow at once.
template <int THREADS>
__device__ __forceinline__ u32 block_rank(bool flag, u32* s_w, u32& total)
{
    const u64 m = __builtin_amdgcn_ballot_w64(flag);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_w[wv] = (u32)__popcll(m);
    __syncthreads();
    u32 off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) { const u32 c = s_w[k]; off += k < wv ? c : 0u; tot += c; }
    __syncthreads();
    total = tot;
    return off + (u32)__popcll(m & ((1ULL << lane) - 1ULL));
}

__device__ __forceinline__ u32 block_shfl_up(u32 x, int d) { return __shfl_up(x, d); }
__device__ __forceinline__ u64 block_shfl_up(u64 x, int d)
{
    const u32 lo = __shfl_up((u32)x, d), hi = __shfl_up((u32)(x >> 32), d);
    return ((u64)hi << 32) | lo;
}

// One step of a one-block exclusive scan, the block of exactly 1,024 threads; T is u32 or u64.  v: this thread's value of
// the step.  Returns the sum of the values of all threads before this one, those of the earlier steps included, and
// moves the carry on by the step's sum.  s_wsum is __shared__ T[16], *s_carry a __shared__ T that thread 0 set to zero
// before a barrier that lies before the first step; behind the last step every thread reads the total there.  Three
// barriers, the last one behind the carry's write: the next step, or the read of the total, may follow at once.
template <typename T>
__device__ __forceinline__ T block_scan_step(T v, T* s_wsum, T* s_carry)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T x = v;                                         // inclusive scan inside the wave
    for (int d = 1; d < 64; d <<= 1) { const T y = block_shfl_up(x, d); if (lane >= d) x += y; }
    if (lane == 63) s_wsum[wv] = x;
    __syncthreads();
    T woff = 0;
    for (int k = 0; k < wv; ++k) woff += s_wsum[k];
    const T carry = *s_carry;
    __syncthreads();
    if (threadIdx.x == 1023) *s_carry = carry + woff + x;
    __syncthreads();
    return carry + woff + x - v;
}

}  // namespace lzani
