// kr_dev_prefix.inc -- part of kr_device.hip (one translation unit, included in order) and of kr_build_keys.hip: the prefix sums of the
// stages that compact variable-length output (rows, `dist` text, `place` text, FASTQ records) and of the builder's key stage (digit
// counts, group positions, row counts).  Every one of them runs the same three steps:
//   1. a workgroup of 256 sums its block of items                                     (block_sum / block_sum_waves)
//   2. ONE workgroup of 1024 turns the block sums into the blocks' first positions     (scan_block_sums)
//   3. a workgroup of 256 scans its block's items from there, thread t owning the items 4t .. 4t+3: the helper gives the thread the
//      sum of the lower threads' totals, the caller keeps its own unrolling, guards and stores   (block_scan_excl)
// T is uint32_t or uint64_t.  The workgroup helpers own their LDS scratch and open with a barrier, so that a call may follow any other
// call -- in a grid-stride loop, or twice in one iteration -- without the caller ordering anything; they must be reached by every
// thread of the workgroup.  kr_debug_prefix (kr_dev_debug.inc) runs the three steps on plain numbers: tests/test_gpu_prefix.py.
// The file stands on its own for 64-bit sums; sums of uint32_t use the wave scan of kr_dev_common.inc, which must come first then.

// Inclusive prefix sum over the wave, 64-bit (the 32-bit one, on the DPP network: kr_dev_common.inc)
__device__ __forceinline__ uint64_t wave_scan_incl(uint64_t v)
{
  const uint32_t lane = __lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(v, d);
    if (lane >= (uint32_t)d) v += up;
  }
  return v;
}

// Sum over the wave; every lane gets it
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Sum over a workgroup of 256 lanes; EVERY lane gets it.  block_sum_waves: of one value per wave, for a caller whose value is
// wave-uniform already (a wave per read) and has no reduction to pay for.
template <typename T>
__device__ __forceinline__ T block_sum_waves(T wave_total)
{
  __shared__ T s_w[4];
  __syncthreads();
  if (__lane_id() == 0) s_w[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
template <typename T>
__device__ __forceinline__ T block_sum(T v) { return block_sum_waves<T>(wave_sum(v)); }

// Exclusive scan over a workgroup of 256 lanes of one total per thread: the sum of the totals of all lower threads
template <typename T>
__device__ __forceinline__ T block_scan_excl(T tot)
{
  __shared__ T s_w[4];
  const uint32_t w = threadIdx.x >> 6;
  const T inc = wave_scan_incl(tot);
  __syncthreads();
  if (__lane_id() == 63u) s_w[w] = inc;
  __syncthreads();
  T run = inc - tot;
  for (uint32_t q = 0; q < w; ++q) run += s_w[q];
  return run;
}

// Exclusive scan of the n block sums a[0 .. n) in place, by all 1024 threads of ONE workgroup; EVERY thread gets the total.  Rounds of
// 1024 sums; every thread carries the running total of the rounds before in a register.
template <typename T>
__device__ __forceinline__ T scan_block_sums(T* a, uint32_t n)
{
  __shared__ T s_w[16];
  const uint32_t w = threadIdx.x >> 6;
  T run = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += 1024u) {
    const uint32_t b = b0 + threadIdx.x;
    const T c = b < n ? a[b] : (T)0;
    const T inc = wave_scan_incl(c);
    __syncthreads();
    if (__lane_id() == 63u) s_w[w] = inc;
    __syncthreads();
    T below = 0, all = 0;
#pragma unroll 4
    for (uint32_t q = 0; q < 16u; ++q) {
      if (q < w) below += s_w[q];
      all += s_w[q];
    }
    if (b < n) a[b] = run + below + inc - c;
    run += all;
  }
  return run;
}
