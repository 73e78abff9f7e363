// kr_dev_sort.inc -- part of kr_build_keys.hip and of kr_index_stats.hip (after kr_dev_prefix.inc, inside the file's unnamed namespace):
// one pass of the least-significant-digit radix sort over (64-bit key, 32-bit rank) pairs, 8-bit digits, out of place between two pairs
// of buffers, and the 64-bit prefix sum over an array in HBM that the pass and the stages around it share.  One pass is
//   kr_keys_hist_kernel      a workgroup per tile of kTile pairs: the tile's digit histogram in LDS -> counts[digit][tile]
//   scan_u64<false>          exclusive prefix sum over the 256 x ntiles counts in that (digit-major) order
//   kr_keys_scatter_kernel   every pair to its digit's running position; STABLE (see kr_build_keys.hip)
// A caller that sorts keys alone passes from_rank = 0 and any two rank buffers of the keys' length: the ranks travel with their keys.
// The kernels hold scalars and statically sized LDS only.

constexpr uint32_t kTile = 2048;        // pairs per workgroup of a pass
constexpr uint32_t kQuarter = kTile / 4; // ... per wave
constexpr uint32_t kScanBlock = 1024;   // items per workgroup of the scans (4 per thread)

// digit `shift / 8` of the rank (from_rank) or of the key
__device__ __forceinline__ uint32_t digit_at(const uint64_t* keys, const uint32_t* ranks, uint64_t i, uint32_t from_rank, uint32_t shift)
{
  return from_rank ? (ranks[i] >> shift) & 255u : (uint32_t)(keys[i] >> shift) & 255u;
}

__global__ __launch_bounds__(256) void kr_keys_hist_kernel(const uint64_t* keys, const uint32_t* ranks, uint64_t n, uint32_t ntiles, uint32_t from_rank,
                                                           uint32_t shift, uint64_t* counts)
{
  __shared__ uint32_t s_h[256];
  const uint32_t tid = threadIdx.x, tile = blockIdx.x;
  s_h[tid] = 0;
  __syncthreads();
  const uint64_t t0 = (uint64_t)tile * kTile;
#pragma unroll
  for (uint32_t q = 0; q < kTile / 256u; ++q) {
    const uint64_t i = t0 + q * 256u + tid;
    if (i < n) atomicAdd(&s_h[digit_at(keys, ranks, i, from_rank, shift)], 1u);
  }
  __syncthreads();
  counts[(uint64_t)tid * ntiles + tile] = s_h[tid];
}

// The three steps of kr_dev_prefix.inc over m 64-bit items, in place; INCL: every item gets the sum up to and including itself
__global__ __launch_bounds__(256) void kr_keys_bsum_kernel(const uint64_t* v, uint64_t m, uint64_t* bsum)
{
  for (uint64_t b = blockIdx.x; b * kScanBlock < m; b += gridDim.x) {
    uint64_t c = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint64_t i = b * kScanBlock + 4u * threadIdx.x + q;
      if (i < m) c += v[i];
    }
    const uint64_t tot = block_sum<uint64_t>(c);
    if (threadIdx.x == 0) bsum[b] = tot;
  }
}
__global__ __launch_bounds__(1024) void kr_keys_bscan_kernel(uint64_t* bsum, uint32_t nblk, uint64_t* total)
{
  const uint64_t tot = scan_block_sums<uint64_t>(bsum, nblk);
  if (threadIdx.x == 0) *total = tot;
}
template <bool INCL>
__global__ __launch_bounds__(256) void kr_keys_bwrite_kernel(uint64_t* v, uint64_t m, const uint64_t* bsum)
{
  for (uint64_t b = blockIdx.x; b * kScanBlock < m; b += gridDim.x) {
    const uint64_t i0 = b * kScanBlock + 4u * threadIdx.x;
    const uint64_t c0 = i0 < m ? v[i0] : 0, c1 = i0 + 1 < m ? v[i0 + 1] : 0, c2 = i0 + 2 < m ? v[i0 + 2] : 0, c3 = i0 + 3 < m ? v[i0 + 3] : 0;
    uint64_t run = bsum[b] + block_scan_excl<uint64_t>(c0 + c1 + c2 + c3);
    if (INCL) run += c0;
    if (i0 < m) v[i0] = run;
    run += INCL ? c1 : c0;
    if (i0 + 1 < m) v[i0 + 1] = run;
    run += INCL ? c2 : c1;
    if (i0 + 2 < m) v[i0 + 2] = run;
    run += INCL ? c3 : c2;
    if (i0 + 3 < m) v[i0 + 3] = run;
  }
}

// offs: the scanned counts.  Positions stay below n because the histogram counted these very pairs.
__global__ __launch_bounds__(256) void kr_keys_scatter_kernel(const uint64_t* kin, const uint32_t* rin, uint64_t* kout, uint32_t* rout, uint64_t n,
                                                              uint32_t ntiles, uint32_t from_rank, uint32_t shift, const uint64_t* offs)
{
  __shared__ uint32_t s_cnt[4][256];  // pairs of a digit in each wave's quarter
  __shared__ uint64_t s_pos[4][256];  // where the wave's next pair of a digit goes
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
  s_cnt[0][tid] = 0, s_cnt[1][tid] = 0, s_cnt[2][tid] = 0, s_cnt[3][tid] = 0;
  __syncthreads();
  const uint64_t w0 = (uint64_t)tile * kTile + (uint64_t)wave * kQuarter;
#pragma unroll
  for (uint32_t s = 0; s < kQuarter / 64u; ++s) {
    const uint64_t i = w0 + s * 64u + lane;
    if (i < n) atomicAdd(&s_cnt[wave][digit_at(kin, rin, i, from_rank, shift)], 1u);
  }
  __syncthreads();
  { // thread = digit: the digit's first position in this tile, then quarter by quarter
    uint64_t run = offs[(uint64_t)tid * ntiles + tile];
    s_pos[0][tid] = run, run += s_cnt[0][tid];
    s_pos[1][tid] = run, run += s_cnt[1][tid];
    s_pos[2][tid] = run, run += s_cnt[2][tid];
    s_pos[3][tid] = run;
  }
  __syncthreads();
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t s = 0; s < kQuarter / 64u; ++s) { // (from here on a wave touches its own row of s_pos only)
    const uint64_t i = w0 + s * 64u + lane;
    const bool valid = i < n;
    uint64_t key = 0;
    uint32_t rank = 0;
    if (valid) key = kin[i], rank = rin[i];
    const uint32_t d = from_rank ? (rank >> shift) & 255u : (uint32_t)(key >> shift) & 255u;
    uint64_t peers = __ballot(valid); // the valid lanes with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    if (valid) {
      const uint64_t at = s_pos[wave][d] + (uint64_t)__popcll(peers & below);
      if (at < n) kout[at] = key, rout[at] = rank;
    }
    __builtin_amdgcn_wave_barrier(); // every peer has read the digit's position before its first lane moves it on
    if (valid && (peers & below) == 0) s_pos[wave][d] += (uint64_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
}

uint32_t ceil_log2(uint64_t v)
{ // bits needed to tell v values apart
  uint32_t b = 0;
  while (b < 64 && (1ull << b) < v) ++b;
  return b;
}
struct Pass {
  uint32_t from_rank, shift;
};

uint64_t scan_blocks(uint64_t m) { return (m + kScanBlock - 1) / kScanBlock; }
uint32_t grid_for(uint64_t blocks) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 65536); }

// In-place exclusive (or inclusive) prefix sum over v[0 .. m) on the null stream; the total into *d_total
template <bool INCL>
void scan_u64(uint64_t* v, uint64_t m, uint64_t* bsum, uint64_t* d_total)
{
  const uint64_t nblk = scan_blocks(m);
  hipLaunchKernelGGL(kr_keys_bsum_kernel, dim3(grid_for(nblk)), dim3(256), 0, 0, v, m, bsum);
  hipLaunchKernelGGL(kr_keys_bscan_kernel, dim3(1), dim3(1024), 0, 0, bsum, (uint32_t)nblk, d_total);
  hipLaunchKernelGGL(kr_keys_bwrite_kernel<INCL>, dim3(grid_for(nblk)), dim3(256), 0, 0, v, m, bsum);
}
