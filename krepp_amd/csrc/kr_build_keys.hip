// kr_build_keys.hip — the key stage of the index and sketch builds on gfx950: all genomes' (key, leaf rank) pairs sorted by
// (key, rank), duplicates dropped, cut into groups of equal key, rows counted (kr_key_groups_device; the builder's pool of keys).
//
// Sort: least-significant-digit radix sort, 8-bit digits, out of place between two buffers; the rank's digits first, then the
// key's, so that the final order is (key, rank).  Only digits that can differ are sorted: ceil(log2(nleaves)) bits of rank,
// 32 bits of enc plus ceil(log2(nrows)) bits of row (digit_passes).  One pass (kr_dev_sort.inc, shared with kr_index_stats.hip) is
//   kr_keys_hist_kernel      a workgroup per tile of kTile pairs: the tile's digit histogram in LDS -> counts[digit][tile]
//   three scan kernels       exclusive prefix sum over the 256 x ntiles counts in that (digit-major) order: a pair's digit
//                            bucket starts where all smaller digits and the same digit's earlier tiles end (kr_dev_prefix.inc)
//   kr_keys_scatter_kernel   the waves of a workgroup own consecutive quarters of the tile; a wave takes 64 pairs at a time in
//                            tile order, finds each pair's peers of equal digit by eight ballots, and puts it at the digit's
//                            running position plus the number of peers in lower lanes
// Every pass is STABLE: tiles, a tile's quarters, a quarter's steps and a step's lanes all keep the input order within a digit.
// The leaf stage appends keys by atomics, so the arrival order differs between runs; the output does not.
//
// Grouping, on the sorted pairs: a pair is kept unless it equals its predecessor, and is a head if its key differs from the
// predecessor's.  Block sums of both flags, their scans, and one kernel that recomputes the flags, scans them within the block and
// writes ranks[kept position], keys / goff[head position], and adds 1 to inc[row] at a head (an ordinary vector atomic); a 64-bit
// inclusive scan over the rows turns inc into the cumulative counts.
//
// Colour classes (kr_colour_classes_device; KR_BUILD_GPU_COLOURS), on the groups while they are on the device: the distinct rank
// sequences among the groups of two or more ranks, numbered in the order of their first groups.
//   kr_classes_term_kernel     a 64-bit term per kept rank, fmix64(rank + 1); ONE exclusive scan (wrapping sums) over all of them
//   kr_classes_flag_kernel     1 per group of >= 2 ranks; its exclusive scan is the group's place in the multi-rank list
//   kr_classes_list_kernel     list entry = (fingerprint, group index), fingerprint = S[goff[i+1]] - S[goff[i]] + fmix64(length):
//                              work in proportion to the ranks, whatever the group lengths
//   the sort above             key passes only, the group index in the rank slot; stable, and the list is in group order, so
//                              equal fingerprints stay in ascending group index
//   kr_classes_head_kernel     an entry is a head unless fingerprint, length AND ranks equal its predecessor's.  The hash only
//                              brings candidates together; the ranks decide.  A lane compares up to kLaneCompare ranks alone,
//                              longer groups are compared by the whole wave, one after the other
//   two scans                  of the head flags over the sorted list (the entry's run) and of the heads' flags over the groups
//                              (class numbers in group order = order of first appearance)
//   kr_classes_rep_kernel      a head writes rep[class] and its run's leading group; kr_classes_member_kernel gives every entry
//                              the class of its run's leading group
// With A, B, A under one fingerprint the second A opens a class of its own: more work for the builder (a repeated fold creates
// nothing), the same files.
//
// No per-lane private arrays, no dynamic LDS: the kernels hold scalars and statically sized LDS only.
#include "kr_common.h"
#include "kr_devutil.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

#include "kr_dev_prefix.inc" // (64-bit sums only here: the 32-bit wave scan on the DPP network is kr_dev_common.inc's)
#include "kr_dev_sort.inc"   // the radix sort's pass (kTile, hist / scatter kernels), scan_u64, Pass: shared with kr_index_stats.hip

// bit 0: a row >= nrows, bit 1: a rank >= nleaves
__global__ __launch_bounds__(256) void kr_keys_check_kernel(const uint64_t* keys, const uint32_t* ranks, uint64_t n, uint32_t nrows, uint32_t nleaves,
                                                            uint32_t* bad)
{
  uint32_t f = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    if ((uint32_t)(keys[i] >> 32) >= nrows) f |= 1u;
    if (ranks[i] >= nleaves) f |= 2u;
  }
  if (f) atomicOr(bad, f);
}

// ranks[i] = the leaf rank of the segment that holds i: seg_off[0 .. nseg] ascending, seg_off[nseg] = n
__global__ __launch_bounds__(256) void kr_keys_expand_kernel(const uint64_t* seg_off, const uint32_t* seg_rank, uint32_t nseg, uint64_t n, uint32_t* ranks)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    uint32_t lo = 0, hi = nseg; // the last segment with seg_off <= i (empty segments share an offset: the last of them is skipped over)
    while (hi - lo > 1u) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (seg_off[mid] <= i) lo = mid;
      else hi = mid;
    }
    ranks[i] = seg_rank[lo];
  }
}

// flags of the sorted pair i: kept (not a repeat of pair i - 1), head (first pair of its key)
__device__ __forceinline__ void pair_flags(const uint64_t* keys, const uint32_t* ranks, uint64_t i, uint64_t n, uint32_t& keep, uint32_t& head)
{
  keep = head = 0;
  if (i >= n) return;
  if (i == 0) {
    keep = head = 1;
    return;
  }
  const bool same_key = keys[i] == keys[i - 1];
  head = !same_key;
  keep = !same_key || ranks[i] != ranks[i - 1];
}

__global__ __launch_bounds__(256) void kr_keys_flag_bsum_kernel(const uint64_t* keys, const uint32_t* ranks, uint64_t n, uint64_t* bsum_keep, uint64_t* bsum_head)
{
  for (uint64_t b = blockIdx.x; b * kScanBlock < n; b += gridDim.x) {
    uint64_t ck = 0, ch = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      uint32_t keep, head;
      pair_flags(keys, ranks, b * kScanBlock + 4u * threadIdx.x + q, n, keep, head);
      ck += keep, ch += head;
    }
    const uint64_t tk = block_sum<uint64_t>(ck), th = block_sum<uint64_t>(ch);
    if (threadIdx.x == 0) bsum_keep[b] = tk, bsum_head[b] = th;
  }
}

// bsum_*: scanned.  keys_out / goff have room for the heads, ranks_out for the kept pairs, inc for nrows (rows were checked).
__global__ __launch_bounds__(256) void kr_keys_group_kernel(const uint64_t* keys, const uint32_t* ranks, uint64_t n, const uint64_t* bsum_keep,
                                                            const uint64_t* bsum_head, uint64_t* keys_out, uint64_t* goff, uint32_t* ranks_out,
                                                            unsigned long long* inc, uint32_t nrows)
{
  for (uint64_t b = blockIdx.x; b * kScanBlock < n; b += gridDim.x) {
    const uint64_t i0 = b * kScanBlock + 4u * threadIdx.x;
    uint32_t k0, k1, k2, k3, h0, h1, h2, h3;
    pair_flags(keys, ranks, i0, n, k0, h0);
    pair_flags(keys, ranks, i0 + 1, n, k1, h1);
    pair_flags(keys, ranks, i0 + 2, n, k2, h2);
    pair_flags(keys, ranks, i0 + 3, n, k3, h3);
    uint64_t pk = bsum_keep[b] + block_scan_excl<uint64_t>((uint64_t)(k0 + k1 + k2 + k3));
    uint64_t ph = bsum_head[b] + block_scan_excl<uint64_t>((uint64_t)(h0 + h1 + h2 + h3));
    auto put = [&](uint64_t i, uint32_t keep, uint32_t head) {
      if (keep) ranks_out[pk] = ranks[i];
      if (head) {
        const uint64_t key = keys[i];
        keys_out[ph] = key, goff[ph] = pk;
        if ((uint32_t)(key >> 32) < nrows) atomicAdd(&inc[key >> 32], 1ull);
      }
      pk += keep, ph += head;
    };
    put(i0, k0, h0);
    put(i0 + 1, k1, h1);
    put(i0 + 2, k2, h2);
    put(i0 + 3, k3, h3);
  }
}

// ---- colour classes ----
constexpr uint32_t kLaneCompare = 64; // a group of up to this many ranks is compared by one lane, a longer one by the wave

__device__ __forceinline__ uint64_t mix64(uint64_t v)
{ // kr::fmix64
  v ^= v >> 33;
  v *= 0xff51afd7ed558ccdull;
  v ^= v >> 33;
  v *= 0xc4ceb9fe1a85ec53ull;
  v ^= v >> 33;
  return v;
}

// term[0 .. npairs]: the rank's term, and 0 behind the last, so that the exclusive scan has the sum of all at [npairs]
__global__ __launch_bounds__(256) void kr_classes_term_kernel(const uint32_t* ranks, uint64_t npairs, uint64_t* term)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= npairs; i += (uint64_t)gridDim.x * 256u)
    term[i] = i < npairs ? mix64((uint64_t)ranks[i] + 1u) : 0;
}

__global__ __launch_bounds__(256) void kr_classes_flag_kernel(const uint64_t* goff, uint64_t nkeys, uint64_t* flag)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nkeys; i += (uint64_t)gridDim.x * 256u) flag[i] = goff[i + 1] - goff[i] >= 2u;
}

// sums: the scanned terms, pos: the scanned flags, m: their total (the list's length)
__global__ __launch_bounds__(256) void kr_classes_list_kernel(const uint64_t* goff, uint64_t nkeys, const uint64_t* sums, const uint64_t* pos, uint64_t m,
                                                              uint64_t mask, uint64_t* fp, uint32_t* gi)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nkeys; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t a = goff[i], b = goff[i + 1];
    if (b - a < 2u) continue;
    const uint64_t p = pos[i];
    if (p < m) fp[p] = (sums[b] - sums[a] + mix64(b - a)) & mask, gi[p] = (uint32_t)i;
  }
}

// fp / gi: the sorted list.  head[j] = 1 where entry j opens a class, is_rep[group] = 1 for its group (zeroed by the caller);
// *raised counts the heads whose fingerprint equals the predecessor's.  A wave takes 64 entries at a time.
__global__ __launch_bounds__(256) void kr_classes_head_kernel(const uint64_t* fp, const uint32_t* gi, uint64_t m, const uint64_t* goff, const uint32_t* ranks,
                                                              uint64_t* head, uint64_t* is_rep, unsigned long long* raised)
{
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; w0 < m; w0 += (uint64_t)gridDim.x * 256u) { // (wave-uniform)
    const uint64_t j = w0 + lane;
    uint32_t h = 0, same_fp = 0; // h: 0 a member, 1 a head, 2 left to the wave
    uint64_t a = 0, b = 0, len = 0;
    if (j < m) {
      h = 1;
      if (j > 0 && fp[j] == fp[j - 1]) {
        same_fp = 1;
        const uint32_t g = gi[j], pg = gi[j - 1];
        a = goff[g], len = goff[g + 1] - a, b = goff[pg];
        if (goff[pg + 1] - b == len) {
          if (len <= kLaneCompare) {
            h = 0;
            for (uint64_t q = 0; q < len; ++q)
              if (ranks[a + q] != ranks[b + q]) {
                h = 1;
                break;
              }
          } else {
            h = 2;
          }
        }
      }
    }
    for (uint64_t todo = __ballot(h == 2u); todo; todo &= todo - 1) { // the long candidates of these 64, each by all lanes
      const int src = __ffsll((unsigned long long)todo) - 1;
      const uint64_t sa = __shfl(a, src), sb = __shfl(b, src), sl = __shfl(len, src);
      uint32_t differs = 0;
      for (uint64_t q0 = 0; q0 < sl; q0 += 64u) {
        const uint64_t q = q0 + lane;
        const bool d = q < sl && ranks[sa + q] != ranks[sb + q];
        if (__ballot(d)) {
          differs = 1;
          break;
        }
      }
      if (lane == (uint32_t)src) h = differs;
    }
    if (j < m) {
      head[j] = h;
      if (h) is_rep[gi[j]] = 1;
    }
    const uint64_t r = __ballot(h && same_fp);
    if (lane == 0 && r) atomicAdd(raised, (unsigned long long)__popcll(r));
  }
}

// run: the head flags scanned inclusively (entry j belongs to run run[j] - 1), cls: the is_rep flags scanned exclusively (a leading
// group's class).  lead has room for the runs, rep for the classes: there are as many of either as heads.
__global__ __launch_bounds__(256) void kr_classes_rep_kernel(const uint64_t* run, const uint32_t* gi, uint64_t m, const uint64_t* cls, uint32_t* lead,
                                                             uint64_t* rep)
{
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < m; j += (uint64_t)gridDim.x * 256u) {
    const uint64_t r = run[j];
    if (j > 0 && run[j - 1] == r) continue;
    const uint32_t g = gi[j];
    if (r - 1 < m) lead[r - 1] = g;
    if (cls[g] < m) rep[cls[g]] = g;
  }
}
__global__ __launch_bounds__(256) void kr_classes_member_kernel(const uint64_t* run, const uint32_t* gi, uint64_t m, const uint64_t* cls, uint64_t nkeys,
                                                                const uint32_t* lead, uint32_t* class_of)
{
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < m; j += (uint64_t)gridDim.x * 256u) {
    const uint64_t r = run[j];
    if (r - 1 >= m) continue;
    const uint32_t g = lead[r - 1];
    if (g < nkeys) class_of[gi[j]] = (uint32_t)cls[g];
  }
}

#define HIP_TRY(expr)                                                                                \
  do {                                                                                                  \
    hipError_t e__ = (expr);                                                                            \
    if (e__ != hipSuccess)                                                                              \
      return kr::fail(e__ == hipErrorOutOfMemory ? KR_ERR_NOMEM : KR_ERR_NO_DEVICE,                      \
                      std::string(#expr) + ": " + hipGetErrorString(e__));                              \
  } while (0)

// kr_debug_build_keys: {pairs in, pairs out, keys out, passes, pool growths, path, kTile, 0}
std::atomic<uint64_t> g_stat[8];
void note(uint64_t in, uint64_t pairs, uint64_t keys, uint64_t passes, uint64_t growths, uint64_t path)
{
  const uint64_t v[8] = {in, pairs, keys, passes, growths, path, kTile, 0};
  for (int q = 0; q < 8; ++q) g_stat[q].store(v[q]);
}

int set_device(int device, const char* who)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return kr::fail(KR_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return kr::fail(KR_ERR_ARG, std::string(who) + ": bad device ordinal");
  HIP_TRY(hipSetDevice(device));
  return KR_OK;
}

// The digits that can differ, least significant first: the rank's, then the key's
std::vector<Pass> digit_passes(uint32_t nrows, uint32_t nleaves)
{
  std::vector<Pass> p;
  for (uint32_t s = 0; s < ceil_log2(nleaves); s += 8) p.push_back(Pass{1u, s});
  for (uint32_t s = 0; s < 32u + ceil_log2(nrows); s += 8) p.push_back(Pass{0u, s});
  return p;
}


// Device bytes of the stage for n pairs: the two sort buffers (24 B a pair), the digit counts, the block sums, goff and inc
uint64_t stage_bytes(uint64_t n, uint32_t nrows)
{
  const uint64_t ntiles = (n + kTile - 1) / kTile;
  const uint64_t nblk = std::max(std::max(scan_blocks(256 * ntiles), scan_blocks(n)), scan_blocks(nrows));
  return 24 * n + 8 * 256 * ntiles + 2 * 8 * nblk + 8 * (n + 1) + 8 * (uint64_t)nrows + 4096;
}
// Does the stage fit?  `held`: bytes of it the caller has on the device already.  KR_BUILD_KEYS_MAX_MB caps the whole stage.
bool stage_fits(uint64_t n, uint32_t nrows, uint64_t held)
{
  const uint64_t need = stage_bytes(n, nrows);
  if (const char* e = getenv("KR_BUILD_KEYS_MAX_MB"))
    if (need > (uint64_t)strtoull(e, nullptr, 10) << 20) return false;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
  const uint64_t margin = 64ull << 20;
  return need - std::min(need, held) + margin <= (uint64_t)fr;
}

// ---- colour classes ----
// KR_BUILD_COLOUR_HASH_BITS: the low bits of a fingerprint that are kept (tests of the content compare)
uint32_t colour_hash_bits()
{
  const char* e = getenv("KR_BUILD_COLOUR_HASH_BITS");
  return e ? (uint32_t)std::min<unsigned long long>(strtoull(e, nullptr, 10), 64) : 64u;
}
// the list can have no more entries than there are groups, or pairs of ranks
uint64_t classes_list_max(uint64_t nkeys, uint64_t npairs) { return std::min(nkeys, npairs / 2); }
uint64_t classes_block_sums(uint64_t nkeys, uint64_t npairs)
{
  const uint64_t ntiles = (classes_list_max(nkeys, npairs) + kTile - 1) / kTile;
  return std::max(std::max(scan_blocks(npairs + 1), scan_blocks(nkeys)), scan_blocks(256 * ntiles));
}
// Device bytes of the class stage: terms, flags, class_of, the list twice over (12 B an entry), digit counts, block sums
uint64_t classes_bytes(uint64_t nkeys, uint64_t npairs)
{
  const uint64_t mmax = classes_list_max(nkeys, npairs), ntiles = (mmax + kTile - 1) / kTile;
  return 8 * (npairs + 1) + 8 * nkeys + 4 * nkeys + 24 * mmax + 8 * 256 * ntiles + 8 * classes_block_sums(nkeys, npairs) + 4096;
}
bool classes_fit(uint64_t nkeys, uint64_t npairs)
{
  const uint64_t need = classes_bytes(nkeys, npairs);
  if (const char* e = getenv("KR_BUILD_KEYS_MAX_MB"))
    if (need > (uint64_t)strtoull(e, nullptr, 10) << 20) return false;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
  return need + (64ull << 20) <= (uint64_t)fr;
}

// The classes of nkeys > 0 groups that are on the device in effect (d_goff[nkeys + 1], d_ranks[npairs]).  Every buffer is had before
// the first kernel runs.  KR_ERR_NOMEM: the stage is not for the device (no room, or group indices that do not fit the sort's rank
// slot); `out` holds nothing, and the caller takes the classes from the host.
int classes_on_device(const uint64_t* d_goff, const uint32_t* d_ranks, uint64_t nkeys, uint64_t npairs, kr_colour_classes* out)
{
  memset(out, 0, sizeof(*out));
  if (nkeys >= KR_NO_CLASS) return kr::fail(KR_ERR_NOMEM, "colour classes: 2^32 - 1 groups or more");
  const uint64_t mmax = classes_list_max(nkeys, npairs);
  if (mmax == 0) { // fewer than two ranks in all
    int rc = kr::colour_classes_alloc(out, nkeys, 0);
    if (rc == KR_OK) kr::colour_stats_note(nkeys, 0, 0, 0, 1, 0);
    return rc;
  }
  const uint64_t nblk = classes_block_sums(nkeys, npairs);
  DevBuf<uint64_t> b_term, b_flag, b_fa, b_fb, b_counts, b_bsum, b_small; // (freed at every return)
  DevBuf<uint32_t> b_ga, b_gb, b_class;
  if (!b_term.reserve(npairs + 1) || !b_flag.reserve(nkeys) || !b_fa.reserve(mmax) || !b_fb.reserve(mmax) || !b_ga.reserve(mmax) || !b_gb.reserve(mmax) ||
      !b_counts.reserve(256 * ((mmax + kTile - 1) / kTile)) || !b_bsum.reserve(nblk) || !b_small.reserve(4) || !b_class.reserve(nkeys)) {
    (void)hipGetLastError();
    return kr::fail(KR_ERR_NOMEM, "colour classes: out of device memory");
  }
  uint64_t* d_total = b_small.get(); // [0]: list entries, then classes; [1]: the other scans' totals; [2]: raised by the content compare
  HIP_TRY(hipMemset(d_total, 0, 32));
  HIP_TRY(hipMemset(b_class.get(), 0xFF, nkeys * 4));
  hipLaunchKernelGGL(kr_classes_term_kernel, dim3(grid_for((npairs + 256) / 256)), dim3(256), 0, 0, d_ranks, npairs, b_term.get());
  scan_u64<false>(b_term.get(), npairs + 1, b_bsum.get(), d_total + 1);
  hipLaunchKernelGGL(kr_classes_flag_kernel, dim3(grid_for((nkeys + 255) / 256)), dim3(256), 0, 0, d_goff, nkeys, b_flag.get());
  scan_u64<false>(b_flag.get(), nkeys, b_bsum.get(), d_total);
  HIP_TRY(hipGetLastError());
  uint64_t m = 0;
  HIP_TRY(hipMemcpy(&m, d_total, 8, hipMemcpyDeviceToHost)); // (synchronises: null stream)
  if (m > mmax) return kr::fail(KR_ERR_STATE, "colour classes: inconsistent group offsets");
  uint64_t res[3] = {0, 0, 0}; // classes, -, raised
  uint32_t npasses = 0;
  uint64_t* d_rep = b_term.get(); // the sums are done with once the list is made: room for npairs + 1 > m classes
  if (m) {
    const uint32_t bits = colour_hash_bits();
    hipLaunchKernelGGL(kr_classes_list_kernel, dim3(grid_for((nkeys + 255) / 256)), dim3(256), 0, 0, d_goff, nkeys, (const uint64_t*)b_term.get(),
                       (const uint64_t*)b_flag.get(), m, bits >= 64 ? ~0ull : (1ull << bits) - 1ull, b_fa.get(), b_ga.get());
    const uint32_t ntiles = (uint32_t)((m + kTile - 1) / kTile);
    const uint64_t ncounts = 256ull * ntiles;
    uint64_t *fin = b_fa.get(), *fout = b_fb.get();
    uint32_t *gin = b_ga.get(), *gout = b_gb.get();
    for (uint32_t shift = 0; shift < bits; shift += 8, ++npasses) {
      hipLaunchKernelGGL(kr_keys_hist_kernel, dim3(ntiles), dim3(256), 0, 0, fin, gin, m, ntiles, 0u, shift, b_counts.get());
      scan_u64<false>(b_counts.get(), ncounts, b_bsum.get(), d_total + 1);
      hipLaunchKernelGGL(kr_keys_scatter_kernel, dim3(ntiles), dim3(256), 0, 0, fin, gin, fout, gout, m, ntiles, 0u, shift, b_counts.get());
      std::swap(fin, fout), std::swap(gin, gout);
    }
    // fin / gin: sorted.  The other pair of buffers takes the head flags (then the runs) and the runs' leading groups.
    HIP_TRY(hipMemset(b_flag.get(), 0, nkeys * 8));
    hipLaunchKernelGGL(kr_classes_head_kernel, dim3(grid_for((m + 255) / 256)), dim3(256), 0, 0, fin, gin, m, d_goff, d_ranks, fout, b_flag.get(),
                       (unsigned long long*)(d_total + 2));
    scan_u64<true>(fout, m, b_bsum.get(), d_total + 1);
    scan_u64<false>(b_flag.get(), nkeys, b_bsum.get(), d_total);
    hipLaunchKernelGGL(kr_classes_rep_kernel, dim3(grid_for((m + 255) / 256)), dim3(256), 0, 0, fout, gin, m, (const uint64_t*)b_flag.get(), gout, d_rep);
    hipLaunchKernelGGL(kr_classes_member_kernel, dim3(grid_for((m + 255) / 256)), dim3(256), 0, 0, fout, gin, m, (const uint64_t*)b_flag.get(), nkeys,
                       (const uint32_t*)gout, b_class.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(res, d_total, 24, hipMemcpyDeviceToHost));
    if (res[0] == 0 || res[0] > m) return kr::fail(KR_ERR_STATE, "colour classes: inconsistent class counts");
  }
  int rc = kr::colour_classes_alloc(out, nkeys, res[0]);
  if (rc) return rc;
  hipError_t e = hipMemcpy(out->class_of, b_class.get(), nkeys * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && res[0]) e = hipMemcpy(out->rep, d_rep, res[0] * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    kr_colour_classes_free(out);
    return kr::fail(KR_ERR_NO_DEVICE, std::string("colour classes: ") + hipGetErrorString(e));
  }
  out->nclasses = res[0];
  kr::colour_stats_note(nkeys, m, res[0], res[2], 1, npasses);
  return KR_OK;
}

// The stage on n > 0 pairs that are on the device: ka / ra are sorted between themselves and two buffers made here.  Every buffer
// is had before the first kernel runs: KR_ERR_NOMEM means that ka / ra are as they were (the callers finish on the host then).
// cls: the groups' colour classes too, while the groups are here (left empty where the device has no room for that stage).
int run_stage(uint64_t* ka, uint32_t* ra, uint64_t n, uint32_t nrows, uint32_t nleaves, kr_key_groups* out, uint64_t* npasses,
              kr_colour_classes* cls = nullptr, double* cls_seconds = nullptr)
{
  const uint64_t ntiles64 = (n + kTile - 1) / kTile;
  if (ntiles64 >= (1ull << 31)) return kr::fail(KR_ERR_ARG, "key stage: too many pairs for one sort");
  const uint32_t ntiles = (uint32_t)ntiles64;
  const uint64_t ncounts = 256ull * ntiles;
  const uint64_t nblk = std::max(std::max(scan_blocks(ncounts), scan_blocks(n)), scan_blocks(nrows));
  DevBuf<uint64_t> b_kb, b_counts, b_bsum, b_bsum2, b_small, b_goff, b_inc; // (freed at every return)
  DevBuf<uint32_t> b_rb;
  if (!b_kb.reserve(n) || !b_rb.reserve(n) || !b_counts.reserve(ncounts) || !b_bsum.reserve(nblk) || !b_bsum2.reserve(nblk) || !b_small.reserve(4) ||
      !b_goff.reserve(n + 1) || !b_inc.reserve(nrows)) {
    (void)hipGetLastError();
    return kr::fail(KR_ERR_NOMEM, "key stage: out of device memory");
  }
  uint64_t* d_total = b_small.get();       // [0], [1]: totals of the scans
  uint32_t* d_bad = (uint32_t*)(d_total + 2);
  HIP_TRY(hipMemset(d_total, 0, 32));
  hipLaunchKernelGGL(kr_keys_check_kernel, dim3(grid_for((n + 255) / 256)), dim3(256), 0, 0, ka, ra, n, nrows, nleaves, d_bad);
  HIP_TRY(hipGetLastError());
  uint32_t bad = 0;
  HIP_TRY(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost)); // (synchronises with the kernel: null stream)
  if (bad & 1u) return kr::fail(KR_ERR_FORMAT, "row out of range");
  if (bad & 2u) return kr::fail(KR_ERR_ARG, "key stage: leaf rank out of range");

  uint64_t *kin = ka, *kout = b_kb.get();
  uint32_t *rin = ra, *rout = b_rb.get();
  const std::vector<Pass> passes = digit_passes(nrows, nleaves);
  for (const Pass& p : passes) {
    hipLaunchKernelGGL(kr_keys_hist_kernel, dim3(ntiles), dim3(256), 0, 0, kin, rin, n, ntiles, p.from_rank, p.shift, b_counts.get());
    scan_u64<false>(b_counts.get(), ncounts, b_bsum.get(), d_total);
    hipLaunchKernelGGL(kr_keys_scatter_kernel, dim3(ntiles), dim3(256), 0, 0, kin, rin, kout, rout, n, ntiles, p.from_rank, p.shift, b_counts.get());
    std::swap(kin, kout), std::swap(rin, rout);
  }
  *npasses = passes.size();
  // kin / rin: sorted.  The other pair of buffers takes the distinct keys and the kept ranks.
  const uint64_t nfb = scan_blocks(n);
  hipLaunchKernelGGL(kr_keys_flag_bsum_kernel, dim3(grid_for(nfb)), dim3(256), 0, 0, kin, rin, n, b_bsum.get(), b_bsum2.get());
  hipLaunchKernelGGL(kr_keys_bscan_kernel, dim3(1), dim3(1024), 0, 0, b_bsum.get(), (uint32_t)nfb, d_total);
  hipLaunchKernelGGL(kr_keys_bscan_kernel, dim3(1), dim3(1024), 0, 0, b_bsum2.get(), (uint32_t)nfb, d_total + 1);
  HIP_TRY(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  HIP_TRY(hipMemcpy(tot, d_total, 16, hipMemcpyDeviceToHost));
  const uint64_t npairs = tot[0], nkeys = tot[1];
  if (npairs > n || nkeys > npairs || nkeys == 0) return kr::fail(KR_ERR_STATE, "key stage: inconsistent group counts");
  HIP_TRY(hipMemset(b_inc.get(), 0, (uint64_t)nrows * 8));
  HIP_TRY(hipMemcpy(b_goff.get() + nkeys, &npairs, 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kr_keys_group_kernel, dim3(grid_for(nfb)), dim3(256), 0, 0, kin, rin, n, b_bsum.get(), b_bsum2.get(), kout, b_goff.get(), rout,
                     (unsigned long long*)b_inc.get(), nrows);
  scan_u64<true>(b_inc.get(), nrows, b_bsum.get(), d_total);
  HIP_TRY(hipGetLastError());
  int rc = kr::key_groups_alloc(out, nkeys, npairs, nrows);
  if (rc) return rc;
  hipError_t e = hipMemcpy(out->keys, kout, nkeys * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out->goff, b_goff.get(), (nkeys + 1) * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out->ranks, rout, npairs * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out->inc, b_inc.get(), (uint64_t)nrows * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    kr_key_groups_free(out);
    return kr::fail(KR_ERR_NO_DEVICE, std::string("key stage: ") + hipGetErrorString(e));
  }
  if (cls) { // on the groups where the group kernel left them
    const auto t0 = std::chrono::steady_clock::now();
    rc = classes_fit(nkeys, npairs) ? classes_on_device(b_goff.get(), rout, nkeys, npairs, cls) : KR_ERR_NOMEM;
    if (rc == KR_ERR_NOMEM) {
      kr::clear_error(); // the caller has the groups and takes their classes from the host
    } else if (rc) {
      kr_key_groups_free(out);
      return rc;
    } else if (cls_seconds) {
      *cls_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  return KR_OK;
}

} // namespace

// ---------------------------------------------------------------------------
// The builder's pool
// ---------------------------------------------------------------------------
struct kr::KeyPool {
  int device = 0;
  DevBuf<uint64_t> keys; // capacity keys.size(), `used` of it filled
  uint64_t used = 0, growths = 0;
  struct Seg {
    uint64_t off, count;
    uint32_t rank;
  };
  std::vector<Seg> segs;
  bool on_host = false;           // the device had no room to grow: everything is in `spill` from then on
  std::vector<kr::KeyRank> spill;
};

namespace {
uint64_t pool_start_pairs()
{
  const char* e = getenv("KR_BUILD_POOL_PAIRS");
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? v : 64ull << 20;
}
// the pool's pairs as host (key, rank) records behind what `spill` holds; the device block is given back
int pool_to_host(kr::KeyPool* p)
{
  std::vector<uint64_t> tmp(p->used);
  if (p->used) HIP_TRY(hipMemcpy(tmp.data(), p->keys.get(), p->used * 8, hipMemcpyDeviceToHost));
  p->keys.reset();
  p->spill.reserve(p->spill.size() + p->used);
  for (const auto& s : p->segs)
    for (uint64_t q = 0; q < s.count; ++q) p->spill.push_back(kr::KeyRank{tmp[s.off + q], s.rank});
  p->segs.clear();
  p->used = 0, p->on_host = true;
  return KR_OK;
}
// room for n more pairs: doubling, with a device-to-device copy; false: no room to be had (the pool is as it was)
bool pool_room(kr::KeyPool* p, uint64_t n)
{
  if (p->used + n <= p->keys.size()) return true;
  uint64_t cap = std::max<uint64_t>(p->keys.size(), 1);
  const bool first = p->keys.size() == 0;
  if (first) cap = pool_start_pairs();
  while (cap < p->used + n) cap *= 2;
  DevBuf<uint64_t> bigger;
  if (!bigger.reserve(cap)) {
    (void)hipGetLastError();
    return false;
  }
  if (p->used && hipMemcpy(bigger.get(), p->keys.get(), p->used * 8, hipMemcpyDeviceToDevice) != hipSuccess) return false;
  p->keys = std::move(bigger);
  if (!first) p->growths++;
  return true;
}
int pool_append(kr::KeyPool* p, const uint64_t* src, uint64_t n, uint32_t rank, bool src_on_device)
{
  if (!p) return kr::fail(KR_ERR_ARG, "key pool: null");
  if (n == 0) return KR_OK;
  if (!p->on_host && !pool_room(p, n)) {
    if (int rc = pool_to_host(p)) return rc;
  }
  if (p->on_host) {
    std::vector<uint64_t> tmp;
    if (src_on_device) {
      tmp.resize(n);
      HIP_TRY(hipMemcpy(tmp.data(), src, n * 8, hipMemcpyDeviceToHost));
      src = tmp.data();
    }
    for (uint64_t q = 0; q < n; ++q) p->spill.push_back(kr::KeyRank{src[q], rank});
    return KR_OK;
  }
  HIP_TRY(hipMemcpy(p->keys.get() + p->used, src, n * 8, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  p->segs.push_back(kr::KeyPool::Seg{p->used, n, rank});
  p->used += n;
  return KR_OK;
}
} // namespace

int kr::key_pool_create(int device, KeyPool** out)
{
  if (int rc = set_device(device, "key pool")) return rc;
  *out = new KeyPool();
  (*out)->device = device;
  return KR_OK;
}
void kr::key_pool_free(KeyPool* p)
{
  if (!p) return;
  if (p->keys.get()) (void)hipSetDevice(p->device);
  delete p;
}
int kr::key_pool_append_device(KeyPool* p, const uint64_t* d_keys, uint64_t n, uint32_t rank) { return pool_append(p, d_keys, n, rank, true); }
int kr::key_pool_append_host(KeyPool* p, const uint64_t* keys, uint64_t n, uint32_t rank) { return pool_append(p, keys, n, rank, false); }
void kr::key_stage_note_path(uint64_t path) { note(0, 0, 0, 0, 0, path); }

namespace {
// the pool's segments expanded into a rank array, and the stage on both, in place
int pool_on_device(kr::KeyPool* p, uint32_t nrows, uint32_t nleaves, kr_key_groups* out, uint64_t* npasses, kr_colour_classes* cls, double* cls_seconds)
{
  const uint64_t n = p->used;
  const uint32_t nseg = (uint32_t)p->segs.size();
  std::vector<uint64_t> seg_off(nseg + 1);
  std::vector<uint32_t> seg_rank(nseg);
  for (uint32_t q = 0; q < nseg; ++q) seg_off[q] = p->segs[q].off, seg_rank[q] = p->segs[q].rank;
  seg_off[nseg] = n;
  DevBuf<uint64_t> b_off;
  DevBuf<uint32_t> b_rank, b_ra;
  if (!b_off.reserve(nseg + 1) || !b_rank.reserve(nseg) || !b_ra.reserve(n)) {
    (void)hipGetLastError();
    return kr::fail(KR_ERR_NOMEM, "key pool: out of device memory");
  }
  HIP_TRY(hipMemcpy(b_off.get(), seg_off.data(), (nseg + 1) * 8ull, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_rank.get(), seg_rank.data(), nseg * 4ull, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kr_keys_expand_kernel, dim3(grid_for((n + 255) / 256)), dim3(256), 0, 0, (const uint64_t*)b_off.get(), (const uint32_t*)b_rank.get(), nseg, n,
                     b_ra.get());
  HIP_TRY(hipGetLastError());
  return run_stage(p->keys.get(), b_ra.get(), n, nrows, nleaves, out, npasses, cls, cls_seconds);
}
} // namespace

int kr::key_pool_finish(KeyPool* p, uint32_t nrows, uint32_t nleaves, kr_key_groups* out, kr_colour_classes* cls, double* cls_seconds)
{
  if (!p || !out) return kr::fail(KR_ERR_ARG, "key pool: null");
  if (cls) memset(cls, 0, sizeof(*cls));
  if (cls_seconds) *cls_seconds = 0;
  if (int rc = set_device(p->device, "key pool")) return rc;
  const uint64_t n = p->on_host ? p->spill.size() : p->used;
  if (!p->on_host && n) {
    uint64_t npasses = 0;
    int rc = stage_fits(n, nrows, n * 8) ? pool_on_device(p, nrows, nleaves, out, &npasses, cls, cls_seconds) : KR_ERR_NOMEM;
    if (rc != KR_ERR_NOMEM) {
      if (rc == KR_OK) note(n, out->npairs, out->nkeys, npasses, p->growths, 1);
      p->keys.reset();
      p->used = 0, p->segs.clear();
      return rc;
    }
    kr::clear_error(); // no room on the device: the pool is as it was, and the host can finish
    if ((rc = pool_to_host(p))) return rc;
  }
  int rc = kr::key_groups_host(p->spill, nrows, nleaves, out);
  if (rc == KR_OK) note(n, out->npairs, out->nkeys, 0, p->growths, n ? 2 : 1);
  return rc;
}

extern "C" int kr_key_groups_device(int device, const uint64_t* keys, const uint32_t* ranks, uint64_t n, uint32_t nrows, uint32_t nleaves, kr_key_groups* out)
{
  kr::clear_error();
  if (!out || (n && (!keys || !ranks))) return kr::fail(KR_ERR_ARG, "kr_key_groups_device: null argument");
  memset(out, 0, sizeof(*out));
  if (nleaves > 65536u) return kr::fail(KR_ERR_ARG, "kr_key_groups_device: more than 65536 leaves");
  if (int rc = set_device(device, "kr_key_groups_device")) return rc;
  if (n == 0) {
    int rc = kr::key_groups_alloc(out, 0, 0, nrows);
    if (rc == KR_OK) note(0, 0, 0, 0, 0, 1);
    return rc;
  }
  int rc = KR_ERR_NOMEM;
  if (stage_fits(n, nrows, 0)) {
    DevBuf<uint64_t> b_ka; // (freed where the block is left)
    DevBuf<uint32_t> b_ra;
    uint64_t npasses = 0;
    if (b_ka.reserve(n) && b_ra.reserve(n)) {
      HIP_TRY(hipMemcpy(b_ka.get(), keys, n * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(b_ra.get(), ranks, n * 4, hipMemcpyHostToDevice));
      rc = run_stage(b_ka.get(), b_ra.get(), n, nrows, nleaves, out, &npasses);
    } else {
      (void)hipGetLastError();
    }
    if (rc == KR_OK) note(n, out->npairs, out->nkeys, npasses, 0, 1);
  }
  if (rc != KR_ERR_NOMEM) return rc;
  kr::clear_error(); // no room on the device: the twin, with the same result
  rc = kr_key_groups_cpu(keys, ranks, n, nrows, nleaves, out);
  if (rc == KR_OK) note(n, out->npairs, out->nkeys, 0, 0, 2);
  return rc;
}

extern "C" int kr_colour_classes_device(int device, const uint64_t* goff, const uint32_t* ranks, uint64_t nkeys, kr_colour_classes* out)
{
  kr::clear_error();
  if (!out || !goff) return kr::fail(KR_ERR_ARG, "kr_colour_classes_device: null argument");
  memset(out, 0, sizeof(*out));
  if (goff[0] != 0 || !std::is_sorted(goff, goff + nkeys + 1)) return kr::fail(KR_ERR_ARG, "kr_colour_classes_device: goff must ascend from 0");
  const uint64_t npairs = goff[nkeys];
  if (npairs && !ranks) return kr::fail(KR_ERR_ARG, "kr_colour_classes_device: null argument");
  if (int rc = set_device(device, "kr_colour_classes_device")) return rc;
  if (nkeys == 0) {
    int rc = kr::colour_classes_alloc(out, 0, 0);
    if (rc == KR_OK) kr::colour_stats_note(0, 0, 0, 0, 1, 0);
    return rc;
  }
  int rc = KR_ERR_NOMEM;
  if (classes_fit(nkeys, npairs)) {
    DevBuf<uint64_t> b_goff; // (freed where the block is left)
    DevBuf<uint32_t> b_ranks;
    if (b_goff.reserve(nkeys + 1) && b_ranks.reserve(std::max<uint64_t>(npairs, 1))) {
      HIP_TRY(hipMemcpy(b_goff.get(), goff, (nkeys + 1) * 8, hipMemcpyHostToDevice));
      if (npairs) HIP_TRY(hipMemcpy(b_ranks.get(), ranks, npairs * 4, hipMemcpyHostToDevice));
      rc = classes_on_device(b_goff.get(), b_ranks.get(), nkeys, npairs, out);
    } else {
      (void)hipGetLastError();
    }
  }
  if (rc != KR_ERR_NOMEM) return rc;
  kr::clear_error(); // not for the device: the canonical classes from the host
  rc = kr::colour_classes_host(goff, ranks, nkeys, out);
  if (rc == KR_OK) {
    uint64_t multi = 0;
    for (uint64_t i = 0; i < nkeys; ++i) multi += out->class_of[i] != KR_NO_CLASS;
    kr::colour_stats_note(nkeys, multi, out->nclasses, 0, 2, 0);
  }
  return rc;
}

extern "C" void kr_debug_build_keys(uint64_t out[8])
{
  if (!out) return;
  for (int q = 0; q < 8; ++q) out[q] = g_stat[q].load();
  out[6] = kTile; // (also before the first call)
}
