// kr_index_stats.hip — the statistics of `krepp inspect` on gfx950 (kr_index_stats_device; the canonical form is kr_index_stats_cpu,
// kr_inspect.cpp, and both return the same arrays).  Per library:
//   kr_stats_count_kernel    k-mers per colour: one increment per cmer entry, the hot pass.  A workgroup walks a contiguous run of
//                            kRun entries (8 bytes each: uint2 loads, uint4 loads of two entries where the run starts on 16 bytes).
//                            Colour ids below the LDS cap -- the tree's nodes have the lowest ids and carry most k-mers -- are
//                            counted in 32-bit LDS counters, which a run of kRun entries cannot wrap, and flushed at the end with one
//                            64-bit global atomic per non-zero counter.  Ids at or above the cap are millions with few collisions:
//                            64-bit global atomics straight away.  An id >= nsubsets is not counted: the smallest such entry index
//                            is kept by an atomic min.
//   kr_stats_outdeg_kernel   se_to_pse[1 .. nsubsets): two guarded 64-bit atomics per entry (small; not privatised)
//   value histograms         of count[1 ..] and outdeg[1 ..]: maximum -> the digits that can differ -> key-only passes of the radix
//                            sort of kr_dev_sort.inc -> head flags -> their scan (kr_dev_prefix.inc) -> (value, start) per head ->
//                            run lengths.  Only the compact lists come back; the full arrays with KR_STATS_KEEP_COUNTS.
// From a host view cmer crosses PCIe in chunks through two page-locked buffers and two device buffers: the copy of chunk i + 1 runs
// on a stream of its own beside the count kernel of chunk i (both streams are made for the call; neither is the null stream, which
// does not synchronise with them, so the call waits for them before the null-stream stages).  With KR_VIEW_DEVICE cmer is read in
// place, chunk by chunk too.  When the counters, sort buffers and staging do not fit, the call finishes through kr_index_stats_cpu.
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

#include "kr_dev_prefix.inc"
#include "kr_dev_sort.inc"

constexpr uint32_t kLdsColours = 8192; // 32 KiB of 32-bit counters a workgroup: four such workgroups fit the 160 KiB of a CU
constexpr uint32_t kRun = 65536;       // cmer entries a workgroup counts before it flushes (256 per thread)
constexpr uint32_t kSlack = 64;        // counter entries behind nsubsets that nothing may ever touch
static_assert((uint64_t)kRun < (1ull << 32), "a 32-bit LDS counter must hold a whole run");
static_assert(kRun % 512u == 0, "a run is whole rounds of 256 threads x 2 entries");
static_assert(kLdsColours * 4u * 2u <= 160u * 1024u, "two workgroups or more a CU");

// One entry's increment.  idx: the entry's index in the whole table (for the error report).
__device__ __forceinline__ void count_one(uint32_t se, uint64_t idx, uint32_t nsubsets, uint32_t cap, uint32_t* s_cnt, unsigned long long* se_count,
                                          unsigned long long* bad_min, uint32_t& nl, uint32_t& ng)
{
  if (se >= nsubsets) {
    atomicMin(bad_min, (unsigned long long)idx);
  } else if (se < cap) {
    atomicAdd(&s_cnt[se], 1u);
    ++nl;
  } else {
    atomicAdd(&se_count[se], 1ull);
    ++ng;
  }
}

// cmer: n interleaved (enc, se) entries, entry 0 of which is entry `base` of the table.  cap <= kLdsColours.  route[0] / [1]:
// increments served from LDS / sent as global atomics.  se_count has nsubsets (+ slack) entries; only ids < nsubsets are touched.
__global__ __launch_bounds__(256) void kr_stats_count_kernel(const uint32_t* cmer, uint64_t n, uint64_t base, uint32_t nsubsets, uint32_t cap,
                                                             unsigned long long* se_count, unsigned long long* bad_min, unsigned long long* route)
{
  __shared__ uint32_t s_cnt[kLdsColours];
  const uint32_t tid = threadIdx.x;
  for (uint32_t c = tid; c < kLdsColours; c += 256u) s_cnt[c] = 0;
  __syncthreads();
  const uint64_t r0 = (uint64_t)blockIdx.x * kRun;
  const uint64_t r1 = r0 + kRun < n ? r0 + kRun : n;
  uint32_t nl = 0, ng = 0;
  if (r0 < r1) {
    if ((((uintptr_t)cmer) & 15u) == 0) { // r0 is even: the run starts on 16 bytes, two entries a load
      const uint64_t even_end = r0 + ((r1 - r0) & ~1ull);
      for (uint64_t j = r0 + 2u * tid; j < even_end; j += 2048u) { // four loads in flight a thread, then their eight increments
        const uint64_t j1 = j + 512u, j2 = j + 1024u, j3 = j + 1536u;
        const bool h1 = j1 < even_end, h2 = j2 < even_end, h3 = j3 < even_end;
        const uint4 z = make_uint4(0, 0, 0, 0);
        const uint4 v0 = *reinterpret_cast<const uint4*>(cmer + 2 * j);
        const uint4 v1 = h1 ? *reinterpret_cast<const uint4*>(cmer + 2 * j1) : z;
        const uint4 v2 = h2 ? *reinterpret_cast<const uint4*>(cmer + 2 * j2) : z;
        const uint4 v3 = h3 ? *reinterpret_cast<const uint4*>(cmer + 2 * j3) : z;
        count_one(v0.y, base + j, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
        count_one(v0.w, base + j + 1, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
        if (h1) {
          count_one(v1.y, base + j1, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
          count_one(v1.w, base + j1 + 1, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
        }
        if (h2) {
          count_one(v2.y, base + j2, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
          count_one(v2.w, base + j2 + 1, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
        }
        if (h3) {
          count_one(v3.y, base + j3, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
          count_one(v3.w, base + j3 + 1, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
        }
      }
      if (even_end < r1 && tid == 0) { // the odd last entry
        const uint2 v = *reinterpret_cast<const uint2*>(cmer + 2 * even_end);
        count_one(v.y, base + even_end, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
      }
    } else {
      for (uint64_t j = r0 + tid; j < r1; j += 256u) {
        const uint2 v = *reinterpret_cast<const uint2*>(cmer + 2 * j);
        count_one(v.y, base + j, nsubsets, cap, s_cnt, se_count, bad_min, nl, ng);
      }
    }
  }
  __syncthreads();
  for (uint32_t c = tid; c < cap && c < nsubsets; c += 256u) {
    const uint32_t v = s_cnt[c];
    if (v) atomicAdd(&se_count[c], (unsigned long long)v);
  }
  const uint64_t tl = wave_sum((uint64_t)nl), tg = wave_sum((uint64_t)ng);
  if ((tid & 63u) == 0) {
    if (tl) atomicAdd(&route[0], (unsigned long long)tl);
    if (tg) atomicAdd(&route[1], (unsigned long long)tg);
  }
}

// pse: nsubsets (first, second) pairs; entry 0 is not a parent.  A child >= nsubsets is not counted: the smallest such entry by atomic min.
__global__ __launch_bounds__(256) void kr_stats_outdeg_kernel(const uint2* pse, uint32_t nsubsets, unsigned long long* outdeg, unsigned long long* bad_min)
{
  for (uint64_t ix = 1 + (uint64_t)blockIdx.x * 256u + threadIdx.x; ix < nsubsets; ix += (uint64_t)gridDim.x * 256u) {
    const uint2 p = pse[ix];
    if (p.x >= nsubsets || p.y >= nsubsets) {
      atomicMin(bad_min, (unsigned long long)ix);
      continue;
    }
    atomicAdd(&outdeg[p.x], 1ull);
    atomicAdd(&outdeg[p.y], 1ull);
  }
}

// dst[i] = src[i] for i < m, and the maximum of all into *vmax
__global__ __launch_bounds__(256) void kr_stats_copy_max_kernel(const uint64_t* src, uint64_t m, uint64_t* dst, unsigned long long* vmax)
{
  uint64_t mx = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t v = src[i];
    dst[i] = v;
    mx = v > mx ? v : mx;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t o = __shfl_xor(mx, d);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63u) == 0 && mx) atomicMax(vmax, (unsigned long long)mx);
}

// v: sorted.  flag[i] = 1 where v[i] opens a run
__global__ __launch_bounds__(256) void kr_stats_head_kernel(const uint64_t* v, uint64_t m, uint64_t* flag)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256u) flag[i] = i == 0 || v[i] != v[i - 1];
}
// pos: the scanned flags.  A head writes its value and its index; there are at most m heads.
__global__ __launch_bounds__(256) void kr_stats_compact_kernel(const uint64_t* v, uint64_t m, const uint64_t* pos, uint64_t* value, uint64_t* start)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256u) {
    if (i != 0 && v[i] == v[i - 1]) continue;
    const uint64_t p = pos[i];
    if (p < m) value[p] = v[i], start[p] = i;
  }
}
// start[0 .. *nheads): where the runs open; freq[p] = the run's length (the last run ends at m)
__global__ __launch_bounds__(256) void kr_stats_runs_kernel(const uint64_t* start, const uint64_t* nheads, uint64_t m, uint64_t* freq)
{
  const uint64_t nh = *nheads < m ? *nheads : m;
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nh; p += (uint64_t)gridDim.x * 256u)
    freq[p] = (p + 1 < nh ? start[p + 1] : m) - start[p];
}

#define HIP_TRY(expr)                                                                                \
  do {                                                                                                  \
    hipError_t e__ = (expr);                                                                            \
    if (e__ != hipSuccess)                                                                              \
      return kr::fail(e__ == hipErrorOutOfMemory ? KR_ERR_NOMEM : KR_ERR_NO_DEVICE,                      \
                      std::string(#expr) + ": " + hipGetErrorString(e__));                              \
  } while (0)

// kr_debug_index_stats: {path, chunks, LDS increments, global increments, LDS cap, passes (mer), passes (deg), kRun}
std::atomic<uint64_t> g_stat[8];
std::atomic<float> g_ms[4];

uint64_t env_u64(const char* name, uint64_t dflt)
{
  const char* e = getenv(name);
  return e && *e ? strtoull(e, nullptr, 10) : dflt;
}

// The streams, events and staging of one call; everything is given back at every return
struct Staging {
  hipStream_t st_copy = nullptr, st_kern = nullptr;
  hipEvent_t c0[2] = {nullptr, nullptr}, c1[2] = {nullptr, nullptr}, k0[2] = {nullptr, nullptr}, k1[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  PinBuf<uint64_t> pin[2];
  DevBuf<uint64_t> dev[2];
  float copy_ms = 0, kern_ms = 0;
  ~Staging()
  {
    if (st_copy) (void)hipStreamSynchronize(st_copy);
    if (st_kern) (void)hipStreamSynchronize(st_kern);
    for (int s = 0; s < 2; ++s)
      for (hipEvent_t e : {c0[s], c1[s], k0[s], k1[s]})
        if (e) (void)hipEventDestroy(e);
    if (st_copy) (void)hipStreamDestroy(st_copy);
    if (st_kern) (void)hipStreamDestroy(st_kern);
  }
  int open()
  {
    HIP_TRY(hipStreamCreateWithFlags(&st_copy, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&st_kern, hipStreamNonBlocking));
    for (int s = 0; s < 2; ++s) {
      HIP_TRY(hipEventCreate(&c0[s]));
      HIP_TRY(hipEventCreate(&c1[s]));
      HIP_TRY(hipEventCreate(&k0[s]));
      HIP_TRY(hipEventCreate(&k1[s]));
    }
    return KR_OK;
  }
  // waits until slot s's last kernel has run, and takes its times
  int retire(int s)
  {
    if (!used[s]) return KR_OK;
    HIP_TRY(hipEventSynchronize(k1[s]));
    float a = 0, b = 0;
    if (hipEventElapsedTime(&a, c0[s], c1[s]) == hipSuccess) copy_ms += a;
    if (hipEventElapsedTime(&b, k0[s], k1[s]) == hipSuccess) kern_ms += b;
    (void)hipGetLastError();
    used[s] = false;
    return KR_OK;
  }
};

uint32_t count_grid(uint64_t n) { return (uint32_t)((n + kRun - 1) / kRun); }

// Device bytes of one library's call: two counter arrays with slack, the two sort buffers with their rank slots, head flags, starts,
// digit counts and block sums, se_to_pse; `staging`: the two chunk buffers of a host view
uint64_t lib_bytes(uint32_t nsubsets, uint64_t staging, bool pse_on_host)
{
  const uint64_t m = nsubsets, ntiles = (m + kTile - 1) / kTile;
  const uint64_t nblk = std::max(scan_blocks(256 * ntiles), scan_blocks(m));
  return 2 * 8 * (m + kSlack) + 2 * 12 * m + 2 * 8 * m + 8 * 256 * ntiles + 8 * nblk + (pse_on_host ? 8 * m : 0) + 2 * staging + 4096;
}
bool lib_fits(uint64_t need)
{
  if (const char* e = getenv("KR_STATS_MAX_MB"))
    if (need > (uint64_t)strtoull(e, nullptr, 10) << 20) return false;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
  return need + (64ull << 20) <= (uint64_t)fr;
}

// (value, frequency) lists of vals[0 .. m), m > 0, on the null stream into the library's list `which`; *npasses: sort passes run
int histogram_on_device(const uint64_t* vals, uint64_t m, kr_lib_stats* L, int which, uint64_t* npasses)
{
  const uint32_t ntiles = (uint32_t)((m + kTile - 1) / kTile);
  const uint64_t ncounts = 256ull * ntiles;
  const uint64_t nblk = std::max(scan_blocks(ncounts), scan_blocks(m));
  DevBuf<uint64_t> b_a, b_b, b_flag, b_start, b_counts, b_bsum, b_small; // (freed at every return)
  DevBuf<uint32_t> b_ra, b_rb;
  if (!b_a.reserve(m) || !b_b.reserve(m) || !b_ra.reserve(m) || !b_rb.reserve(m) || !b_flag.reserve(m) || !b_start.reserve(m) || !b_counts.reserve(ncounts) ||
      !b_bsum.reserve(nblk) || !b_small.reserve(4)) {
    (void)hipGetLastError();
    return kr::fail(KR_ERR_NOMEM, "index statistics: out of device memory");
  }
  uint64_t* d_total = b_small.get(); // [0]: heads, [1]: the digit scans' totals, [2]: the maximum
  HIP_TRY(hipMemset(d_total, 0, 32));
  HIP_TRY(hipMemset(b_ra.get(), 0, m * 4)); // (the rank slots ride along unused)
  hipLaunchKernelGGL(kr_stats_copy_max_kernel, dim3(grid_for((m + 255) / 256)), dim3(256), 0, 0, vals, m, b_a.get(), (unsigned long long*)(d_total + 2));
  HIP_TRY(hipGetLastError());
  uint64_t vmax = 0;
  HIP_TRY(hipMemcpy(&vmax, d_total + 2, 8, hipMemcpyDeviceToHost)); // (synchronises: null stream)
  uint64_t *kin = b_a.get(), *kout = b_b.get();
  uint32_t *rin = b_ra.get(), *rout = b_rb.get();
  uint32_t bits = 0; // of the maximum: only these digits can differ
  while (bits < 64 && (vmax >> bits)) ++bits;
  *npasses = 0;
  for (uint32_t shift = 0; shift < bits; shift += 8, ++*npasses) {
    hipLaunchKernelGGL(kr_keys_hist_kernel, dim3(ntiles), dim3(256), 0, 0, kin, rin, m, ntiles, 0u, shift, b_counts.get());
    scan_u64<false>(b_counts.get(), ncounts, b_bsum.get(), d_total + 1);
    hipLaunchKernelGGL(kr_keys_scatter_kernel, dim3(ntiles), dim3(256), 0, 0, kin, rin, kout, rout, m, ntiles, 0u, shift, b_counts.get());
    std::swap(kin, kout), std::swap(rin, rout);
  }
  // kin: sorted; kout takes the heads' values
  const uint32_t g = grid_for((m + 255) / 256);
  hipLaunchKernelGGL(kr_stats_head_kernel, dim3(g), dim3(256), 0, 0, kin, m, b_flag.get());
  scan_u64<false>(b_flag.get(), m, b_bsum.get(), d_total);
  hipLaunchKernelGGL(kr_stats_compact_kernel, dim3(g), dim3(256), 0, 0, kin, m, (const uint64_t*)b_flag.get(), kout, b_start.get());
  hipLaunchKernelGGL(kr_stats_runs_kernel, dim3(g), dim3(256), 0, 0, (const uint64_t*)b_start.get(), (const uint64_t*)d_total, m, b_flag.get());
  HIP_TRY(hipGetLastError());
  uint64_t nh = 0;
  HIP_TRY(hipMemcpy(&nh, d_total, 8, hipMemcpyDeviceToHost));
  if (nh == 0 || nh > m) return kr::fail(KR_ERR_STATE, "index statistics: inconsistent run counts");
  std::vector<uint64_t> value(nh), freq(nh);
  HIP_TRY(hipMemcpy(value.data(), kout, nh * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(freq.data(), b_flag.get(), nh * 8, hipMemcpyDeviceToHost));
  return kr::lib_stats_set_list(L, which, value.data(), freq.data(), nh);
}

struct CallStats {
  uint64_t chunks = 0, lds = 0, global = 0, passes_mer = 0, passes_deg = 0;
  float copy_ms = 0, kern_ms = 0, rest_ms = 0;
};

// One library on the device in effect.  KR_ERR_NOMEM: not for the device (the caller takes the whole call to the host).
int lib_on_device(const kr_index_view* v, uint32_t lib, uint32_t flags, uint32_t cap, kr_lib_stats* L, CallStats* cs)
{
  const kr_lib_view& lv = v->libs[lib];
  const uint32_t ns = lv.nsubsets;
  const bool on_dev = (flags & KR_VIEW_DEVICE) != 0;
  if (on_dev && ((((uintptr_t)lv.cmer) & 7u) || (((uintptr_t)lv.pse) & 7u))) return kr::fail(KR_ERR_ARG, "kr_index_stats_device: cmer / pse must be 8-byte aligned");
  const uint64_t chunk_dflt = on_dev ? (1ull << 30) : (16ull << 20);
  uint64_t chunk = std::max<uint64_t>(1, env_u64("KR_STATS_CHUNK_KMERS", chunk_dflt));
  if (chunk / kRun >= (1ull << 31)) chunk = (uint64_t)kRun << 30; // (a grid's width)
  const uint64_t staging = on_dev ? 0 : std::min<uint64_t>(chunk, std::max<uint64_t>(lv.nkmers, 1)) * 8;
  if (!lib_fits(lib_bytes(ns, staging, !on_dev))) return kr::fail(KR_ERR_NOMEM, "index statistics: no room on the device");

  DevBuf<uint64_t> b_count, b_outdeg, b_small, b_pse; // (freed at every return)
  if (!b_count.reserve((uint64_t)ns + kSlack) || !b_outdeg.reserve((uint64_t)ns + kSlack) || !b_small.reserve(4) || (!on_dev && !b_pse.reserve(std::max<uint32_t>(ns, 1)))) {
    (void)hipGetLastError();
    return kr::fail(KR_ERR_NOMEM, "index statistics: out of device memory");
  }
  unsigned long long* d_bad = (unsigned long long*)b_small.get(); // [0]: first bad cmer entry, [1]: first bad se_to_pse entry, [2], [3]: route
  const uint64_t none[4] = {~0ull, ~0ull, 0, 0};
  HIP_TRY(hipMemcpy(d_bad, none, 32, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(b_count.get(), 0, ((uint64_t)ns + kSlack) * 8));
  HIP_TRY(hipMemset(b_outdeg.get(), 0, ((uint64_t)ns + kSlack) * 8));
  const uint2* d_pse = (const uint2*)lv.pse;
  if (!on_dev) {
    if (ns) HIP_TRY(hipMemcpy(b_pse.get(), lv.pse, (uint64_t)ns * 8, hipMemcpyHostToDevice));
    d_pse = (const uint2*)b_pse.get();
  }
  HIP_TRY(hipDeviceSynchronize()); // the counters are zero before a kernel on another stream adds to them

  if (lv.nkmers) {
    Staging S;
    if (int rc = S.open()) return rc;
    if (!on_dev)
      for (int s = 0; s < 2; ++s)
        if (!S.pin[s].reserve(staging / 8) || !S.dev[s].reserve(staging / 8)) {
          (void)hipGetLastError();
          return kr::fail(KR_ERR_NOMEM, "index statistics: out of staging memory");
        }
    uint64_t i = 0;
    for (uint64_t c0 = 0; c0 < lv.nkmers; c0 += chunk, ++i) {
      const uint64_t n = std::min(chunk, lv.nkmers - c0);
      const int s = (int)(i & 1u);
      if (int rc = S.retire(s)) return rc; // the slot's buffers are free again
      const uint32_t* src = lv.cmer + 2 * c0;
      HIP_TRY(hipEventRecord(S.c0[s], S.st_copy));
      if (!on_dev) {
        memcpy(S.pin[s].get(), src, n * 8);
        HIP_TRY(hipMemcpyAsync(S.dev[s].get(), S.pin[s].get(), n * 8, hipMemcpyHostToDevice, S.st_copy));
        src = (const uint32_t*)S.dev[s].get();
      }
      HIP_TRY(hipEventRecord(S.c1[s], S.st_copy));
      HIP_TRY(hipStreamWaitEvent(S.st_kern, S.c1[s], 0));
      HIP_TRY(hipEventRecord(S.k0[s], S.st_kern));
      hipLaunchKernelGGL(kr_stats_count_kernel, dim3(count_grid(n)), dim3(256), 0, S.st_kern, src, n, c0, ns, cap, (unsigned long long*)b_count.get(), d_bad,
                         d_bad + 2);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(S.k1[s], S.st_kern));
      S.used[s] = true;
    }
    if (int rc = S.retire(0)) return rc;
    if (int rc = S.retire(1)) return rc;
    HIP_TRY(hipStreamSynchronize(S.st_kern));
    cs->chunks += i, cs->copy_ms += S.copy_ms, cs->kern_ms += S.kern_ms;
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (ns > 1) hipLaunchKernelGGL(kr_stats_outdeg_kernel, dim3(grid_for(((uint64_t)ns + 255) / 256)), dim3(256), 0, 0, d_pse, ns, (unsigned long long*)b_outdeg.get(), d_bad + 1);
  HIP_TRY(hipGetLastError());
  uint64_t res[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(res, d_bad, 32, hipMemcpyDeviceToHost)); // (synchronises: null stream)
  cs->lds += res[2], cs->global += res[3];
  if (res[0] != ~0ull) { // the entry's value, for the message
    if (res[0] >= lv.nkmers) return kr::fail(KR_ERR_STATE, "index statistics: inconsistent entry index");
    uint32_t se = 0;
    if (on_dev) HIP_TRY(hipMemcpy(&se, lv.cmer + 2 * res[0] + 1, 4, hipMemcpyDeviceToHost));
    else se = lv.cmer[2 * res[0] + 1];
    return kr::stats_bad_id(v, lib, "cmer", res[0], se);
  }
  if (res[1] != ~0ull) {
    if (res[1] >= ns) return kr::fail(KR_ERR_STATE, "index statistics: inconsistent entry index");
    uint32_t pr[2] = {0, 0};
    HIP_TRY(hipMemcpy(pr, (const uint32_t*)d_pse + 2 * res[1], 8, hipMemcpyDeviceToHost));
    return kr::stats_bad_id(v, lib, "se_to_pse", res[1], pr[0] >= ns ? pr[0] : pr[1]);
  }
  if (ns > 1) {
    if (int rc = histogram_on_device(b_count.get() + 1, (uint64_t)ns - 1, L, 0, &cs->passes_mer)) return rc;
    if (int rc = histogram_on_device(b_outdeg.get() + 1, (uint64_t)ns - 1, L, 1, &cs->passes_deg)) return rc;
  } else {
    cs->passes_mer = cs->passes_deg = 0;
    if (int rc = kr::lib_stats_set_list(L, 0, nullptr, nullptr, 0)) return rc;
    if (int rc = kr::lib_stats_set_list(L, 1, nullptr, nullptr, 0)) return rc;
  }
  if (flags & KR_STATS_KEEP_COUNTS) {
    L->se_count = (uint64_t*)malloc(std::max<uint64_t>(1, ns) * 8);
    L->se_outdeg = (uint64_t*)malloc(std::max<uint64_t>(1, ns) * 8);
    if (!L->se_count || !L->se_outdeg) return kr::fail(KR_ERR_NOMEM, "kr_index_stats: out of memory");
    if (ns) {
      HIP_TRY(hipMemcpy(L->se_count, b_count.get(), (uint64_t)ns * 8, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(L->se_outdeg, b_outdeg.get(), (uint64_t)ns * 8, hipMemcpyDeviceToHost));
    }
  }
  cs->rest_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return KR_OK;
}

// No room on the device: the canonical form from the host, for a device view after its arrays have come back
int finish_on_host(const kr_index_view* v, uint32_t flags, kr_index_stats* out)
{
  if (!(flags & KR_VIEW_DEVICE)) return kr_index_stats_cpu(v, flags & KR_STATS_KEEP_COUNTS, out);
  std::vector<kr_lib_view> libs(v->libs, v->libs + v->nlibs);
  std::vector<std::vector<uint32_t>> cmer(v->nlibs), pse(v->nlibs);
  for (uint32_t i = 0; i < v->nlibs; ++i) {
    cmer[i].resize(2 * libs[i].nkmers), pse[i].resize(2 * (uint64_t)libs[i].nsubsets);
    if (!cmer[i].empty()) HIP_TRY(hipMemcpy(cmer[i].data(), libs[i].cmer, cmer[i].size() * 4, hipMemcpyDeviceToHost));
    if (!pse[i].empty()) HIP_TRY(hipMemcpy(pse[i].data(), libs[i].pse, pse[i].size() * 4, hipMemcpyDeviceToHost));
    libs[i].cmer = cmer[i].data(), libs[i].pse = pse[i].data();
  }
  kr_index_view hv = *v;
  hv.libs = libs.data();
  return kr_index_stats_cpu(&hv, flags & KR_STATS_KEEP_COUNTS, out);
}

} // namespace

extern "C" int kr_index_stats_device(const kr_index_view* v, int device, uint32_t flags, kr_index_stats* out)
{
  kr::clear_error();
  if (!v || !out || (v->nlibs && !v->libs)) return kr::fail(KR_ERR_ARG, "kr_index_stats_device: null argument");
  memset(out, 0, sizeof(*out));
  for (uint32_t i = 0; i < v->nlibs; ++i)
    if ((v->libs[i].nkmers && !v->libs[i].cmer) || (v->libs[i].nsubsets && !v->libs[i].pse))
      return kr::fail(KR_ERR_ARG, "kr_index_stats_device: null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return kr::fail(KR_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return kr::fail(KR_ERR_ARG, "kr_index_stats_device: bad device ordinal");
  HIP_TRY(hipSetDevice(device));
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t cap = (uint32_t)std::min<uint64_t>(env_u64("KR_STATS_LDS_CAP", kLdsColours), kLdsColours);
  CallStats cs;
  int rc = kr::index_stats_alloc(v, out);
  for (uint32_t i = 0; rc == KR_OK && i < v->nlibs; ++i) rc = lib_on_device(v, i, flags, cap, &out->libs[i], &cs);
  uint64_t path = 1;
  if (rc == KR_ERR_NOMEM) {
    kr::clear_error(); // no room on the device: the twin, with the same result
    kr_index_stats_free(out);
    (void)hipGetLastError();
    cs = CallStats();
    path = 2;
    rc = finish_on_host(v, flags, out);
  }
  if (rc != KR_OK) {
    const std::string msg = kr_last_error();
    kr_index_stats_free(out);
    return kr::fail(rc, msg);
  }
  const uint64_t st[8] = {path, cs.chunks, cs.lds, cs.global, cap, cs.passes_mer, cs.passes_deg, kRun};
  for (int q = 0; q < 8; ++q) g_stat[q].store(st[q]);
  g_ms[0].store(cs.copy_ms), g_ms[1].store(cs.kern_ms), g_ms[2].store(cs.rest_ms);
  g_ms[3].store(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return KR_OK;
}

extern "C" void kr_debug_index_stats(uint64_t out[8])
{
  if (!out) return;
  for (int q = 0; q < 8; ++q) out[q] = g_stat[q].load();
  if (!out[4] && !out[0]) out[4] = kLdsColours; // (also before the first call)
  out[7] = kRun;
}

extern "C" void kr_debug_index_stats_ms(float out[4])
{
  if (!out) return;
  for (int q = 0; q < 4; ++q) out[q] = g_ms[q].load();
}
