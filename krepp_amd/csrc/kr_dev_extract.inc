// kr_dev_extract.inc -- part of kr_device.hip (one translation unit, included in order): the reads of a seek batch split into two
// byte strings on the device (kr_stream_extract_enable; docs/design/13_seek.md section 13.6).
//
// A seek batch that a record finder queued has its chunk in d_raw, and the accepted records tile [0, consumed) without a gap: record r
// is the bytes [rec_start[r], rec_start[r + 1]).  With the verdict
//   matched[r] = !isnan(d[r]) && (isnan(max_dist) || d[r] <= max_dist)          (in double, on the d[r] the text kernel formats)
// and mpre[r] = the matched records' bytes in front of record r (M = all of them), record r moves as ONE block:
//   matched      out[mpre[r] ..)
//   unmatched    out[M + (rec_start[r] - mpre[r]) ..)        (rec_start[r] - mpre[r]: the unmatched bytes in front of it)
// so that out[0, M) is the matched reads and out[M, consumed) the unmatched ones, both in file order -- a stable partition of the
// chunk's bytes in one buffer of the chunk's size, which cannot overflow.
//   kr_ex_len_kernel    rec_start[0 .. n] from the record finder's lists (FASTQ: the newline list, FASTA: the start list), and per
//                       block of kRowBlock records the matched records' bytes and number
//   kr_ex_scan_kernel   one workgroup: the blocks' first matched byte, the summary {M, matched records, n, consumed}
//   kr_ex_pre_kernel    mpre[0 .. n]
//   kr_ex_copy_kernel   a workgroup per source tile of kFqTile bytes, a lane per 16 of them: parallel over BYTES, never over records.
//                       One binary search finds the record of the tile's first byte; the starts of the records that begin inside the
//                       tile are counted into the lanes' 16-byte groups (LDS), a scan gives every lane the record of its first byte,
//                       and the lane steps through the records its 16 bytes touch.  Within a record destination - source is a
//                       constant: a tile inside one long record is a shifted straight copy, a tile of 2-byte records costs what its
//                       bytes cost.
// The record count n comes from the record finder's device summary; every index is bounded by it and by the list capacities before
// it indexes anything, every load of the chunk starts in front of `consumed` (d_raw is padded for 16 bytes), and every store is
// checked against `consumed`, the size of what `out` holds.
// Paired reads (the end of this file): kr_ex_pair_kernel writes one value per pair, the four kernels take it through ExIO::d in place
// of the read's own distance and run unchanged -- both mates of a pair land in the same part.
struct ExIO {
  const uint8_t* raw;
  const kr_fastq_parse* sum; // the record finder's summary on the device: nreads, consumed
  const uint32_t* nl;        // FASTQ: newline positions [nl_cap]; nullptr: FASTA
  uint32_t nl_cap;
  const uint32_t* hs;        // FASTA: record starts [max_reads + 2]
  uint32_t max_reads;
  uint64_t raw_cap;          // bytes `out` holds (and d_raw, without its padding)
  const double* d;           // [n] the seek batch's reported distances
  double max_dist;           // NaN: every read with a DIST is matched
  uint32_t* rec_start;       // [max_reads + 1]
  uint32_t* mpre;            // [max_reads + 1]
  uint64_t* bsum;            // [max_reads / kRowBlock + 2] per block (matched records << 32 | matched bytes), then the blocks' first
  uint8_t* out;
  unsigned long long* res;   // [0] M  [1] matched records  [2] n  [3] consumed
  uint32_t wide;             // 1: a lane whose 16 bytes lie in one record stores them at once; 0: byte stores only
};

__device__ __forceinline__ uint32_t ex_nrec(const ExIO& x) { return min(x.sum->nreads, x.max_reads); }
__device__ __forceinline__ uint32_t ex_consumed(const ExIO& x) { return (uint32_t)min((uint64_t)x.sum->consumed, x.raw_cap); }

// first byte of record r <= n (r == n: the end of the accepted prefix)
__device__ __forceinline__ uint32_t ex_start(const ExIO& x, uint32_t r, uint32_t n, uint32_t consumed)
{
  if (r >= n) return consumed;
  if (r == 0) return 0u;
  uint32_t p;
  if (x.nl) {
    const uint64_t i = 4ull * r - 1ull;
    p = i < x.nl_cap ? x.nl[i] + 1u : consumed;
  } else
    p = x.hs[r]; // (r < n <= max_reads)
  return min(p, consumed);
}

__device__ __forceinline__ bool ex_matched(double d, double max_dist) { return d == d && (max_dist != max_dist || d <= max_dist); }

__global__ __launch_bounds__(256) void kr_ex_len_kernel(ExIO x)
{
  const uint32_t n = ex_nrec(x), consumed = ex_consumed(x);
  for (uint32_t b = blockIdx.x; b * kRowBlock <= n; b += gridDim.x) { // (<=: the block of entry n writes the sentinel)
    const uint32_t r0 = b * kRowBlock + 4u * threadIdx.x;
    uint64_t tot = 0;
    uint32_t s = r0 <= n ? ex_start(x, r0, n, consumed) : 0u;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t r = r0 + q;
      if (r > n) break;
      x.rec_start[r] = s;
      if (r == n) break;
      const uint32_t e = ex_start(x, r + 1u, n, consumed);
      if (e > s && ex_matched(x.d[r], x.max_dist)) tot += (1ull << 32) | (uint64_t)(e - s); // (the bytes of a chunk stay below 2^32)
      s = e;
    }
    const uint64_t bs = block_sum(tot);
    if (threadIdx.x == 0) x.bsum[b] = bs;
  }
}

__global__ __launch_bounds__(1024) void kr_ex_scan_kernel(ExIO x)
{
  const uint32_t n = ex_nrec(x);
  const uint64_t total = scan_block_sums(x.bsum, n / kRowBlock + 1u);
  if (threadIdx.x == 0) x.res[0] = total & 0xFFFFFFFFull, x.res[1] = total >> 32, x.res[2] = n, x.res[3] = ex_consumed(x);
}

__global__ __launch_bounds__(256) void kr_ex_pre_kernel(ExIO x)
{
  const uint32_t n = ex_nrec(x);
  for (uint32_t b = blockIdx.x; b * kRowBlock <= n; b += gridDim.x) {
    const uint32_t r0 = b * kRowBlock + 4u * threadIdx.x;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t r = r0 + q;
      c[q] = 0;
      if (r < n) {
        const uint32_t s = x.rec_start[r], e = x.rec_start[r + 1u];
        if (e > s && ex_matched(x.d[r], x.max_dist)) c[q] = e - s;
      }
      tot += c[q];
    }
    uint32_t run = (uint32_t)x.bsum[b] + block_scan_excl(tot);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (r0 + q <= n) x.mpre[r0 + q] = run;
      run += c[q];
    }
  }
}

struct __attribute__((packed, aligned(1))) ExBytes16 {
  uint32_t w[4];
};

__global__ __launch_bounds__(256) void kr_ex_copy_kernel(ExIO x)
{
  __shared__ uint32_t s_cnt[256];
  const uint32_t n = (uint32_t)x.res[2], consumed = (uint32_t)x.res[3];
  const uint64_t M = x.res[0];
  if (n == 0) return;
  const uint32_t ntiles = (uint32_t)(((uint64_t)consumed + kFqTile - 1) / kFqTile);
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t tile0 = t * kFqTile; // (< consumed < 2^32)
    const uint64_t tile_end = (uint64_t)tile0 + kFqTile;
    // the record of the tile's first byte: the last r < n with rec_start[r] <= tile0 (rec_start[0] = 0); every lane the same loads
    uint32_t lo = 0, hi = n; // the smallest i in [lo, hi] with rec_start[i] > tile0; rec_start[n] = consumed > tile0
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (x.rec_start[mid] > tile0) hi = mid; else lo = mid + 1u;
    }
    const uint32_t r_lo = lo ? lo - 1u : 0u;
    // the records that begin inside the tile behind its first byte, counted into the 16-byte group of their start
    __syncthreads(); // (the last tile's counts have been read)
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t j = (uint64_t)r_lo + 1u + threadIdx.x; j < n; j += 256u) {
      const uint32_t st = x.rec_start[j];
      if (st >= tile_end) break;
      if (st > tile0) atomicAdd(&s_cnt[(st - tile0) >> 4], 1u); // (st - tile0 < kFqTile)
    }
    __syncthreads();
    const uint32_t mine = s_cnt[threadIdx.x];
    uint32_t r = r_lo + block_scan_excl(mine); // the record of the byte in front of the lane's group (of the tile's first byte: lane 0)
    const uint32_t base = tile0 + 16u * threadIdx.x;
    if (base >= consumed) continue; // (no barrier is skipped: the next iteration's first one is reached by every thread)
    const uint4 v = *reinterpret_cast<const uint4*>(x.raw + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t end16 = (uint32_t)min((uint64_t)base + 16u, (uint64_t)consumed);
    uint32_t p = base;
    for (uint32_t step = 0; step < 17u && p < end16; ++step) {
      while (r + 1u < n && x.rec_start[r + 1u] <= p) ++r; // (at most the starts counted for this lane)
      const uint32_t re = min(x.rec_start[r + 1u], end16); // (r + 1 <= n)
      if (re <= p) break;                                  // (cannot be: the starts rise)
      const uint64_t pre = x.mpre[r];
      // destination of byte p: matched p - (rec_start[r] - mpre[r]); unmatched M + p - mpre[r]
      const uint64_t dst = ex_matched(x.d[r], x.max_dist) ? (uint64_t)p - ((uint64_t)x.rec_start[r] - pre) : M + (uint64_t)p - pre;
      const uint32_t len = re - p;
      if (dst + len > (uint64_t)consumed) break; // (cannot be: the two parts tile [0, consumed))
      uint8_t* o = x.out + dst;
      if (x.wide && len == 16u) {
        ExBytes16 b16;
        b16.w[0] = w[0], b16.w[1] = w[1], b16.w[2] = w[2], b16.w[3] = w[3];
        *reinterpret_cast<ExBytes16*>(o) = b16;
      } else {
        const uint32_t b0 = p - base;
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b)
          if (b >= b0 && b < b0 + len) o[b - b0] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
      }
      p = re;
    }
  }
}

// ---- paired reads: one verdict per PAIR in front of the partition (kr_batch_extract_pair; docs/design/13_seek.md section 13.7) ----
// Two seek batches hold the mates of the same pairs -- record r of stream A and record r of stream B -- or one batch holds them as
// neighbours (interleaved: the mate of record r is record r ^ 1).  kr_ex_pair_kernel writes, per record and per stream, one PAIR VALUE
// that the four kernels above take in place of the read's own distance (ExIO::d):
//   KR_PAIR_ANY    the smaller of the two distances that are not NaN; NaN when both are
//   KR_PAIR_BOTH   NaN when either is NaN, otherwise the larger
// so that ex_matched(pair value, max_dist) == matched(d1) || matched(d2), respectively matched(d1) && matched(d2): d <= max_dist holds
// for the smaller of two numbers iff it holds for one of them, for the larger iff for both.  Both mates carry the same value, so both
// land in the same part, and record i of A's matched part is the mate of record i of B's matched part (the partition is stable).
// The pair count is the smaller of the two record finders' device counts, each clamped to its stream's max_reads; a record of either
// stream behind it (the host refuses unequal counts: never) has no mate and takes the value a NaN mate gives.  Nothing is indexed
// before it is compared with its stream's own clamped count.
struct ExPairIO {
  const kr_fastq_parse *sum_a, *sum_b; // the record finders' device summaries (interleaved: the same)
  uint32_t max_a, max_b;               // the streams' max_reads: what d_* and pv_* hold
  const double *d_a, *d_b;             // the seek batches' reported distances
  double *pv_a, *pv_b;                 // [max_reads] the pair values (interleaved: pv_b == pv_a)
  uint32_t rule;                       // KR_PAIR_ANY, KR_PAIR_BOTH
  uint32_t interleaved;
};

__device__ __forceinline__ double ex_pair_value(double x, double y, uint32_t rule)
{
  const bool nx = x != x, ny = y != y;
  if (rule == KR_PAIR_BOTH) return (nx || ny) ? __builtin_nan("") : (x > y ? x : y);
  if (nx) return y; // (NaN when both are)
  if (ny) return x;
  return x < y ? x : y;
}

__global__ __launch_bounds__(256) void kr_ex_pair_kernel(ExPairIO p)
{
  const uint32_t na = min(p.sum_a->nreads, p.max_a), nb = min(p.sum_b->nreads, p.max_b);
  const uint32_t n = min(na, nb), top = max(na, nb);
  const double none = __builtin_nan("");
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < top; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t r = (uint32_t)i;
    if (p.interleaved) { // (na == nb == n)
      const uint32_t m = r ^ 1u;
      p.pv_a[r] = ex_pair_value(p.d_a[r], m < n ? p.d_a[m] : none, p.rule);
      continue;
    }
    const double x = r < na ? p.d_a[r] : none, y = r < nb ? p.d_b[r] : none;
    const double v = ex_pair_value(x, y, p.rule);
    if (r < na) p.pv_a[r] = v;
    if (r < nb) p.pv_b[r] = v;
  }
}
