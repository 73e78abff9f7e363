// kr_dev_text.inc -- part of kr_device.hip (one translation unit, included in order): the report rows of `krepp dist` as TEXT,
// written on the device.
//
// IBatch::report_distances (src/query.cpp:158-196) appends, per read and per reference the read keeps,
//     SEQ_ID '\t' REFERENCE_NAME '\t' DIST '\n'       DIST with std::fixed and 5 decimals (src/query.cpp:152-153)
// and SEQ_ID "\tNA\tNaN\n" for a read that keeps none (:173-176).  The reference does it inside the parallel batch task; the host
// formatter of rounds 1-4 (kr_format_dist) did it on the box's CPUs at ~100 M rows/s -- 45 times under the kernels on the benchmark
// index (33 rows per read).  Here the batch's compact rows (kr_rows_* kernels: (key, DIST) of the selected records, a read's rows
// contiguous, in record order) become the batch's text in HBM:
//   kr_text_len_kernel    bytes of every read's text (a wave per read, a lane per row), bytes per block of kRowBlock reads
//   kr_text_bscan_kernel  the blocks' first bytes (64-bit), the batch's total
//   kr_text_write_kernel  a block's reads: their first bytes (LDS scan), then a wave per read: a lane per row finds its place by a
//                         wave prefix sum of the row lengths and writes id, name and digits
// The digits are printf's: round-half-even of the exact binary value (fixed5_exact, kr_common.h), so the text is byte-identical to
// the host formatter's and to the oracle's.  A DIST outside [0, 1000) (never produced by the minimiser, whose bracket is
// [1e-10, 0.5]) raises a flag and the caller formats that batch on the host.  The text leaves the device as bytes; the host only
// writes them.
// Bits of the text kernels' flag word (TextIO::total[1], PlaceText::total[1]); any of them leaves the text to the host
enum TextFlag : uint32_t {
  kTextBadNum = 1u,  // a number outside what the device formats exactly
  kTextOverCap = 2u, // more text than text_cap
  kTextNearTie = 8u, // `place`: a value too close to a rounding tie after exp / log
  kTextNoRange = 16u // `place`: nothing was formatted (a range about to be run again), or a node number was out of range
};
struct TextIO {
  const char* ids;          // the reads' ids back to back
  const uint32_t* id_off;   // [nreads + 1] id r = ids[id_off[r] .. id_off[r + 1] - id_sep)
  uint32_t id_sep;          // separator bytes behind every id in the blob (1: NUL-terminated names)
  const char* names;        // node names by colour id: names[name_off[se] .. name_off[se + 1])
  const uint32_t* name_off; // [tree_nnodes + 2]
  uint32_t* rd_tlen;        // [nreads] bytes of the read's text
  uint64_t* t_bsum;         // [ceil(nreads / kRowBlock) + 1] bytes per block, then (in place) the blocks' first bytes
  char* text;
  uint64_t text_cap;
  uint64_t* total;          // [0] bytes of the batch's text  [1] TextFlag bits
};

// bytes of "%.5f" of d, and its rounded integer; an unprintable d counts as the 7-byte placeholder that nobody will read
__device__ __forceinline__ uint32_t text_num(double d, uint32_t& n, bool& ok)
{
  ok = kr::fixed5_exact(d, &n);
  if (!ok) n = 0;
  return n < 1000000u ? 7u : (n < 10000000u ? 8u : 9u);
}

__global__ __launch_bounds__(256) void kr_text_len_kernel(BatchOut out, TextIO t, uint32_t nreads)
{
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  for (uint32_t b = blockIdx.x; b * kRowBlock < nreads; b += gridDim.x) {
    const uint32_t rb = b * kRowBlock;
    uint32_t wsum = 0; // wave-uniform
    bool bad = false;
    for (uint32_t q = w; q < kRowBlock && rb + q < nreads; q += 4u) {
      const uint32_t r = rb + q, o = out.rd_roff[r], n = out.rd_rcnt[r];
      const uint32_t idl = t.id_off[r + 1] - t.id_off[r] - t.id_sep;
      uint32_t len = 0;
      for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
        const uint32_t i = i0 + lane;
        if (i < n) {
          const uint32_t se = out.row_key[o + i] >> 1;
          uint32_t nn;
          bool ok;
          len += idl + (t.name_off[se + 1] - t.name_off[se]) + text_num(out.row_d[o + i], nn, ok) + 3u;
          bad = bad || !ok;
        }
      }
      len = wave_sum(len);
      if (out.rd_na[r]) len += idl + 8u; // "\tNA\tNaN\n"
      if (lane == 0) t.rd_tlen[r] = len;
      wsum += len;
    }
    if (__ballot(bad) != 0 && lane == 0) atomicOr((unsigned long long*)&t.total[1], (unsigned long long)kTextBadNum);
    const uint64_t tot = block_sum_waves<uint64_t>(wsum);
    if (threadIdx.x == 0) t.t_bsum[b] = tot;
  }
}

// (the text of `dist` and of `place`, kr_dev_place.inc: nblk is the caller's number of blocks, whatever reads a block holds)
__global__ __launch_bounds__(1024) void kr_text_bscan_kernel(uint64_t* t_bsum, uint32_t nblk, uint64_t text_cap, uint64_t* total)
{ // one workgroup: exclusive prefix of t_bsum in place (64-bit: an 8 M-read batch on the benchmark index is 7 GB of text)
  const uint64_t bytes = scan_block_sums(t_bsum, nblk);
  if (threadIdx.x == 0) {
    total[0] = bytes;
    if (bytes > text_cap) atomicOr((unsigned long long*)&total[1], (unsigned long long)kTextOverCap);
  }
}

__global__ __launch_bounds__(256) void kr_text_write_kernel(BatchOut out, TextIO t, uint32_t nreads)
{
  __shared__ uint32_t s_off[kRowBlock];
  if (t.total[0] > t.text_cap) return; // (the flag is up: the caller splits the batch)
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  for (uint32_t b = blockIdx.x; b * kRowBlock < nreads; b += gridDim.x) {
    // ---- first byte of every read of the block, relative to the block's: thread t owns the reads 4t .. 4t+3
    const uint32_t rb = b * kRowBlock, q0 = 4u * threadIdx.x;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      c[q] = rb + q0 + q < nreads ? t.rd_tlen[rb + q0 + q] : 0u;
      tot += c[q];
    }
    uint32_t run = block_scan_excl(tot);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      s_off[q0 + q] = run;
      run += c[q];
    }
    __syncthreads();
    char* const tb = t.text + t.t_bsum[b];
    // ---- a wave per read, a lane per row
    for (uint32_t q = w; q < kRowBlock && rb + q < nreads; q += 4u) {
      const uint32_t r = rb + q, o = out.rd_roff[r], n = out.rd_rcnt[r];
      const uint32_t id0 = t.id_off[r], idl = t.id_off[r + 1] - id0 - t.id_sep;
      const char* id = t.ids + id0;
      uint32_t pos = s_off[q]; // wave-uniform
      for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
        const uint32_t i = i0 + lane;
        uint32_t len = 0, nn = 0, nl = 0, n0 = 0, dl = 0;
        bool ok = true;
        if (i < n) {
          const uint32_t se = out.row_key[o + i] >> 1;
          n0 = t.name_off[se], nl = t.name_off[se + 1] - n0;
          dl = text_num(out.row_d[o + i], nn, ok);
          len = idl + nl + dl + 3u;
        }
        const uint32_t incl = wave_scan_incl(len);
        if (i < n) {
          char* p = tb + pos + (incl - len);
          for (uint32_t x = 0; x < idl; ++x) p[x] = id[x];
          p += idl;
          *p++ = '\t';
          const char* nm = t.names + n0;
          for (uint32_t x = 0; x < nl; ++x) p[x] = nm[x];
          p += nl;
          *p++ = '\t';
          // "%.5f": dl - 6 integer digits, '.', five decimals (straight into place: no private array)
          uint32_t ip = nn / 100000u, fp = nn - ip * 100000u;
          const uint32_t nd = dl - 6u;
          for (uint32_t x = nd; x-- > 0u;) {
            p[x] = (char)('0' + ip % 10u);
            ip /= 10u;
          }
          p[nd] = '.';
#pragma unroll
          for (int x = 4; x >= 0; --x) {
            p[nd + 1u + (uint32_t)x] = (char)('0' + fp % 10u);
            fp /= 10u;
          }
          p[dl] = '\n';
        }
        pos += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      }
      if (out.rd_na[r]) { // SEQ_ID "\tNA\tNaN\n"
        char* p = tb + pos;
        for (uint32_t x = lane; x < idl; x += 64u) p[x] = id[x];
        if (lane < 8u) p[idl + lane] = "\tNA\tNaN\n"[lane];
      }
    }
    __syncthreads();
  }
}
