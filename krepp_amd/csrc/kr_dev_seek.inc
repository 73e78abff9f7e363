// kr_dev_seek.inc -- part of kr_device.hip (one translation unit, included in order): `krepp seek` on kernels of its own, from the
// reads' bases to the report text (docs/design/13_seek.md).
//
// SBatch::seek_sequences (src/seek.cpp:22-126): per k-mer and strand the MINIMUM Hamming distance over one bucket of the sketch, counted
// into a histogram of hdist_th + 1 bins per strand; onmers = the read's valid k-mers; one Brent minimisation per strand; the smaller d,
// or NaN when neither strand matched.  No colours, no tree, no minimum across references: a read's histogram is a SUM of independent
// per-position contributions, so a sequence of any length is cut into units of kSeekUnit positions, a wave per unit, and the units'
// counts are added with integer atomics -- exact, in any order.
//   kr_seek_count_kernel / kr_seek_uscan_kernel / kr_seek_first_kernel   units per read, the reads' first units (kr_dev_prefix.inc)
//   kr_seek_hist_kernel    a wave per unit: front end, one bucket walk per (position, strand), counts into the read's counters
//   kr_seek_solve_kernel   a lane per (read, strand): load_problem + brent_min of the likelihood stage, the read's d
//   kr_seek_text_len_kernel / kr_text_bscan_kernel / kr_seek_text_write_kernel   "id \t %.5f \n" or "id \tNaN\n"
constexpr uint32_t kSeekUnit = 256; // k-mer positions of a unit: two segments, so that a 150-base read is one unit
static_assert(kSeekUnit % kSegPos == 0, "a unit is whole segments: load_segment / front_end serve it as they serve the scan");
constexpr uint32_t kSeekHistWaves = 4; // waves of a workgroup of kr_seek_hist_kernel (they share nothing)

struct SeekIO {
  const uint8_t* bases;
  const uint64_t* offsets; // [nreads + 1]
  uint32_t nreads, np;     // np = hdist_th + 1
  uint32_t* first;         // [nreads + 1] the read's first unit; [nreads] = units of the batch
  uint32_t* bsum;          // [ceil(nreads / kRowBlock) + 1] units per block of reads, then (in place) the blocks' first units
  uint32_t* hist;          // [nreads][2][np] matched k-mers by minimum Hamming distance; cleared per batch
  uint32_t* onmers;        // [nreads] valid k-mers; cleared per batch
  double* d;               // [nreads] the reported distance, NaN: no match on either strand
  double* d_strand;        // [2 * nreads]
};

__device__ __forceinline__ uint32_t seek_units(const SeekIO& io, uint32_t k, uint32_t r)
{ // a read shorter than k has no unit
  const uint64_t len = io.offsets[r + 1] - io.offsets[r];
  const uint64_t npos = len >= k ? len - k + 1 : 0;
  return (uint32_t)((npos + kSeekUnit - 1) / kSeekUnit);
}

__global__ __launch_bounds__(256) void kr_seek_count_kernel(SeekIO io, uint32_t k)
{
  for (uint32_t b = blockIdx.x; b * kRowBlock < io.nreads; b += gridDim.x) {
    const uint32_t r0 = b * kRowBlock + 4u * threadIdx.x;
    uint32_t tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
      if (r0 + q < io.nreads) tot += seek_units(io, k, r0 + q);
    const uint32_t bs = block_sum(tot);
    if (threadIdx.x == 0) io.bsum[b] = bs;
  }
}

__global__ __launch_bounds__(1024) void kr_seek_uscan_kernel(SeekIO io)
{
  const uint32_t total = scan_block_sums(io.bsum, (io.nreads + kRowBlock - 1) / kRowBlock);
  if (threadIdx.x == 0) io.first[io.nreads] = total;
}

__global__ __launch_bounds__(256) void kr_seek_first_kernel(SeekIO io, uint32_t k)
{
  for (uint32_t b = blockIdx.x; b * kRowBlock < io.nreads; b += gridDim.x) {
    const uint32_t r0 = b * kRowBlock + 4u * threadIdx.x;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      c[q] = r0 + q < io.nreads ? seek_units(io, k, r0 + q) : 0u;
      tot += c[q];
    }
    uint32_t run = io.bsum[b] + block_scan_excl(tot);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (r0 + q < io.nreads) io.first[r0 + q] = run;
      run += c[q];
    }
  }
}

// One wave per unit.  Lane i of a group of 64 positions has position i; per strand it walks the bucket of its row in the PACKED arrays
// and keeps the smallest hd.  The wave's counts live in registers, bin x of either strand in lane x (np <= 17 lanes hold one): a ballot
// per bin, its popcount added by the bin's lane.  Every k-mer belongs to the unit its first base's position falls in; a unit's segments
// are loaded from the sequence itself (load_segment reads the k - 1 bases past a segment's positions: the halo), so whether a k-mer is
// valid never depends on where the seams fall.
// TAB: the front end from the byte tables in LDS (front_end_tab: 8 LDS reads + ~30 vector instructions per position pair) instead of
// the windows + software PEXT (front_end_words); bit-exact with each other.
template <bool SL, bool TAB>
__global__ __launch_bounds__(kSeekHistWaves* kWave) void kr_seek_hist_kernel(DevIndex ix, SeekIO io, uint32_t th)
{
  __shared__ __attribute__((aligned(16))) uint4 s_fetab[TAB ? 1024 : 1];
  if (TAB) {
    fe_tab_to_lds(ix, (lds_u32x4*)s_fetab);
    __syncthreads();
  }
  const uint32_t lane = lane_id();
  // A wave takes a contiguous range of units: one search for the read of its first unit (20 dependent loads on a million reads), then
  // a step from read to read; and the counts of consecutive units of one read are added to the read's counters once
  const uint32_t nwaves = gridDim.x * kSeekHistWaves, nunits = io.first[io.nreads];
  const uint32_t per_wave = (nunits + nwaves - 1) / nwaves;
  const uint64_t u0 = (uint64_t)(blockIdx.x * kSeekHistWaves + threadIdx.x / kWave) * per_wave;
  if (u0 >= nunits) return;
  const uint32_t u1 = (uint32_t)min((uint64_t)nunits, u0 + per_wave);
  uint32_t r;
  { // the read of unit u0: the last r with first[r] <= u0 (reads without units share their successor's first unit)
    uint32_t lo = 0, hi = io.nreads; // the smallest i in [lo, hi] with first[i] > u0; first[nreads] = nunits > u0
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (io.first[mid] > (uint32_t)u0) hi = mid; else lo = mid + 1;
    }
    r = lo - 1u;
  }
  uint32_t r_first = io.first[r], r_next = io.first[r + 1];
  uint32_t c0 = 0, c1 = 0, onmers = 0; // lane x: bin x of the forward / reverse strand; onmers wave-uniform
  auto flush = [&]() {
    if (lane <= th) {
      uint32_t* h = io.hist + (uint64_t)r * 2u * io.np;
      if (c0) atomicAdd(h + lane, c0);
      if (c1) atomicAdd(h + io.np + lane, c1);
    }
    if (lane == 0 && onmers) atomicAdd(io.onmers + r, onmers);
    c0 = 0, c1 = 0, onmers = 0;
  };
  for (uint32_t u = (uint32_t)u0; u < u1; ++u) {
    if (r_next <= u) { // (r + 1 <= nreads: first[nreads] = nunits > u)
      flush();
      do {
        ++r, r_first = r_next, r_next = io.first[r + 1];
      } while (r_next <= u);
    }
    const uint64_t off0 = io.offsets[r], len = io.offsets[r + 1] - off0;
    const uint8_t* seq = io.bases + off0;
    const uint64_t nkm = len - ix.k + 1; // (the read has a unit: len >= k)
    const uint64_t ubase = (uint64_t)(u - r_first) * kSeekUnit;
    for (uint32_t sg = 0; sg < kSeekUnit / kSegPos; ++sg) {
      const uint64_t base0 = ubase + (uint64_t)sg * kSegPos;
      if (base0 >= nkm) break;
      const uint32_t npos_seg = (uint32_t)min((uint64_t)kSegPos, nkm - base0);
      SegBits sb;
      load_segment(seq, len, base0, sb);
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) { // unrolled: SegBits stays in scalar registers
        if (pp == 1 && npos_seg <= 64) break;
        const FrontEnd fe = TAB ? front_end_tab_sel(ix, (const lds_u32x4*)s_fetab, sb, (uint32_t)pp, npos_seg) : front_end(ix, sb, pp, npos_seg);
        onmers += (uint32_t)__popcll(__ballot(fe.valid));
        // (both strands' bucket descriptors are asked for before either bucket is walked)
        uint64_t bk0 = 0, bk1 = 0;
        const uint32_t *e0 = nullptr, *e1 = nullptr;
        {
          int lib = 0;
          uint32_t row = 0;
          if (fe.valid && locate_row<SL>(ix, fe.rix[0], lib, row)) {
            const DevLib L = get_lib<SL>(ix, (uint32_t)lib);
            bk0 = L.bkt[row], e0 = L.enc;
          }
          if (fe.valid && locate_row<SL>(ix, fe.rix[1], lib, row)) {
            const DevLib L = get_lib<SL>(ix, (uint32_t)lib);
            bk1 = L.bkt[row], e1 = L.enc;
          }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          uint32_t best = 0xFFu;
          {
            const uint64_t b = st ? bk1 : bk0; // (0: no row for this k-mer, or an empty bucket)
            const uint32_t* e = (st ? e1 : e0) + (b >> 24);
            const uint32_t n = (uint32_t)(b & 0xFFFFFFu), q = fe.enc32[st];
            for (uint32_t i = 0; i < n; ++i) best = min(best, hd_lr32(e[i], q));
          }
          for (uint32_t x = 0; x <= th; ++x) {
            const uint32_t hits = (uint32_t)__popcll(__ballot(best == x));
            if (lane == x) (st ? c1 : c0) += hits;
          }
        }
      }
    }
  }
  flush();
}

// A lane per (read, strand), the two strands of a read in neighbouring lanes.  A read without a match on either strand is NaN and
// takes no part in the minimisation (its lanes are switched off for the loop, which ends with the slowest busy lane of the wave);
// otherwise BOTH strands are minimised -- the empty one on an all-zero histogram, uc = onmers (src/seek.cpp:40-41).
template <int NPT>
__global__ __launch_bounds__(256) void kr_seek_solve_kernel(LlhConst C, DevIndex ix, SeekIO io)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables T{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, T.bk, T.hnk);
  const double rho = ix.lib0.rho[1];
  const uint64_t n2 = 2ull * io.nreads;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n2; i0 += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = i0 + threadIdx.x; // (n2 is even: a read's two lanes are in or out together)
    const bool in = i < n2;
    const uint32_t r = (uint32_t)(i >> 1);
    const uint32_t* h = io.hist + (in ? i : 0ull) * io.np;
    uint32_t mine = 0;
    if (in)
      for (uint32_t x = 0; x <= C.th; ++x) mine += h[x];
    const uint32_t other = (uint32_t)__shfl_xor((int)mine, 1);
    double d = __builtin_nan("");
    if (in && mine + other != 0u) {
      LlhProblem p;
      double v;
      load_problem<NPT>(C, h, 1, io.onmers[r], rho, p);
      brent_min<NPT>(C, T, p, d, v);
    }
    const double dn = __shfl_xor(d, 1);
    if (in) {
      io.d_strand[i] = d;
      if (!(i & 1ull)) io.d[r] = d < dn ? d : dn; // d_or < d_rc ? d_or : d_rc; NaN stays NaN (both strands are)
    }
  }
}

// The report: SEQ_ID '\t' DIST '\n' with DIST as "%.5f" (the exact formatter of the `dist` text), or SEQ_ID "\tNaN\n".  A thread per
// read, four reads a thread: a row is some twenty bytes.
__device__ __forceinline__ uint32_t seek_row_len(const TextIO& t, const SeekIO& io, uint32_t r, uint32_t& n, bool& ok)
{
  const uint32_t idl = t.id_off[r + 1] - t.id_off[r] - t.id_sep;
  const double d = io.d[r];
  ok = true, n = 0xFFFFFFFFu;
  if (d != d) return idl + 5u;
  return idl + 2u + text_num(d, n, ok);
}

__global__ __launch_bounds__(256) void kr_seek_text_len_kernel(SeekIO io, TextIO t)
{
  for (uint32_t b = blockIdx.x; b * kRowBlock < io.nreads; b += gridDim.x) {
    const uint32_t r0 = b * kRowBlock + 4u * threadIdx.x;
    uint64_t tot = 0;
    bool bad = false;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
      if (r0 + q < io.nreads) {
        uint32_t n;
        bool ok;
        const uint32_t len = seek_row_len(t, io, r0 + q, n, ok);
        t.rd_tlen[r0 + q] = len;
        tot += len;
        bad = bad || !ok;
      }
    if (bad) atomicOr((unsigned long long*)&t.total[1], (unsigned long long)kTextBadNum);
    const uint64_t bs = block_sum(tot);
    if (threadIdx.x == 0) t.t_bsum[b] = bs;
  }
}

__global__ __launch_bounds__(256) void kr_seek_text_write_kernel(SeekIO io, TextIO t)
{
  if (t.total[0] > t.text_cap) return; // (the flag is up: the caller splits the batch)
  for (uint32_t b = blockIdx.x; b * kRowBlock < io.nreads; b += gridDim.x) {
    const uint32_t r0 = b * kRowBlock + 4u * threadIdx.x;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      c[q] = r0 + q < io.nreads ? t.rd_tlen[r0 + q] : 0u;
      tot += c[q];
    }
    char* p = t.text + t.t_bsum[b] + block_scan_excl(tot);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (r0 + q >= io.nreads) break;
      const uint32_t r = r0 + q;
      uint32_t nn;
      bool ok;
      const uint32_t len = seek_row_len(t, io, r, nn, ok);
      const uint32_t idl = t.id_off[r + 1] - t.id_off[r] - t.id_sep;
      const char* id = t.ids + t.id_off[r];
      for (uint32_t x = 0; x < idl; ++x) p[x] = id[x];
      char* w = p + idl;
      *w++ = '\t';
      if (nn == 0xFFFFFFFFu) {
        w[0] = 'N', w[1] = 'a', w[2] = 'N', w[3] = '\n';
      } else { // "%.5f": dl - 6 integer digits, '.', five decimals
        const uint32_t dl = len - idl - 2u, nd = dl - 6u;
        uint32_t ip = nn / 100000u, fp = nn - ip * 100000u;
        for (uint32_t x = nd; x-- > 0u;) {
          w[x] = (char)('0' + ip % 10u);
          ip /= 10u;
        }
        w[nd] = '.';
#pragma unroll
        for (int x = 4; x >= 0; --x) {
          w[nd + 1u + (uint32_t)x] = (char)('0' + fp % 10u);
          fp /= 10u;
        }
        w[dl] = '\n';
      }
      p += c[q];
    }
  }
}
