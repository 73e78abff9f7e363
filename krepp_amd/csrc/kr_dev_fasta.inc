// kr_dev_fasta.inc -- part of kr_device.hip (one translation unit, included in order): FASTA records found on the device in a chunk
// of raw file bytes (kr_batch_submit_fasta).
//
// A FASTA record has any number of lines and may be megabases long, so nothing here walks a record: every pass that looks at the
// chunk's bytes is parallel over BYTES, in tiles of kFqTile bytes (a lane loads 16 bytes at once), and what a byte needs to know
// about its record comes from prefix counts.  With
//   start      a '>' at byte 0 or directly behind a '\n': record r runs from its start hs[r] to hs[r + 1]
//   graphic    a byte in 33..126
//   A(p)       the graphic bytes in front of p
// the record of byte p is (starts at or in front of p) - 1, and the batch's bases -- the records' sequences back to back -- are one
// global compaction: a graphic body byte p of record r lands at offsets[r] + A(p) - ga[r] - hg[r], ga[r] = A(hs[r]), hg[r] = the
// header's graphic bytes.
//   kr_fa_count_kernel   per tile: record starts, graphic bytes, newlines
//   kr_fa_scan_kernel    one workgroup: the tiles' first numbers of each, the chunk's totals, the sentinel hs[nrec] = nbytes
//   kr_fa_write_kernel   hs[i], ga[i] of the first max_reads + 1 starts (starts past the capacity are counted, not stored)
//   kr_fa_rec_kernel     a wave per record, HEADER ONLY: the header's '\n', the name's end, NUL in the name, hg[r]; rec_slen[r] =
//                        ga[r + 1] - ga[r] - hg[r]; INCOMPLETE / NOT_CLEAN / LONG by the FASTQ finder's atomicMin on (record << 8 |
//                        status).  The one pass that is serial in something: a wave reads its header 64 bytes a step, so its work is
//                        bounded by the header's length -- tens of bytes in a real file -- and at worst by the record's end: a hostile
//                        chunk that is one '>' and megabytes without a '\n' has one wave walk all of it (nbytes / 64 steps) and
//                        ends INCOMPLETE, without a stray access
//   kr_fa_check_kernel   per tile: a body byte among '+' '@', a '>' that is no start, or >= 128 makes its record NOT_CLEAN
//   kr_fq_bsum / bscan / off (kr_dev_fastq.inc)   offsets and id offsets of the records, CAPACITY
//   kr_fa_copy_kernel    per tile: the kept body bytes of the accepted records, compacted in LDS and written as one run; then a wave per
//                        accepted record copies its name, and one lane writes the summary.  (The run is written a byte a lane,
//                        coalesced; dword stores behind an alignment step on d0 would take a quarter of the store instructions: untried)
// Every index made from file bytes is bounded by the list capacities (a record number is compared with the record count before it
// indexes anything), by nbytes, and by the padding of d_raw (a lane's 16-byte load starts in front of nbytes).
struct FaIO {
  FqIO q;                      // raw, nbytes, tile_nl, rec_slen / rec_npos / rec_nlen, bsum_*, ctl, bases, offsets, ids, limits, sum (nl: unused; rec_lines 0)
  uint32_t *tile_st, *tile_gr; // [ceil(nbytes / kFqTile) + 1] starts / graphic bytes per tile, then (in place) the tiles' first numbers
  uint32_t *hs, *ga;           // [max_reads + 1] start of record i, graphic bytes in front of it; hs[nrec] = nbytes when every start is stored
  uint32_t *rec_hg, *rec_he;   // [max_reads] graphic bytes of the header, position of its '\n' (hs[r + 1]: it has none)
  uint32_t closed;             // the last record ends where the chunk does
};

struct FaMask {
  uint32_t nl, gt, gr, bad; // bit i: byte i of the 16 is '\n' / is '>' / is graphic / is one of '+' '@' '>' or >= 128
};

// 0x80 exactly in the bytes of w that equal the byte c4 repeats
__device__ __forceinline__ uint32_t fa_eq(uint32_t w, uint32_t c4)
{
  const uint32_t x = w ^ c4;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t fa_pack(uint32_t z) { return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u); }

// raw[base .. base + 16) classified (base + 16 lies inside the padded buffer; bytes at or past nbytes are in no mask)
__device__ __forceinline__ FaMask fa_masks(const uint8_t* raw, uint64_t base, uint64_t nbytes)
{
  const uint4 v = *reinterpret_cast<const uint4*>(raw + base);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  FaMask m{0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t lo = w[j] & 0x7F7F7F7Fu, hi = w[j] & 0x80808080u;
    const uint32_t gt = fa_eq(w[j], 0x3E3E3E3Eu);
    // 33 <= low seven bits (bit 7 of the sum), not 127 (no bit 7 after + 1), no high bit
    const uint32_t gr = (lo + 0x5F5F5F5Fu) & ~(lo + 0x01010101u) & ~w[j] & 0x80808080u;
    m.nl |= fa_pack(fa_eq(w[j], 0x0A0A0A0Au)) << (4 * j);
    m.gt |= fa_pack(gt) << (4 * j);
    m.gr |= fa_pack(gr) << (4 * j);
    m.bad |= fa_pack(gt | fa_eq(w[j], 0x2B2B2B2Bu) | fa_eq(w[j], 0x40404040u) | hi) << (4 * j);
  }
  const uint64_t left = nbytes - base;
  if (left < 16u) {
    const uint32_t in = (1u << left) - 1u;
    m.nl &= in, m.gt &= in, m.gr &= in, m.bad &= in;
  }
  return m;
}

// the record starts among the 16 bytes: a '>' behind a '\n' -- for byte 0 of the group the byte in front of it (never raw[-1])
__device__ __forceinline__ uint32_t fa_starts(const uint8_t* raw, uint64_t base, const FaMask& m)
{
  const uint32_t prev = base == 0 ? 1u : (raw[base - 1] == '\n' ? 1u : 0u);
  return m.gt & ((m.nl << 1) | prev) & 0xFFFFu;
}

__global__ __launch_bounds__(256) void kr_fa_count_kernel(FaIO f)
{
  const uint64_t ntiles = (f.q.nbytes + kFqTile - 1) / kFqTile;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = t * kFqTile + 16u * threadIdx.x;
    uint64_t c = 0; // three counts of at most kFqTile each, 16 bits apart
    if (base < f.q.nbytes) {
      const FaMask m = fa_masks(f.q.raw, base, f.q.nbytes);
      c = (uint64_t)__popc(fa_starts(f.q.raw, base, m)) | ((uint64_t)__popc(m.gr) << 16) | ((uint64_t)__popc(m.nl) << 32);
    }
    const uint64_t tot = block_sum(c);
    if (threadIdx.x == 0) f.tile_st[t] = (uint32_t)(tot & 0xFFFFu), f.tile_gr[t] = (uint32_t)((tot >> 16) & 0xFFFFu), f.q.tile_nl[t] = (uint32_t)(tot >> 32);
  }
}

__global__ __launch_bounds__(1024) void kr_fa_scan_kernel(FaIO f)
{ // one workgroup: exclusive prefixes of the three tile counts in place (a chunk below 4 GB: every total fits 32 bits)
  const uint32_t ntiles = (uint32_t)((f.q.nbytes + kFqTile - 1) / kFqTile);
  const uint32_t nst = scan_block_sums(f.tile_st, ntiles);
  const uint32_t ngr = scan_block_sums(f.tile_gr, ntiles);
  const uint32_t newlines = scan_block_sums(f.q.tile_nl, ntiles);
  if (threadIdx.x == 0) {
    f.q.ctl[0] = newlines, f.q.ctl[3] = nst;
    if (nst <= f.q.max_reads) f.hs[nst] = (uint32_t)f.q.nbytes, f.ga[nst] = ngr; // (else entry max_reads is a start of its own)
    if (f.q.raw[0] != '>') f.q.ctl[1] = KR_FASTQ_NOT_CLEAN; // record 0: the chunk does not begin with a record start
  }
}

__global__ __launch_bounds__(256) void kr_fa_write_kernel(FaIO f)
{
  const uint64_t ntiles = (f.q.nbytes + kFqTile - 1) / kFqTile;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = t * kFqTile + 16u * threadIdx.x;
    FaMask m{0, 0, 0, 0};
    uint32_t st = 0;
    if (base < f.q.nbytes) m = fa_masks(f.q.raw, base, f.q.nbytes), st = fa_starts(f.q.raw, base, m);
    const uint32_t below = block_scan_excl((uint32_t)__popc(st) | ((uint32_t)__popc(m.gr) << 16)); // (both at most kFqTile)
    uint32_t idx = f.tile_st[t] + (below & 0xFFFFu);
    const uint32_t g0 = f.tile_gr[t] + (below >> 16);
    for (; st; st &= st - 1u, ++idx) {
      const uint32_t b = (uint32_t)__ffs(st) - 1u;
      if (idx <= f.q.max_reads) f.hs[idx] = (uint32_t)base + b, f.ga[idx] = g0 + (uint32_t)__popc(m.gr & ((1u << b) - 1u));
    }
  }
}

__global__ __launch_bounds__(256) void kr_fa_rec_kernel(FaIO f)
{
  const FqIO& q = f.q;
  const uint32_t nrec = fq_nrec(q), nst = (uint32_t)q.ctl[3], lane = lane_id();
  const uint32_t nw = gridDim.x * 4u;
  for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < nrec; r += nw) {
    const uint32_t start = f.hs[r], end = f.hs[r + 1];
    uint32_t he = end, ne = end, hg = 0;
    bool nul = false;
    for (uint32_t p0 = start; p0 < end; p0 += 64u) {
      const uint64_t p = (uint64_t)p0 + lane;
      const bool in = p < end;
      const uint32_t c = in ? q.raw[p] : 0u;
      const unsigned long long nlb = __ballot(in && c == '\n'), spb = __ballot(in && fq_isspace(c));
      const unsigned long long zb = __ballot(in && c == 0u), gb = __ballot(in && c - 33u <= 93u);
      const unsigned long long hdr = nlb ? (1ull << (__ffsll(nlb) - 1)) - 1ull : ~0ull; // the lanes in front of the header's '\n'
      if (ne == end) { // the name has not ended yet: it ends at the first isspace byte ('\n' is one)
        unsigned long long name = ~0ull;
        if (spb) ne = p0 + (uint32_t)__ffsll(spb) - 1u, name = (1ull << (__ffsll(spb) - 1)) - 1ull;
        nul = nul || (zb & name) != 0;
      }
      hg += (uint32_t)__popcll(gb & hdr);
      if (nlb) {
        he = p0 + (uint32_t)__ffsll(nlb) - 1u;
        break;
      }
      if (p0 > 0xFFFFFFFFu - 64u) break; // (a chunk may end 63 bytes below 4 GB: p0 must not wrap)
    }
    uint32_t status = 0;
    if (he == end) {
      status = KR_FASTQ_INCOMPLETE; // the header's '\n' is not in the chunk
    } else {
      const uint32_t slen = f.ga[r + 1] - f.ga[r] - hg;
      const uint32_t nkm = slen >= q.k ? slen - q.k + 1u : 0u;
      if (nul) status = KR_FASTQ_NOT_CLEAN;
      else if (r + 1u == nst && !f.closed) status = KR_FASTQ_INCOMPLETE; // nothing says where the chunk's last record ends
      else if (nkm > q.tile_min_pos) status = KR_FASTQ_LONG;
      if (lane == 0) q.rec_slen[r] = slen, q.rec_npos[r] = start + 1u, q.rec_nlen[r] = ne - start - 1u, f.rec_hg[r] = hg;
    }
    if (lane == 0) {
      f.rec_he[r] = he;
      if (status) atomicMin(&q.ctl[1], ((unsigned long long)r << 8) | status);
    }
  }
}

// the record of byte b of a lane's 16: (starts at or in front of it) - 1; 0xFFFFFFFF in front of the chunk's first start
__device__ __forceinline__ uint32_t fa_record(uint32_t starts_below, uint32_t st, uint32_t b) { return starts_below + (uint32_t)__popc(st & ((2u << b) - 1u)) - 1u; }

__global__ __launch_bounds__(256) void kr_fa_check_kernel(FaIO f)
{
  const FqIO& q = f.q;
  const uint32_t nrec = fq_nrec(q);
  const uint64_t ntiles = (q.nbytes + kFqTile - 1) / kFqTile;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = t * kFqTile + 16u * threadIdx.x;
    FaMask m{0, 0, 0, 0};
    uint32_t st = 0;
    if (base < q.nbytes) m = fa_masks(q.raw, base, q.nbytes), st = fa_starts(q.raw, base, m);
    const uint32_t below = f.tile_st[t] + block_scan_excl((uint32_t)__popc(st));
    for (uint32_t bad = m.bad & ~st; bad; bad &= bad - 1u) { // (rare: headers may hold these bytes, bodies of clean records do not)
      const uint32_t b = (uint32_t)__ffs(bad) - 1u, r = fa_record(below, st, b);
      if (r >= nrec || (uint32_t)base + b <= f.rec_he[r]) continue; // past the records checked, or a header byte
      const unsigned long long mine = ((unsigned long long)r << 8) | KR_FASTQ_NOT_CLEAN;
      if (mine < *(volatile unsigned long long*)&q.ctl[1]) atomicMin(&q.ctl[1], mine);
    }
  }
}

__global__ __launch_bounds__(256) void kr_fa_copy_kernel(FaIO f)
{
  __shared__ uint8_t s_out[kFqTile];
  __shared__ uint64_t s_d0;
  __shared__ uint32_t s_cnt;
  const FqIO& q = f.q;
  const unsigned long long bad = q.ctl[1];
  const uint32_t nscan = (uint32_t)q.ctl[2], nacc = (uint32_t)min((unsigned long long)nscan, bad >> 8), lane = lane_id();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    kr_fastq_parse s{};
    s.nreads = nacc;
    s.rejected = nacc;
    s.consumed = nacc ? f.hs[nacc] : 0u; // the first start that was not accepted, or the sentinel
    s.newlines = q.ctl[0];
    s.nbases = q.offsets[nacc];
    s.id_bytes = q.ids ? q.id_off[nacc] : 0u;
    if ((bad >> 8) <= nscan) s.status = (uint32_t)(bad & 0xFFu);
    else if (s.consumed == q.nbytes) s.status = KR_FASTQ_OK;
    else s.status = KR_FASTQ_CAPACITY; // (nacc == max_reads: more starts than a batch has reads)
    *q.sum = s;
  }
  const uint64_t ntiles = (q.nbytes + kFqTile - 1) / kFqTile;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = t * kFqTile + 16u * threadIdx.x;
    uint4 v = make_uint4(0, 0, 0, 0);
    FaMask m{0, 0, 0, 0};
    uint32_t st = 0;
    if (base < q.nbytes) v = *reinterpret_cast<const uint4*>(q.raw + base), m = fa_masks(q.raw, base, q.nbytes), st = fa_starts(q.raw, base, m);
    const uint32_t below = block_scan_excl((uint32_t)__popc(st) | ((uint32_t)__popc(m.gr) << 16));
    const uint32_t r0 = f.tile_st[t] + (below & 0xFFFFu), g0 = f.tile_gr[t] + (below >> 16);
    // the graphic bytes that are body bytes of an accepted record; `first`: where the lane's first one goes
    uint32_t keep = 0, rcur = 0xFFFFFFFFu, he = 0;
    uint64_t first = 0;
    bool acc = false;
    for (uint32_t g = m.gr; g; g &= g - 1u) {
      const uint32_t b = (uint32_t)__ffs(g) - 1u, r = fa_record(r0, st, b);
      if (r != rcur) {
        rcur = r, acc = r < nacc;
        he = acc ? f.rec_he[r] : 0u;
      }
      if (!acc || (uint32_t)base + b <= he) continue;
      if (!keep) first = q.offsets[r] + (uint64_t)(g0 + (uint32_t)__popc(m.gr & ((1u << b) - 1u)) - f.ga[r] - f.rec_hg[r]);
      keep |= 1u << b;
    }
    const uint32_t nk = (uint32_t)__popc(keep), k0 = block_scan_excl(nk);
    if (threadIdx.x == 255u) s_cnt = k0 + nk;
    if (nk && k0 == 0u) s_d0 = first; // (one lane: the tile's first kept byte)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o = k0;
#pragma unroll
    for (uint32_t b = 0; b < 16u; ++b)
      if ((keep >> b) & 1u) s_out[o++] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
    __syncthreads();
    // consecutive kept bytes go to consecutive places, across records too: the tile's kept bytes are one run of the batch's bases
    const uint32_t cnt = s_cnt;
    const uint64_t d0 = cnt ? s_d0 : 0u;
    for (uint32_t i = threadIdx.x; i < cnt; i += 256u)
      if (d0 + i < q.max_bases) q.bases[d0 + i] = s_out[i];
  }
  if (!q.ids) return;
  const uint32_t nw = gridDim.x * 4u;
  for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < nacc; r += nw) {
    const uint8_t* ns = q.raw + q.rec_npos[r];
    char* nd = q.ids + q.id_off[r];
    const uint32_t nl = q.rec_nlen[r];
    for (uint32_t i = lane; i < nl; i += 64u) nd[i] = (char)ns[i];
  }
}
