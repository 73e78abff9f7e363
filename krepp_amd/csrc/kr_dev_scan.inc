// kr_dev_scan.inc -- part of kr_device.hip (one translation unit, included in order): kernel 1: probe list, bucket scan, hit items.

// ---------------------------------------------------------------------------
// Probe list of one group (64 positions x 2 strands) and the bucket scan.
// ---------------------------------------------------------------------------
constexpr int kListCap = 128;
// The numbers of a scan shape (2^LOG_G lanes x CPL 16-byte chunks per probe), in one place for the kernels and for the host
// (kr_debug_scan_layout): words of a slot (2 header words + CAP entries), steps of scan_group before it flushes its hit bits.
constexpr uint32_t scan_slot_words(int log_g, int cpl) { return (1u << log_g) * (uint32_t)cpl * 4u; }
constexpr uint32_t scan_slot_cap(int log_g, int cpl) { return scan_slot_words(log_g, cpl) - 2u; }
constexpr uint32_t scan_step_bits(int cpl) { return 64u / (uint32_t)cpl * (uint32_t)cpl; }
struct ProbeList {
  lds_u64* bkt; // [128] (start << 24) | len
  lds_u32* q;   // [128] residual code of the query k-mer
  lds_u32* tag; // [128] pos | strand<<7 | lib<<8
};

struct Cand { // one lane's two candidate probes (forward, reverse) of a position
  uint64_t b0, b1;
  uint32_t q0, q1;
  uint32_t lib0, lib1;
};

// front end + descriptor loads for positions 64*pp + lane.  SLOT: the table has a slotted copy, the bucket is
// found by its row alone (b = 1 << 32 | row, no load here).
template <bool SL, bool SLOT>
__device__ __forceinline__ Cand fetch_group_fe(const DevIndex& ix, const FrontEnd& fe, uint32_t& nvalid)
{
  Cand c;
  nvalid = __popcll(__ballot(fe.valid));
  int lib = -1;
  c.b0 = 0, c.b1 = 0, c.lib0 = 0, c.lib1 = 0;
  c.q0 = fe.enc32[0];
  c.q1 = fe.enc32[1];
  // Sparse tables (a small index in a 2^21..2^25-row table: most buckets are empty) carry one bit per row, a bitmap
  // of a few hundred KB that lives in L2: an empty bucket costs no descriptor fetch from HBM / the Infinity Cache --
  // on the 25-reference index two probes in three, and the kernel runs at the fabric's request rate there.
  const uint32_t* d0 = nullptr;
  const uint32_t* d1 = nullptr; // (both bitmap words are requested before either descriptor)
  uint32_t row0 = 0, row1 = 0, w0 = 0xFFFFFFFFu, w1 = 0xFFFFFFFFu;
  const bool l0 = fe.valid && locate_row<SL>(ix, fe.rix[0], lib, row0);
  if (l0) {
    c.lib0 = (uint32_t)lib;
    if (!SLOT) d0 = get_lib<SL>(ix, (uint32_t)lib).occ;
  }
  const bool l1 = fe.valid && locate_row<SL>(ix, fe.rix[1], lib, row1);
  if (l1) {
    c.lib1 = (uint32_t)lib;
    if (!SLOT) d1 = get_lib<SL>(ix, (uint32_t)lib).occ;
  }
  if (!SLOT) {
    if (d0) w0 = d0[row0 >> 5];
    if (d1) w1 = d1[row1 >> 5];
  }
  if (l0) c.b0 = SLOT ? (1ull << 32) | row0 : (((w0 >> (row0 & 31u)) & 1u) ? get_lib<SL>(ix, c.lib0).bkt[row0] : 0ull);
  if (l1) c.b1 = SLOT ? (1ull << 32) | row1 : (((w1 >> (row1 & 31u)) & 1u) ? get_lib<SL>(ix, c.lib1).bkt[row1] : 0ull);
  return c;
}
template <bool SL, bool SLOT>
__device__ __forceinline__ Cand fetch_group(const DevIndex& ix, const SegBits& sb, int pp, uint32_t npos_seg, uint32_t& nvalid)
{
  return fetch_group_fe<SL, SLOT>(ix, front_end(ix, sb, pp, npos_seg), nvalid);
}
template <bool SL, bool SLOT> // pp wave-uniform at run time
__device__ __forceinline__ Cand fetch_group_sel(const DevIndex& ix, const SegBits& sb, uint32_t pp, uint32_t npos_seg, uint32_t& nvalid)
{
  return fetch_group_fe<SL, SLOT>(ix, front_end_sel(ix, sb, pp, npos_seg), nvalid);
}

// the same for a slotted table through the byte-table front end (kr_dev_common.inc: front_end_tab)
template <bool SL>
__device__ __forceinline__ Cand fetch_group_tab(const DevIndex& ix, const lds_u32x4* tab, const SegBits& sb, uint32_t pp, uint32_t npos_seg, uint32_t& nvalid)
{
  return fetch_group_fe<SL, true>(ix, front_end_tab_sel(ix, tab, sb, pp, npos_seg), nvalid);
}
// the same for a slotted table through the bit-plane front end (kr_dev_common.inc: front_end_planes)
template <bool SL>
__device__ __forceinline__ Cand fetch_group_planes(const DevIndex& ix, const SegBits& sb, uint32_t pp, uint32_t npos_seg, uint32_t& nvalid)
{
  const PlaneFe fe = front_end_planes(ix, sb, pp, npos_seg);
  nvalid = (uint32_t)__popcll(fe.valid);
  const bool valid = ((fe.valid >> lane_id()) & 1ull) != 0ull;
  Cand c;
  c.b0 = 0, c.b1 = 0, c.lib0 = 0, c.lib1 = 0;
  c.q0 = fe.enc32[0];
  c.q1 = fe.enc32[1];
  int lib = -1;
  uint32_t row = 0;
  if (valid && locate_row<SL>(ix, fe.rix[0], lib, row)) c.b0 = (1ull << 32) | row, c.lib0 = (uint32_t)lib;
  if (valid && locate_row<SL>(ix, fe.rix[1], lib, row)) c.b1 = (1ull << 32) | row, c.lib1 = (uint32_t)lib;
  return c;
}

// 4 entries of one 16-byte chunk against the query code.  `lo`/`hi` bound the entries of the chunk
// that belong to the bucket (0..4).  Returns the 4-bit hit mask; hds = 4 x 8-bit Hamming distances.
__device__ __forceinline__ uint32_t chunk_hits(uint4 v, int lo, int hi, uint32_t q, uint32_t th, uint32_t& hds)
{
  uint32_t h0 = hd_lr32(v.x, q), h1 = hd_lr32(v.y, q), h2 = hd_lr32(v.z, q), h3 = hd_lr32(v.w, q);
  hds = h0 | (h1 << 8) | (h2 << 16) | (h3 << 24);
  uint32_t m = (h0 <= th ? 1u : 0u) | (h1 <= th ? 2u : 0u) | (h2 <= th ? 4u : 0u) | (h3 <= th ? 8u : 0u);
  lo = max(lo, 0), hi = min(hi, 4);
  uint32_t in = hi > lo ? (((1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u;
  return m & in;
}

// ---------------------------------------------------------------------------
// Kernel 1: the table scan.  One wave per read; per group of 64 positions the wave builds the probe
// list (front end + bucket descriptors) and scans the listed buckets: G = 2^LOG_G consecutive lanes
// share one probe and read consecutive aligned 16-byte chunks of its bucket (G*16 contiguous bytes per
// step), 64/G probes per pass, CPL chunks per lane per pass.  No search, no prefix sums: the probe of a
// lane is fixed by its lane id.  A pass covers G*CPL*4 entries of each bucket; longer buckets take
// extra rounds.  The kernel keeps no accumulator state, so it runs at 8 waves per SIMD and hides the
// HBM latency of its dependent steps (descriptor -> bucket -> colour) by occupancy alone.
//
// The scan proper only asks, per chunk, "is the smallest of the four Hamming distances within th?"
// (hits are ~1 % of the entries) and keeps the answers as one bit per (pass, chunk) in a per-lane
// register.  After the group's last pass the hit chunks of all lanes are dealt out again, one per
// lane: the lane re-reads its chunk (L2), applies the bucket bounds, fetches the colour of every
// matching entry and appends (colour, tag) items to the read's item list in HBM, which the
// accumulate kernel consumes.
// ---------------------------------------------------------------------------
struct ScanWave {
  uint32_t it_next, it_end; // wave-private range of item slots (wave-uniform)
  uint32_t rd_start;        // first item of the current read
  uint32_t err;
  uint32_t filt0, filt1;    // per-lane running min hd per strand (hdist_filt, src/query.cpp:366-368)
  uint32_t cur_seg;         // segment of the read's most recent item (wave-uniform)
  uint32_t n_st;            // items of the current read waiting in the wave's LDS stage (wave-uniform)
  lds_u64* stage;           // [kItemStage] x | y << 32
};
// A read's items wait in LDS and leave together when the read is done (or the stage is full): whole 128-byte lines from a
// 128-byte aligned start, where every hit chunk used to append its few 8-byte items on its own -- a trickle of partial-line
// writes into a kernel at the HBM wall, whose cost depended on where the stream's item buffer happened to lie (the same
// launch took 42.6 or 48.6 ms from stream to stream).
constexpr uint32_t kItemStage = 256;
#ifndef KR_ITEM_CHUNK
#define KR_ITEM_CHUNK 2048
#endif
constexpr uint32_t kItemChunk = KR_ITEM_CHUNK; // item slots a wave takes from the shared counter at a time
#ifndef KR_SCAN_READ_CHUNK
#define KR_SCAN_READ_CHUNK 32
#endif
// reads a wave takes per visit to a read cursor; their per-read results (item range, valid k-mers, hdist_filt) wait in LDS and
// leave together at the end of the visit -- 32 consecutive reads are whole 128-byte lines of each array, where one read at a
// time was five scattered 4-byte stores: 40 M partial-line writes per 8 M reads trickling into a kernel at the HBM wall
constexpr uint32_t kReadChunk = KR_SCAN_READ_CHUNK;
// Reads are handed out in small chunks (heavy reads do not pile up on one wave, no tail).  One shared
// cursor would serve only ~90 M atomics/s -- 1.4 ms for a million reads -- so the batch is cut into
// kCursors ranges with a cursor each (on cache lines of their own); a wave starts on its "home" range
// and moves on to the next when that is used up.
constexpr uint32_t kCursors = 32, kCursorStride = 32; // words
struct ReadCursor {
  uint32_t* cur;   // [kCursors * kCursorStride]
  uint32_t nreads, range, c, tried, chunk;
  __device__ __forceinline__ void init(uint32_t* base, uint32_t n, uint32_t home, uint32_t reads_per_visit = kReadChunk)
  {
    cur = base, nreads = n, range = (n + kCursors - 1) / kCursors, c = home % kCursors, tried = n ? 0 : kCursors, chunk = reads_per_visit;
  }
  // next chunk [r0, r1); false when every range is used up (wave-uniform)
  __device__ __forceinline__ bool next(uint32_t& r0, uint32_t& r1)
  {
    while (tried < kCursors) {
      const uint32_t lo = c * range, hi = min(lo + range, nreads);
      uint32_t o = 0;
      if (lane_id() == 0) o = atomicAdd(&cur[c * kCursorStride], chunk);
      o = __shfl(o, 0);
      if (lo + o < hi) {
        r0 = lo + o, r1 = min(r0 + chunk, hi);
        return true;
      }
      c = (c + 1) % kCursors, ++tried;
    }
    return false;
  }
};

// Make room for n more items directly behind the current read's items (wave-uniform).
__device__ __forceinline__ bool item_reserve(const BatchOut& out, ScanWave& sw, uint32_t n)
{
  if (sw.it_next + n <= sw.it_end) return true;
  const uint32_t have = sw.it_next - sw.rd_start;
  const uint32_t size = (have + n + kItemChunk + 15u) & ~15u; // (chunks start on 128-byte lines)
  uint32_t base = 0;
  if (lane_id() == 0) base = atomicAdd(&out.counters[kCtItemSlots], size);
  base = __shfl(base, 0);
  if ((uint64_t)base + size > out.item_cap) {
    sw.err |= kErrItemCap;
    return false;
  }
  if (have) { // the read's items so far move to the new chunk (they were written by this wave: read them from L2)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (uint32_t i = lane_id(); i < have; i += 64) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(out.items + sw.rd_start + i);
      out.items[base + i] = make_uint2(gload(src), gload(src + 1));
    }
  }
  sw.rd_start = base;
  sw.it_next = base + have;
  sw.it_end = base + size;
  return true;
}

__device__ __forceinline__ void flush_stage(const BatchOut& out, ScanWave& sw)
{
  if (sw.n_st == 0) return;
  WAVE_SYNC();
  const uint32_t n16 = (sw.n_st + 15u) & ~15u; // the last line is written whole too (its tail is never read: the next read starts on the next line)
  if (item_reserve(out, sw, n16)) {
    for (uint32_t i = lane_id(); i < n16; i += 64) {
      const uint64_t v = i < sw.n_st ? sw.stage[i] : 0ull;
      out.items[sw.it_next + i] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
    sw.it_next += sw.n_st;
  }
  sw.n_st = 0;
  WAVE_SYNC();
}

// Entries `pend` (4-bit mask) of chunk c of the bucket at e_al matched: append one item per entry.  The item
// names the entry (its colour id is fetched by the accumulate kernel: this kernel runs at the chip's
// random-request rate, that one has memory bandwidth to spare).  Reads of more than one segment get a
// marker item in front of the first item of every later segment.
constexpr uint32_t kItemMarker = 0x80000000u;
// FK: the batch's items are in the filter-slot form (kr_dev_common.inc: BatchOut::items); these are verified entries of the
// packed arrays (hd12 field = 7, hd in bits 15..19, index high bits from bit 23)
template <bool SL, bool TAP, bool FK = false>
__device__ __forceinline__ void emit_hits(const DevIndex& ix, const BatchOut& out, ScanWave& sw, uint32_t read, uint32_t base0,
                                          uint32_t tg, uint64_t e_al, uint32_t c, uint32_t pend, uint32_t hds)
{
  const uint64_t lt = (1ull << lane_id()) - 1ull;
  const uint32_t seg = base0 >> 7;
  while (__ballot(pend != 0) != 0) {
    const bool has = pend != 0;
    const uint32_t e = has ? (uint32_t)__ffs((int)pend) - 1u : 0u;
    const uint32_t hd = (hds >> (8u * e)) & 31u;
    const uint64_t idx = e_al + 4ull * c + e;
    if (has) {
      if (tag_strand(tg))
        sw.filt1 = min(sw.filt1, hd);
      else
        sw.filt0 = min(sw.filt0, hd);
      if (TAP) {
        const uint32_t se = get_lib<SL>(ix, tag_lib(tg)).se[idx];
        const uint32_t hix = atomicAdd(&out.counters[kCtTapHits], 1u);
        if (hix < out.hit_cap) {
          kr_hit h;
          h.read = read;
          h.kpos = base0 + tag_pos(tg);
          h.strand = tag_strand(tg);
          h.lib = tag_lib(tg);
          h.cmer_index = idx;
          h.hd = hd;
          h.se = (se >> 30) == 1u ? ix.leaf_se[se & kColMask] : (se & kColMask);
          out.hits[hix] = h;
        } else {
          atomicOr(&out.counters[kCtErr], kErrHitCap);
        }
      }
    }
    const uint64_t hm = __ballot(has);
    const uint32_t mark = seg != sw.cur_seg ? 1u : 0u; // wave-uniform
    if (sw.n_st + (uint32_t)__popcll(hm) + mark > kItemStage) flush_stage(out, sw); // (a read of more than 256 items)
    if (mark && lane_id() == 0) sw.stage[sw.n_st] = (uint64_t)seg | ((uint64_t)kItemMarker << 32);
    sw.n_st += mark;
    sw.cur_seg = seg;
    if (has)
      sw.stage[sw.n_st + __popcll(hm & lt)] =
        (uint64_t)(uint32_t)idx | ((uint64_t)(FK ? ((tg & 0xFFFu) | (7u << 12) | (hd << 15) | ((uint32_t)(idx >> 32) << 23))
                                                 : ((tg & 0xFFFu) | (hd << 12) | ((uint32_t)(idx >> 32) << 17))) << 32);
    sw.n_st += (uint32_t)__popcll(hm);
    pend &= pend - 1u;
  }
}

// Scan of one group's probe list.  Step s of the scan = (pass p0, chunk block cb): lane l looks at chunk
// (l mod G) + cb*G of probe p0 + l/G and records in bit s of `hitbits` whether it holds an entry
// within th; stepinfo[s] (LDS, wave-uniform) remembers (p0, cb*G).  When the group is done -- or the
// bits are used up, for very long buckets -- the hit chunks are dealt out and resolved.
template <int LOG_G, int CPL, bool SL, bool TAP>
__device__ __forceinline__ void scan_group(const DevIndex& ix, const DevParams& P, const BatchOut& out, ScanWave& sw,
                                           const ProbeList& pl, lds_u32* queue, lds_u32* stepinfo, uint32_t nact, uint32_t read,
                                           uint32_t base0)
{
  constexpr uint32_t G = 1u << LOG_G, PPS = 64u >> LOG_G;
  constexpr uint32_t kBits = scan_step_bits(CPL); // steps per flush
  const uint32_t lane = lane_id(), sub = lane & (G - 1u);
  uint32_t p0 = 0, cb = 0; // scan position: pass start, chunk block (units of G chunks)
  while (p0 < nact) {
    // ---- scan until the group is done or the step bits are used up
    uint64_t hitbits = 0;
    uint32_t step = 0;
    while (p0 < nact && step < kBits) {
      const uint32_t pi = p0 + (lane >> LOG_G);
      const bool on = pi < nact;
      const uint64_t b = on ? pl.bkt[pi] : 0ull;
      const uint32_t q = on ? pl.q[pi] : 0u;
      const uint64_t st = b >> 24;
      const uint32_t tot = (uint32_t)(st & 3u) + (uint32_t)(b & 0xFFFFFFu);
      const uint32_t nch = on ? (tot + 3u) >> 2 : 0u;
      const uint32_t* enc = get_lib<SL>(ix, SL ? 0u : tag_lib(pl.tag[on ? pi : 0u])).enc + (st & ~3ull);
      for (; step < kBits && __ballot(sub + cb * G < nch) != 0; cb += CPL, step += CPL) {
        if (lane < (uint32_t)CPL) stepinfo[step + lane] = p0 | (((cb + lane) * G) << 8);
        // (loads stay masked for chunks past the end of the bucket: clamping them onto the last chunk instead
        //  saves instructions but costs 20 % in run time -- the extra lanes load the texture path)
        uint4 v[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const uint32_t c = sub + (cb + (uint32_t)j) * G;
          v[j] = make_uint4(0, 0, 0, 0);
          if (c < nch) v[j] = *reinterpret_cast<const uint4*>(enc + 4u * c);
        }
        // entries of the neighbouring buckets in the first / last chunk may give false positives, rejected below
        uint32_t r = 0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const uint32_t m = min(min(hd_lr32(v[j].x, q), hd_lr32(v[j].y, q)), min(hd_lr32(v[j].z, q), hd_lr32(v[j].w, q)));
          r |= (m <= P.th && sub + (cb + (uint32_t)j) * G < nch) ? (1u << j) : 0u;
        }
        hitbits |= (uint64_t)r << step;
      }
      if (__ballot(sub + cb * G < nch) == 0) p0 += PPS, cb = 0; // pass finished
    }
    if (P.dbg & 1u) hitbits = 0;
    // ---- deal the hit chunks out, 64 at a time: re-read the chunk, apply the bucket bounds, emit
    const uint32_t cnt = (uint32_t)__popcll(hitbits);
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= (uint32_t)d) inc += o;
    }
    const uint32_t H = __shfl(inc, 63);
    uint64_t hb = hitbits;
    uint32_t slot = inc - cnt;
    WAVE_SYNC();
    for (uint32_t w0 = 0; w0 < H; w0 += 64) {
      while (__ballot(hb != 0 && slot < w0 + 64u) != 0) {
        if (hb != 0 && slot < w0 + 64u) {
          const uint32_t si = stepinfo[(uint32_t)__ffsll((long long)hb) - 1u];
          queue[slot - w0] = ((si & 255u) + (lane >> LOG_G)) | ((sub + (si >> 8)) << 8);
          hb &= hb - 1;
          ++slot;
        }
      }
      WAVE_SYNC();
      uint32_t pend = 0, hds = 0, tg = 0, c = 0;
      uint64_t e_al = 0;
      if (lane < min(64u, H - w0)) {
        const uint32_t d = queue[lane], probe = d & 255u;
        c = d >> 8;
        const uint64_t b = pl.bkt[probe];
        const uint32_t q = pl.q[probe];
        tg = pl.tag[probe];
        const uint64_t st = b >> 24;
        e_al = st & ~3ull;
        const int rel0 = (int)(st & 3u), tot = rel0 + (int)(uint32_t)(b & 0xFFFFFFu);
        const uint4 v = *reinterpret_cast<const uint4*>(get_lib<SL>(ix, tag_lib(tg)).enc + e_al + 4u * c);
        pend = chunk_hits(v, rel0 - 4 * (int)c, tot - 4 * (int)c, q, P.th, hds);
      }
      WAVE_SYNC();
      emit_hits<SL, TAP>(ix, out, sw, read, base0, tg, e_al, c, pend, hds);
    }
  }
}

// Scan of one group's probe list through the SLOTTED table (dense tables): row r owns an aligned slot of
// W = G*CPL*4 words = {bucket length, packed start index, the first W-2 residual codes}.  One pass reads the
// whole slot of 64/G probes -- no descriptor gather in front (one dependent HBM round trip and one
// L2->fabric request per probe less: the kernel runs at the chip's random-request rate), always the same
// two lines per probe.  The two header words take part in the hit test like entries and are rejected, like
// every entry beyond the bucket's length, when the hit chunks are resolved.  The rest of a bucket longer than
// W-2 entries is read from the packed array and resolved on the spot.
template <int LOG_G, int CPL, bool SL, bool TAP>
__device__ __forceinline__ void scan_group_slots(const DevIndex& ix, const DevParams& P, const BatchOut& out, ScanWave& sw,
                                                 const ProbeList& pl, lds_u32* queue, uint32_t nact, uint32_t read, uint32_t base0)
{
  constexpr uint32_t G = 1u << LOG_G, PPS = 64u >> LOG_G, W = scan_slot_words(LOG_G, CPL), CAP = scan_slot_cap(LOG_G, CPL);
  static_assert((kListCap / PPS) * CPL <= 64, "one hit bit per (pass, chunk)");
  const uint32_t lane = lane_id(), sub = lane & (G - 1u);
  uint64_t hitbits = 0;
  uint32_t step = 0;
  for (uint32_t p0 = 0; p0 < nact; p0 += PPS, step += CPL) {
    const uint32_t pi = p0 + (lane >> LOG_G);
    const bool on = pi < nact;
    const uint32_t row = on ? (uint32_t)pl.bkt[pi] : 0u;
    const uint32_t q = on ? pl.q[pi] : 0u;
    const DevLib L = get_lib<SL>(ix, SL ? 0u : tag_lib(pl.tag[on ? pi : 0u]));
    const uint32_t* slot = L.slots + (uint64_t)row * W;
    uint4 v[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      v[j] = make_uint4(0, 0, 0, 0);
      if (on) v[j] = *reinterpret_cast<const uint4*>(slot + 4u * (sub + (uint32_t)j * G));
    }
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const uint32_t m = min(min(hd_lr32(v[j].x, q), hd_lr32(v[j].y, q)), min(hd_lr32(v[j].z, q), hd_lr32(v[j].w, q)));
      r |= (m <= P.th && on) ? (1u << j) : 0u;
    }
    hitbits |= (uint64_t)r << step;
    // ---- buckets longer than the slot: the rest from the packed array, resolved on the spot
    if (__ballot(on && sub == 0 && v[0].x > CAP) != 0) {
      const uint32_t blen = __shfl(v[0].x, lane & ~(G - 1u)), bstart = __shfl(v[0].y, lane & ~(G - 1u));
      const bool lg = on && blen > CAP;
      const uint64_t st = (uint64_t)bstart + CAP;
      const uint64_t e_al = st & ~3ull;
      const int rel0 = (int)(st & 3u), tot = rel0 + (lg ? (int)(blen - CAP) : 0);
      const uint32_t nch = lg ? (uint32_t)(tot + 3) >> 2 : 0u;
      const uint32_t tg = pl.tag[on ? pi : 0u];
      for (uint32_t c = sub; __ballot(c < nch) != 0; c += G) {
        uint32_t pend = 0, hds = 0;
        if (c < nch) {
          const uint4 w = *reinterpret_cast<const uint4*>(L.enc + e_al + 4u * c);
          pend = chunk_hits(w, rel0 - 4 * (int)c, tot - 4 * (int)c, q, P.th, hds);
        }
        if (P.dbg & 1u) pend = 0;
        emit_hits<SL, TAP>(ix, out, sw, read, base0, tg, e_al, c, pend, hds);
      }
    }
  }
  if (P.dbg & 1u) hitbits = 0;
  // ---- deal the hit chunks out, 64 at a time: re-read header + chunk, apply the bucket bounds, emit
  const uint32_t cnt = (uint32_t)__popcll(hitbits);
  uint32_t inc = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= (uint32_t)d) inc += o;
  }
  const uint32_t H = __shfl(inc, 63);
  uint64_t hb = hitbits;
  uint32_t slot_i = inc - cnt;
  for (uint32_t w0 = 0; w0 < H; w0 += 64) {
    while (__ballot(hb != 0 && slot_i < w0 + 64u) != 0) {
      if (hb != 0 && slot_i < w0 + 64u) {
        const uint32_t bit = (uint32_t)__ffsll((long long)hb) - 1u;
        const uint32_t pass = bit / (uint32_t)CPL, j = bit - pass * (uint32_t)CPL;
        queue[slot_i - w0] = (pass * PPS + (lane >> LOG_G)) | ((sub + j * G) << 8);
        hb &= hb - 1;
        ++slot_i;
      }
    }
    WAVE_SYNC();
    uint32_t pend = 0, hds = 0, tg = 0, c = 0;
    uint64_t e_al = 0;
    if (lane < min(64u, H - w0)) {
      const uint32_t d = queue[lane], probe = d & 255u;
      c = d >> 8;
      const uint32_t row = (uint32_t)pl.bkt[probe];
      const uint32_t q = pl.q[probe];
      tg = pl.tag[probe];
      const uint32_t* slot = get_lib<SL>(ix, tag_lib(tg)).slots + (uint64_t)row * W;
      const uint2 hdr = *reinterpret_cast<const uint2*>(slot);
      const uint4 v = *reinterpret_cast<const uint4*>(slot + 4u * c);
      // word 4c+e of the slot is entry 4c+e-2 of the bucket = packed index start + 4c+e-2
      const int nin = (int)min(hdr.x, CAP);
      pend = chunk_hits(v, 2 - 4 * (int)c, nin + 2 - 4 * (int)c, q, P.th, hds);
      e_al = (uint64_t)hdr.y - 2ull;
    }
    WAVE_SYNC();
    emit_hits<SL, TAP>(ix, out, sw, read, base0, tg, e_al, c, pend, hds);
  }
}

template <int LOG_G, int CPL, bool SL, bool TAP, bool SLOT>
__device__ __forceinline__ void scan_read(const DevIndex& ix, const DevParams& P, const BatchIn& in, const BatchOut& out,
                                          uint32_t read, ScanWave& sw, const ProbeList& pl, lds_u32* queue, lds_u32* stepinfo, lds_u32* meta)
{
  const uint32_t lane = lane_id();
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint64_t off0 = in.offsets[read], off1 = in.offsets[read + 1];
  const uint8_t* seq = in.bases + off0;
  const uint64_t len = off1 - off0;
  const uint32_t k = ix.k;
  const uint64_t nkm = len >= k ? len - k + 1 : 0; // enmers (src/query.cpp:42)
  uint32_t onmers = 0;
  sw.it_next = min((sw.it_next + 15u) & ~15u, sw.it_end); // the read's items start on a 128-byte line
  sw.rd_start = sw.it_next;
  sw.n_st = 0;
  sw.cur_seg = 0;
  sw.filt0 = 0xFFFFFFFFu, sw.filt1 = 0xFFFFFFFFu;
  for (uint64_t base0 = 0; base0 < nkm; base0 += kSegPos) {
    const uint32_t npos_seg = (uint32_t)min((uint64_t)kSegPos, nkm - base0);
    SegBits sb;
    load_segment(seq, len, base0, sb);
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) { // unrolled: SegBits stays in scalar registers
      if (pp == 1 && npos_seg <= 64) break;
      uint32_t nv = 0;
      const Cand cur = fetch_group<SL, SLOT>(ix, sb, pp, npos_seg, nv);
      onmers += nv;
      // ---- compact the non-empty probes of this group into the LDS list (slotted: every located probe)
      const bool a0 = SLOT ? cur.b0 != 0 : (cur.b0 & 0xFFFFFFu) != 0, a1 = SLOT ? cur.b1 != 0 : (cur.b1 & 0xFFFFFFu) != 0;
      const uint64_t m0 = __ballot(a0), m1 = __ballot(a1);
      const uint32_t n0 = __popcll(m0), nact = n0 + __popcll(m1);
      if (a0) {
        const uint32_t i = __popcll(m0 & lt);
        pl.bkt[i] = cur.b0;
        pl.q[i] = cur.q0;
        pl.tag[i] = (64u * pp + lane) | (cur.lib0 << 8);
      }
      if (a1) {
        const uint32_t i = n0 + __popcll(m1 & lt);
        pl.bkt[i] = cur.b1;
        pl.q[i] = cur.q1;
        pl.tag[i] = (64u * pp + lane) | (1u << 7) | (cur.lib1 << 8);
      }
      WAVE_SYNC();
      if (!(P.dbg & 4u)) {
        if (SLOT)
          scan_group_slots<LOG_G, CPL, SL, TAP>(ix, P, out, sw, pl, queue, nact, read, (uint32_t)base0);
        else
          scan_group<LOG_G, CPL, SL, TAP>(ix, P, out, sw, pl, queue, stepinfo, nact, read, (uint32_t)base0);
      }
      WAVE_SYNC();
    }
  }
  flush_stage(out, sw);
  // ---- per-strand hdist_filt = min hd over kept table entries (src/query.cpp:366-368)
  uint32_t f0 = sw.filt0, f1 = sw.filt1;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    f0 = min(f0, (uint32_t)__shfl_xor(f0, d));
    f1 = min(f1, (uint32_t)__shfl_xor(f1, d));
  }
  if (lane == 0) { // (slot of this read within the visit: see the kernel)
    meta[0 * kReadChunk] = sw.rd_start;
    meta[1 * kReadChunk] = sw.it_next - sw.rd_start;
    meta[2 * kReadChunk] = onmers;
    meta[3 * kReadChunk] = f0;
    meta[4 * kReadChunk] = f1;
  }
}

#ifndef KR_SCAN_WPE
#define KR_SCAN_WPE 6 // resident scan waves per SIMD the register allocation is sized for (8 spills, 5 hides less latency)
#endif
#ifndef KR_SCAN_WPE_SLOT
#define KR_SCAN_WPE_SLOT 4 // ... of the slotted variant (one more chunk per lane; 5: 6.0 ms, 6 spills: 7.3 ms, 4: 5.6 ms)
#endif
constexpr int kScanWaves = 4; // waves per workgroup of the scan kernel (they share nothing)
template <int LOG_G, int CPL, bool SL, bool TAP, bool SLOT>
__global__ __launch_bounds__(kScanWaves* kWave, (SLOT ? KR_SCAN_WPE_SLOT : KR_SCAN_WPE)) void kr_scan_kernel_t(DevIndex ix, DevParams P, BatchIn in, BatchOut out)
{
  __shared__ __attribute__((aligned(16))) uint64_t s_bkt[kScanWaves][kListCap];
  __shared__ uint32_t s_q[kScanWaves][kListCap], s_tag[kScanWaves][kListCap], s_queue[kScanWaves][64], s_step[kScanWaves][64];
  __shared__ uint32_t s_meta[kScanWaves][5 * kReadChunk];
  __shared__ __attribute__((aligned(16))) uint64_t s_stage[kScanWaves][kItemStage];
  static_assert(kReadChunk <= 64, "one lane per read of a visit");
  const uint32_t w = threadIdx.x / kWave;
  ProbeList pl{(lds_u64*)s_bkt[w], (lds_u32*)s_q[w], (lds_u32*)s_tag[w]};
  lds_u32* queue = (lds_u32*)s_queue[w];
  lds_u32* stepinfo = (lds_u32*)s_step[w];
  ScanWave sw;
  sw.it_next = sw.it_end = sw.rd_start = 0;
  sw.err = 0;
  sw.cur_seg = 0;
  sw.n_st = 0;
  sw.stage = (lds_u64*)s_stage[w];
  sw.filt0 = sw.filt1 = 0xFFFFFFFFu;
  ReadCursor rc;
  rc.init(out.cursors + kCurScan * kCursors * kCursorStride, in.nreads, blockIdx.x * kScanWaves + w);
  uint32_t r0, r1;
  lds_u32* meta = (lds_u32*)s_meta[w];
  while (rc.next(r0, r1)) {
    for (uint32_t r = r0; r < r1; ++r) scan_read<LOG_G, CPL, SL, TAP, SLOT>(ix, P, in, out, r, sw, pl, queue, stepinfo, meta + (r - r0));
    WAVE_SYNC();
    const uint32_t l = lane_id();
    if (l < r1 - r0) {
      out.rd_it_off[r0 + l] = meta[0 * kReadChunk + l];
      out.rd_it_cnt[r0 + l] = meta[1 * kReadChunk + l];
      out.rd_onmers[r0 + l] = meta[2 * kReadChunk + l];
      reinterpret_cast<uint2*>(out.rd_filt)[r0 + l] = make_uint2(meta[3 * kReadChunk + l], meta[4 * kReadChunk + l]);
    }
    WAVE_SYNC();
  }
  if (sw.err && lane_id() == 0) atomicOr(&out.counters[kCtErr], sw.err);
}

