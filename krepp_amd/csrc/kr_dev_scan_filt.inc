// kr_dev_scan_filt.inc -- part of kr_device.hip (included after kr_dev_scan_pipe.inc): the scan of FILTER slots (format 9,
// kr_dev_common.inc) -- one 128-byte line per probe instead of two.
//
// Same software pipeline across probe groups as kr_scan_pipe_kernel_t (front end + probe list of the next group while the
// loads of this one are in flight; hit chunks dealt out and re-read from the L2 while the next group's loads are in
// flight), with one more kind of group: while a group's first lines are tested, the probes whose bucket goes on in the second
// line (bit 7 of the chunks' count bytes: 28 % of the probes on the 10 GB table) are listed in a third LDS list, and that
// list is scanned as a group of its own -- second lines, same read, same segment -- before the pipeline moves on to the next
// group.  A dependent load, but never one a wave waits for on the spot.
//
// What leaves the kernel are CANDIDATES: entries within th on the 12 positions their 24-bit code covers.  The item names
// the entry's place in the slot (row * 80 + e: its colour and rest bits lie at sx[that]) and carries hd12 and the query's rest
// bits; kr_acc_kernel_t<..., FK = true> completes hd beside its colour gather, drops the false candidates and takes the
// read's hdist_filt (src/query.cpp:366-368) from the true hits.  Buckets of more than 80 entries continue in the packed
// arrays: their tail is scanned on the spot with the full codes, and those items are marked as verified.
// Semantics (src/query.cpp:352-368): the union of a read's true hits is what scan_read<..., SLOT> finds.

// candidates of one chunk: 5-bit mask of the valid codes within th on their 12 positions; hds = 5 x 4-bit hd12
__device__ __forceinline__ uint32_t filt_chunk_cands(uint4 v, uint32_t q24, uint32_t th, uint32_t& hds)
{
  const uint32_t cnt = (v.w >> 24) & 7u;
  const uint32_t h0 = hd_code24(v.x, q24), h1 = hd_code24(__builtin_amdgcn_alignbit(v.y, v.x, 24), q24),
                 h2 = hd_code24(__builtin_amdgcn_alignbit(v.z, v.y, 16), q24), h3 = hd_code24(v.z >> 8, q24), h4 = hd_code24(v.w, q24);
  hds = h0 | (h1 << 4) | (h2 << 8) | (h3 << 12) | (h4 << 16);
  const uint32_t m = (h0 <= th ? 1u : 0u) | (h1 <= th ? 2u : 0u) | (h2 <= th ? 4u : 0u) | (h3 <= th ? 8u : 0u) | (h4 <= th ? 16u : 0u);
  return m & ((1u << cnt) - 1u);
}
// ... is there one at all? (the hit test proper: the codes beyond the count are 0xFFFFFF and the count bounds them again when
// the chunk is resolved)
__device__ __forceinline__ bool filt_chunk_any(uint4 v, uint32_t q24, uint32_t th)
{
  const uint32_t m = min(min(min(hd_code24(v.x, q24), hd_code24(__builtin_amdgcn_alignbit(v.y, v.x, 24), q24)),
                             min(hd_code24(__builtin_amdgcn_alignbit(v.z, v.y, 16), q24), hd_code24(v.z >> 8, q24))),
                         hd_code24(v.w, q24));
  return m <= th && ((v.w >> 24) & 7u) != 0u;
}

struct FiltGroup { // wave-uniform
  uint32_t nact, read, base0, slot, line;
  bool last;
};

// the loads of passes [c * DEPTH, (c + 1) * DEPTH) of a group: 4 lanes per probe, 2 chunks per lane = one 128-byte line
template <int DEPTH, bool SL>
__device__ __forceinline__ void filt_issue(const DevIndex& ix, const SlotList& L, uint32_t nact, uint32_t line, uint32_t c, uint4 (&v)[DEPTH * 2])
{
  const uint32_t lane = lane_id(), sub = lane & 3u;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    const uint32_t pi = (c * DEPTH + (uint32_t)d) * 16u + (lane >> 2);
    const bool on = pi < nact;
    const uint32_t row = on ? L.row[pi] : 0u;
    const uint32_t* slot = get_lib<SL>(ix, SL ? 0u : tag_lib(L.tag[on ? pi : 0u])).slots + (uint64_t)row * 64u + 32u * line;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      v[d * 2 + j] = make_uint4(0, 0, 0, 0);
      if (on) v[d * 2 + j] = *reinterpret_cast<const uint4*>(slot + 4u * (sub + (uint32_t)j * 4u));
    }
  }
}

// Candidates `pend` (5-bit mask) of chunk `cidx` of line `line` of row `row`: one item per entry.  TAP (tests): the kernel
// verifies the candidate itself and reports the true hits (the items are what they are either way).
template <bool SL, bool TAP>
__device__ __forceinline__ void filt_emit(const DevIndex& ix, const DevParams& P, const BatchOut& out, ScanWave& sw, uint32_t read, uint32_t base0,
                                          uint32_t tg, uint32_t q, uint32_t row, uint32_t ent0, uint32_t pend, uint32_t hds)
{
  const uint64_t lt = (1ull << lane_id()) - 1ull;
  const uint32_t seg = base0 >> 7;
  const uint32_t qr = filt_rest8(q);
  while (__ballot(pend != 0) != 0) {
    const bool has = pend != 0;
    const uint32_t e = has ? (uint32_t)__ffs((int)pend) - 1u : 0u;
    const uint32_t hd12 = (hds >> (4u * e)) & 15u;
    const uint64_t idx = (uint64_t)row * kFiltSlotCodes + ent0 + e;
    if (TAP && has) {
      const DevLib Lb = get_lib<SL>(ix, tag_lib(tg));
      const uint2 sv = Lb.sx[idx];
      const uint32_t hd = hd12 + hd_rest8(sv.y, qr);
      if (hd <= P.th) {
        const uint32_t hix = atomicAdd(&out.counters[kCtTapHits], 1u);
        if (hix < out.hit_cap) {
          kr_hit h;
          h.read = read;
          h.kpos = base0 + tag_pos(tg);
          h.strand = tag_strand(tg);
          h.lib = tag_lib(tg);
          h.cmer_index = (Lb.bkt[row] >> 24) + ent0 + e;
          h.hd = hd;
          h.se = (sv.x >> 30) == 1u ? ix.leaf_se[sv.x & kColMask] : (sv.x & kColMask);
          out.hits[hix] = h;
        } else {
          atomicOr(&out.counters[kCtErr], kErrHitCap);
        }
      }
    }
    const uint64_t hm = __ballot(has);
    const uint32_t mark = seg != sw.cur_seg ? 1u : 0u; // wave-uniform
    if (sw.n_st + (uint32_t)__popcll(hm) + mark > kItemStage) flush_stage(out, sw);
    if (mark && lane_id() == 0) sw.stage[sw.n_st] = (uint64_t)seg | ((uint64_t)kItemMarker << 32);
    sw.n_st += mark;
    sw.cur_seg = seg;
    if (has)
      sw.stage[sw.n_st + __popcll(hm & lt)] =
        (uint64_t)(uint32_t)idx | ((uint64_t)((tg & 0xFFFu) | (hd12 << 12) | (qr << 15) | ((uint32_t)(idx >> 32) << 23)) << 32);
    sw.n_st += (uint32_t)__popcll(hm);
    pend &= pend - 1u;
  }
}

// hit test of those passes; returns the hit bits (bit (p * 2 + j) of the group's word).  line 0: the probes that go on are
// appended to the list O (`no` entries so far).  line 1: a bucket of more than 80 entries has its tail scanned on the spot.
template <int DEPTH, bool SL, bool TAP>
__device__ __forceinline__ uint64_t filt_test(const DevIndex& ix, const DevParams& P, const BatchOut& out, ScanWave& sw, const SlotList& L,
                                              const SlotList& O, uint32_t& no, const FiltGroup& g, uint32_t c, const uint4 (&v)[DEPTH * 2])
{
  const uint32_t lane = lane_id(), sub = lane & 3u;
  const uint64_t lt = (1ull << lane) - 1ull;
  uint64_t bits = 0;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    const uint32_t p = c * DEPTH + (uint32_t)d;
    const uint32_t pi = p * 16u + (lane >> 2);
    const bool on = pi < g.nact;
    const uint32_t q = on ? L.q[pi] : 0u;
    const uint32_t q24 = filt_code24(q);
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) r |= (on && filt_chunk_any(v[d * 2 + j], q24, P.th)) ? (1u << j) : 0u;
    bits |= (uint64_t)r << (p * 2u);
    const uint32_t fl = v[d * 2].w | v[d * 2 + 1].w; // (every chunk of a line carries the line's flag)
    if (g.line == 0) {
      const bool more = on && (fl >> 31) != 0u && sub == 0u;
      const uint64_t mm = __ballot(more);
      if (mm != 0) {
        if (more) {
          const uint32_t o = no + (uint32_t)__popcll(mm & lt);
          O.row[o] = L.row[pi];
          O.q[o] = q;
          O.tag[o] = L.tag[pi];
        }
        no += (uint32_t)__popcll(mm);
      }
    } else if (__ballot(on && ((fl >> 30) & 1u) != 0u) != 0) {
      // ---- more than 80 entries: the rest from the packed arrays, full codes, resolved on the spot (Poisson tail)
      const bool lg = on && ((fl >> 30) & 1u) != 0u;
      const uint32_t tg = L.tag[on ? pi : 0u];
      const DevLib Lb = get_lib<SL>(ix, SL ? 0u : tag_lib(tg));
      const uint64_t b = lg ? Lb.bkt[L.row[pi]] : 0ull;
      const uint32_t blen = (uint32_t)(b & 0xFFFFFFu);
      const uint64_t st = (b >> 24) + kFiltSlotCodes;
      const uint64_t e_al = st & ~3ull;
      const int rel0 = (int)(st & 3u), tot = rel0 + (lg && blen > kFiltSlotCodes ? (int)(blen - kFiltSlotCodes) : 0);
      const uint32_t nch = lg ? (uint32_t)(tot + 3) >> 2 : 0u;
      for (uint32_t cc = sub; __ballot(cc < nch) != 0; cc += 4u) {
        uint32_t pend = 0, hds = 0;
        if (cc < nch) {
          const uint4 w = *reinterpret_cast<const uint4*>(Lb.enc + e_al + 4u * cc);
          pend = chunk_hits(w, rel0 - 4 * (int)cc, tot - 4 * (int)cc, q, P.th, hds);
        }
        if (P.dbg & 1u) pend = 0;
        emit_hits<SL, TAP, true>(ix, out, sw, g.read, g.base0, tg, e_al, cc, pend, hds);
      }
    }
  }
  return (P.dbg & 1u) ? 0ull : bits;
}

// deal the hit chunks of a group out, 64 at a time: re-read the chunk (L2), bound by its count, emit the candidates
template <bool SL, bool TAP>
__device__ __forceinline__ void filt_resolve(const DevIndex& ix, const DevParams& P, const BatchOut& out, ScanWave& sw, const SlotList& L,
                                             lds_u32* queue, const FiltGroup& g, uint64_t hitbits)
{
  const uint32_t lane = lane_id(), sub = lane & 3u;
  const uint32_t cnt = (uint32_t)__popcll(hitbits);
  const uint32_t inc = wave_scan_incl(cnt);
  const uint32_t H = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  uint64_t hb = hitbits;
  uint32_t slot_i = inc - cnt;
  for (uint32_t w0 = 0; w0 < H; w0 += 64) {
    while (__ballot(hb != 0 && slot_i < w0 + 64u) != 0) {
      if (hb != 0 && slot_i < w0 + 64u) {
        const uint32_t bit = (uint32_t)__ffsll((long long)hb) - 1u;
        const uint32_t pass = bit >> 1, j = bit & 1u;
        queue[slot_i - w0] = (pass * 16u + (lane >> 2)) | ((sub + j * 4u) << 8);
        hb &= hb - 1;
        ++slot_i;
      }
    }
    WAVE_SYNC();
    uint32_t pend = 0, hds = 0, tg = 0, q = 0, row = 0, cidx = 0;
    if (lane < min(64u, H - w0)) {
      const uint32_t d = queue[lane], probe = d & 255u;
      cidx = d >> 8;
      row = L.row[probe];
      q = L.q[probe];
      tg = L.tag[probe];
      const uint32_t* slot = get_lib<SL>(ix, tag_lib(tg)).slots + (uint64_t)row * 64u + 32u * g.line;
      const uint4 v = *reinterpret_cast<const uint4*>(slot + 4u * cidx);
      pend = filt_chunk_cands(v, filt_code24(q), P.th, hds);
    }
    WAVE_SYNC();
    filt_emit<SL, TAP>(ix, P, out, sw, g.read, g.base0, tg, q, row, kFiltLineCodes * g.line + 5u * cidx, pend, hds);
  }
}

// the shape of this scan, as kr_debug_scan_layout reports it: 4 lanes x 2 chunks per probe = one 128-byte line, 16 probes per pass
constexpr uint32_t kFiltG = 4u, kFiltCpl = 2u, kFiltPps = 64u / kFiltG;
static_assert(kFiltG * kFiltCpl * 5u == kFiltLineCodes && 2u * kFiltLineCodes == kFiltSlotCodes, "five 24-bit codes per chunk, two lines per slot");
#ifndef KR_SCAN_FILT_DEPTH
#define KR_SCAN_FILT_DEPTH 2 // passes (16 probes = 16 lines each) a wave keeps in flight: 32 lines, as many as the 256-byte scan
#endif
#ifndef KR_SCAN_FILT_WPE
#define KR_SCAN_FILT_WPE 4
#endif

template <int DEPTH, int WPE, bool SL, bool TAP>
__global__ __launch_bounds__(kScanWaves* kWave, WPE) void kr_scan_filt_kernel_t(DevIndex ix, DevParams P, BatchIn in, BatchOut out)
{
  static_assert((kListCap / kFiltPps) * kFiltCpl <= 64, "one hit bit per (pass, chunk)");
  // three probe lists per wave: two take turns holding the current and the next group, the third the current group's probes
  // that go on in the second line
  __shared__ uint32_t s_row[kScanWaves][3][kListCap], s_q[kScanWaves][3][kListCap], s_tag[kScanWaves][3][kListCap], s_queue[kScanWaves][64];
  __shared__ uint32_t s_meta[kScanWaves][5 * kReadChunk];
  __shared__ __attribute__((aligned(16))) uint64_t s_stage[kScanWaves][kItemStage];
  static_assert(kReadChunk <= 64, "one lane per read of a visit");
  const uint32_t w = threadIdx.x / kWave;
  const SlotList LA{(lds_u32*)s_row[w][0], (lds_u32*)s_q[w][0], (lds_u32*)s_tag[w][0]};
  const SlotList LB{(lds_u32*)s_row[w][1], (lds_u32*)s_q[w][1], (lds_u32*)s_tag[w][1]};
  const SlotList LO{(lds_u32*)s_row[w][2], (lds_u32*)s_q[w][2], (lds_u32*)s_tag[w][2]};
  lds_u32* queue = (lds_u32*)s_queue[w];
  lds_u32* meta = (lds_u32*)s_meta[w];
  ScanWave sw;
  sw.it_next = sw.it_end = sw.rd_start = 0;
  sw.err = 0;
  sw.cur_seg = 0;
  sw.n_st = 0;
  sw.stage = (lds_u64*)s_stage[w];
  sw.filt0 = sw.filt1 = 0xFFFFFFFFu;
  ReadCursor rc;
  rc.init(out.cursors + kCurScan * kCursors * kCursorStride, in.nreads, blockIdx.x * kScanWaves + w);
  uint32_t r0v, r1v;
  GroupGen<SL, 0> gen;
  uint4 v[DEPTH * 2];
  while (rc.next(r0v, r1v)) {
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r0v), r1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r1v);
    gen.init(r0, r1);
    GroupDesc gd;
    FiltGroup ga, gb;
    bool flip = false;   // which of LA / LB holds the current first-line group (or held it, while its second lines are scanned)
    bool b_ready = false; // the next group's list has been made
    bool has_a = gen.next(ix, P, in, LA, meta, gd), has_b = false;
    ga = FiltGroup{gd.nact, gd.read, gd.base0, gd.slot, 0u, gd.last};
    gb = ga;
    if (has_a) {
      gen.prefetch(ix, in);
      pipe_begin_read(sw);
      filt_issue<DEPTH, SL>(ix, LA, ga.nact, 0u, 0u, v);
    }
    uint32_t c = 0, no = 0;
    uint64_t hitbits = 0;
    while (has_a) {
      const SlotList& N1 = flip ? LB : LA; // the current first-line group's list
      const SlotList& N2 = flip ? LA : LB; // the next group's
      const SlotList& A = ga.line ? LO : N1;
      if (c == 0 && !b_ready) { // the next group's front end and probe list, while A's loads are in flight
        has_b = gen.next(ix, P, in, N2, meta, gd);
        gb = FiltGroup{gd.nact, gd.read, gd.base0, gd.slot, 0u, gd.last};
        if (has_b) gen.prefetch(ix, in);
        b_ready = true;
      }
      hitbits |= filt_test<DEPTH, SL, TAP>(ix, P, out, sw, A, LO, no, ga, c, v);
      const uint32_t npass = (ga.nact + 15u) / 16u;
      if ((c + 1u) * (uint32_t)DEPTH < npass) { // more passes of A than the registers hold
        ++c;
        filt_issue<DEPTH, SL>(ix, A, ga.nact, ga.line, c, v);
        continue;
      }
      const bool go_on = ga.line == 0u && no != 0u; // this group's second lines come next
      WAVE_SYNC(); // (the list O is complete)
      if (go_on)
        filt_issue<DEPTH, SL>(ix, LO, no, 1u, 0u, v);
      else if (has_b)
        filt_issue<DEPTH, SL>(ix, N2, gb.nact, 0u, 0u, v);
      filt_resolve<SL, TAP>(ix, P, out, sw, A, queue, ga, hitbits);
      if (go_on) {
        ga.nact = no, ga.line = 1u; // same read, same segment; the read ends (if it does) after them
        no = 0;
      } else {
        if (ga.last) {
          pipe_end_read(out, sw, meta + ga.slot);
          pipe_begin_read(sw);
        }
        ga = gb, has_a = has_b, flip = !flip, b_ready = false;
      }
      WAVE_SYNC();
      c = 0, hitbits = 0;
    }
    WAVE_SYNC();
    const uint32_t l = lane_id();
    if (l < r1 - r0) {
      out.rd_it_off[r0 + l] = meta[0 * kReadChunk + l];
      out.rd_it_cnt[r0 + l] = meta[1 * kReadChunk + l];
      out.rd_onmers[r0 + l] = meta[2 * kReadChunk + l];
      // (hdist_filt of the bucket tails only: the accumulate kernel completes it from the candidates it verifies)
      reinterpret_cast<uint2*>(out.rd_filt)[r0 + l] = make_uint2(meta[3 * kReadChunk + l], meta[4 * kReadChunk + l]);
    }
    WAVE_SYNC();
  }
  if (sw.err && lane_id() == 0) atomicOr(&out.counters[kCtErr], sw.err);
}

// ---------------------------------------------------------------------------
// Upload: the filter slots and the slot-ordered (colour, rest bits) array of a library, from its packed arrays
// ---------------------------------------------------------------------------
// one thread per 16-byte chunk: reads are contiguous within a bucket, writes fully coalesced
__global__ void kr_build_fslots(const uint64_t* bkt, const uint32_t* enc, uint32_t nrows, uint4* slots)
{
  const uint64_t n = (uint64_t)nrows * 16u;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t row = (uint32_t)(i >> 4), c = (uint32_t)(i & 15u), line = c >> 3, e0 = 5u * c;
    const uint64_t b = bkt[row];
    const uint64_t st = b >> 24;
    const uint32_t ln = (uint32_t)(b & 0xFFFFFFu);
    const uint32_t cnt = ln > e0 ? min(ln - e0, 5u) : 0u;
    uint32_t cd[5];
#pragma unroll
    for (uint32_t k = 0; k < 5u; ++k) cd[k] = k < cnt ? filt_code24(enc[st + e0 + k]) : 0xFFFFFFu;
    const uint32_t meta = cnt | ((line == 0u && ln > kFiltLineCodes) ? 0x80u : 0u) | ((line == 1u && ln > kFiltSlotCodes) ? 0x40u : 0u);
    slots[i] = make_uint4(cd[0] | (cd[1] << 24), (cd[1] >> 8) | (cd[2] << 16), (cd[2] >> 16) | (cd[3] << 8), cd[4] | (meta << 24));
  }
}
__global__ void kr_build_sx(const uint64_t* bkt, const uint32_t* enc, const uint32_t* se, uint32_t nrows, uint2* sx)
{
  const uint64_t n = (uint64_t)nrows * kFiltSlotCodes;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t row = (uint32_t)(i / kFiltSlotCodes), e = (uint32_t)(i - (uint64_t)row * kFiltSlotCodes);
    const uint64_t b = bkt[row];
    const uint64_t st = b >> 24;
    const uint32_t ln = (uint32_t)(b & 0xFFFFFFu);
    sx[i] = e < ln ? make_uint2(se[st + e], filt_rest8(enc[st + e])) : make_uint2(0u, 0u);
  }
}
