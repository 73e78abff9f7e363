// kr_dev_expand.inc -- part of kr_device.hip (included after the scan kernels): what only the accumulate kernel uses --
// accumulator tables, the wave's state, leaf events, colour classes and the colour expansion.

// ---------------------------------------------------------------------------
// Accumulators.  Level 1: 64-slot open-addressing hash table in LDS, keyed
// (se << 1) | strand, probe sequences bounded to 8 slots.  Level 2 (only for reads whose
// keys do not fit level 1): direct-indexed by slot2 = 2 * leaf_rank + strand in a per-wave
// global scratch region, with an LDS bitmap of the touched slots.  A key lives in exactly one
// level: slots never empty during a read, so a bounded probe that failed once fails again.
// ---------------------------------------------------------------------------
struct Acc {
  // level 1 (LDS)
  lds_u32* keys;    // [kLdsSlots]
  lds_u32* planes;  // [kLdsSlots * np * 4]
  lds_u32* counts;  // [kLdsSlots * np]
  // level 2
  lds_u32* bitmap;   // LDS [bm_words] (bm_words even, 8-byte aligned)
  lds_u32* rbitmap;  // LDS [bm_words]: keys of the READ so far (event mode over several segments)
  lds_u16* pre;      // LDS [bm_words / 2]: key ordinal prefix per 64-bit bitmap block (event mode)
  uint32_t* g_planes; // global [nslots2 * np * 4]
  uint32_t* g_counts; // global [nslots2 * np]
  uint32_t* g_list;   // global [nslots2]
  uint32_t nslots2, bm_words, np;
};

struct WaveState {
  lds_u64* stack;   // LDS [stack_cap]: lo | hi << 32
  uint32_t stack_cap; // entries (wave-uniform)
  uint32_t top;   // wave-uniform
  uint64_t* gstk; // global spill of the stack's oldest entries (wave-private)
  uint32_t gs_top; // entries spilled (wave-uniform)
  bool l2;        // this lane sent something to level 2 during this read
  uint32_t err;
  uint32_t rec_next, rec_end; // wave-private range of record slots (wave-uniform)
  uint32_t n_l2;              // reads of this wave that used level 2
  uint32_t n_rec;             // records this wave emitted
  uint32_t n_spill;           // times the work stack moved its older half to global memory
  uint32_t ll_next, ll_end;   // wave-private chunk of out.long_list (wave-uniform)
  // event mode (reads of a single segment): leaf updates are appended as 32-bit events
  bool evmode;      // wave-uniform
  bool ev_full;     // wave-uniform: the event buffer overflowed
  uint32_t nev;     // events buffered (wave-uniform)
  uint32_t ev_cap;  // power of two
  uint32_t ev_words; // words of the region the events and the epilogue's batch arrays share (level-1 planes + counts)
  bool dirty;       // wave-uniform: event mode left data in the level-1 table regions (zeroed on demand)
  bool lean;        // single-segment instantiation: the key bitmap aliases the (idle) work stack, zeroed per read
  uint32_t* gev;    // global spill: events beyond ev_cap, then table entries beyond the LDS table
  uint32_t gev_cap, gtab_cap, gkt_cap; // spill capacities (events / table entries / keys)
  lds_u32* ev;      // aliases the level-1 planes + counts region
};

// A leaf update as one 32-bit event, ordered so that an ascending sort groups by (leaf, strand),
// then position, then Hamming distance:  rank << (PB + 6) | strand << (PB + 5) | pos << 5 | hd.
// PB = position bits: 7 (one segment of 128 k-mer positions), or 8 for the two-segment instantiation of the accumulate
// kernel, where bit 17 of the tag says that the item belongs to the read's second segment.
template <int PB = 7>
__device__ __forceinline__ uint32_t make_event(uint32_t rank, uint32_t tag)
{
  const uint32_t pos = PB == 8 ? (tag_pos(tag) | (((tag >> 17) & 1u) << 7)) : tag_pos(tag);
  return (rank << (PB + 6)) | (tag_strand(tag) << (PB + 5)) | (pos << 5) | tag_hd(tag);
}

// Minfo::update_match (src/query.hpp:153-176) as an idempotent OR: bit `pos` of plane `hd`.
// Keys are (leaf rank + 1) << 1 | strand; level 2 is indexed by slot2 = 2 * rank + strand.
__device__ __forceinline__ void accumulate_planes(const Acc& A, WaveState& ws, uint32_t ev)
{
  const uint32_t rs = ev >> 12; // rank << 1 | strand
  const uint32_t key = rs + 2u;
  const uint32_t hd = ev & 31u, pos = (ev >> 5) & 127u;
  uint32_t s = (hash_key(key) >> 8) & (kLdsSlots - 1);
#pragma unroll 1
  for (int i = 0; i < kLdsProbeMax; ++i) {
    uint32_t cur = lds_ld(&A.keys[s]);
    if (cur == 0) {
      uint32_t old = lds_cas(&A.keys[s], 0u, key);
      cur = old == 0 ? key : old;
    }
    if (cur == key) {
      lds_or(&A.planes[(s * A.np + hd) * kPlaneWords + (pos >> 5)], 1u << (pos & 31));
      return;
    }
    s = (s + 1) & (kLdsSlots - 1);
  }
  // level 2
  lds_or(&A.bitmap[rs >> 5], 1u << (rs & 31));
  __hip_atomic_fetch_or(&A.g_planes[((uint64_t)rs * A.np + hd) * kPlaneWords + (pos >> 5)], 1u << (pos & 31),
                        __ATOMIC_RELAXED, KR_SCRATCH_SCOPE);
  ws.l2 = true;
}

// One leaf update per lane (f = this lane has one): event append, or plane OR after fallback.
__device__ __forceinline__ void add_leaf_events(const Acc& A, WaveState& ws, bool f, uint32_t ev)
{
  const uint64_t m = __ballot(f);
  if (m == 0) return;
  if (ws.evmode) {
    const uint32_t c = __popcll(m);
    if (ws.nev + c <= ws.ev_cap + ws.gev_cap) {
      if (f) {
        const uint32_t i = ws.nev + __popcll(m & ((1ull << lane_id()) - 1ull));
        if (i < ws.ev_cap)
          ws.ev[i] = ev;
        else
          gstore(&ws.gev[i - ws.ev_cap], ev); // long event lists continue in (L2-resident) global scratch
      }
      ws.nev += c;
    } else {
      ws.ev_full = true; // the read is redone with the plane tables (rare)
    }
    return;
  }
  if (f) accumulate_planes(A, ws, ev);
}


// Leaf updates of the flat colours held by the lanes (cnt ranks from fbase each; bit 31 of fbase: the ranks are listed in
// leaflist): the wave-wide concatenation of their ranks, 64 at a time; output slot t belongs to the first lane whose
// inclusive prefix of the counts exceeds t.  FAST: event mode, the appends go straight to the LDS list while it has room.
#ifndef KR_ACC_FLAT_SCATTER
#define KR_ACC_FLAT_SCATTER 1
#endif
template <bool SL, bool FAST, int PB = 7>
__device__ __forceinline__ void emit_flat(const DevIndex& ix, const Acc& A, WaveState& ws, uint32_t cnt, uint32_t fbase, uint32_t tag)
{
  const uint32_t lane = lane_id();
  const uint32_t inc = wave_scan_incl(cnt);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  if (total == 0) return;
  const uint32_t excl = inc - cnt;
  const bool roomy = FAST && ws.nev + total <= ws.ev_cap;
  // Round 6 (scripts/calib_issue.hip): a ds_bpermute costs the LDS pipe 24 cycles a wave instruction, and the six-step search
  // below is a chain of six of them, each waiting for the one before -- four rounds a read.  In the lean layout the 64 key slots
  // (A.keys) are idle during the expansion: the lanes that hold ranks write their lane number at the slot where their run starts
  // (runs of different lanes start at different slots), a slot without a start takes the nearest start to its left -- a max-scan
  // on the DPP network -- and the run that reaches in from the tile before is carried over: two LDS writes, one read and six DPP
  // operations instead of six dependent permutes.
  uint32_t carry = 0; // (FAST) lane + 1 of the source of the tile's last slot
  for (uint32_t t0 = 0; t0 < total; t0 += 64) {
    const uint32_t t = t0 + lane;
    uint32_t j = 0;
    if (FAST && KR_ACC_FLAT_SCATTER) {
      lds_u32* const sl = A.keys;
      sl[lane] = 0;
      if (cnt != 0 && excl - t0 < 64u) sl[excl - t0] = lane + 1u; // (unsigned: t0 <= excl < t0 + 64)
      WAVE_SYNC();
      uint32_t sv = sl[lane];
      WAVE_SYNC(); // (read before the next tile's writes)
      if (lane == 0) sv = max(sv, carry);
      sv = max(sv, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sv, 0x111, 0xF, 0xF, false)); // row_shr:1
      sv = max(sv, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sv, 0x112, 0xF, 0xF, false)); // row_shr:2
      sv = max(sv, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sv, 0x114, 0xF, 0xF, false)); // row_shr:4
      sv = max(sv, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sv, 0x118, 0xF, 0xF, false)); // row_shr:8
      sv = max(sv, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sv, 0x142, 0xA, 0xF, false)); // row_bcast:15 into rows 1 and 3
      sv = max(sv, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sv, 0x143, 0xC, 0xF, false)); // row_bcast:31 into rows 2 and 3
      carry = (uint32_t)__builtin_amdgcn_readlane((int)sv, 63);
      j = sv - 1u; // (slot 0 of the first tile is the start of the first run: every slot has a source)
    } else {
#pragma unroll
      for (uint32_t step = 32; step >= 1; step >>= 1) {
        const uint32_t v = (uint32_t)__shfl((int)inc, (int)(j + step - 1u));
        if (v <= t) j += step;
      }
    }
    j = min(j, 63u); // (slots past the end, masked below)
    const uint32_t b_j = (uint32_t)__shfl((int)fbase, (int)j), ex_j = (uint32_t)__shfl((int)excl, (int)j);
    const uint32_t tg_j = (uint32_t)__shfl((int)tag, (int)j);
    const bool on = t < total;
    uint32_t r = (b_j & 0x7FFFFFFFu) + (t - ex_j);
    if (on && (b_j >> 31)) r = get_lib<SL>(ix, tag_lib(tg_j)).leaflist[r];
    if (roomy) {
      if (on) ws.ev[ws.nev + t] = make_event<PB>(r, tg_j);
    } else {
      add_leaf_events(A, ws, on, make_event<PB>(r, tg_j));
    }
  }
  if (roomy) ws.nev += total;
}

// One step of the colour expansion (the BFS of src/query.cpp:369-387, order-free here) for one item
// per lane: a leaf becomes an event, a colour that expands is looked up in se_to_pse and its two
// parts become events or new work items.  The caller guarantees room for 128 pushes.
template <bool SL>
__device__ __forceinline__ void expand_step(const DevIndex& ix, const Acc& A, WaveState& ws, bool have, uint32_t se, uint32_t tag)
{
  const uint64_t lt = (1ull << lane_id()) - 1ull;
  uint32_t c0 = 0, c1 = 0;
  bool p0 = false, p1 = false;
  bool f0 = false, f1 = false, f2 = false; // leaf updates found by this lane: the item, child 0, child 1
  bool rg = false;                         // the item is a run of ranks: c0 = first rank, c1 = count
  if (have) {
    f0 = (se >> 30) == 1u;
    if ((se >> 30) >= 2u) {
      const uint2 pr = get_lib<SL>(ix, tag_lib(tag)).pse[se & kColMask];
      c0 = pr.x;
      c1 = pr.y;
      if ((se >> 30) == 2u) { // (a part that is a run goes through the stack and comes back as an item)
        f1 = (c0 >> 30) == 1u, p0 = (c0 >> 30) >= 2u;
        f2 = (c1 >> 30) == 1u, p1 = (c1 >> 30) >= 2u;
      } else {
        rg = true;
      }
    }
  }
  add_leaf_events(A, ws, f0, make_event(se & kColMask, tag));
  add_leaf_events(A, ws, f1, make_event(c0 & kColMask, tag));
  add_leaf_events(A, ws, f2, make_event(c1 & kColMask, tag));
  emit_flat<SL, false>(ix, A, ws, rg ? c1 : 0u, c0, tag);
  const uint64_t m0 = __ballot(p0), m1 = __ballot(p1);
  if (p0) ws.stack[ws.top + __popcll(m0 & lt)] = (uint64_t)c0 | ((uint64_t)tag << 32);
  ws.top += __popcll(m0);
  if (p1) ws.stack[ws.top + __popcll(m1 & lt)] = (uint64_t)c1 | ((uint64_t)tag << 32);
  ws.top += __popcll(m1);
  WAVE_SYNC();
}

// The same step for the single-segment kernel, which is always in event mode (the kernel is bound by instruction issue --
// 2,340 wave instructions per read before, half of them in this loop -- not by memory: `scripts/pmc_insts_by_phase.sh`):
// leaves and flat colours leave through emit_flat; a colour that is still walked (rare: everything of <= 64 leaves is flat)
// appends its leaf parts with one capacity test and puts the parts that are colours back on the stack.
#ifndef KR_ACC_LEAN_STEP
#define KR_ACC_LEAN_STEP 1
#endif
template <bool SL, int PB = 7>
__device__ __forceinline__ void expand_step_ev(const DevIndex& ix, const Acc& A, WaveState& ws, bool have, uint32_t se, uint32_t tag)
{
  const uint32_t cls = have ? se >> 30 : 0u;
  uint2 pr = make_uint2(0, 0); // (class 0: nothing to do)
  if (cls >= 2u) pr = get_lib<SL>(ix, tag_lib(tag)).pse[se & kColMask];
  // ---- leaves (a run of one rank) and flat colours (pr = {base, count})
  emit_flat<SL, true, PB>(ix, A, ws, cls == 1u ? 1u : (cls == 3u ? pr.y : 0u), cls == 1u ? (se & kColMask) : pr.x, tag);
  // ---- walked colours (pr = the two parts)
  if (__ballot(cls == 2u) != 0) {
    const uint32_t k0 = cls == 2u ? pr.x >> 30 : 0u, k1 = cls == 2u ? pr.y >> 30 : 0u;
    const bool f1 = k0 == 1u, f2 = k1 == 1u, p0 = k0 >= 2u, p1 = k1 >= 2u;
    const uint64_t m1 = __ballot(f1), m2 = __ballot(f2);
    if ((m1 | m2) != 0) { // parts that are leaves
      const uint32_t n1 = (uint32_t)__popcll(m1), n2 = (uint32_t)__popcll(m2);
      if (ws.nev + n1 + n2 <= ws.ev_cap) {
        const uint32_t tb = make_event<PB>(0u, tag); // make_event: rank << (PB + 6) | tb
        lds_u32* const e = ws.ev + ws.nev;
        if (f1) e[lanes_below(m1)] = (pr.x << (PB + 6)) | tb; // (the class bits leave at the top)
        if (f2) e[n1 + lanes_below(m2)] = (pr.y << (PB + 6)) | tb;
        ws.nev += n1 + n2;
      } else { // the list continues in global scratch, or overflows
        add_leaf_events(A, ws, f1, make_event<PB>(pr.x & kColMask, tag));
        add_leaf_events(A, ws, f2, make_event<PB>(pr.y & kColMask, tag));
      }
    }
    // parts that are colours themselves: back on the stack
    const uint64_t q0 = __ballot(p0), q1 = __ballot(p1);
    if (p0) ws.stack[ws.top + lanes_below(q0)] = (uint64_t)pr.x | ((uint64_t)tag << 32);
    ws.top += (uint32_t)__popcll(q0);
    if (p1) ws.stack[ws.top + lanes_below(q1)] = (uint64_t)pr.y | ((uint64_t)tag << 32);
    ws.top += (uint32_t)__popcll(q1);
  }
  WAVE_SYNC();
}

// drain the work stack
// The LDS stack is the top of a two-level stack.  A colour that covers a large clade fans out faster than it is
// consumed (64 items popped, up to 128 pushed): when no room is left the OLDER half moves to the wave's global spill
// (LIFO never needs it before the newer half is gone), and it comes back when the LDS part has run empty.
constexpr uint32_t kStackSpill = 8192; // entries per wave (64 KiB)
// (by value: a WaveState passed by reference to a real call would have to live in scratch memory)
__device__ __noinline__ uint32_t stack_spill(lds_u64* stack, uint64_t* gstk, uint32_t top, uint32_t gs_top)
{ // returns the number of entries moved out (0: the spill is full)
  const uint32_t lane = lane_id(), half = top / 2u;
  if (half == 0 || gs_top + half > kStackSpill) return 0;
  for (uint32_t i = lane; i < half; i += 64) gstk[gs_top + i] = stack[i];
  WAVE_SYNC();
  for (uint32_t i0 = 0; i0 < top - half; i0 += 64) { // move the newer part down, tile by tile (ascending: no overlap hazard)
    const uint32_t i = i0 + lane;
    uint64_t v = 0;
    if (i < top - half) v = stack[half + i];
    WAVE_SYNC();
    if (i < top - half) stack[i] = v;
    WAVE_SYNC();
  }
  return half;
}
__device__ __noinline__ uint32_t stack_refill(lds_u64* stack, const uint64_t* gstk, uint32_t cap, uint32_t gs_top)
{ // returns the number of entries brought back
  const uint32_t lane = lane_id(), m = min(gs_top, cap / 2u);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // this wave's earlier spill stores have landed
  for (uint32_t i = lane; i < m; i += 64) stack[i] = gstk[gs_top - m + i];
  WAVE_SYNC();
  return m;
}

template <bool SL, bool EV = false, int PB = 7>
__device__ __forceinline__ void expand_all(const DevIndex& ix, const Acc& A, WaveState& ws)
{
  const uint32_t lane = lane_id();
  for (;;) {
    if (ws.top == 0) {
      if (ws.gs_top == 0) break;
      const uint32_t m = stack_refill(ws.stack, ws.gstk, ws.stack_cap, ws.gs_top);
      ws.gs_top -= m, ws.top = m;
    }
    const uint32_t room = ws.stack_cap - ws.top;
    const uint32_t n = min(min(64u, ws.top), room);
    if (n == 0) { // no room for the children of even one item
      const uint32_t half = stack_spill(ws.stack, ws.gstk, ws.top, ws.gs_top);
      if (half) {
        ws.gs_top += half, ws.top -= half;
        ws.n_spill++;
        continue;
      }
      ws.err |= kErrStack; // the spill is full too: report, drop the rest
      ws.top = 0, ws.gs_top = 0;
      break;
    }
    const uint32_t base = ws.top - n;
    const bool have = lane < n;
    uint64_t raw = 0;
    if (have) raw = ws.stack[base + lane];
    ws.top = base;
    if (EV)
      expand_step_ev<SL, PB>(ix, A, ws, have, (uint32_t)raw, (uint32_t)(raw >> 32));
    else
      expand_step<SL>(ix, A, ws, have, (uint32_t)raw, (uint32_t)(raw >> 32));
  }
}


// fold the planes of one level-1 slot / level-2 slot into its running counts and zero them
__device__ __forceinline__ void fold_l1(const Acc& A, uint32_t s)
{
  uint32_t cum0 = 0, cum1 = 0, cum2 = 0, cum3 = 0;
  for (uint32_t x = 0; x < A.np; ++x) {
    lds_u32* p = &A.planes[(s * A.np + x) * kPlaneWords];
    uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
    uint32_t add = __popc(w0 & ~cum0) + __popc(w1 & ~cum1) + __popc(w2 & ~cum2) + __popc(w3 & ~cum3);
    cum0 |= w0, cum1 |= w1, cum2 |= w2, cum3 |= w3;
    if (w0 | w1 | w2 | w3) p[0] = 0, p[1] = 0, p[2] = 0, p[3] = 0;
    if (add) A.counts[s * A.np + x] += add;
  }
}
__device__ __forceinline__ void fold_l2(const Acc& A, uint32_t slot2)
{
  uint32_t cum0 = 0, cum1 = 0, cum2 = 0, cum3 = 0;
  for (uint32_t x = 0; x < A.np; ++x) {
    uint32_t* p = &A.g_planes[((uint64_t)slot2 * A.np + x) * kPlaneWords];
    uint32_t w0 = gload(p), w1 = gload(p + 1), w2 = gload(p + 2), w3 = gload(p + 3);
    uint32_t add = __popc(w0 & ~cum0) + __popc(w1 & ~cum1) + __popc(w2 & ~cum2) + __popc(w3 & ~cum3);
    cum0 |= w0, cum1 |= w1, cum2 |= w2, cum3 |= w3;
    if (w0) gstore(p, 0);
    if (w1) gstore(p + 1, 0);
    if (w2) gstore(p + 2, 0);
    if (w3) gstore(p + 3, 0);
    if (add) {
      uint32_t* cp = &A.g_counts[(uint64_t)slot2 * A.np + x];
      gstore(cp, gload(cp) + add);
    }
  }
}

// list of touched level-2 slots, ascending (= ascending key); returns its length
__device__ __forceinline__ uint32_t l2_build_list(const Acc& A, lds_u32* bitmap)
{
  const uint32_t lane = lane_id();
  uint32_t n = 0;
  for (uint32_t w0 = 0; w0 < A.bm_words; w0 += 64) {
    uint32_t wi = w0 + lane;
    uint32_t word = wi < A.bm_words ? bitmap[wi] : 0u;
    uint32_t c = __popc(word), inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint32_t t = __shfl_up(inc, d);
      if (lane >= (uint32_t)d) inc += t;
    }
    uint32_t o = n + inc - c;
    while (word) {
      uint32_t bit = (uint32_t)__ffs((int)word) - 1u;
      A.g_list[o++] = wi * 32u + bit;
      word &= word - 1u;
    }
    n += __shfl(inc, 63);
  }
  __syncthreads();
  return n;
}

__device__ __forceinline__ uint32_t hmin_l1(const Acc& A, uint32_t s)
{
  for (uint32_t x = 0; x < A.np; ++x)
    if (A.counts[s * A.np + x]) return x;
  return 0xFFFFFFFFu;
}
__device__ __forceinline__ uint32_t hmin_l2(const Acc& A, uint32_t slot2)
{
  for (uint32_t x = 0; x < A.np; ++x)
    if (gload(&A.g_counts[(uint64_t)slot2 * A.np + x])) return x;
  return 0xFFFFFFFFu;
}

// Record slots are handed out in wave-private chunks: one returning atomic on the shared counter
// per ~1000 records instead of one per read (a single word sustains only ~90 M atomics/s chip-wide,
// which is the read rate of the small-index configuration).  Unused slots at the end of a chunk stay
// zero (key 0 = hole; the record arrays are zeroed per batch).
#ifndef KR_REC_CHUNK
#define KR_REC_CHUNK 256
#endif
constexpr uint32_t kRecChunk = KR_REC_CHUNK; // largest chunk; BatchOut::rec_chunk is what a batch uses (smaller for small batches)
constexpr uint32_t kEvSpill = 64512; // events of one read beyond the LDS buffer (252 KiB of global scratch per wave): a read
                                     // that does not fit is set aside for the second launch, where it is a tail (one wave, idle chip)
__device__ __forceinline__ uint32_t alloc_records(const BatchOut& out, WaveState& ws, uint32_t n)
{
  if (ws.rec_next + n > ws.rec_end) {
    uint32_t chunk = max(n, out.rec_chunk), base = 0;
    if (lane_id() == 0) base = atomicAdd(&out.counters[kCtRecSlots], chunk);
    base = __shfl(base, 0);
    if ((uint64_t)base + chunk > out.rec_cap) {
      if (lane_id() == 0) atomicOr(&out.counters[kCtErr], kErrRecCap);
      return 0xFFFFFFFFu;
    }
    ws.rec_next = base;
    ws.rec_end = base + chunk;
  }
  uint32_t r = ws.rec_next;
  ws.rec_next += n;
  ws.n_rec += n;
  return r;
}

