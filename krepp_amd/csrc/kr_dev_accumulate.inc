// kr_dev_accumulate.inc -- part of kr_device.hip (one translation unit, included in order): kernel 2: event epilogue, plane tables, records.

// ---------------------------------------------------------------------------
// Event mode epilogue.  No sort:
//  1. the keys (2 * leaf rank + strand) of the read's events are marked in the LDS bitmap; a popcount
//     prefix over the bitmap gives every key its ORDINAL among the read's keys (ascending key =
//     ascending colour id, strands adjacent);
//  2. every event is rewritten in place as  ordinal << 12 | pos << 5 | hd  and its key stored in
//     keytab[ordinal];
//  3. the per-position minimum of Minfo::update_match (src/query.hpp:153-176) is taken by visiting the
//     events in ascending hd LEVELS: an event sets bit `pos` of its key's 128-bit position map with a
//     returning LDS atomic OR, and only the event that finds the bit clear increments the key's
//     histogram counter of that level (8-bit counters, four per word: a segment has <= 128 positions);
//  4. keys that pass `hdist_min <= 2*hdist_filt+1` (src/query.cpp:101-106,119) are appended to a
//     compact table (counters + key) and written out at the end.
// Position maps and counters hold KB keys at a time (4 + hw words per key, all of the idle LDS behind
// the events: a single batch for all but the largest reads).  LDS use: [tab ... keytab] in the idle
// stack / probe-list / level-1 key region, [events | batch arrays] in the level-1 plane region.
// Returns false if the read does not fit (more keys than keytab holds, more passing keys than the
// table and its global spill hold): the caller falls back to the plane tables.
// ---------------------------------------------------------------------------
// (Combining lanes that OR into the same LDS word in registers first -- a segmented OR-scan on DPP -- was
//  measured: the serialisation it removes costs less than its ~45 instructions, +1..5 % run time.)
// Batch arrays of the event epilogue live in LDS, or -- for the rare read with more keys than the LDS
// holds -- in the wave's global scratch (L2): same code, memory operations by pointer type.
// Statistics of KR_DEBUG_SKIP=512 (tuning only; printed and cleared by kr_batch_wait): [0..31] reads by log2(events + 1), [32..63] by
// log2(marked keys + 1), [64..95] by log2(records + 1), [96] straight-line epilogue, [97] general epilogue, [98] set aside: events
// beyond the spill, [99] set aside: the epilogue's tables, [110..119] records by min(9, events counted in the record)
// (the paths -- sparse, planes in global scratch, fused, key batches, key table in global scratch -- are counted in the production
//  build: `witness`, CounterSlot kCtFp* / kCtGe* / kCtRd*)
// Compiled in with -DKR_STATS=1 only (scripts/build_variant.sh stats -DKR_STATS=1): the extra live values cost the 80-register kernel a spill.
#ifndef KR_STATS
#define KR_STATS 0
#endif
__device__ uint32_t g_kr_stats[128];
__device__ __forceinline__ uint32_t stat_log2(uint32_t v) { return 32u - (uint32_t)__clz((int)v); } // 0 -> 0, 1 -> 1, 2..3 -> 2, ...
__device__ __forceinline__ void stat_records(uint64_t w0, bool on)
{ // one record per lane: w0 = five 8-bit counts
  const uint32_t tot = (uint32_t)(w0 & 255u) + (uint32_t)((w0 >> 8) & 255u) + (uint32_t)((w0 >> 16) & 255u) + (uint32_t)((w0 >> 24) & 255u) + (uint32_t)((w0 >> 32) & 255u);
  if (KR_STATS && on) atomicAdd(&g_kr_stats[110u + min(tot, 9u)], 1u);
}
// path witness (KR_DEBUG_SKIP=512; CounterSlot kCtFp* / kCtGe* / kCtRd*): lane 0 counts where the path is entered
__device__ __forceinline__ void witness(const BatchOut& out, uint32_t dbg, CounterSlot slot, uint32_t n = 1u)
{
  if ((dbg & 512u) && lane_id() == 0) atomicAdd(&out.counters[slot], n);
}
__device__ __forceinline__ void mem_or(lds_u32* p, uint32_t v) { lds_or(p, v); }
__device__ __forceinline__ void mem_or(uint32_t* p, uint32_t v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, KR_SCRATCH_SCOPE); }
__device__ __forceinline__ void mem_st(lds_u32* p, uint32_t v) { *p = v; }
__device__ __forceinline__ void mem_st(uint32_t* p, uint32_t v) { gstore(p, v); }
__device__ __forceinline__ constexpr bool planes_stay_zero(lds_u32*) { return false; }
__device__ __forceinline__ constexpr bool planes_stay_zero(uint32_t*) { return true; }
__device__ __forceinline__ void mem_zero(lds_u32* p, uint32_t n) // n a multiple of 4 words, p 16-byte aligned: ds_write_b128
{
  for (uint32_t i = 4u * lane_id(); i < n; i += 256u) *(KR_LDS u32x4*)(p + i) = u32x4{0, 0, 0, 0};
}
__device__ __forceinline__ void mem_zero(uint32_t* p, uint32_t n)
{
  for (uint32_t i = lane_id(); i < n; i += 64u) gstore(p + i, 0u);
}
__device__ __forceinline__ void mem_sync(lds_u32*) { WAVE_SYNC(); }
__device__ __forceinline__ void mem_sync(uint32_t*)
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // this wave's global atomics / stores have landed in L2
  WAVE_SYNC();
}

// One pass over the events whose key ordinal lies in [k0, k0 + kn): an event ORs its position bit into
// plane `hd` of its key (np planes of 128 bits per key; bit `pos >> 2` of word `pos & 3`, so that a run
// of neighbouring positions spreads over the four words).  The per-position minimum is taken afterwards,
// by the lane that owns the key: count[hd] = popc(plane[hd] & ~(plane[0] | ... | plane[hd-1])).
// PB = position bits of the events (7: planes of 128 bits = 4 words; 8: two segments, 256 bits = 8 words)
template <int PB, typename PT, typename EV>
__device__ __forceinline__ void plane_pass(PT bt, uint32_t np, uint32_t k0, uint32_t kn, uint32_t nev, EV ev_at)
{
  constexpr uint32_t PW = 1u << (PB - 5);
  const uint32_t lane = lane_id();
  if (!planes_stay_zero(bt)) { // (the global planes are all-zero between reads: plane_counts puts back what it read)
    mem_zero(bt, kn * np * PW);
    mem_sync(bt);
  }
  for (uint32_t t0 = 0; t0 < nev; t0 += 64) {
    const uint32_t i = t0 + lane;
    if (i < nev) {
      const uint32_t v = ev_at(t0, i);
      const uint32_t o = (v >> (PB + 5)) - k0;
      if (o < kn) {
        const uint32_t pos = (v >> 5) & ((1u << PB) - 1u);
        mem_or(bt + (o * np + (v & 31u)) * PW + (pos & (PW - 1u)), 1u << (pos >> (PB - 5)));
      }
    }
  }
  mem_sync(bt);
}
// packed counters of key j of the batch: CB bits per hd value (8: four per word, a segment has at most 128 positions;
// 16 for two segments)
template <int PB>
struct CountPack {
  static constexpr uint32_t CB = PB == 7 ? 8u : 16u, CPW = 32u / CB, MASK = (1u << CB) - 1u;
  static constexpr int WORDS = (kMaxPlanes + (int)CPW - 1) / (int)CPW;
  static __device__ __forceinline__ uint32_t words(uint32_t np) { return (np + CPW - 1u) / CPW; }
  static __device__ __forceinline__ uint32_t get(const uint32_t* c, uint32_t x) { return (c[x / CPW] >> (CB * (x % CPW))) & MASK; }
};
template <int PB>
__device__ __forceinline__ void plane_counts(lds_u32* bt, uint32_t np, uint32_t j, uint32_t* c)
{
  constexpr uint32_t PW = 1u << (PB - 5), CB = CountPack<PB>::CB, CPW = CountPack<PB>::CPW;
  u32x4 seen[PW / 4];
#pragma unroll
  for (uint32_t q = 0; q < PW / 4; ++q) seen[q] = u32x4{0, 0, 0, 0};
#pragma unroll
  for (int x = 0; x < kMaxPlanes; ++x)
    if ((uint32_t)x < np) {
      uint32_t add = 0;
#pragma unroll
      for (uint32_t q = 0; q < PW / 4; ++q) {
        const u32x4 pw = *(KR_LDS u32x4*)(bt + (j * np + x) * PW + 4u * q); // ds_read_b128
        add += (uint32_t)(__popc(pw.x & ~seen[q].x) + __popc(pw.y & ~seen[q].y) + __popc(pw.z & ~seen[q].z) + __popc(pw.w & ~seen[q].w));
        seen[q] |= pw;
      }
      c[(uint32_t)x / CPW] += add << (CB * ((uint32_t)x % CPW));
    }
}
template <int PB>
__device__ __forceinline__ void plane_counts(uint32_t* bt, uint32_t np, uint32_t j, uint32_t* c)
{
  constexpr uint32_t PW = 1u << (PB - 5), CB = CountPack<PB>::CB, CPW = CountPack<PB>::CPW;
  uint32_t s_[PW];
#pragma unroll
  for (uint32_t q = 0; q < PW; ++q) s_[q] = 0;
#pragma unroll
  for (int x = 0; x < kMaxPlanes; ++x)
    if ((uint32_t)x < np) {
      uint32_t* p = bt + (uint64_t)(j * np + x) * PW;
      uint32_t add = 0, w[PW];
#pragma unroll
      for (uint32_t q = 0; q < PW; ++q) w[q] = gload(p + q); // (all of a plane's loads leave together: one round trip, not PW)
#pragma unroll
      for (uint32_t q = 0; q < PW; ++q) {
        add += (uint32_t)__popc(w[q] & ~s_[q]);
        s_[q] |= w[q];
      }
      // back to all-zero for the next read (and for the plane path, which shares the table): only the words an event set,
      // one or two per key -- clearing all the words of every key, before and after, was 1.5 GB of HBM writes per 1 M reads
#pragma unroll
      for (uint32_t q = 0; q < PW; ++q)
        if (w[q]) gstore(p + q, 0u);
      c[(uint32_t)x / CPW] += add << (CB * ((uint32_t)x % CPW));
    }
}

__device__ __forceinline__ uint32_t key_ordinal(const Acc& A, uint32_t rs)
{
  const uint32_t blk = rs >> 6;
  const uint64_t bits = *(lds_u64*)(A.bitmap + 2u * blk);
  return (uint32_t)A.pre[blk] + __popcll(bits & ((1ull << (rs & 63u)) - 1ull));
}

// MERGE: one segment of a longer read -- every key is kept (the hdist_filt test needs the whole read), the
// segment's counts are added to the wave's global count table (disjoint positions: histograms add) and the key
// is noted in the read's bitmap; records are written by the caller when the read is complete.
template <bool MERGE, int PB = 7>
__device__ __forceinline__ bool finalize_events(const DevIndex& ix, const BatchOut& out, const Acc& A, WaveState& ws,
                                                lds_u32* lo, uint32_t lo_words, uint32_t read, uint32_t onmers,
                                                uint32_t filt0, uint32_t filt1, uint32_t dbg)
{
  const uint32_t lane = lane_id();
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint32_t nev = ws.nev;
  const uint32_t lim0 = 2u * filt0 + 1u, lim1 = 2u * filt1 + 1u; // u32 wrap keeps "none" = max
  typedef CountPack<PB> CP;             // packed per-key counters: 8 bits per hd value (16 for two segments)
  constexpr int KH = CP::WORDS;
  constexpr uint32_t PW = 1u << (PB - 5), KS = PB + 5; // plane words; an event's key (rank << 1 | strand) starts at bit KS
  constexpr uint32_t PMASK = (1u << PB) - 1u, LOWM = (1u << KS) - 1u;
  const uint32_t hw = CP::words(A.np);  // histogram words per key
  const uint32_t ew = hw + 1u;          // table entry: packed counters, key
  const uint32_t kw = A.np * PW;        // batch words per key: np planes of 128 (256) position bits
  lds_u32* e = ws.ev;
  uint32_t nrec = 0;
  bool fits = true;
  // event i of the read (a 64-aligned tile is entirely in LDS or entirely spilled)
  auto ev_at = [&](uint32_t t0, uint32_t i) -> uint32_t { return t0 < ws.ev_cap ? e[i] : gload(&ws.gev[i - ws.ev_cap]); };
  uint32_t* gtab = ws.gev + ws.gev_cap;
  if (nev) {
    if (nev > ws.ev_cap) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // spilled events are complete
    if (ws.lean) { // the bitmap aliases the work stack (empty now)
      for (uint32_t q = lane; q < A.bm_words; q += 64) A.bitmap[q] = 0;
      WAVE_SYNC();
    }
    // ---- 1. mark keys, ordinal prefix per 64-bit block
    for (uint32_t t0 = 0; t0 < nev; t0 += 64) {
      const uint32_t i = t0 + lane;
      // only keys that can pass `hdist_min <= 2*hdist_filt+1` at all: an event within the limit marks its key; the
      // events of unmarked keys are dropped in step 2 (a read with an exact match keeps a third of its keys)
      const uint32_t v = i < nev ? ev_at(t0, i) : 0xFFFFFFFFu;
      const uint32_t rs = v >> KS;
      if (i < nev && (MERGE || (v & 31u) <= ((rs & 1u) ? lim1 : lim0))) lds_or(&A.bitmap[rs >> 5], 1u << (rs & 31u));
    }
    WAVE_SYNC();
    uint32_t nkeys = 0;
    const uint32_t nblk = A.bm_words >> 1;
    for (uint32_t b0 = 0; b0 < nblk; b0 += 64) {
      const uint32_t b = b0 + lane;
      const uint32_t c = b < nblk ? __popcll(*(lds_u64*)(A.bitmap + 2u * b)) : 0u;
      const uint32_t inc = wave_scan_incl(c);
      if (b < nblk) A.pre[b] = (uint16_t)(nkeys + inc - c);
      nkeys += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    WAVE_SYNC();
    // keytab[nkeys] behind the events if that leaves room for a batch of 8 keys, else in global scratch
    const uint32_t nev_lds = (min(nev, ws.ev_cap) + 1u) & ~1u;
    const bool kt_lds = nev_lds + nkeys + 4u + 8u * kw <= ws.ev_words;
    fits = kt_lds || nkeys <= ws.gkt_cap;
    lds_u32* keytab = e + nev_lds;
    uint32_t* gkt = gtab + (uint64_t)ws.gtab_cap * ew;
    const uint32_t tab_cap = lo_words / ew;
    // ---- 2. ordinals into the events, keys into keytab, events per key into kinfo
    //         (most keys of a read have ONE event -- relatives reached by a single k-mer -- and need no planes)
    lds_u32* kinfo = keytab + nkeys;
    // only where the plain planes would need more than one batch
    const bool sparse_try = kt_lds && nev_lds + 2u * nkeys + 4u <= ws.ev_words && !(dbg & 4096u) &&
                            nkeys > (ws.ev_words - ((nev_lds + nkeys + 3u) & ~3u)) / kw;
    if (sparse_try) {
      for (uint32_t o = lane; o < nkeys; o += 64) kinfo[o] = 0;
      WAVE_SYNC();
    }
    uint32_t lv = 0;
    // One LDS batch holds the planes of every key (nearly every read): they are filled right here, while the ordinals are
    // computed -- no rewrite of the events, no second pass over them (step 3 then only counts).
#ifndef KR_ACC_FUSED
#define KR_ACC_FUSED 1
#endif
    const uint32_t bt_off1 = (nev_lds + nkeys + 3u) & ~3u;
    const bool fused = KR_ACC_FUSED && fits && kt_lds && !sparse_try && nkeys != 0 && nkeys * kw <= ws.ev_words - bt_off1 && !(dbg & (64u | 128u));
    if (fused) {
      mem_zero(e + bt_off1, nkeys * kw);
      WAVE_SYNC();
    }
    if (fits)
      for (uint32_t t0 = 0; t0 < nev; t0 += 64) {
        const uint32_t i = t0 + lane;
        if (i < nev) {
          const uint32_t v = ev_at(t0, i), rs = v >> KS;
          const bool live = (A.bitmap[rs >> 5] >> (rs & 31u)) & 1u; // its key was marked
          const uint32_t o = key_ordinal(A, rs);
          if (!fused) {
            const uint32_t nv = live ? (o << KS) | (v & LOWM) : 0xFFFFFFFFu; // dead events match no batch
            if (t0 < ws.ev_cap)
              e[i] = nv;
            else
              gstore(&ws.gev[i - ws.ev_cap], nv);
          }
          if (live) {
            if (kt_lds)
              keytab[o] = rs;
            else
              gstore(&gkt[o], rs);
            if (sparse_try) __hip_atomic_fetch_add(&kinfo[o], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (fused) {
              const uint32_t pos = (v >> 5) & PMASK;
              lds_or(e + bt_off1 + (o * A.np + (v & 31u)) * PW + (pos & (PW - 1u)), 1u << (pos >> (PB - 5)));
            }
          }
          lv |= 1u << (v & 31u);
        }
      }
    if (dbg & 512u) { // (statistics only)
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) lv |= __shfl_xor(lv, d);
    }
    if (nev > ws.ev_cap || !kt_lds) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    WAVE_SYNC();
    // the bitmap goes back to all-zero
    if (fits) {
      for (uint32_t o = lane; o < nkeys; o += 64) A.bitmap[(kt_lds ? keytab[o] : gload(&gkt[o])) >> 5] = 0;
    } else {
      for (uint32_t t0 = 0; t0 < nev; t0 += 64) {
        const uint32_t i = t0 + lane;
        if (i < nev) A.bitmap[ev_at(t0, i) >> (KS + 5)] = 0;
      }
      nkeys = 0;
    }
    if (dbg & 64u) nkeys = 0;
    // ---- 3. batches of KB ordinals; a read with more than 16 LDS batches of keys runs as ONE batch in the
    //         wave's global scratch (A.g_planes, all-zero between reads like the plane path needs it):
    //         L2 atomics are ~10x slower than LDS ones, the batches re-read the events
    // kinfo[o] becomes: keys with several events -> their plane slot (consecutive); keys with one event ->
    // 0x80000000 | hd of that event (filled in by the plane pass)
    constexpr uint32_t kSingle = 0x80000000u;
    uint32_t nmulti = 0;
    if (sparse_try) {
      for (uint32_t j0 = 0; j0 < nkeys; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool multi = j < nkeys && kinfo[j] > 1u;
        const uint64_t mm = __ballot(multi);
        if (j < nkeys) kinfo[j] = multi ? nmulti + (uint32_t)__popcll(mm & lt) : (kSingle | 0x40u);
        nmulti += (uint32_t)__popcll(mm);
      }
      WAVE_SYNC();
    }
    const bool sparse = sparse_try && nkeys != 0 && ((nev_lds + 2u * nkeys + 3u) & ~3u) + nmulti * kw <= ws.ev_words;
    const uint32_t bt_off = (nev_lds + (kt_lds ? nkeys : 0u) + (sparse ? nkeys : 0u) + 3u) & ~3u; // 16-byte aligned
    lds_u32* bt = e + bt_off; // [KB][kw]
    const uint32_t KB_lds = sparse ? nkeys : (ws.ev_words - bt_off) / kw;
    const bool many = !sparse && nkeys > ((dbg & 2048u) ? 1u : 16u) * KB_lds && !(dbg & 1024u);
    const bool big = many && (uint64_t)nkeys * kw <= (uint64_t)A.nslots2 * A.np * kPlaneWords; // (the global planes: 4 words per plane)
    if (PB != 7 && many && !big) { // thousands of keys with 256-bit planes: more than the global planes hold, and hundreds of LDS
      fits = false;                // batches otherwise -- the merge instantiation takes the read
      nkeys = 0;
    }
    const uint32_t KB = big ? nkeys : KB_lds;
    for (uint32_t k0 = 0; k0 < nkeys; k0 += KB) {
      const uint32_t kn = min(KB, nkeys - k0);
      const uint64_t tl0 = (dbg & 512u) ? __builtin_readcyclecounter() : 0;
      if (!(dbg & 128u) && !fused) {
        if (sparse) { // one pass, planes for the keys with several events only
          mem_zero(bt, nmulti * kw);
          WAVE_SYNC();
          for (uint32_t t0 = 0; t0 < nev; t0 += 64) {
            const uint32_t i = t0 + lane;
            if (i < nev) {
              const uint32_t v = ev_at(t0, i), o = v >> KS, ki = o < nkeys ? kinfo[o] : 0u;
              if (o >= nkeys) {
                // dead event
              } else if (ki & kSingle) {
                kinfo[o] = kSingle | (v & 31u);
              } else {
                const uint32_t pos = (v >> 5) & PMASK;
                lds_or(bt + (ki * A.np + (v & 31u)) * PW + (pos & (PW - 1u)), 1u << (pos >> (PB - 5)));
              }
            }
          }
          WAVE_SYNC();
        } else if (big)
          plane_pass<PB>(A.g_planes, A.np, k0, kn, nev, ev_at);
        else
          plane_pass<PB>(bt, A.np, k0, kn, nev, ev_at);
      }
      if ((dbg & 512u) && lane == 0) atomicAdd(&out.counters[kCtCycLevel], (uint32_t)((__builtin_readcyclecounter() - tl0) >> 6));
      // ---- 4. one lane per key of the batch
      for (uint32_t j0 = 0; j0 < kn; j0 += 64) {
        const uint32_t j = j0 + lane;
        uint32_t c[KH]; // packed counters (CountPack)
        bool ok = false;
        uint32_t rs = 0;
#pragma unroll
        for (int q = 0; q < KH; ++q) c[q] = 0;
        if (j < kn) {
          if (sparse) {
            const uint32_t ki = kinfo[j];
            if (ki & kSingle) {
              const uint32_t hd1 = ki & 31u;
#pragma unroll
              for (int q = 0; q < KH; ++q)
                if ((hd1 / CP::CPW) == (uint32_t)q && !(ki & 0x40u)) c[q] = 1u << (CP::CB * (hd1 % CP::CPW));
            } else {
              plane_counts<PB>(bt, A.np, ki, c);
            }
          } else if (big)
            plane_counts<PB>(A.g_planes, A.np, j, c);
          else
            plane_counts<PB>(bt, A.np, j, c);
          rs = kt_lds ? keytab[k0 + j] : gload(&gkt[k0 + j]);
          uint32_t hmin = 0xFFFFFFFFu; // hdist_min = lowest hd with a non-zero counter
#pragma unroll
          for (int q = KH - 1; q >= 0; --q)
            if (c[q]) hmin = CP::CPW * q + ((uint32_t)(__ffs((int)c[q]) - 1) / CP::CB);
          ok = !MERGE && hmin <= ((rs & 1u) ? lim1 : lim0);
          if (MERGE && hmin != 0xFFFFFFFFu) { // this lane owns the key: plain read-modify-write
            for (uint32_t x = 0; x < A.np; ++x) {
              const uint32_t cnt = CP::get(c, x);
              if (cnt) {
                uint32_t* cp = &A.g_counts[(uint64_t)rs * A.np + x];
                gstore(cp, gload(cp) + cnt);
              }
            }
            lds_or(&A.rbitmap[rs >> 5], 1u << (rs & 31u));
          }
        }
        const uint64_t okm = __ballot(ok);
        if (ok) {
          const uint32_t t = nrec + __popcll(okm & lt);
          if (t < tab_cap) {
#pragma unroll
            for (int q = 0; q < KH; ++q)
              if ((uint32_t)q < hw) lo[t * ew + q] = c[q];
            lo[t * ew + hw] = rs;
          } else if (t - tab_cap < ws.gtab_cap) {
            uint32_t* g = gtab + (uint64_t)(t - tab_cap) * ew;
#pragma unroll
            for (int q = 0; q < KH; ++q)
              if ((uint32_t)q < hw) gstore(&g[q], c[q]);
            gstore(&g[hw], rs);
          }
        }
        nrec += __popcll(okm);
      }
      WAVE_SYNC();
    }
    if ((dbg & 512u) && lane == 0) { // statistics for tuning
      atomicAdd(&out.counters[kCtStEvents], nev);
      atomicAdd(&out.counters[kCtStKeys], nkeys);
      atomicAdd(&out.counters[kCtStBatches], KB ? (nkeys + KB - 1) / KB : 0u);
      atomicAdd(&out.counters[kCtStBig], big ? 1u : 0u);
      atomicAdd(&out.counters[kCtStLevelTiles], (uint32_t)__popc(lv) * ((nev + 63) / 64));
      atomicMax(&out.counters[kCtStMaxKeys], nkeys);
      atomicMax(&out.counters[kCtStMaxEvents], nev);
    }
    if (KR_STATS && (dbg & 512u) && lane == 0) {
      atomicAdd(&g_kr_stats[32u + stat_log2(nkeys)], 1u);
      atomicAdd(&g_kr_stats[64u + stat_log2(nrec)], 1u);
      atomicAdd(&g_kr_stats[97], 1u);
    }
    if (fits) {
      fits = nrec <= tab_cap + ws.gtab_cap;
      if (nrec > tab_cap) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    if ((dbg & 512u) && lane == 0) { // path witnesses (all of them here: one at the entry cost the any-threshold instantiation its register allocation)
      atomicAdd(&out.counters[MERGE ? kCtGeEnteredMerge : (PB == 8 ? kCtGeEntered2 : kCtGeEntered1)], 1u);
      if (!fits) atomicAdd(&out.counters[kCtGeNoFit], 1u);
      if (sparse) atomicAdd(&out.counters[kCtGeSparse], 1u);
      if (big) atomicAdd(&out.counters[kCtGeBig], 1u);
      if (fused) atomicAdd(&out.counters[kCtGeFused], 1u);
      if (KB && nkeys > KB) atomicAdd(&out.counters[kCtGeExtraBatches], (nkeys + KB - 1) / KB - 1u);
      if (!kt_lds) atomicAdd(&out.counters[kCtGeKeytabGlobal], 1u);
    }
    if (fits && !MERGE) {
      const uint32_t rbase = nrec ? alloc_records(out, ws, nrec) : 0u;
      if (lane == 0) {
        out.rd_off[read] = rbase == 0xFFFFFFFFu ? 0 : rbase;
        out.rd_cnt[read] = rbase == 0xFFFFFFFFu ? 0 : nrec;
      }
      if (nrec && rbase != 0xFFFFFFFFu && !(dbg & 256u)) {
        for (uint32_t t0 = 0; t0 < nrec; t0 += 64) {
          const uint32_t t = t0 + lane;
          if (t >= nrec) break;
          const uint32_t ri = rbase + t;
          const uint32_t* g = gtab + (uint64_t)(t - tab_cap) * ew;
          const bool in_lds = t < tab_cap;
          const uint32_t rs = in_lds ? lo[t * ew + hw] : gload(&g[hw]);
          out.rec_key[ri] = (ix.leaf_se[rs >> 1] << 1) | (rs & 1u);
          // the likelihood problem in one word (kr_dedup_kernel): five 8-bit counts, #k-mers, bit 63.  With the word the
          // planes and the read index are redundant: 12 bytes per record leave the kernel instead of 36 (they are
          // written when the batch keeps histograms, or when the word cannot hold the problem)
          bool packs = A.np == 5u && onmers < 65536u;
          if (PB != 7) // (a count may reach 256 over two segments: the word holds 8 bits each)
            for (uint32_t x = 0; x < A.np; ++x) {
              const uint32_t w = in_lds ? lo[t * ew + x / CP::CPW] : gload(&g[x / CP::CPW]);
              packs = packs && ((w >> (CP::CB * (x % CP::CPW))) & CP::MASK) < 256u;
            }
          const bool planes = out.hist_always || !packs;
          uint64_t w0 = 0;
          for (uint32_t x = 0; x < A.np; ++x) {
            const uint32_t w = in_lds ? lo[t * ew + x / CP::CPW] : gload(&g[x / CP::CPW]);
            const uint32_t hv = (w >> (CP::CB * (x % CP::CPW))) & CP::MASK;
            if (planes) out.rec_hist[(uint64_t)x * out.rec_stride + ri] = hv;
            if (x < 5) w0 |= (uint64_t)(hv & 255u) << (8u * x);
          }
          if (planes) out.rec_read[ri] = read;
          out.rec_w0[ri] = packs ? (w0 | ((uint64_t)onmers << 40) | (1ull << 63)) : 0ull;
          if (KR_STATS && (dbg & 512u)) stat_records(w0, true);
        }
      }
    }
  } else if (!MERGE && lane == 0) {
    out.rd_off[read] = 0;
    out.rd_cnt[read] = 0;
  }
  WAVE_SYNC();
  return fits;
}

// One position of a key hit twice (finalize_events_fast): the events (rank, strand, position) of vd's group, all in the LDS; the one
// counted so far carries bit 4.  Count and flag move to an event of the group's smallest hd -- among ALL of the group's events, also
// those the pass has not reached yet (they will find the bit set and come here, to no effect).  cnt = the key's two counter words.
// Returns whether count and flag moved (a path witness).
__device__ __noinline__ bool fix_dup(lds_u32* e, uint32_t nev, uint32_t vd, lds_u32* cnt)
{
  const uint32_t lane = lane_id();
  uint32_t best = 0xFFFFFFFFu, win = 0xFFFFFFFFu; // hd << 16 | event index
  for (uint32_t t0 = 0; t0 < nev; t0 += 64) {
    const uint32_t i = t0 + lane;
    if (i < nev) {
      const uint32_t v = e[i];
      if ((v >> 5) == (vd >> 5)) {
        best = min(best, ((v & 7u) << 16) | i);
        if (v & 16u) win = ((v & 7u) << 16) | i;
      }
    }
  }
#pragma unroll
  for (int x = 32; x; x >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, x)), win = min(win, (uint32_t)__shfl_xor((int)win, x));
  if (lane == 0 && win != 0xFFFFFFFFu && (best >> 16) < (win >> 16)) {
    const uint32_t hw = win >> 16, hm = best >> 16;
    cnt[hw >> 2] -= 1u << (8u * (hw & 3u));
    cnt[hm >> 2] += 1u << (8u * (hm & 3u));
    e[win & 0xFFFFu] &= ~16u;
    e[best & 0xFFFFu] |= 16u;
  }
  WAVE_SYNC();
  return win != 0xFFFFFFFFu && (best >> 16) < (win >> 16); // (wave-uniform) count and flag moved
}

#ifndef KR_ACC_BIG_READS
#define KR_ACC_BIG_READS 1
#endif
// finalize_events_fast for a read whose live events overflow the LDS (whole clades reached by one k-mer: up to 20,000 keys a read on the
// 10,000-genome index, 0.7 % of its reads and 30 % of its events).  Five planes of 128 position bits a key in the wave's GLOBAL scratch
// (A.g_planes, all-zero between reads as finalize_events needs it), indexed by the key's ordinal: ONE pass over the events, two tiles
// at a time, nothing in it waits for the L2 -- an or without return on the plane of the event's hd, the key's rank stored into its
// record by every event of the key.  Then one lane per key: a position counts for the lowest plane that has it (what
// Minfo::update_match keeps when a position is hit twice), the record's word, the planes back to zero.
// finalize_events' global planes, which these reads took before, walk the events three times, a tile at a time.
// (Position maps + counters with returning atomics, as in the LDS, were built first: the keys with a position hit twice had to be
//  counted again from the events, and the reads that reach every genome on both strands -- repeats -- have hundreds of those: the
//  launch waited 4 ms for a few such reads of the 1000-genome index, sessions 25-27.)
__device__ __forceinline__ void finish_big_read(lds_u32* e, uint32_t ev_cap, uint32_t* gev, uint32_t* st, lds_u32* bitmap, lds_u16* pre, uint32_t bm_words,
                                             uint32_t rbase, uint32_t nev, uint32_t nkeys, uint32_t read, uint32_t onmers, uint32_t* rec_key,
                                             uint64_t* rec_w0, uint32_t* rec_hist, uint32_t* rec_read, uint64_t rec_stride, bool keep_hist,
                                             const uint32_t* leaf_se)
{
  constexpr uint32_t KS = 12u, kSt = 20u;
  const uint32_t lane = lane_id();
  auto ordinal = [&](uint32_t rs) -> uint32_t { // (key_ordinal)
    const uint32_t blk = rs >> 6;
    return (uint32_t)pre[blk] + __popcll(*(lds_u64*)(bitmap + 2u * blk) & ((1ull << (rs & 63u)) - 1ull));
  };
  if (rbase != 0xFFFFFFFFu) {
    if (nev > ev_cap) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // (the compaction's stores)
    for (uint32_t t0 = 0; t0 < nev; t0 += 128) { // (ev_cap is a multiple of 128 here: a tile is the LDS's or the scratch's)
      uint32_t v[2];
#pragma unroll
      for (uint32_t u = 0; u < 2; ++u) {
        const uint32_t i = t0 + 64u * u + lane;
        v[u] = i < nev ? (t0 < ev_cap ? e[i] : gload(&gev[i - ev_cap])) : 0u;
      }
#pragma unroll
      for (uint32_t u = 0; u < 2; ++u)
        if (t0 + 64u * u + lane < nev) {
          const uint32_t rs = v[u] >> KS, pos = (v[u] >> 5) & 127u, hd = v[u] & 7u;
          const uint32_t o = ordinal(rs);
          mem_or(st + (uint64_t)o * kSt + hd * 4u + (pos & 3u), 1u << (pos >> 2));
          rec_key[rbase + o] = (leaf_se[rs >> 1] << 1) | (rs & 1u);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // every bit has arrived
    const bool packs = onmers < 65536u;
    for (uint32_t j0 = 0; j0 < nkeys; j0 += 64) {
      const uint32_t j = j0 + lane;
      if (j < nkeys) {
        uint64_t* k = (uint64_t*)(st + (uint64_t)j * kSt); // (80 bytes a key: 16-byte aligned)
        // (what the L2 holds, past the CU's cache; in two parts: the function stays within the registers its caller leaves alone)
        uint64_t s0 = 0, s1 = 0, w0 = 0;
        {
          uint64_t pl[6];
#pragma unroll
          for (uint32_t q = 0; q < 6u; ++q) pl[q] = __hip_atomic_load(k + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
          for (uint32_t h = 0; h < 3u; ++h) {
            w0 |= (uint64_t)(__popcll(pl[2u * h] & ~s0) + __popcll(pl[2u * h + 1u] & ~s1)) << (8u * h);
            s0 |= pl[2u * h], s1 |= pl[2u * h + 1u];
          }
        }
        {
          uint64_t pl[4];
#pragma unroll
          for (uint32_t q = 0; q < 4u; ++q) pl[q] = __hip_atomic_load(k + 6u + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
          for (uint32_t h = 0; h < 2u; ++h) {
            w0 |= (uint64_t)(__popcll(pl[2u * h] & ~s0) + __popcll(pl[2u * h + 1u] & ~s1)) << (8u * (3u + h));
            s0 |= pl[2u * h], s1 |= pl[2u * h + 1u];
          }
        }
        const uint32_t ri = rbase + j;
        if (keep_hist || !packs) {
#pragma unroll
          for (uint32_t x = 0; x < 5u; ++x) rec_hist[(uint64_t)x * rec_stride + ri] = (uint32_t)(w0 >> (8u * x)) & 255u;
          rec_read[ri] = read;
        }
        rec_w0[ri] = packs ? (w0 | ((uint64_t)onmers << 40) | (1ull << 63)) : 0ull;
#pragma unroll
        for (uint32_t q = 0; q < 5u; ++q) ((uint4*)k)[q] = make_uint4(0, 0, 0, 0);
      }
    }
  }
  WAVE_SYNC();
  for (uint32_t q = lane; q < bm_words; q += 64) bitmap[q] = 0;
  WAVE_SYNC();
}

// ---------------------------------------------------------------------------
// The epilogue of the COMMON read as straight-line code (round 4; the kernel is bound by instruction issue, docs/design/02, and
// finalize_events is a general loop nest -- key batches, sparse keys, spills to global scratch, the merge form -- whose uniform
// branches and staging table a 150-bp read pays for without using them).  Same steps, same results (src/query.hpp:153-176,
// src/query.cpp:101-106,119): keys marked, ordinals, one pass over the events into per-key state, one lane per key writing its
// record straight from its registers -- no staging table, no second loop.
// Since round 5 it takes every read of threshold 4 but the few whose live events fill the LDS without overflowing it: events of
// keys that cannot pass the hdist_filt test are dropped first (the rest compacted to the front of the LDS), the keys go in batches
// of as many as fit behind the events, a position hit twice is settled in place (fix_dup), and a read whose live events overflow
// the LDS is finished from planes in the wave's global scratch (finish_big_read).  Returns false, with the events possibly
// compacted but no record and no state written, if the read does not qualify: the caller runs finalize_events.
// ---------------------------------------------------------------------------
#ifndef KR_ACC_FAST_EPILOGUE
#define KR_ACC_FAST_EPILOGUE 1
#endif
__device__ __forceinline__ bool finalize_events_fast(const DevIndex& ix, const BatchOut& out, const Acc& A, WaveState& ws, uint32_t read,
                                                     uint32_t onmers, uint32_t filt0, uint32_t filt1, uint32_t dbg)
{
  constexpr uint32_t KS = 12u; // one segment: an event is key << 12 | 7 position bits | 5 hd bits
  const uint32_t lane = lane_id(), np = A.np;
  uint32_t nev = ws.nev;
#ifndef KR_ACC_COMPACT_SPILLED
#define KR_ACC_COMPACT_SPILLED 1
#endif
  const bool spilled = nev > ws.ev_cap; // (wave-uniform) the read's later events lie in the wave's global scratch
  if (nev == 0 || (spilled && !KR_ACC_COMPACT_SPILLED) || np != 5u) return false; // (witnessed by the caller: kCtFpEntered, kCtFpFalseEarly)
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint32_t lim0 = 2u * filt0 + 1u, lim1 = 2u * filt1 + 1u; // u32 wrap keeps "none" = max
  lds_u32* e = ws.ev;
  if (spilled) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // the spilled events are complete
  for (uint32_t q = lane; q < A.bm_words; q += 64) A.bitmap[q] = 0; // (aliases the work stack, empty now)
  WAVE_SYNC();
  // ---- 1. keys that can pass at all (the spilled part four tiles at a time: their loads leave together)
  const uint32_t nev_lds = min(nev, ws.ev_cap);
  auto mark = [&](uint32_t v) {
    const uint32_t rs = v >> KS;
    if ((v & 31u) <= ((rs & 1u) ? lim1 : lim0)) lds_or(&A.bitmap[rs >> 5], 1u << (rs & 31u));
  };
  for (uint32_t i = lane; i < nev_lds; i += 64) mark(e[i]);
  for (uint32_t t0 = ws.ev_cap; t0 < nev; t0 += 256) {
    uint32_t v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) v[u] = t0 + 64u * u + lane < nev ? gload(&ws.gev[t0 + 64u * u + lane - ws.ev_cap]) : 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u)
      if (t0 + 64u * u + lane < nev) mark(v[u]);
  }
  WAVE_SYNC();
  uint32_t nkeys = 0;
  const uint32_t nblk = A.bm_words >> 1;
  for (uint32_t b0 = 0; b0 < nblk; b0 += 64) {
    const uint32_t b = b0 + lane;
    const uint32_t c = b < nblk ? __popcll(*(lds_u64*)(A.bitmap + 2u * b)) : 0u;
    const uint32_t inc = wave_scan_incl(c);
    if (b < nblk) A.pre[b] = (uint16_t)(nkeys + inc - c);
    nkeys += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  }
  // (keys per batch behind n events: seven words a key -- below)
  auto batch_keys = [&](uint32_t n) -> uint32_t { n = (n + 3u) & ~3u; return n < ws.ev_words ? ((ws.ev_words - n) / kFastKeyWords) & ~3u : 0u; };
  if (spilled || batch_keys(nev) < nkeys) {
    witness(out, dbg, kCtFpCompact);
    // Round 5: a read whose events spilled out of the LDS took the general epilogue, every pass of which walks the spilled part
    // through the L2 -- with 512 events in the LDS 31 % of the kernel's time for 7 % of the reads of the 1000-genome index (45 % on
    // the 10,000-genome index: profiles/round5_general_epilogue_ablation.txt).  Two thirds of a read's events belong to keys that
    // cannot pass the hdist_filt test and are dropped by either epilogue: dropped HERE, in one pass and in order, what is left
    // nearly always fits the LDS and the read goes on like any other.  What does not fit goes back to the front of the global
    // scratch (a write lands at or in front of the tile it was read from): the layout finalize_events expects, shorter.
    // The same for a read whose keys do not fit behind its events in one batch.
    uint32_t wpos = 0;
    auto keep = [&](uint32_t v, bool there) {
      const uint32_t rs = v >> KS;
      const bool live = there && ((A.bitmap[rs >> 5] >> (rs & 31u)) & 1u);
      const uint64_t lm = __ballot(live);
      WAVE_SYNC(); // (every lane has read its event)
      const uint32_t p = wpos + (uint32_t)__popcll(lm & lt);
      if (live) {
        if (p < ws.ev_cap)
          e[p] = v;
        else
          gstore(&ws.gev[p - ws.ev_cap], v);
      }
      wpos += (uint32_t)__popcll(lm);
      WAVE_SYNC();
    };
    for (uint32_t t0 = 0; t0 < nev_lds; t0 += 64) keep(t0 + lane < nev_lds ? e[t0 + lane] : 0u, t0 + lane < nev_lds);
    for (uint32_t t0 = ws.ev_cap; t0 < nev; t0 += 256) {
      uint32_t v[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) v[u] = t0 + 64u * u + lane < nev ? gload(&ws.gev[t0 + 64u * u + lane - ws.ev_cap]) : 0u;
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u)
        if (t0 + 64u * u < nev) keep(v[u], t0 + 64u * u + lane < nev);
    }
    ws.nev = nev = wpos; // (whichever epilogue finishes the read sees these events)
    // this one if they are all in the LDS with the room of a batch of 64 keys behind them
    if (nev > ws.ev_cap || batch_keys(nev) < min(nkeys, 64u)) {
      // (finalize_events zeroes the bitmap itself; it keeps the reads whose live events fill the LDS but do not overflow it)
      if (!KR_ACC_BIG_READS || nev <= ws.ev_cap || (ws.ev_cap & 127u)) {
        witness(out, dbg, kCtFpFalseCompacted);
        return false;
      }
      witness(out, dbg, kCtFpBigRead);
      const uint32_t rbase = alloc_records(out, ws, nkeys);
      if (lane == 0) {
        out.rd_off[read] = rbase == 0xFFFFFFFFu ? 0 : rbase;
        out.rd_cnt[read] = rbase == 0xFFFFFFFFu ? 0 : nkeys;
      }
      finish_big_read(e, ws.ev_cap, ws.gev, A.g_planes, A.bitmap, A.pre, A.bm_words, rbase, nev, nkeys, read, onmers, out.rec_key, out.rec_w0,
                      out.rec_hist, out.rec_read, out.rec_stride, out.hist_always != 0, ix.leaf_se);
      return true;
    }
  }
  // Round 5: COUNTS instead of planes.  Minfo::update_match counts, per read position, only the smallest hd among the hits that
  // reach a leaf -- which matters only when one (leaf, strand) is hit twice at ONE position (two entries of a bucket within the
  // threshold whose colours share the leaf: paralogous k-mers).  So a key keeps a 128-bit map of the positions it has seen and its
  // five counters (six words instead of twenty): an event sets its position bit with a RETURNING or; if the bit was clear it
  // counts itself and flags itself as the position's counted event (bit 4 of the word: an hd of this path is at most 4).  An
  // event that finds the bit set has the wave look at the position's events and move count and flag to the smallest hd
  // (fix_dup): exact for any input, no read leaves this epilogue once the pass has begun.  Counters come out in the packing the
  // record wants.
  // Keys in BATCHES of as many as fit behind the events (seven words a key: its rank, the position map's four, the counters' two)
  // -- one batch for nearly every read; the reads of many keys (the spilled ones above, mostly) pass over their events once per
  // batch, all of it in the LDS, where the general epilogue walked planes of twenty words a key and events in global scratch.
  constexpr uint32_t kKeyWords = kFastKeyWords - 1u /* the rank: keytab */, kWinner = 16u;
  const uint32_t st_off = (nev + 3u) & ~3u;
  uint32_t KB = batch_keys(nev);
  if (KB < 64u && KB < nkeys) { // (the keys of a crowded read that was not compacted: more than 768 events, few keys -- not seen)
    WAVE_SYNC();
    return false;
  }
  KB = min(KB, (nkeys + 3u) & ~3u);
  lds_u32* bt = e + st_off;
  lds_u32* keytab = bt + KB * kKeyWords;
  // Every marked key passes the hdist_filt test: it was marked by an event within its strand's limit, and that event or one of a
  // smaller hd at its position is counted, so hdist_min <= the limit: nkeys records, in key order
  const uint32_t nrec = nkeys;
  const uint32_t rbase = nrec ? alloc_records(out, ws, nrec) : 0u;
  if (lane == 0) {
    out.rd_off[read] = rbase == 0xFFFFFFFFu ? 0 : rbase;
    out.rd_cnt[read] = rbase == 0xFFFFFFFFu ? 0 : nrec;
  }
  for (uint32_t k0 = 0; k0 < nkeys; k0 += KB) {
    const uint32_t kb = min(KB, nkeys - k0);
    mem_zero(bt, (kb * kKeyWords + 3u) & ~3u);
    WAVE_SYNC();
    // ---- 2. + 3. ordinals, keys, position maps and counters in one pass over the events
    for (uint32_t t0 = 0; t0 < nev; t0 += 64) {
      const uint32_t i = t0 + lane;
      bool dup = false;
      uint32_t v = 0, o = 0;
      if (i < nev) {
        v = e[i];
        const uint32_t rs = v >> KS;
        if ((A.bitmap[rs >> 5] >> (rs & 31u)) & 1u) {
          o = key_ordinal(A, rs) - k0;
          if (o < kb) {
            keytab[o] = rs;
            const uint32_t pos = (v >> 5) & 127u, hd = v & 7u;
            const uint32_t bit = 1u << (pos >> 2);
            const uint32_t old = __hip_atomic_fetch_or(bt + o * kKeyWords + (pos & 3u), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            dup = (old & bit) != 0;
            if (!dup) {
              __hip_atomic_fetch_add(bt + o * kKeyWords + 4u + (hd >> 2), 1u << (8u * (hd & 3u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              e[i] = v | kWinner;
            }
          }
        }
      }
      uint64_t dm = __ballot(dup);
      if (dm) { // one position twice for a key (rare)
        WAVE_SYNC();
        witness(out, dbg, kCtFpDupCalls, (uint32_t)__popcll(dm));
        do {
          const int l = __builtin_ctzll(dm);
          if (fix_dup(e, nev, (uint32_t)__builtin_amdgcn_readlane((int)v, l), bt + (uint32_t)__builtin_amdgcn_readlane((int)o, l) * kKeyWords + 4u))
            witness(out, dbg, kCtFpDupMoved);
          dm &= dm - 1ull;
        } while (dm);
      }
    }
    WAVE_SYNC();
    // ---- 4. one lane per key: the record
    for (uint32_t j0 = 0; j0 < kb; j0 += 64) { // (one round for nearly every read)
      const uint32_t j = j0 + lane;
      if (j < kb) {
        const uint32_t c0 = bt[j * kKeyWords + 4u], c1 = bt[j * kKeyWords + 5u];
        const uint32_t rs = keytab[j];
        if (kb == nkeys) A.bitmap[rs >> 5] = 0; // the bitmap goes back to all-zero
        if (rbase != 0xFFFFFFFFu) { // ascending ordinal = ascending key
          const uint32_t ri = rbase + k0 + j;
          out.rec_key[ri] = (ix.leaf_se[rs >> 1] << 1) | (rs & 1u);
          const bool packs = onmers < 65536u; // (a count is at most 128: the 8-bit fields hold it)
          const uint64_t w0 = (uint64_t)c0 | ((uint64_t)(c1 & 255u) << 32);
          if (out.hist_always || !packs) {
#pragma unroll
            for (uint32_t x = 0; x < 5u; ++x) out.rec_hist[(uint64_t)x * out.rec_stride + ri] = (uint32_t)(w0 >> (8u * x)) & 255u;
            out.rec_read[ri] = read;
          }
          out.rec_w0[ri] = packs ? (w0 | ((uint64_t)onmers << 40) | (1ull << 63)) : 0ull;
          if (KR_STATS && (dbg & 512u)) stat_records(w0, true);
        }
      }
    }
    if (kb != nkeys) WAVE_SYNC(); // (the next batch zeroes what these lanes read)
  }
  if (KB < nkeys) { // several batches: the ordinals needed the bitmap to the end
    WAVE_SYNC();
    for (uint32_t q = lane; q < A.bm_words; q += 64) A.bitmap[q] = 0;
    witness(out, dbg, kCtFpMultiBatch);
    witness(out, dbg, kCtFpExtraBatches, (nkeys - 1u) / KB);
  } else
    witness(out, dbg, kCtFpOneBatch);
  if (KR_STATS && (dbg & 512u) && lane == 0) { // statistics for tuning: the same counters finalize_events keeps
    atomicAdd(&out.counters[kCtStEvents], nev);
    atomicAdd(&out.counters[kCtStKeys], nkeys);
    atomicAdd(&out.counters[kCtStBatches], 1u);
    atomicMax(&out.counters[kCtStMaxKeys], nkeys);
    atomicMax(&out.counters[kCtStMaxEvents], nev);
    atomicAdd(&g_kr_stats[32u + stat_log2(nkeys)], 1u);
    atomicAdd(&g_kr_stats[64u + stat_log2(nrec)], 1u);
    atomicAdd(&g_kr_stats[96], 1u);
  }
  WAVE_SYNC();
  return true;
}

// ---------------------------------------------------------------------------
// Kernel 2: accumulate.  One wave per read: the read's items (colour, tag) are expanded through the
// colour DAG to leaf events, the events are reduced to per-(leaf, strand) histograms and the
// records that pass the hdist_filt test are written out.
// ---------------------------------------------------------------------------
// fold this segment's planes into running counts (positions of different segments are distinct,
// so histograms add)
__device__ __forceinline__ void segment_fold(const Acc& A, WaveState& ws, bool& l2_any)
{
  WAVE_SYNC();
  if (A.keys[lane_id()]) fold_l1(A, lane_id()); // kLdsSlots == 64: lane t owns slot t
  l2_any = __ballot(ws.l2) != 0;
  if (l2_any) {
    const uint32_t n2 = l2_build_list(A, A.bitmap);
    for (uint32_t t = lane_id(); t < n2; t += 64) fold_l2(A, A.g_list[t]);
  }
  __syncthreads();
}

// MULTI: the instantiation for reads of several segments.  The single-segment instantiation only notes such
// reads in out.long_list (the kernel is launched a second time for them): with both in one kernel the merge code's
// registers cost the common case 5 %.
// PB (single-segment layout only): 7 = reads of one segment; 8 = the instantiation for reads of TWO segments (129..256 k-mer
// positions: 250-bp reads), which works through the list the first launch set aside: events carry 8 position bits, planes
// 256, and the read is finished like a one-segment read -- no merge through the global count table.  Returns true if
// the read is done (PB = 8: false leaves it on the list for the MULTI launch).
// FK: the items are candidates of filter slots (format 9): the colour gather brings the entry's rest bits along, hd is completed
// here, false candidates are dropped and the read's hdist_filt (src/query.cpp:366-368) is taken from the true hits.
template <bool SL, bool MULTI, int PB = 7, bool FK = false>
__device__ __forceinline__ bool process_read(const DevIndex& ix, const DevParams& P, const BatchIn& in,
                                             const BatchOut& out, uint32_t read, const Acc& A, WaveState& ws,
                                             lds_u32* hist_tbl, uint32_t hist_words)
{
  const uint32_t lane = lane_id();
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint64_t len = in.offsets[read + 1] - in.offsets[read];
  const uint32_t k = ix.k;
  const uint64_t nkm = len >= k ? len - k + 1 : 0; // enmers (src/query.cpp:42)
  const uint32_t nit = out.rd_it_cnt[read];
  const uint2* items = out.items + out.rd_it_off[read];
  const uint32_t onmers = out.rd_onmers[read];
  // (FK: what the scan kernel knows -- the bucket tails it verified itself; the candidates verified below complete it.  A tile of
  //  a long sequence is not judged by its own minima: they are left in rd_filt for kr_tile_merge_kernel)
  uint32_t filt0 = out.rd_filt[2 * read], filt1 = out.rd_filt[2 * read + 1];
  const bool is_tile = FK && out.v_tile != nullptr && out.v_tile[read] != 0;
  if (is_tile) filt0 = filt1 = 0xFFFFFFFFu;
  bool l2_any = false; // wave-uniform: some key of this read lives in level 2
  const uint64_t tr0 = (P.dbg & 512u) ? __builtin_readcyclecounter() : 0;
  // Event mode: always for reads of one segment; reads of several segments run it per segment and merge the
  // segments' counts in the wave's global count table (debug bit 8192 sends them to the plane tables instead).
  // set aside for the second launch: list slots in wave-private chunks of 16 (one shared word serves ~90 M atomics/s)
  auto set_aside = [&]() {
    if (ws.ll_next == ws.ll_end) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&out.counters[kCtLongReads], 16u);
      ws.ll_next = __shfl(base, 0);
      ws.ll_end = ws.ll_next + 16u;
    }
    if (lane == 0) out.long_list[ws.ll_next] = read;
    ++ws.ll_next;
    witness(out, P.dbg, kCtRdSetAside);
  };
  // (PB = 8 takes the reads of two segments only: a one-segment read is on the list because it did not fit the first launch,
  //  and would not fit here either; 8192: tests want the plane tables)
  if (!MULTI && (nkm > (uint64_t)(1u << PB) || (P.dbg & 8u) || (PB == 8 && (nkm <= (uint64_t)kSegPos || (P.dbg & 8192u))))) {
    if (PB == 7) set_aside();
    return false;
  }
  const bool multi = MULTI;
  ws.evmode = !MULTI || (!(P.dbg & 8u) && !(P.dbg & 8192u));
  bool merged = false; // wave-uniform: the read's segments were merged through the count table
  // A read is processed once; only if its events do not fit (buffer or tables) is it processed a
  // second time with the plane tables.
  for (;;) {
  if (ws.evmode) {
    ws.dirty = true;
  } else if (MULTI && ws.dirty) { // the plane tables must start empty
    WAVE_SYNC();
    A.keys[lane] = 0;
    for (uint32_t i = lane; i < ws.ev_words; i += 64) A.planes[i] = 0;
    WAVE_SYNC();
    ws.dirty = false;
  }
  ws.top = 0;
  ws.l2 = false;
  ws.nev = 0;
  ws.ev_full = false;
  uint32_t hd_seen = 0; // FK: bit (8 * strand + hd) for every verified hit this lane saw
  bool seg_ok = true; // every segment so far went through the event epilogue
  bool seg2 = false;  // (PB = 8) wave-uniform: the marker of the second segment has been seen
  // the segment before a marker (or the last one) is complete
  auto segment_done = [&]() {
    if (MULTI && !ws.evmode) {
      segment_fold(A, ws, l2_any);
    } else if (multi) {
      seg_ok = seg_ok && !ws.ev_full &&
               finalize_events<true>(ix, out, A, ws, hist_tbl, hist_words, read, onmers, 0xFFFFFFFFu, 0xFFFFFFFFu, P.dbg); // (MERGE: no limits)
      ws.nev = 0;
      ws.ev_full = false;
    }
  };
#if KR_ACC_PIPE
  // Two-stage read-ahead over the read's item tiles: the items of tile t+2 and the colour gather of tile t+1 are in
  // flight while tile t is expanded (a 150-bp read has ~71 items = two tiles: both item loads leave at once, both
  // gathers follow together, instead of items -> colours -> expansion twice in a row).
  auto load_item = [&](uint32_t i) -> uint2 { return i < nit ? items[i] : make_uint2(0, kItemMarker); };
  // the colour of the table entry the scan kernel matched; FK: {colour, rest bits} of the slot entry it found a candidate in
  // (.y unused otherwise: the compiler drops it)
  auto load_se = [&](uint32_t i, uint2 v) -> uint2 {
    if (i >= nit || (v.y & kItemMarker)) return make_uint2(0u, 0u);
    if (FK) {
      const uint64_t idx = (uint64_t)v.x | ((uint64_t)((v.y >> 23) & 0xFFu) << 32);
      if (((v.y >> 12) & 7u) == 7u) return make_uint2(get_lib<SL>(ix, tag_lib(v.y)).se[idx], 0u); // a verified entry of the packed arrays
      return get_lib<SL>(ix, tag_lib(v.y)).sx[idx];
    }
    return make_uint2(get_lib<SL>(ix, tag_lib(v.y)).se[(uint64_t)v.x | ((uint64_t)((v.y >> 17) & 0xFFu) << 32)], 0u);
  };
  // the item's tag in the form the expansion uses (pos | strand << 7 | lib << 8 | hd << 12); FK: hd completed, false if beyond th
  auto item_tag = [&](uint2 it_, uint2 sv, uint32_t& tagv) -> bool {
    if (!FK) {
      tagv = it_.y & 0x1FFFFu;
      return true;
    }
    const uint32_t h3 = (it_.y >> 12) & 7u;
    const uint32_t hd = h3 == 7u ? (it_.y >> 15) & 31u : h3 + hd_rest8(sv.y, (it_.y >> 15) & 0xFFu);
    tagv = (it_.y & 0xFFFu) | (hd << 12);
    return hd <= P.th;
  };
  const uint32_t nit_eff = (P.dbg & 2u) ? 0u : nit;
  uint2 it_a = load_item(lane), it_b = load_item(64u + lane);
  uint2 se_a = load_se(lane, it_a);
  for (uint32_t t0 = 0; t0 < nit_eff; t0 += 64) {
    const uint32_t i = t0 + lane;
    const bool valid = i < nit;
    const uint2 it = it_a;
    const uint2 sv = se_a;
    const uint32_t se = sv.x;
    it_a = it_b;
    se_a = load_se(i + 64u, it_a);     // tile t+1: its items arrived an iteration ago
    it_b = load_item(i + 128u);        // tile t+2
    const bool marker = (it.y & kItemMarker) != 0;
    uint32_t tagv0 = 0;
    const bool hit = item_tag(it, sv, tagv0) && valid && !marker; // (FK: a true hit)
    if (FK && hit) hd_seen |= 1u << (8u * tag_strand(tagv0) + tag_hd(tagv0));
    uint64_t todo = __ballot(valid);
#else
  for (uint32_t t0 = 0; t0 < ((P.dbg & 2u) ? 0u : nit); t0 += 64) {
    const uint32_t i = t0 + lane;
    const bool valid = i < nit;
    uint2 it = make_uint2(0, kItemMarker);
    if (valid) it = items[i];
    const bool marker = (it.y & kItemMarker) != 0;
    static_assert(!FK, "filter slots need the read-ahead form of the item loop (KR_ACC_PIPE)");
    uint32_t se = 0;
    if (valid && !marker) // the colour of the table entry the scan kernel matched
      se = get_lib<SL>(ix, tag_lib(it.y)).se[(uint64_t)it.x | ((uint64_t)((it.y >> 17) & 0xFFu) << 32)];
    const uint32_t tagv0 = it.y & 0x1FFFFu;
    const bool hit = valid && !marker;
    uint64_t todo = __ballot(valid);
#endif
    if (!MULTI && KR_ACC_LEAN_STEP) { // one segment: no markers, always event mode
      if (ws.top + 128u > ws.stack_cap) expand_all<SL, true, PB>(ix, A, ws);
      uint32_t tagv = tagv0;
      if (PB == 8) { // two segments: the items behind the marker belong to the second one (bit 17 of the tag: make_event)
        const uint64_t mk = __ballot(valid && marker);
        if (seg2 || (mk & ((1ull << lane) - 1ull)) != 0) tagv |= 1u << 17;
        seg2 = seg2 || mk != 0;
      }
      expand_step_ev<SL, PB>(ix, A, ws, hit, se, tagv);
      continue;
    }
    for (;;) { // markers (reads of more than one segment only) split the tile
      const uint64_t mk = __ballot(valid && marker) & todo;
      const uint64_t upto = mk ? (1ull << (__ffsll((long long)mk) - 1)) - 1ull : ~0ull;
      if (ws.top + 128u > ws.stack_cap) expand_all<SL>(ix, A, ws);
      expand_step<SL>(ix, A, ws, hit && ((todo & upto) >> lane & 1ull), se, tagv0);
      if (mk == 0) break;
      expand_all<SL>(ix, A, ws);
      segment_done();
      todo &= ~(upto | (upto + 1ull));
    }
  }
  if (!MULTI && KR_ACC_LEAN_STEP)
    expand_all<SL, true, PB>(ix, A, ws);
  else
    expand_all<SL>(ix, A, ws);
  if (FK) { // hdist_filt of the true hits (the same on every pass of the redo loop), for the limits below and for the taps
    const uint32_t seen = wave_or(hd_seen);
    const uint32_t m0 = (seen & 0xFFu) ? (uint32_t)__ffs((int)(seen & 0xFFu)) - 1u : 0xFFFFFFFFu;
    const uint32_t m1 = (seen & 0xFF00u) ? (uint32_t)__ffs((int)((seen >> 8) & 0xFFu)) - 1u : 0xFFFFFFFFu;
    if (is_tile) { // judged by its sequence's minima in kr_tile_merge_kernel: leave the tile's own beside what the scan moved aside
      if (lane == 0) out.rd_filt[2 * read] = m0, out.rd_filt[2 * read + 1] = m1;
    } else {
      filt0 = min(filt0, m0), filt1 = min(filt1, m1);
      if (lane == 0) out.rd_filt[2 * read] = filt0, out.rd_filt[2 * read + 1] = filt1;
    }
  }
  if (MULTI) segment_done();
  if (ws.err && lane == 0) atomicOr(&out.counters[kCtErr], ws.err);
  ws.err = 0;
  if (MULTI && !ws.evmode) break;
  if (multi) {
    if (seg_ok) { // records from the merged counts, below
      merged = true;
      break;
    }
    // a segment did not fit: take back what the others added, then the plane tables
    const uint32_t n2 = l2_build_list(A, A.rbitmap);
    for (uint32_t t = lane; t < n2; t += 64)
      for (uint32_t x = 0; x < A.np; ++x) gstore(&A.g_counts[(uint64_t)A.g_list[t] * A.np + x], 0);
    for (uint32_t w = lane; w < A.bm_words; w += 64) A.rbitmap[w] = 0;
    __syncthreads();
    ws.evmode = false;
    witness(out, P.dbg, kCtRdPlaneRedo);
    continue;
  }
  if (P.dbg & 16u) ws.nev = 0, ws.ev_full = false;
  if ((P.dbg & 32u) && ws.ev_full) ws.nev = 0, ws.ev_full = false;
  const uint64_t tf0 = (P.dbg & 512u) ? __builtin_readcyclecounter() : 0;
  // path witnesses: finalize_events_fast is called below, and returns at once (counted here: inside it, or behind the call, they cost
  // an instantiation its register allocation)
  if (KR_ACC_FAST_EPILOGUE && !MULTI && PB == 7 && !ws.ev_full && !(P.dbg & ~(2u | 512u)) && (P.dbg & 512u) && lane == 0) {
    atomicAdd(&out.counters[kCtFpEntered], 1u);
    if (ws.nev == 0 || A.np != 5u) atomicAdd(&out.counters[kCtFpFalseEarly], 1u);
  }
  const bool fin_ok = !ws.ev_full && ((KR_ACC_FAST_EPILOGUE && !MULTI && PB == 7 && !(P.dbg & ~(2u | 512u)) && finalize_events_fast(ix, out, A, ws, read, onmers, filt0, filt1, P.dbg)) ||
                                      finalize_events<false, PB>(ix, out, A, ws, hist_tbl, hist_words, read, onmers, filt0, filt1, P.dbg));
  if ((P.dbg & 512u) && lane == 0) {
    const uint64_t tf1 = __builtin_readcyclecounter();
    atomicAdd(&out.counters[kCtCycFinalize], (uint32_t)((tf1 - tf0) >> 6));
    atomicAdd(&out.counters[kCtCycRead], (uint32_t)((tf1 - tr0) >> 6));
    if (KR_STATS) atomicAdd(&g_kr_stats[stat_log2(ws.nev)], 1u);
    if (KR_STATS && !fin_ok) atomicAdd(&g_kr_stats[ws.ev_full ? 98 : 99], 1u);
  }
  if (fin_ok) return true;
  if (!MULTI) { // does not fit: the last launch has the plane tables
    if (PB == 7) set_aside();
    return false;
  }
  ws.evmode = false; // does not fit: redo the read with the plane tables
  witness(out, P.dbg, kCtRdPlaneRedo);
  } // redo loop
  if (!MULTI) return true; // (unreachable: keeps the plane code out of this instantiation)
  // records that pass `hdist_min <= 2*hdist_filt+1` (src/query.cpp:101-106,119), ordered by key so
  // that the two strands of a leaf are adjacent
  const uint32_t lim0 = 2u * filt0 + 1u, lim1 = 2u * filt1 + 1u; // u32 wrap keeps "none" = max

  if (!l2_any && !merged) {
    // ---- level 1 only: lane t owns slot t
    const uint32_t key = A.keys[lane]; // (rank + 1) << 1 | strand: ascending key == ascending colour id
    const bool ok = key && hmin_l1(A, lane) <= ((key & 1u) ? lim1 : lim0);
    uint64_t okm = __ballot(ok);
    const uint32_t nrec = __popcll(okm);
    const uint32_t rbase = nrec ? alloc_records(out, ws, nrec) : 0u;
    if (lane == 0) {
      out.rd_off[read] = rbase == 0xFFFFFFFFu ? 0 : rbase;
      out.rd_cnt[read] = rbase == 0xFFFFFFFFu ? 0 : nrec;
    }
    uint32_t rank = 0; // number of passing keys smaller than mine
    while (okm) {
      int u = __ffsll((long long)okm) - 1;
      uint32_t kb = __shfl(key, u);
      rank += (kb < key) ? 1u : 0u;
      okm &= okm - 1;
    }
    if (ok && rbase != 0xFFFFFFFFu) {
      uint32_t ri = rbase + rank;
      out.rec_key[ri] = (ix.leaf_se[(key >> 1) - 1u] << 1) | (key & 1u);
      uint64_t w0 = 0; // the likelihood problem in one word (kr_dedup_kernel), if the counts fit 8 bits
      bool fit = A.np == 5u && onmers < 65536u;
      for (uint32_t x = 0; x < A.np; ++x) {
        const uint32_t hv = A.counts[lane * A.np + x];
        fit = fit && hv < 256u;
        if (x < 5) w0 |= (uint64_t)(hv & 255u) << (8u * x);
      }
      if (out.hist_always || !fit) { // (see finalize_events: a record with a word needs neither)
        out.rec_read[ri] = read;
        for (uint32_t x = 0; x < A.np; ++x) out.rec_hist[(uint64_t)x * out.rec_stride + ri] = A.counts[lane * A.np + x];
      }
      out.rec_w0[ri] = fit ? (w0 | ((uint64_t)onmers << 40) | (1ull << 63)) : 0ull;
    }
    if (key) { // leave the slot empty for the next read
      A.keys[lane] = 0;
      for (uint32_t x = 0; x < A.np; ++x) A.counts[lane * A.np + x] = 0;
    }
    WAVE_SYNC();
    return true;
  }

  // ---- level 2 in use (or segments merged through the count table): move the level-1 entries over, then emit
  //      from the sorted slot list
  lds_u32* const bitmap = merged ? A.rbitmap : A.bitmap;
  if (!merged) {
    const uint32_t key = A.keys[lane];
    if (key) {
      uint32_t slot2 = key - 2u;
      for (uint32_t x = 0; x < A.np; ++x) {
        uint32_t c = A.counts[lane * A.np + x];
        if (c) {
          uint32_t* cp = &A.g_counts[(uint64_t)slot2 * A.np + x];
          gstore(cp, gload(cp) + c);
          A.counts[lane * A.np + x] = 0;
        }
      }
      lds_or(&A.bitmap[slot2 >> 5], 1u << (slot2 & 31));
      A.keys[lane] = 0;
    }
    __syncthreads();
  }
  const uint32_t n2 = l2_build_list(A, bitmap);
  uint32_t nrec = 0;
  for (uint32_t t0 = 0; t0 < n2; t0 += 64) {
    uint32_t t = t0 + lane;
    bool ok = false;
    if (t < n2) {
      uint32_t slot2 = A.g_list[t];
      ok = hmin_l2(A, slot2) <= ((slot2 & 1u) ? lim1 : lim0);
    }
    nrec += __popcll(__ballot(ok));
  }
  if (!merged) ws.n_l2++;
  const uint32_t rbase = nrec ? alloc_records(out, ws, nrec) : 0u;
  if (lane == 0) {
    out.rd_off[read] = rbase == 0xFFFFFFFFu ? 0 : rbase;
    out.rd_cnt[read] = rbase == 0xFFFFFFFFu ? 0 : nrec;
  }
  uint32_t run = 0;
  for (uint32_t t0 = 0; t0 < n2; t0 += 64) {
    uint32_t t = t0 + lane;
    bool ok = false;
    uint32_t slot2 = 0;
    if (t < n2) {
      slot2 = A.g_list[t];
      ok = hmin_l2(A, slot2) <= ((slot2 & 1u) ? lim1 : lim0);
    }
    uint64_t okm = __ballot(ok);
    if (ok && rbase != 0xFFFFFFFFu) {
      uint32_t ri = rbase + run + __popcll(okm & lt);
      out.rec_key[ri] = (ix.leaf_se[slot2 >> 1] << 1) | (slot2 & 1u);
      uint64_t w0 = 0;
      bool fit = A.np == 5u && onmers < 65536u;
      for (uint32_t x = 0; x < A.np; ++x) {
        const uint32_t hv = gload(&A.g_counts[(uint64_t)slot2 * A.np + x]);
        fit = fit && hv < 256u;
        if (x < 5) w0 |= (uint64_t)(hv & 255u) << (8u * x);
      }
      if (out.hist_always || !fit) {
        out.rec_read[ri] = read;
        for (uint32_t x = 0; x < A.np; ++x) out.rec_hist[(uint64_t)x * out.rec_stride + ri] = gload(&A.g_counts[(uint64_t)slot2 * A.np + x]);
      }
      out.rec_w0[ri] = fit ? (w0 | ((uint64_t)onmers << 40) | (1ull << 63)) : 0ull;
    }
    if (t < n2)
      for (uint32_t x = 0; x < A.np; ++x) gstore(&A.g_counts[(uint64_t)slot2 * A.np + x], 0);
    run += __popcll(okm);
  }
  for (uint32_t w = lane; w < A.bm_words; w += 64) bitmap[w] = 0;
  __syncthreads();
  return true;
}

// NP = th + 1 planes when known at compile time (5: --hdist-th default; the plane loops unroll and the address
// arithmetic folds), 0 = any threshold.
// Three launches per batch: <MULTI = false, PB = 7> every read (those of more than one segment are listed in out.long_list);
// <false, 8> the listed reads of two segments (done ones are struck off the list); <true, 7> what is left on the list.
template <bool SL, int NP, bool MULTI, int PB = 7, bool FK = false>
__global__ __launch_bounds__(kWave, (MULTI || PB == 8 ? 4 : KR_ACC_LEAN_WPE)) void kr_acc_kernel_t(DevIndex ix, DevParams P, BatchIn in, BatchOut out)
{
  static_assert(!MULTI || PB == 7, "the position width is a property of the single-segment layout");
  constexpr bool LISTED = MULTI || PB == 8; // works through out.long_list
  if (NP) P.np = NP, P.th = NP - 1;
  // One carve of dynamic LDS (base is 16-byte aligned: no static __shared__ in front):
  //   MULTI : stack | level-1 table (keys, planes, counts) | level-2 bitmap | read bitmap | ordinal prefix
  //   !MULTI: stack (the key bitmap and its prefix alias its start: the stack is empty in the epilogue)
  //           | table region for the passing keys (the level-1 key slots) | event / batch region
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  KR_LDS uint8_t* s_base = (KR_LDS uint8_t*)s_dyn;
  lds_u64* s_stack = (lds_u64*)s_base;
  const uint32_t stack_bytes = MULTI ? kStackCap * 8u : lean_stack_bytes(out.bm_words);
  lds_u32* s_tbl = (lds_u32*)(s_base + stack_bytes);

  Acc A;
  A.np = P.np;
  A.keys = s_tbl;
  A.planes = A.keys + kLdsSlots;
  A.counts = A.planes + kLdsSlots * P.np * kPlaneWords;
  A.bitmap = MULTI ? A.counts + kLdsSlots * P.np : (lds_u32*)s_base;
  A.rbitmap = A.bitmap + out.bm_words; // MULTI only
  A.pre = (lds_u16*)((MULTI ? A.rbitmap : A.bitmap) + out.bm_words);
  A.nslots2 = out.nslots2;
  A.bm_words = out.bm_words;
  const uint64_t w = blockIdx.x;
  A.g_planes = out.g_planes + w * (uint64_t)out.nslots2 * P.np * kPlaneWords;
  A.g_counts = out.g_counts + w * (uint64_t)out.nslots2 * P.np;
  A.g_list = out.g_list + w * (uint64_t)out.g_list_words;
  if (MULTI)
  { // tables start empty; every read leaves them empty again
    const uint32_t lane = lane_id();
    A.keys[lane] = 0;
    for (uint32_t x = 0; x < P.np; ++x) {
      A.counts[lane * P.np + x] = 0;
#pragma unroll
      for (int q = 0; q < kPlaneWords; ++q) A.planes[(lane * P.np + x) * kPlaneWords + q] = 0;
    }
    for (uint32_t q = lane; q < A.bm_words; q += 64) A.bitmap[q] = 0, A.rbitmap[q] = 0;
  }
  __syncthreads();
  WaveState ws;
  ws.stack = s_stack;
  ws.stack_cap = stack_bytes / 8u;
  ws.lean = !MULTI;
  ws.top = 0;
  ws.gstk = out.stk_spill + w * (uint64_t)kStackSpill;
  ws.gs_top = 0;
  ws.l2 = false;
  ws.err = 0;
  ws.rec_next = 0;
  ws.rec_end = 0;
  ws.n_l2 = 0;
  ws.n_rec = 0;
  ws.n_spill = 0;
  ws.ll_next = ws.ll_end = 0;
  ws.evmode = false;
  ws.nev = 0;
  ws.ev = A.planes; // planes + counts are contiguous: kLdsSlots * np * 5 words
  const AccLayout lay = acc_layout(P.np, PB == 8 ? 2u : 1u, MULTI);
  ws.ev_words = lay.ev_words;
  ws.ev_cap = lay.ev_cap;
  ws.dirty = false;
  ws.gev = A.g_list;
  ws.gev_cap = out.ev_spill;
  ws.gtab_cap = out.tab_spill;
  ws.gkt_cap = out.kt_spill;
  ReadCursor rc;
  // later launches: the reads the first one set aside (their number is final: kernel boundary)
  rc.init(out.cursors + (MULTI ? kCurAccMerge : (PB == 8 ? kCurAcc2 : kCurAcc1)) * kCursors * kCursorStride, LISTED ? out.counters[kCtLongReads] : in.nreads, blockIdx.x, 8u);
  uint32_t r0, r1;
  while (rc.next(r0, r1))
    for (uint32_t r = r0; r < r1; ++r)
    {
#ifndef KR_ACC_SCALAR_READ
#define KR_ACC_SCALAR_READ 1
#endif
      // the read index is wave-uniform: told so, its metadata come by scalar loads and the loops over its items, events
      // and keys branch on scalar conditions instead of lane masks
      const uint32_t rd = KR_ACC_SCALAR_READ ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(LISTED ? out.long_list[r] : r)) : (LISTED ? out.long_list[r] : r);
      if (rd != 0xFFFFFFFFu) { // else: unused list slot, or a read an earlier launch has done
        const bool done = process_read<SL, MULTI, PB, FK>(ix, P, in, out, rd, A, ws, (lds_u32*)s_base, stack_bytes / 4u + kLdsSlots);
        if (!MULTI && PB == 8 && done && lane_id() == 0) out.long_list[r] = 0xFFFFFFFFu;
      }
    }
  for (uint32_t q = ws.ll_next + lane_id(); q < ws.ll_end; q += 64) out.long_list[q] = 0xFFFFFFFFu;
  if (ws.n_l2 && lane_id() == 0) atomicAdd(&out.counters[kCtL2Reads], ws.n_l2);
  if (ws.n_rec && lane_id() == 0) atomicAdd(&out.counters[kCtRecords], ws.n_rec);
  if (ws.n_spill && lane_id() == 0) atomicAdd(&out.counters[kCtStackSpills], ws.n_spill);
}

