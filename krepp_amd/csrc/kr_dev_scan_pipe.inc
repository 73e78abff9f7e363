// kr_dev_scan_pipe.inc -- part of kr_device.hip (included after kr_dev_scan.inc): the slotted table scan as a software
// pipeline across probe groups.
//
// kr_scan_kernel_t handles a read's groups one after the other: front end -> probe list -> for every pass {load one pass
// of slots, wait, test} -> resolve the hits.  Only a pass's loads (4 KB per wave) are ever in flight, and nothing is while
// the wave computes a front end or resolves hits: the kernel hides HBM latency by occupancy alone and so needs every
// register of the SIMD (4 waves x 128 VGPRs).  Here a wave keeps DEPTH passes of slot loads in flight AT ALL TIMES, across
// groups and reads:
//
//      F(g+1)   front end + probe list of the NEXT group (second LDS list)      } while the loads of group g are in flight
//      T(g)     hit test of group g's passes (waits for them)
//      L(g+1)   the next group's slot loads leave as soon as the registers are free
//      R(g)     hit chunks of group g dealt out, re-read (L2), items emitted    } while the loads of group g+1 are in flight
//
// The base bytes of the next segment are requested one group ahead (3 VGPRs), so that no wait inside F() falls behind
// the slot loads issued before it (vector loads return in order).  (Built so that the scan could share a SIMD's registers
// with the accumulate / likelihood kernels of the previous batch: at half the resident waves it loses 26 % instead of
// 33 %; run side by side, every split of the registers was slower than the kernels one after the other -- DESIGN.md 3.7 --
// but at full occupancy the pipeline alone is 16 % faster than the kernel it replaces.)
//
// Semantics are those of scan_read<..., SLOT = true> (same items per read, same per-read results); the order of a read's
// items is the same too (groups in order, the tail of an over-long bucket before the group's other hits).

// DEPTH = passes of slot loads (CPL x 16 bytes per lane each) a wave keeps in flight; WPE = resident waves per SIMD the
// registers are sized for.  Measured on the 10 GB index, ms per 8 M reads, kernel alone (DESIGN.md 3.1b):
//   DEPTH 1, WPE 4 (127 VGPRs): 40.5 at 4 waves per SIMD, 45.0 at 3, 58.8 at 2   <- built (48.0 / 52.3 / 63.9 without the pipeline)
//   DEPTH 2, WPE 3 (160 VGPRs): 41.7 at 3 waves per SIMD, 51.2 at 2
//   DEPTH 2 in 128 VGPRs spills (67 ms); DEPTH 4, WPE 2 (227 VGPRs): 48.5 at 2 waves per SIMD
#ifndef KR_SCAN_DEPTH
#define KR_SCAN_DEPTH 1
#endif
#ifndef KR_SCAN_PIPE_WPE
#define KR_SCAN_PIPE_WPE 4
#endif
#ifndef KR_SCAN_PIPE_FE
#define KR_SCAN_PIPE_FE 2 // front end: byte tables in LDS (0: windows + software PEXT as before round 4)
#endif

struct SlotList { // probe list of one group, slotted table: the row is the address
  lds_u32* row; // [kListCap]
  lds_u32* q;   // [kListCap] residual code of the query k-mer
  lds_u32* tag; // [kListCap] pos | strand<<7 | lib<<8
};
struct GroupDesc { // wave-uniform
  uint32_t nact, read, base0, slot;
  bool last; // the read's last group: its per-read results are complete after this group's hits
};

struct SegRaw {
  uint32_t c[3];
};
__device__ __forceinline__ SegRaw segment_request(const uint8_t* seq, uint64_t len, uint64_t base0)
{
  SegRaw raw;
  const uint32_t lane = lane_id();
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const uint64_t bi = base0 + 64u * p + lane;
    raw.c[p] = 0x80u; // (beyond the read: not a base)
    if (bi < len) raw.c[p] = seq[bi];
  }
  return raw;
}
__device__ __forceinline__ void segment_bits(const SegRaw& raw, SegBits& sb)
{
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const uint32_t code = base_code(raw.c[p]);
    sb.L[p] = __ballot(code & 1u && code < 4);
    sb.H[p] = __ballot((code >> 1) & 1u && code < 4);
    sb.N[p] = __ballot(code >= 4);
  }
}

// The groups of the reads [r0, r1) of one visit, in order.  Every read yields at least one group (possibly empty), so
// that its per-read results are written by the same path.
// FE: the front end (kr_dev_common.inc): 0 per-lane windows + software PEXTs, 1 bit planes, 2 byte tables in LDS (`tab`)
template <bool SL, int FE = 0>
struct GroupGen {
  const lds_u32x4* tab = nullptr;
  uint32_t r, r0, r1;   // next read to start; the visit
  bool in_read;         // (wave-uniform state throughout)
  const uint8_t* seq;
  uint64_t len, nkm, base0;
  uint32_t pp, npos_seg, onmers;
  SegBits sb;
  SegRaw raw;           // requested bytes of the segment the next group starts (raw_valid)
  bool raw_valid;

  __device__ __forceinline__ void init(uint32_t a, uint32_t b)
  {
    r = r0 = a, r1 = b, in_read = false, raw_valid = false;
    seq = nullptr, len = nkm = base0 = 0, pp = npos_seg = onmers = 0;
  }
  __device__ __forceinline__ void open_read(const DevIndex& ix, const BatchIn& in)
  {
    const uint64_t off0 = in.offsets[r], off1 = in.offsets[r + 1];
    seq = in.bases + off0;
    len = off1 - off0;
    nkm = len >= ix.k ? len - ix.k + 1 : 0; // enmers (src/query.cpp:42)
    base0 = 0, pp = 0, onmers = 0;
    in_read = true;
  }
  // request the bytes the NEXT call of next() will need, if it starts a segment (call after next())
  __device__ __forceinline__ void prefetch(const DevIndex& ix, const BatchIn& in)
  {
    if (raw_valid) return;
    if (!in_read) {
      if (r >= r1) return;
      open_read(ix, in);
    }
    if (pp == 0 && nkm != 0) {
      raw = segment_request(seq, len, base0);
      raw_valid = true;
    }
  }
  __device__ __forceinline__ bool next(const DevIndex& ix, const DevParams& P, const BatchIn& in, const SlotList& L, lds_u32* meta, GroupDesc& g)
  {
    const uint32_t lane = lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
    if (!in_read) {
      if (r >= r1) return false;
      open_read(ix, in);
    }
    uint32_t nact = 0;
    bool more_pp = false;
    if (nkm != 0) {
      if (pp == 0) {
        if (!raw_valid) raw = segment_request(seq, len, base0);
        raw_valid = false;
        npos_seg = (uint32_t)min((uint64_t)kSegPos, nkm - base0);
        segment_bits(raw, sb);
      }
      uint32_t nv = 0;
      const Cand cur = FE == 2 ? fetch_group_tab<SL>(ix, tab, sb, pp, npos_seg, nv)
                               : (FE == 1 ? fetch_group_planes<SL>(ix, sb, pp, npos_seg, nv) : fetch_group_sel<SL, true>(ix, sb, pp, npos_seg, nv));
      onmers += nv;
      const bool a0 = cur.b0 != 0, a1 = cur.b1 != 0;
      const uint64_t m0 = __ballot(a0), m1 = __ballot(a1);
      const uint32_t n0 = __popcll(m0);
      nact = n0 + __popcll(m1);
      if (a0) {
        const uint32_t i = __popcll(m0 & lt);
        L.row[i] = (uint32_t)cur.b0;
        L.q[i] = cur.q0;
        L.tag[i] = (64u * pp + lane) | (cur.lib0 << 8);
      }
      if (a1) {
        const uint32_t i = n0 + __popcll(m1 & lt);
        L.row[i] = (uint32_t)cur.b1;
        L.q[i] = cur.q1;
        L.tag[i] = (64u * pp + lane) | (1u << 7) | (cur.lib1 << 8);
      }
      more_pp = pp == 0 && npos_seg > 64u;
    }
    g.nact = (P.dbg & 4u) ? 0u : nact;
    g.read = r, g.base0 = (uint32_t)base0, g.slot = r - r0;
    g.last = false;
    if (more_pp) {
      pp = 1;
    } else {
      pp = 0;
      base0 += kSegPos;
      if (base0 >= nkm) {
        g.last = true;
        if (lane == 0) meta[2 * kReadChunk + g.slot] = onmers;
        in_read = false;
        ++r;
      }
    }
    WAVE_SYNC();
    return true;
  }
};

// the slot loads of passes [c * DEPTH, (c + 1) * DEPTH) of a group
template <int LOG_G, int CPL, int DEPTH, bool SL>
__device__ __forceinline__ void pipe_issue(const DevIndex& ix, const SlotList& L, uint32_t nact, uint32_t c, uint4 (&v)[DEPTH * CPL])
{
  constexpr uint32_t G = 1u << LOG_G, PPS = 64u >> LOG_G, W = scan_slot_words(LOG_G, CPL);
  const uint32_t lane = lane_id(), sub = lane & (G - 1u);
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    const uint32_t pi = (c * DEPTH + (uint32_t)d) * PPS + (lane >> LOG_G);
    const bool on = pi < nact;
    const uint32_t row = on ? L.row[pi] : 0u;
    const uint32_t* slot = get_lib<SL>(ix, SL ? 0u : tag_lib(L.tag[on ? pi : 0u])).slots + (uint64_t)row * W;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      v[d * CPL + j] = make_uint4(0, 0, 0, 0);
      if (on) v[d * CPL + j] = *reinterpret_cast<const uint4*>(slot + 4u * (sub + (uint32_t)j * G));
    }
  }
}

// hit test of those passes; returns the hit bits (bit (p * CPL + j) of the group's 64-bit word, already shifted)
template <int LOG_G, int CPL, int DEPTH, bool SL, bool TAP>
__device__ __forceinline__ uint64_t pipe_test(const DevIndex& ix, const DevParams& P, const BatchOut& out, ScanWave& sw, const SlotList& L,
                                              const GroupDesc& g, uint32_t c, const uint4 (&v)[DEPTH * CPL])
{
  constexpr uint32_t G = 1u << LOG_G, PPS = 64u >> LOG_G, W = scan_slot_words(LOG_G, CPL), CAP = scan_slot_cap(LOG_G, CPL);
  const uint32_t lane = lane_id(), sub = lane & (G - 1u);
  uint64_t bits = 0;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    const uint32_t p = c * DEPTH + (uint32_t)d;
    const uint32_t pi = p * PPS + (lane >> LOG_G);
    const bool on = pi < g.nact;
    const uint32_t q = on ? L.q[pi] : 0u;
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const uint4 w = v[d * CPL + j];
      const uint32_t m = min(min(hd_lr32(w.x, q), hd_lr32(w.y, q)), min(hd_lr32(w.z, q), hd_lr32(w.w, q)));
      r |= (m <= P.th && on) ? (1u << j) : 0u;
    }
    bits |= (uint64_t)r << (p * CPL);
    // ---- buckets longer than the slot: the rest from the packed array, resolved on the spot (Poisson tail, ~1e-4)
    const uint32_t blen0 = v[d * CPL].x;
    if (__ballot(on && sub == 0 && blen0 > CAP) != 0) {
      const uint32_t blen = __shfl(blen0, lane & ~(G - 1u)), bstart = __shfl(v[d * CPL].y, lane & ~(G - 1u));
      const bool lg = on && blen > CAP;
      const uint64_t st = (uint64_t)bstart + CAP;
      const uint64_t e_al = st & ~3ull;
      const int rel0 = (int)(st & 3u), tot = rel0 + (lg ? (int)(blen - CAP) : 0);
      const uint32_t nch = lg ? (uint32_t)(tot + 3) >> 2 : 0u;
      const uint32_t tg = L.tag[on ? pi : 0u];
      const DevLib Lb = get_lib<SL>(ix, SL ? 0u : tag_lib(tg));
      for (uint32_t cc = sub; __ballot(cc < nch) != 0; cc += G) {
        uint32_t pend = 0, hds = 0;
        if (cc < nch) {
          const uint4 w = *reinterpret_cast<const uint4*>(Lb.enc + e_al + 4u * cc);
          pend = chunk_hits(w, rel0 - 4 * (int)cc, tot - 4 * (int)cc, q, P.th, hds);
        }
        if (P.dbg & 1u) pend = 0;
        emit_hits<SL, TAP>(ix, out, sw, g.read, g.base0, tg, e_al, cc, pend, hds);
      }
    }
  }
  return (P.dbg & 1u) ? 0ull : bits;
}

// deal the hit chunks of a group out, 64 at a time: re-read header + chunk (L2), apply the bucket bounds, emit
template <int LOG_G, int CPL, bool SL, bool TAP>
__device__ __forceinline__ void pipe_resolve(const DevIndex& ix, const DevParams& P, const BatchOut& out, ScanWave& sw, const SlotList& L,
                                             lds_u32* queue, const GroupDesc& g, uint64_t hitbits)
{
  constexpr uint32_t G = 1u << LOG_G, PPS = 64u >> LOG_G, W = scan_slot_words(LOG_G, CPL), CAP = scan_slot_cap(LOG_G, CPL);
  const uint32_t lane = lane_id(), sub = lane & (G - 1u);
  const uint32_t cnt = (uint32_t)__popcll(hitbits);
  const uint32_t inc = wave_scan_incl(cnt);
  const uint32_t H = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
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
      const uint32_t row = L.row[probe];
      const uint32_t q = L.q[probe];
      tg = L.tag[probe];
      const uint32_t* slot = get_lib<SL>(ix, tag_lib(tg)).slots + (uint64_t)row * W;
      const uint2 hdr = *reinterpret_cast<const uint2*>(slot);
      const uint4 v = *reinterpret_cast<const uint4*>(slot + 4u * c);
      // word 4c+e of the slot is entry 4c+e-2 of the bucket = packed index start + 4c+e-2
      const int nin = (int)min(hdr.x, CAP);
      pend = chunk_hits(v, 2 - 4 * (int)c, nin + 2 - 4 * (int)c, q, P.th, hds);
      e_al = (uint64_t)hdr.y - 2ull;
    }
    WAVE_SYNC();
    emit_hits<SL, TAP>(ix, out, sw, g.read, g.base0, tg, e_al, c, pend, hds);
  }
}

__device__ __forceinline__ void pipe_begin_read(ScanWave& sw)
{
  sw.it_next = min((sw.it_next + 15u) & ~15u, sw.it_end); // the read's items start on a 128-byte line
  sw.rd_start = sw.it_next;
  sw.n_st = 0;
  sw.cur_seg = 0;
  sw.filt0 = 0xFFFFFFFFu, sw.filt1 = 0xFFFFFFFFu;
}
__device__ __forceinline__ void pipe_end_read(const BatchOut& out, ScanWave& sw, lds_u32* meta)
{
  flush_stage(out, sw);
  // per-strand hdist_filt = min hd over kept table entries (src/query.cpp:366-368)
  uint32_t f0 = sw.filt0, f1 = sw.filt1;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    f0 = min(f0, (uint32_t)__shfl_xor(f0, d));
    f1 = min(f1, (uint32_t)__shfl_xor(f1, d));
  }
  if (lane_id() == 0) {
    meta[0 * kReadChunk] = sw.rd_start;
    meta[1 * kReadChunk] = sw.it_next - sw.rd_start;
    meta[3 * kReadChunk] = f0;
    meta[4 * kReadChunk] = f1;
  }
}

template <int LOG_G, int CPL, int DEPTH, int WPE, bool SL, bool TAP>
__global__ __launch_bounds__(kScanWaves* kWave, WPE) void kr_scan_pipe_kernel_t(DevIndex ix, DevParams P, BatchIn in, BatchOut out)
{
  constexpr uint32_t PPS = 64u >> LOG_G;
  static_assert((kListCap / PPS) * CPL <= 64, "one hit bit per (pass, chunk)");
  __shared__ uint32_t s_row[kScanWaves][2][kListCap], s_q[kScanWaves][2][kListCap], s_tag[kScanWaves][2][kListCap], s_queue[kScanWaves][64];
  __shared__ uint32_t s_meta[kScanWaves][5 * kReadChunk];
  __shared__ __attribute__((aligned(16))) uint64_t s_stage[kScanWaves][kItemStage];
  __shared__ __attribute__((aligned(16))) uint4 s_fetab[KR_SCAN_PIPE_FE == 2 ? 1024 : 1];
  static_assert(kReadChunk <= 64, "one lane per read of a visit");
  if (KR_SCAN_PIPE_FE == 2) {
    fe_tab_to_lds(ix, (lds_u32x4*)s_fetab);
    __syncthreads();
  }
  const uint32_t w = threadIdx.x / kWave;
  SlotList LA{(lds_u32*)s_row[w][0], (lds_u32*)s_q[w][0], (lds_u32*)s_tag[w][0]};
  SlotList LB{(lds_u32*)s_row[w][1], (lds_u32*)s_q[w][1], (lds_u32*)s_tag[w][1]};
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
  GroupGen<SL, KR_SCAN_PIPE_FE> gen;
  gen.tab = (const lds_u32x4*)s_fetab;
  uint4 v[DEPTH * CPL];
  while (rc.next(r0v, r1v)) {
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r0v), r1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r1v);
    gen.init(r0, r1);
    GroupDesc ga, gb;
    bool flip = false; // which list holds group A
    bool has_a = gen.next(ix, P, in, LA, meta, ga);
    if (has_a) {
      gen.prefetch(ix, in);
      pipe_begin_read(sw);
      pipe_issue<LOG_G, CPL, DEPTH, SL>(ix, LA, ga.nact, 0, v);
    }
    uint32_t c = 0;
    uint64_t hitbits = 0;
    bool has_b = false;
    while (has_a) {
      const SlotList& A = flip ? LB : LA;
      const SlotList& B = flip ? LA : LB;
      if (c == 0) { // the next group's front end and probe list, while A's loads are in flight
        has_b = gen.next(ix, P, in, B, meta, gb);
        if (has_b) gen.prefetch(ix, in);
      }
      hitbits |= pipe_test<LOG_G, CPL, DEPTH, SL, TAP>(ix, P, out, sw, A, ga, c, v);
      const uint32_t npass = (ga.nact + PPS - 1u) / PPS;
      if ((c + 1u) * (uint32_t)DEPTH < npass) { // more passes of A than the registers hold
        ++c;
        pipe_issue<LOG_G, CPL, DEPTH, SL>(ix, A, ga.nact, c, v);
        continue;
      }
      if (has_b) pipe_issue<LOG_G, CPL, DEPTH, SL>(ix, B, gb.nact, 0, v);
      pipe_resolve<LOG_G, CPL, SL, TAP>(ix, P, out, sw, A, queue, ga, hitbits);
      if (ga.last) {
        pipe_end_read(out, sw, meta + ga.slot);
        pipe_begin_read(sw);
      }
      WAVE_SYNC();
      ga = gb, has_a = has_b, flip = !flip, c = 0, hitbits = 0;
    }
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
