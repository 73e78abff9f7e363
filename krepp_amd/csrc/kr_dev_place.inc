// kr_dev_place.inc -- part of kr_device.hip (included after kr_dev_likelihood.inc): the back end of `krepp place`
// for one batch, on the records the dist kernels left in HBM.
//
// IBatch::report_placement (src/query.cpp:218-333) per read, one wave per read:
//   closest leaf and its tau gate (:220); the chosen record of every leaf mapped onto the placement tree; a single
//   leaf -> one placement (:233-244); otherwise every leaf's histogram is added to each of its ancestors with weight
//   prod 1/eff_nchildren (Minfo::add, src/query.hpp:139-152; :248-265), candidates are the nodes whose children are all
//   covered and that pass the tau gate (:268-272), internal candidates get a Brent minimisation on their fractional
//   histogram (:273-275), every candidate a chi-square against the closest leaf (:276, :420-424).
// The sums are formed in the order the host path (kr_place.cpp) and the oracle use -- leaves in ascending node number,
// each ancestor's accumulator by itself, the weight by successive divisions from the leaf upwards -- with the same
// fp64 operations (-ffp-contract=off), so the two paths give identical bits.  What stays on the host: the chi-square
// filter, exp / LWR, the Jukes-Cantor distance and the text (glibc's exp and log, as the reference calls them).
//
// Two launches: kr_place_kernel (a wave per read) lists the candidates and, for the internal ones, their accumulated
// problem; kr_place_llh_kernel (a lane per candidate, every lane busy) runs the Brent minimisations and the chi-squares.
// With the minimisations inside the per-read kernel two or three lanes of a wave worked while the rest waited:
// 5.7 ms per 400,000 reads against 0.6 ms for the same minimisations run densely.
//
// Parallel form of the first kernel: a lane per ancestor.  Node numbers are post-order, so the leaves below a node are a contiguous run of
// the read's leaves sorted by node number, and an ancestor is "new" at a leaf iff the previous leaf is not below it:
// every distinct ancestor is listed exactly once without a hash set, and the walk up from a leaf stops at the first
// ancestor it shares with its predecessor.
constexpr uint32_t kPlLeaves = 256;  // leaves of one read the LDS arrays hold (more: the read goes to the second launch, arrays in global scratch)
constexpr uint32_t kPlNodes = 1024;  // distinct ancestors of one read
#ifndef KR_PLACE_PROF
#define KR_PLACE_PROF 0 // 1: cycles / 256 per phase of place_read into kPlProf0 .. + 5 (experiments)
#endif
constexpr uint32_t kPlBlock = 8;     // leaves of its run an ancestor's lane handles at a time
constexpr uint32_t kPlCnt = 32;      // words between two of PlaceOut::cnt's counters: a 128-byte line each (atomics on words of ONE line serialise
                                     // in its L2 channel at ~90 M/s, and the first launch makes ~200,000 of them per 400,000 reads)
enum PlaceCnt : uint32_t { // the counters of PlaceOut::cnt (pl_cnt below), cleared per range and copied to the host behind its kernels
  kPlCandSlots = 0,    // candidate slots handed out (beyond cap: what the reads asked for)
  kPlFlags = 1,        // PlaceFlag bits
  kPlHeavySlots = 2,   // slots of the heavy list handed out, in chunks of 8
  kPlKept = 3,         // kept candidates' slots handed out by the compaction (beyond kcap likewise)
  kPlProf0 = 4,        // .. 9: KR_PLACE_PROF cycles / 256 of place_read's six phases (KR_PL_MARK)
  kPlReadsOut = 10,    // reads handed out to the waves of the first launch
  kPlBigListed = 11,   // reads with many records, listed by kr_place_big_first_kernel
  kPlListSlots = 12,   // entries of the internal candidates' list handed out (k_se until the compaction)
  kPlBigOut = 13,      // ... of the listed big reads handed out
  kPlInlineReads = 14, // reads beyond the LDS arrays done at once in global scratch by the first launch
  // 15 .. 26: path witnesses of place_read, counted by lane 0 in the WIT instantiations only (launched under KR_DEBUG_PLACE_PATHS=1;
  // kr_debug_place_paths, names: PLACE_WITNESSES in krepp_amd/capi.py).  A read is counted where it is FINISHED -- a read that exceeds the arrays of one home
  // counts in the home that does it -- and only if it has two leaves or more and got its candidate slots, but for the two early exits.
  kPlWitChained = 15,       // reads whose (leaf, ancestor) weights went through the wave's global scratch
  kPlWitWalkedShallow = 16, // reads whose weights were walked: tot_chain <= kPlChainFactor * nl
  kPlWitWalkedDeep = 17,    // ... tot_chain beyond the chain scratch of the read's home
  kPlWitWide = 18,          // reads whose histograms were re-read from the records (a count above 255, or th >= 8)
  kPlWitRunsOff = 19,       // reads whose ancestor lanes walked the whole leaf list (more than kPlRunsLeaves leaves)
  kPlWitDup = 20,           // reads with a record dropped for a later one on the same node
  kPlWitSingle = 21,        // single placements (one leaf)
  kPlWitTau = 22,           // reads stopped by the tau gate of their closest leaf
  kPlWitLds = 23,           // reads finished with their arrays in the first launch's LDS
  kPlWitInline = 24,        // ... in global scratch by a wave of the first launch
  kPlWitSecond = 25,        // ... by the second launch (dynamic LDS or global scratch)
  kPlWitMultiBlock = 26,    // ancestor lanes whose walk took more than one block of kPlBlock leaves
  kPlWitEnd = 27,
  kPlCntCount = 32     // lines allocated
};
constexpr uint32_t kPlChainFactor = 12;  // the weights go through global scratch only where tot_chain > kPlChainFactor * leaves (place_read: chained)
constexpr uint32_t kPlRunsLeaves = 4096; // most leaves of a read whose ancestor words still carry their first leaf (place_read: runs)
enum PlaceFlag : uint32_t {
  kPlFlagLimits = 1u,  // a read exceeded even the global arrays (cannot happen: they hold the whole tree)
  kPlFlagCandCap = 2u, // out of candidate slots
  kPlFlagKeepCap = 4u, // out of slots for the kept candidates
  kPlFlagListCut = 8u  // the internal candidates' list is incomplete: kr_place_llh_kernel minimises them itself (no error)
};
__host__ __device__ __forceinline__ uint32_t& pl_cnt(uint32_t* cnt, uint32_t slot) { return cnt[kPlCnt * slot]; }
#ifndef KR_PL_READ_CHUNK
#define KR_PL_READ_CHUNK 4
#endif
constexpr uint32_t kPlReadChunk = KR_PL_READ_CHUNK; // reads a wave of the first launch takes at a time (kPlReadsOut)
constexpr uint32_t kPlChain = 8192; // (leaf, ancestor) weights of one read held in the wave's global scratch (more: they are recomputed by walking up)
constexpr uint32_t kPlInlineChain = 4; // a wave of the first launch that does an over-limit read in global scratch has kPlInlineChain * kPlChain weights for it
constexpr uint32_t kPlChunk = 128;   // candidate slots a wave takes at a time (every wave leaves part of one unused: the host copies slots)

struct PlaceTree {
  const uint32_t* parent;
  const uint32_t* eff;
  const uint8_t* elig;
  const uint32_t* lo;
  const uint32_t* idx_to_pt;
  const uint32_t* depth; // number of ancestors
  const uint4* node;     // {parent, lo, eff, depth}: a walk up the tree is ONE dependent load per level
  uint32_t pn, nidx;
};
struct PlaceOut {
  uint32_t* rd_c0;
  uint32_t* rd_info;
  uint32_t* c_se;   // 0 = unused slot (cleared before the launch)
  uint32_t* c_read; // the candidate's read | kind << 30 (0 leaf: d, v known; 1 internal: to be minimised; 2 single: no chi-square)
  double* c_d;
  double* c_v;
  double* c_chisq;
  double* c_prob;   // [cap][np + 2] internal candidates: fractional histogram, mismatch count, rho
  double* r_prob;   // [nreads][np + 3] the read's closest leaf: histogram, mismatch count, rho, v_llh
  uint32_t* cnt;    // [kPlCntCount lines of kPlCnt words] indexed by PlaceCnt through pl_cnt
  uint32_t cap;
  // reads with more leaves / ancestors than the LDS arrays hold: listed by the first launch, done by the second one with its
  // arrays in global scratch (per wave: 4 * heavy_leaves + heavy_nodes words, 2 * heavy_leaves doubles)
  uint32_t* heavy;    // [nreads + 8 * waves of the first launch]
  uint32_t* heavy_u32;
  double* heavy_f64;
  uint32_t heavy_leaves, heavy_nodes;
  uint32_t lds_leaves, lds_nodes; // what the first launch accepts (<= kPlLeaves / kPlNodes; smaller in tests: KR_DEBUG_PLACE_LDS)
  // kr_place_compact_kernel: the candidates that pass the chi-square test (src/query.cpp:276-277), read after read, without gaps;
  // kPlKept = slots handed out.  These are what the host copies back.
  uint32_t* k_se;
  double* k_d;
  double* k_v;
  double* k_chisq;
  uint32_t kcap;
  double* chain;      // [waves][chain_cap]
  uint32_t chain_cap;
  uint32_t chain_cap_heavy; // the second launch has fewer waves: each takes a larger piece of the same buffer
  uint32_t heavy_in_lds;    // the second launch's arrays are its dynamic LDS (32 * heavy_leaves + 4 * heavy_nodes bytes), not global scratch
  // reads with many records FIRST (kr_place_big_first_kernel lists them: heavy[big_off ..], kPlBigListed entries; kPlBigOut: handed out): the
  // waves of the first launch that own a piece of the global scratch (blockIdx.x < inline_waves) start with them and, where a read
  // exceeds the LDS arrays, do it at once in that scratch -- the reads that used to make up the second launch (2.5 ms with a
  // handful of waves busy) run beside everybody else's ordinary reads.  kPlInlineReads: reads done that way.
  uint32_t big_off, big_min_records, inline_waves;
  double* chain_inline;      // [inline_waves][chain_inline_cap]: the weights of a read such a wave does in global scratch
  uint32_t chain_inline_cap;
  uint32_t lcap;             // entries of k_se the internal candidates' list may take: kcap (less in tests: KR_DEBUG_PLACE_CAPS)
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_prefix_excl(bool flag, uint32_t& total)
{
  const uint64_t m = __ballot(flag);
  total = (uint32_t)__popcll(m);
  return (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
}

// Per-wave arrays of the read in hand: LDS for ordinary reads, the wave's global scratch for the heavy ones (same code,
// memory operations by pointer type: workgroup-scope fences order a wave's own stores and loads there).
struct PlaceLdsMem {
  typedef lds_u32* u32p;
  typedef lds_f64* f64p;
  static __device__ __forceinline__ void sync() { WAVE_SYNC(); }
};
struct PlaceGlobalMem {
  typedef uint32_t* u32p;
  typedef double* f64p;
  static __device__ __forceinline__ void sync()
  {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    WAVE_SYNC();
  }
};
template <typename M>
struct PlaceArrays {
  typename M::u32p lq0, lq1, li0, li1; // the read's leaves: placement node, record; 1 = sorted
  typename M::f64p lmatch, lrho;
  typename M::u32p nodes;              // distinct ancestors
  uint32_t max_leaves, max_nodes;
};

// One read (the whole wave).  Returns false if the read exceeds the arrays (ordinary launch: the read is left to the heavy
// launch); `over_cap` reports candidate slots running out.
// NPT = th + 1 where the launch knows it (5 by default): the histograms' loops unroll and the two LlhProblem of a lane stay in
// registers -- with a run-time bound they are indexed dynamically and live in scratch MEMORY, which made every `mc[x] += ...`
// of the ancestors' loop a round trip (80 % of the kernel on the 1000-genome tree).  NPT = 0: any th.
// WIT: the path witnesses are counted.  A template parameter and not a flag in PlaceOut: every form of run-time flag tried -- even one
// that guarded two atomics in the early exits -- moved the register allocation of some instantiation (docs/design/06_place.md), so the
// kernels that are launched without KR_DEBUG_PLACE_PATHS are compiled from the text they had before, and the switch is the host's.
template <typename M, int NPT, bool WIT>
__device__ __forceinline__ bool place_read(const LlhConst& C, const DevIndex& ix, const BatchOut& o, uint32_t r, const uint32_t* read_len,
                                           const PlaceTree& T, const PlaceOut& po, uint32_t tau, uint32_t no_filter, const PlaceArrays<M>& A,
                                           lds_u32* s_n, uint32_t& c_pos, uint32_t& c_end, uint32_t& i_pos, uint32_t& i_end, double* chain, uint32_t chain_cap,
                                           uint32_t home)
{ // home: the witness slot of the arrays' home (kPlWitLds, kPlWitInline, kPlWitSecond)
  const uint32_t lane = lane_id(), np = NPT ? (uint32_t)NPT : C.th + 1;
  const double kMax = 1.7976931348623157e308;
  const uint32_t ro = o.rd_off[r], n = o.rd_cnt[r];
  uint32_t info = 0, c0 = 0;
#if KR_PLACE_PROF
  uint64_t tp = __builtin_readcyclecounter();
#define KR_PL_MARK(k) do { const uint64_t t_ = __builtin_readcyclecounter(); if (lane == 0) atomicAdd(&pl_cnt(po.cnt, kPlProf0 + (k)), (uint32_t)((t_ - tp) >> 8)); tp = t_; } while (0)
#else
#define KR_PL_MARK(k) do {} while (0)
#endif
  // ---- closest: the smallest d, among equal d the largest (strand, index) (summarize_matches' `<=`)
  double bd = kMax;
  uint32_t bo = 0;
  bool any = false;
  for (uint32_t i = lane; i < n; i += kWave) {
    const uint32_t key = o.rec_key[ro + i];
    const double d = o.rec_d[ro + i];
    const uint32_t ord = ((key & 1u) << 31) | i;
    if (key && d <= kMax && (!any || d < bd || (d == bd && ord > bo))) bd = d, bo = ord, any = true;
  }
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) {
    const double od = __shfl_xor(bd, sft, 64);
    const uint32_t oo = __shfl_xor(bo, sft, 64);
    const bool oa = __shfl_xor(any ? 1 : 0, sft, 64) != 0;
    if (oa && (!any || od < bd || (od == bd && oo > bo))) bd = od, bo = oo, any = true;
  }
  bool go = any; // (wave-uniform from here on)
  LlhProblem pc; // the closest leaf's problem: the chi-square reference
  double v_c = 0, d_c = 0;
  uint32_t closest_pt = 0;
  const double enmers = (double)(read_len[r] >= C.k ? read_len[r] - C.k + 1 : 0u);
  if (go) {
    const uint32_t cl = ro + (bo & 0x7FFFFFFFu), kcl = o.rec_key[cl];
    double mc = 0, leq = 0;
#pragma unroll
    for (uint32_t x = 0; x < np; ++x) {
      pc.mc[x] = (double)o.rec_hist[(uint64_t)x * o.rec_stride + cl];
      mc += pc.mc[x];
      if (x <= tau) leq += pc.mc[x];
    }
    pc.uc = (double)o.rd_onmers[r] - mc; // src/query.cpp:104
    pc.rho = ix.libs[0].rho[kcl >> 1];
    d_c = o.rec_d[cl], v_c = o.rec_v[cl];
    closest_pt = (kcl >> 1) <= T.nidx ? T.idx_to_pt[kcl >> 1] : 0u;
    go = no_filter || leq > 1.0; // src/query.cpp:220
    if (WIT && !go && lane == 0) atomicAdd(&pl_cnt(po.cnt, kPlWitTau), 1u);
  }
  // ---- the read's leaves on the placement tree: the chosen record of every leaf (rec_sel)
  uint32_t nl = 0;
  bool over = false;
  if (go) {
    for (uint32_t t0 = 0; t0 < n; t0 += kWave) {
      const uint32_t t = t0 + lane;
      uint32_t q = 0;
      if (t < n && o.rec_sel[ro + t]) {
        const uint32_t se = o.rec_key[ro + t] >> 1;
        q = se <= T.nidx ? T.idx_to_pt[se] : 0u;
      }
      uint32_t tot;
      const uint32_t pre = wave_prefix_excl(q != 0, tot);
      if (q && nl + pre < A.max_leaves) A.lq0[nl + pre] = q, A.li0[nl + pre] = ro + t;
      nl += tot;
    }
    if (nl > A.max_leaves) over = true, go = false;
    if (nl == 0) go = false;
  }
  M::sync();
  if (go && nl == 1) { // src/query.cpp:233-244: the placement is the closest leaf
    if (c_pos + 1 > c_end) {
      uint32_t b = 0;
      if (lane == 0) b = atomicAdd(&pl_cnt(po.cnt, kPlCandSlots), kPlChunk);
      c_pos = __shfl(b, 0, 64), c_end = c_pos + kPlChunk;
    }
    if (c_end > po.cap) {
      if (lane == 0) atomicOr(&pl_cnt(po.cnt, kPlFlags), kPlFlagCandCap);
    } else {
      c0 = c_pos;
      if (lane == 0)
        po.c_se[c0] = closest_pt ? closest_pt : 0x7FFFFFFFu, po.c_read[c0] = r | (2u << 30), po.c_d[c0] = d_c, po.c_v[c0] = v_c, po.c_chisq[c0] = 0.0;
      c_pos += 1;
      info = (1u << 31) | (1u << 30) | 1u;
      if (WIT && lane == 0) atomicAdd(&pl_cnt(po.cnt, kPlWitSingle), 1u);
    }
    go = false;
  }
  if (go && lane == 0) { // the chi-square reference of the read's candidates, for the second kernel
    double* rp = po.r_prob + (uint64_t)r * (np + 3u);
#pragma unroll
    for (uint32_t x = 0; x < np; ++x) rp[x] = pc.mc[x];
    rp[np] = pc.uc, rp[np + 1] = pc.rho, rp[np + 2] = v_c;
  }
  KR_PL_MARK(0); // closest, leaves gathered, single placement
  uint32_t na = 0;
  uint32_t wit_dup = 0, wit_multi = 0; // (WIT only, per lane: records dropped for a later one on their node; ancestors whose walk took more than one block)
  bool wide = false; // wave-uniform: some count of some leaf does not fit the packed histogram
  bool runs = false; // wave-uniform: the ancestors' words carry their first leaf
  typename M::u32p hpk = (typename M::u32p)A.lmatch; // [2 * leaves]
  if (go) {
    // ---- sort the leaves by (node, record): rank by counting (a few dozen leaves)
    for (uint32_t e = lane; e < nl; e += kWave) {
      const uint32_t q = A.lq0[e], i = A.li0[e];
      uint32_t rank = 0;
      for (uint32_t f = 0; f < nl; ++f) {
        const uint32_t q2 = A.lq0[f], i2 = A.li0[f];
        rank += (q2 < q || (q2 == q && i2 < i)) ? 1u : 0u;
      }
      A.lq1[rank] = q, A.li1[rank] = i;
    }
    if (lane == 0) *s_n = 0;
    M::sync();
    // per leaf: match count and rho (Minfo fields the sums need); two records on one node: the later one stands
    // (the host's `leaf_acc(i, pool[slot])` overwrites), the earlier is skipped by giving it node 0
    // (the histogram itself is parked beside them, 8 bits a count in the two words of the leaf's lmatch slot: the ancestors' lanes
    //  below read every leaf's histogram once per ancestor above it -- from global memory that was 5 scattered loads per pair,
    //  most of the kernel's 680 vector loads per read.  A count above 255 (long reads) keeps the read on the loads.)
    bool wide_l = false;
    for (uint32_t e = lane; e < nl; e += kWave) {
      const uint32_t i = A.li1[e];
      uint32_t w0 = 0, w1 = 0;
#pragma unroll
      for (uint32_t x = 0; x < np; ++x) {
        const uint32_t hv = o.rec_hist[(uint64_t)x * o.rec_stride + i];
        wide_l = wide_l || hv > 255u || x >= 8u;
        if (x < 4u) w0 |= (hv & 255u) << (8u * x);
        else if (x < 8u) w1 |= (hv & 255u) << (8u * (x - 4u));
      }
      hpk[2u * e] = w0, hpk[2u * e + 1u] = w1;
      A.lrho[e] = ix.libs[0].rho[o.rec_key[i] >> 1];
    }
    wide = __ballot(wide_l) != 0;
    M::sync();
    for (uint32_t e = lane; e < nl; e += kWave) A.li0[e] = (e + 1 < nl && A.lq1[e + 1] == A.lq1[e]) ? 1u : 0u;
    M::sync();
    for (uint32_t e = lane; e < nl; e += kWave)
      if (A.li0[e]) {
        A.lq1[e] = 0;
        if (WIT) ++wit_dup;
      }
    M::sync();
    KR_PL_MARK(1); // sort, per-leaf fields
    // (node numbers fit 20 bits -- trees of up to 65,536 leaves; with at most 4,096 leaves in the read the ancestor's word also
    //  says where its leaves start in the sorted list: they are a contiguous run, which its lane then walks instead of the list)
    runs = nl <= kPlRunsLeaves && T.pn < (1u << 20);
    // ---- distinct ancestors: leaf e lists the ancestors its predecessor is not below
    for (uint32_t e0 = 0; e0 < nl; e0 += kWave) {
      const uint32_t e = e0 + lane;
      if (e < nl && A.lq1[e]) {
        uint32_t prev = 0; // the nearest earlier leaf that stands
        for (uint32_t f = e; f-- > 0;)
          if (A.lq1[f]) {
            prev = A.lq1[f];
            break;
          }
        uint32_t a;
        uint4 nd = T.node[A.lq1[e]];
        while ((a = nd.x) != 0) {
          nd = T.node[a];
          if (prev && prev >= nd.y) break; // the predecessor is below a (and below everything above a)
          const uint32_t slot = __hip_atomic_fetch_add(s_n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (slot < A.max_nodes) A.nodes[slot] = a | (runs ? e << 20 : 0u); // e: the FIRST of the read's leaves below a
        }
      }
    }
    M::sync();
    na = *s_n;
    if (na > A.max_nodes) over = true, go = false;
  }
  // ---- the weight of every (leaf, ancestor) pair, once: walking up from a leaf, the weight at an ancestor is the weight
  //      at the node below divided by eff_nchildren -- the very divisions Minfo::add's caller makes (src/query.cpp:248-265),
  //      in the same order, so every ancestor's lane below finds its weights ready instead of walking up from each of its
  //      leaves again (on a 1000-leaf tree: 33 leaves x 25 levels of fp64 divisions per ancestor lane, 34 ms per 400,000 reads)
  KR_PL_MARK(2); // ancestors listed
  bool chained = false;
  bool chain_over = false; // (witnesses: the weights are walked because they exceed the scratch, not because the tree is shallow)
  if (go) {
    uint32_t tot_chain = 0;
    for (uint32_t e0 = 0; e0 < nl; e0 += kWave) {
      const uint32_t e = e0 + lane;
      const uint32_t q = e < nl ? A.lq1[e] : 0u;
      const uint32_t dq = q ? T.depth[q] : 0u;
      const uint32_t inc = wave_scan_incl(dq);
      if (e < nl) A.li0[e] = tot_chain + inc - dq, A.lq0[e] = dq; // (li0 is free again: the duplicate flags are folded into lq1; lq0 since the sort)
      tot_chain += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    // (on a shallow tree the walk is a handful of divisions: cheaper than a round trip through the wave's global scratch --
    //  the 25-leaf toy tree lost a factor of two to it)
    chained = tot_chain <= chain_cap && tot_chain > kPlChainFactor * nl;
    chain_over = tot_chain > chain_cap;
    M::sync();
    if (chained) {
      for (uint32_t e = lane; e < nl; e += kWave) {
        const uint32_t q = A.lq1[e];
        if (q == 0) continue;
        double denom = 1.0;
        uint32_t par, j = A.li0[e];
        uint4 nd = T.node[q];
        while ((par = nd.x) != 0) {
          nd = T.node[par];
          denom /= (double)nd.z;
          chain[j++] = denom;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // the wave's own global stores, read back by its other lanes below
      WAVE_SYNC();
    }
  }
  KR_PL_MARK(3); // weights
  if (go) {
    // ---- reserve slots for every possible candidate of the read (leaves + ancestors), contiguous
    const uint32_t need = nl + na;
    if (c_pos + need > c_end) {
      const uint32_t take = 4u * need > kPlChunk ? 4u * need : kPlChunk; // (a read keeps only what it emits: the rest serves the wave's next reads)
      uint32_t b = 0;
      if (lane == 0) b = atomicAdd(&pl_cnt(po.cnt, kPlCandSlots), take);
      c_pos = __shfl(b, 0, 64), c_end = c_pos + take;
    }
    if (c_end > po.cap) {
      if (lane == 0) atomicOr(&pl_cnt(po.cnt, kPlFlags), kPlFlagCandCap);
      go = false;
    }
  }
  if (go) {
    c0 = c_pos;
    uint32_t emitted = 0;
    // ---- leaf candidates
    for (uint32_t e0 = 0; e0 < nl; e0 += kWave) {
      const uint32_t e = e0 + lane;
      bool cand = false;
      uint32_t q = 0;
      double d = 0, v = 0;
      if (e < nl && (q = A.lq1[e]) != 0 && T.elig[q]) {
        const uint32_t i = A.li1[e];
        double leq = 0;
#pragma unroll
        for (uint32_t x = 0; x < np && x <= tau; ++x) leq += (double)o.rec_hist[(uint64_t)x * o.rec_stride + i];
        if (no_filter || leq > 1.0) {
          cand = true;
          d = o.rec_d[i], v = o.rec_v[i];
        }
      }
      uint32_t tot;
      const uint32_t pre = wave_prefix_excl(cand, tot);
      if (cand) {
        const uint32_t slot = c0 + emitted + pre;
        po.c_se[slot] = q, po.c_read[slot] = r, po.c_d[slot] = d, po.c_v[slot] = v;
      }
      emitted += tot;
    }
    KR_PL_MARK(4); // slots, leaf candidates
    // ---- ancestors: accumulate (Minfo::add in leaf order), gate, Brent, chi-square
    for (uint32_t a0 = 0; a0 < na; a0 += kWave) {
      const uint32_t ai = a0 + lane;
      bool cand = false;
      uint32_t a = 0;
      LlhProblem pa;
      if (ai < na) {
        const uint32_t aw = A.nodes[ai];
        a = runs ? aw & 0xFFFFFu : aw;
        for (uint32_t x = 0; x < np; ++x) pa.mc[x] = 0.0;
        double a_nmers = 0, a_mis = 0, a_match = 0, a_rho = 0;
        const uint4 nda = T.node[a];
        const uint32_t lo = nda.y, da = nda.w;
        // The leaves below a are a contiguous run of the sorted list (post-order numbers): the lane walks ITS run, in leaf order
        // -- walking the whole list, as every lane did, kept one lane in eight busy (825 (leaf, ancestor) pairs in 6,600 steps on the
        // 1000-genome tree) --
        // ... in blocks of kPlBlock leaves: the weights of a block's members -- one load each from the wave's global scratch, half a
        // microsecond away -- are requested together and then used in leaf order (a lane near the root has hundreds of leaves)
        bool past = false; // a leaf beyond the run has been seen
        uint32_t wit_blocks = 0;
        for (uint32_t e0 = runs ? aw >> 20 : 0u; e0 < nl && !past; e0 += kPlBlock) {
          if (WIT) ++wit_blocks;
          double dn[kPlBlock];
          uint32_t w0[kPlBlock], w1[kPlBlock];
          bool mem[kPlBlock];
#pragma unroll
          for (uint32_t u = 0; u < kPlBlock; ++u) {
            const uint32_t e = e0 + u;
            const uint32_t q = e < nl ? A.lq1[e] : 0u;
            past = past || q > a;
            mem[u] = !past && q != 0 && q >= lo;
            dn[u] = 1.0, w0[u] = w1[u] = 0;
            if (mem[u]) {
              if (chained) dn[u] = chain[A.li0[e] + (A.lq0[e] - da - 1u)];
              if (!wide) w0[u] = hpk[2u * e], w1[u] = hpk[2u * e + 1u];
            }
          }
#pragma unroll
          for (uint32_t u = 0; u < kPlBlock; ++u) {
            if (!mem[u]) continue;
            const uint32_t e = e0 + u;
            double denom = dn[u];
            if (!chained) {
              uint32_t par = A.lq1[e];
              do {
                par = T.parent[par];
                denom /= (double)T.eff[par];
              } while (par != a);
            }
            const uint32_t i = A.li1[e];
            double m_match = 0; // (integers: their sum is exact in any order)
            if (!wide) {
#pragma unroll
              for (uint32_t x = 0; x < 8u; ++x)
                if (x < np) m_match += (double)(((x < 4u ? w0[u] : w1[u]) >> (8u * (x & 3u))) & 255u);
            } else {
              for (uint32_t x = 0; x < np; ++x) m_match += (double)o.rec_hist[(uint64_t)x * o.rec_stride + i];
            }
            a_mis = a_nmers != 0.0 ? a_mis : enmers; // Minfo::add (src/query.hpp:139-152)
            a_match += m_match * denom;
            a_mis -= m_match * denom;
            if (!wide) {
#pragma unroll
              for (uint32_t x = 0; x < 8u; ++x)
                if (x < np) pa.mc[x] = pa.mc[x] + (double)(((x < 4u ? w0[u] : w1[u]) >> (8u * (x & 3u))) & 255u) * denom;
            } else {
              for (uint32_t x = 0; x < np; ++x) pa.mc[x] = pa.mc[x] + (double)o.rec_hist[(uint64_t)x * o.rec_stride + i] * denom;
            }
            a_nmers = a_nmers > enmers ? a_nmers : enmers;
            a_rho = a_rho > A.lrho[e] ? a_rho : A.lrho[e];
          }
        }
        if (WIT && wit_blocks > 1u) ++wit_multi;
        if (T.elig[a]) {
          double leq = 0;
#pragma unroll
          for (uint32_t x = 0; x < np && x <= tau; ++x) leq += pa.mc[x];
          if (no_filter || leq > 1.0) {
            cand = true;
            pa.uc = a_mis, pa.rho = a_rho;
          }
        }
      }
      uint32_t tot;
      const uint32_t pre = wave_prefix_excl(cand, tot);
      if (tot) { // the slots of the internal candidates, listed for kr_place_brent_kernel (wave-private chunks of the list, like the slots)
        if (i_pos + tot > i_end) {
          for (uint32_t q = i_pos + lane; q < i_end; q += kWave) po.k_se[q] = 0xFFFFFFFFu; // the rest of the old chunk: unused
          const uint32_t take = tot > kPlChunk ? tot : kPlChunk;
          uint32_t b = 0;
          if (lane == 0) b = atomicAdd(&pl_cnt(po.cnt, kPlListSlots), take);
          i_pos = __shfl(b, 0, 64), i_end = i_pos + take;
          if (i_end > po.lcap) { // (cannot happen with the sizes kr_host_place.inc gives the list: then the likelihood kernel minimises by itself)
            if (lane == 0) atomicOr(&pl_cnt(po.cnt, kPlFlags), kPlFlagListCut);
            i_pos = i_end = 0;
          }
        }
        if (cand && i_end) po.k_se[i_pos + pre] = c0 + emitted + pre;
        if (i_end) i_pos += tot;
      }
      if (cand) { // the minimisation of the fractional histogram is kr_place_brent_kernel's
        const uint32_t slot = c0 + emitted + pre;
        po.c_se[slot] = a, po.c_read[slot] = r | (1u << 30);
        double* cp = po.c_prob + (uint64_t)slot * (np + 2u);
#pragma unroll
        for (uint32_t x = 0; x < np; ++x) cp[x] = pa.mc[x];
        cp[np] = pa.uc, cp[np + 1] = pa.rho;
      }
      emitted += tot;
    }
    KR_PL_MARK(5); // ancestors accumulated and emitted
    c_pos += emitted; // (room for nl + na was made sure of; what was not used serves the wave's next read)
    info = (1u << 31) | emitted;
    if (WIT) { // path witnesses: the read is finished here, in this home; the two per-lane counts were made where the loops ran
      const uint32_t ndup = wave_sum_u32(wit_dup), nmulti = wave_sum_u32(wit_multi);
      if (lane == 0) {
        atomicAdd(&pl_cnt(po.cnt, home), 1u);
        atomicAdd(&pl_cnt(po.cnt, chained ? kPlWitChained : (chain_over ? kPlWitWalkedDeep : kPlWitWalkedShallow)), 1u);
        if (wide) atomicAdd(&pl_cnt(po.cnt, kPlWitWide), 1u);
        if (!runs) atomicAdd(&pl_cnt(po.cnt, kPlWitRunsOff), 1u);
        if (ndup) atomicAdd(&pl_cnt(po.cnt, kPlWitDup), 1u);
        if (nmulti) atomicAdd(&pl_cnt(po.cnt, kPlWitMultiBlock), nmulti);
      }
    }
  }
  if (!over && lane == 0) po.rd_c0[r] = c0, po.rd_info[r] = info;
  M::sync();
  return !over;
}

// the reads with more records than the LDS arrays have leaves, listed for the first launch to start with
__global__ __launch_bounds__(256) void kr_place_big_first_kernel(BatchOut o, uint32_t nreads, PlaceOut po)
{
  for (uint32_t r0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63u; r0 < nreads; r0 += gridDim.x * blockDim.x) { // wave-uniform
    const uint32_t r = r0 + lane_id();
    const bool big = r < nreads && o.rd_cnt[r] > po.big_min_records;
    uint32_t tot;
    const uint32_t pre = wave_prefix_excl(big, tot);
    if (tot == 0) continue;
    uint32_t b = 0;
    if (lane_id() == 0) b = atomicAdd(&pl_cnt(po.cnt, kPlBigListed), tot);
    b = __shfl(b, 0, 64);
    if (big) po.heavy[po.big_off + b + pre] = r;
  }
}

// HEAVY = false: every read of the batch, arrays in LDS; a read with more leaves or ancestors than they hold is put on the
// heavy list (po.heavy, counted in pl_cnt(po.cnt, kPlHeavySlots)).  HEAVY = true (second launch): the listed reads, arrays in the wave's
// global scratch, sized for the whole tree.
template <bool HEAVY, int NPT, bool WIT>
__global__ __launch_bounds__(kWave) void kr_place_kernel(LlhConst C, DevIndex ix, BatchOut o, uint32_t nreads, const uint32_t* read_len,
                                                         PlaceTree T, PlaceOut po, uint32_t tau, uint32_t no_filter)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  __shared__ uint32_t s_lq[HEAVY ? 1 : 2][HEAVY ? 1 : kPlLeaves], s_li[HEAVY ? 1 : 2][HEAVY ? 1 : kPlLeaves];
  __shared__ double s_lmatch[HEAVY ? 1 : kPlLeaves], s_lrho[HEAVY ? 1 : kPlLeaves];
  __shared__ uint32_t s_nodes[HEAVY ? 1 : kPlNodes];
  __shared__ uint32_t s_n; // ancestors listed so far
  LlhTables LT{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, LT.bk, LT.hnk);
  uint32_t c_pos = 0, c_end = 0; // the wave's chunk of candidate slots
  uint32_t i_pos = 0, i_end = 0; // ... of the list of internal candidates (po.k_se until the compaction takes it over)
  if (!HEAVY) {
    PlaceArrays<PlaceLdsMem> A{(lds_u32*)s_lq[0], (lds_u32*)s_lq[HEAVY ? 0 : 1], (lds_u32*)s_li[0], (lds_u32*)s_li[HEAVY ? 0 : 1],
                               (lds_f64*)s_lmatch, (lds_f64*)s_lrho, (lds_u32*)s_nodes, min(po.lds_leaves, kPlLeaves), min(po.lds_nodes, kPlNodes)};
    uint32_t h_pos = 0, h_end = 0; // the wave's chunk of the heavy list
    // a wave that owns a piece of the global scratch does a read that exceeds the LDS arrays there and then; the others list it
    const bool has_scratch = blockIdx.x < po.inline_waves;
    const uint64_t w = blockIdx.x;
    uint32_t* su = po.heavy_u32 + (has_scratch ? w : 0ull) * (4ull * po.heavy_leaves + po.heavy_nodes);
    double* sd = po.heavy_f64 + (has_scratch ? w : 0ull) * (2ull * po.heavy_leaves);
    PlaceArrays<PlaceGlobalMem> AG{su, su + po.heavy_leaves, su + 2ull * po.heavy_leaves, su + 3ull * po.heavy_leaves,
                                   sd, sd + po.heavy_leaves, su + 4ull * po.heavy_leaves, po.heavy_leaves, po.heavy_nodes};
    uint32_t n_inline = 0;
    auto one_read = [&](uint32_t r) {
      if (place_read<PlaceLdsMem, NPT, WIT>(C, ix, o, r, read_len, T, po, tau, no_filter, A, (lds_u32*)&s_n, c_pos, c_end, i_pos, i_end, po.chain + (uint64_t)blockIdx.x * po.chain_cap, po.chain_cap, kPlWitLds))
        return;
      if (has_scratch) {
        ++n_inline;
        if (!place_read<PlaceGlobalMem, NPT, WIT>(C, ix, o, r, read_len, T, po, tau, no_filter, AG, (lds_u32*)&s_n, c_pos, c_end, i_pos, i_end, po.chain_inline + (uint64_t)blockIdx.x * po.chain_inline_cap, po.chain_inline_cap, kPlWitInline))
          if (lane_id() == 0) atomicOr(&pl_cnt(po.cnt, kPlFlags), kPlFlagLimits); // (cannot happen: the arrays hold the whole tree)
        return;
      }
      if (h_pos == h_end) {
        uint32_t b = 0;
        if (lane_id() == 0) b = atomicAdd(&pl_cnt(po.cnt, kPlHeavySlots), 8u);
        h_pos = __shfl(b, 0, 64), h_end = h_pos + 8u;
      }
      if (lane_id() == 0) po.heavy[h_pos] = r;
      ++h_pos;
    };
    // ---- the reads with many records first (their number is final: kr_place_big_first_kernel ran before this launch)
    if (has_scratch) {
      const uint32_t nbig = pl_cnt(po.cnt, kPlBigListed);
      for (;;) {
        uint32_t j = 0;
        if (lane_id() == 0) j = atomicAdd(&pl_cnt(po.cnt, kPlBigOut), 1u);
        j = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(j, 0, 64));
        if (j >= nbig) break;
        one_read((uint32_t)__builtin_amdgcn_readfirstlane((int)po.heavy[po.big_off + j]));
      }
    }
    // ---- everybody: reads in chunks from one counter: their cost varies by orders of magnitude, and the grid is larger than what
    // is resident (LDS): dealt out by stride, the last waves to start each had a full share left when the first were done
    uint32_t r_pos = 0, r_end = 0;
    for (;;) {
      if (r_pos == r_end) {
        uint32_t b = 0;
        if (lane_id() == 0) b = atomicAdd(&pl_cnt(po.cnt, kPlReadsOut), kPlReadChunk);
        r_pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(b, 0, 64)), r_end = min(r_pos + kPlReadChunk, nreads);
        if (r_pos >= nreads) break;
      }
      const uint32_t r = r_pos++;
      if (po.inline_waves && o.rd_cnt[r] > po.big_min_records) continue; // done above
      one_read(r);
    }
    for (uint32_t q = h_pos + lane_id(); q < h_end; q += 64) po.heavy[q] = 0xFFFFFFFFu; // unused list slots
    if (n_inline && lane_id() == 0) atomicAdd(&pl_cnt(po.cnt, kPlInlineReads), n_inline);
  } else if (po.heavy_in_lds) {
    // the whole tree's worth of arrays fits a workgroup's LDS (trees of a few thousand nodes): the same code as the first launch, at
    // LDS latency -- in global scratch a heavy read's passes (the rank-by-counting sort above all: leaves^2 loads) took milliseconds
    extern __shared__ __attribute__((aligned(16))) uint8_t s_hv[];
    const uint32_t hl = po.heavy_leaves, hn = po.heavy_nodes;
    lds_f64* f = (lds_f64*)(KR_LDS uint8_t*)s_hv;
    lds_u32* u = (lds_u32*)(f + 2u * hl);
    PlaceArrays<PlaceLdsMem> A{u, u + hl, u + 2u * hl, u + 3u * hl, f, f + hl, u + 4u * hl, hl, hn};
    const uint32_t nh = pl_cnt(po.cnt, kPlHeavySlots);
    for (uint32_t j = blockIdx.x; j < nh; j += gridDim.x) {
      const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)po.heavy[j]);
      if (r == 0xFFFFFFFFu) continue;
      if (!place_read<PlaceLdsMem, NPT, WIT>(C, ix, o, r, read_len, T, po, tau, no_filter, A, (lds_u32*)&s_n, c_pos, c_end, i_pos, i_end, po.chain + (uint64_t)blockIdx.x * po.chain_cap_heavy, po.chain_cap_heavy, kPlWitSecond))
        if (lane_id() == 0) atomicOr(&pl_cnt(po.cnt, kPlFlags), kPlFlagLimits); // (cannot happen: the arrays hold the whole tree)
    }
  } else {
    const uint64_t w = blockIdx.x;
    uint32_t* su = po.heavy_u32 + w * (4ull * po.heavy_leaves + po.heavy_nodes);
    double* sd = po.heavy_f64 + w * (2ull * po.heavy_leaves);
    PlaceArrays<PlaceGlobalMem> A{su, su + po.heavy_leaves, su + 2ull * po.heavy_leaves, su + 3ull * po.heavy_leaves,
                                  sd, sd + po.heavy_leaves, su + 4ull * po.heavy_leaves, po.heavy_leaves, po.heavy_nodes};
    const uint32_t nh = pl_cnt(po.cnt, kPlHeavySlots);
    for (uint32_t j = blockIdx.x; j < nh; j += gridDim.x) {
      const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)po.heavy[j]);
      if (r == 0xFFFFFFFFu) continue;
      if (!place_read<PlaceGlobalMem, NPT, WIT>(C, ix, o, r, read_len, T, po, tau, no_filter, A, (lds_u32*)&s_n, c_pos, c_end, i_pos, i_end, po.chain + (uint64_t)blockIdx.x * po.chain_cap_heavy, po.chain_cap_heavy, kPlWitSecond))
        if (lane_id() == 0) atomicOr(&pl_cnt(po.cnt, kPlFlags), kPlFlagLimits); // (cannot happen: the arrays hold the whole tree)
    }
  }
  for (uint32_t q = i_pos + lane_id(); q < i_end; q += kWave) po.k_se[q] = 0xFFFFFFFFu; // unused list entries
}

// A lane per candidate slot: Brent on the internal candidates' fractional histograms (Minfo::optimize_likelihood,
// src/query.cpp:273-275, :426-433) and chi-square = 2 (f_closest(d) - v_closest) of every candidate (:276, :420-424).
// The internal candidates' minimisations, a lane per LIST entry: every lane of a wave has one to run.  (As a branch of the kernel
// below, a lane per candidate SLOT, the leaf candidates' lanes waited for their neighbours' Brent iterations.)
template <int NPT>
__global__ __launch_bounds__(256) void kr_place_brent_kernel(LlhConst C, PlaceOut po)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables LT{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, LT.bk, LT.hnk);
  if (pl_cnt(po.cnt, kPlFlags) & kPlFlagListCut) return; // the list is incomplete: kr_place_llh_kernel minimises
  const uint32_t np = NPT ? (uint32_t)NPT : C.th + 1, nlist = min(pl_cnt(po.cnt, kPlListSlots), po.lcap);
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nlist; j += gridDim.x * blockDim.x) {
    const uint32_t i = po.k_se[j];
    if (i == 0xFFFFFFFFu) continue;
    LlhProblem p;
    const double* cp = po.c_prob + (uint64_t)i * (np + 2u);
#pragma unroll
    for (uint32_t x = 0; x < np; ++x) p.mc[x] = cp[x];
    p.uc = cp[np], p.rho = cp[np + 1];
    double d = 0, v = 0;
    brent_min<NPT>(C, LT, p, d, v);
    po.c_d[i] = d, po.c_v[i] = v;
  }
}

template <int NPT>
__global__ __launch_bounds__(256) void kr_place_llh_kernel(LlhConst C, PlaceOut po)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables LT{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, LT.bk, LT.hnk);
  const uint32_t np = NPT ? (uint32_t)NPT : C.th + 1, used = min(pl_cnt(po.cnt, kPlCandSlots), po.cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < used; i += gridDim.x * blockDim.x) {
    if (po.c_se[i] == 0) continue;
    const uint32_t rk = po.c_read[i], kind = rk >> 30, r = rk & 0x3FFFFFFFu;
    if (kind == 2u) continue;
    double d = 0, v = 0;
    LlhProblem p;
    if (kind == 1u && !(pl_cnt(po.cnt, kPlFlags) & kPlFlagListCut)) {
      d = po.c_d[i]; // (kr_place_brent_kernel's)
    } else if (kind == 1u) {
      const double* cp = po.c_prob + (uint64_t)i * (np + 2u);
#pragma unroll
      for (uint32_t x = 0; x < np; ++x) p.mc[x] = cp[x];
      p.uc = cp[np], p.rho = cp[np + 1];
      brent_min<NPT>(C, LT, p, d, v);
      po.c_d[i] = d, po.c_v[i] = v;
    } else {
      d = po.c_d[i];
    }
    const double* rp = po.r_prob + (uint64_t)r * (np + 3u);
#pragma unroll
    for (uint32_t x = 0; x < np; ++x) p.mc[x] = rp[x];
    p.uc = rp[np], p.rho = rp[np + 1];
    po.c_chisq[i] = 2 * (llh_eval<NPT>(C, LT, p, d) - rp[np + 2]);
  }
}

// The candidates the last phase will use: report_placement keeps a candidate iff its chi-square against the read's closest
// leaf is below --chisq and it is not the root (src/query.cpp:276-277; the single placement of :233-244 is kept as it is).
// On a large tree a read has dozens of candidates and a handful of survivors: a wave per read copies the survivors,
// in their order, to compact arrays (slots from wave-private chunks), and only those cross PCIe and reach the host's
// last phase (exp / LWR, Jukes-Cantor, text), which applies the same test again to what it is given.
constexpr uint32_t kPlKeepChunk = 256;
__global__ __launch_bounds__(256) void kr_place_compact_kernel(PlaceOut po, PlaceTree T, uint32_t nreads, double chisq_thr)
{
  const uint32_t lane = lane_id();
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave, nwaves = gridDim.x * blockDim.x / kWave;
  uint32_t k_pos = 0, k_end = 0;
  for (uint32_t r = wave; r < nreads; r += nwaves) {
    const uint32_t info = po.rd_info[r];
    if (!(info >> 31)) continue; // (wave-uniform: nothing reported for this read)
    const uint32_t n = info & 0x3FFFFFFFu, c0 = po.rd_c0[r];
    const bool single = ((info >> 30) & 1u) != 0;
    auto keeps = [&](uint32_t t) -> bool {
      if (t >= n) return false;
      const uint32_t se = po.c_se[c0 + t];
      if (se == 0) return false;
      if (single) return true;
      return po.c_chisq[c0 + t] < chisq_thr && T.parent[se] != 0;
    };
    uint32_t total = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += kWave) total += (uint32_t)__popcll(__ballot(keeps(t0 + lane)));
    if (k_pos + total > k_end) {
      const uint32_t take = total > kPlKeepChunk ? total : kPlKeepChunk;
      uint32_t b = 0;
      if (lane == 0) b = atomicAdd(&pl_cnt(po.cnt, kPlKept), take);
      k_pos = __shfl(b, 0, 64), k_end = k_pos + take;
    }
    if (k_end > po.kcap) { // out of slots for the kept candidates (flag of its own: the host grows THESE arrays from kPlKept and runs the batch again)
      if (lane == 0) atomicOr(&pl_cnt(po.cnt, kPlFlags), kPlFlagKeepCap);
      continue;
    }
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += kWave) {
      const uint32_t t = t0 + lane;
      const bool k = keeps(t);
      uint32_t tot;
      const uint32_t pre = wave_prefix_excl(k, tot);
      if (k) {
        const uint32_t j = k_pos + run + pre;
        po.k_se[j] = po.c_se[c0 + t], po.k_d[j] = po.c_d[c0 + t], po.k_v[j] = po.c_v[c0 + t], po.k_chisq[j] = po.c_chisq[c0 + t];
      }
      run += tot;
    }
    if (lane == 0) po.rd_c0[r] = k_pos, po.rd_info[r] = (info & 0xC0000000u) | total;
    k_pos += total;
  }
}


// ---------------------------------------------------------------------------
// Round 6: the rows of `krepp place` as TEXT, written where the placements are (IBatch::report_placement formats them inside
// the parallel batch task, src/query.cpp:283-333, src/query.hpp:202-206; the host's last phase did it on the box's CPUs: 2 x 13 ms
// of a 38 ms jplace call on a 1000-genome tree).  On the kept candidates of a range (kr_place_compact_kernel), a wave per read,
// a lane per candidate:
//   the read's candidates in ascending node number; the chi-square filter once more (:276-277); LWR = exp(-chi2 / 2) / their sum,
//   the sum formed in node order as the host forms it; --no-multi: the candidate of the largest subtree, then the smallest d,
//   then the last (the host's stable sort); Jukes-Cantor pendant length; then per row
//     jplace   [edge, pendant, distal, -v_llh, LWR, d]  inside  \t\t\t{"n" : ["ID"], "p" : [ ... ]}   (",\n" in front of every
//              read that is reported: the host drops the first one of a file)
//     tabular  ID \t label | NA \t edge \t LWR \t d \n
//   numbers as std::fixed with 5 decimals = printf's "%.5f": fixed5_exact (kr_common.h) on the magnitude, the sign in front.
// exp and log are the device library's, the host path's are glibc's: both are within an ulp or two of the true value, which can only
// change a digit if the number lies within ~1e-10 of a rounding tie of its fifth decimal -- a number that has gone through exp or
// log and lies within 1e-8 of one raises flag 8, and the host formats that range (about one range in a thousand).  A magnitude
// of 1000 or more, or infinite: flag 1, likewise.
// Three kernels, as for `dist` (kr_dev_text.inc): lengths, the blocks' first bytes (kr_text_bscan_kernel), bytes.
// ---------------------------------------------------------------------------
// reads per workgroup of the text kernels: a read is a chain of dependent loads, a sort, exp / log and byte stores by two or three
// lanes -- hundreds of microseconds for the 256 reads a wave got with the `dist` text's 1,024-read blocks, whatever the batch
// (2.3 ms of a 9 ms call at the CLI's 65,536 reads); 64 reads a block put every CU to work on a batch of that size
constexpr uint32_t kPlTextBlock = 64;
struct PlaceText {
  const char* ids;           // ids of the range's reads, back to back
  const uint32_t* id_off;    // [nreads + 1]
  const double* blen;        // [pn + 1] branch length above the node, NaN = none
  const uint32_t* card;      // [pn + 1] leaves below the node
  const char* labels;        // node labels back to back
  const uint32_t* label_off; // [pn + 2]
  uint32_t* rd_tlen;         // [nreads] bytes of the read's text
  uint64_t* t_bsum;          // [ceil(nreads / kPlTextBlock) + 1] bytes per block, then (in place) the blocks' first bytes
  char* text;
  uint64_t text_cap;
  uint64_t* total;           // [0] bytes  [1] TextFlag bits (kr_dev_text.inc); kTextNoRange: see kr_place_text_len_kernel
  uint32_t tabular;          // 0 jplace, 1 tabular
  uint32_t multi;
  double chisq;
  // the kept candidates of every read once more, in ascending node number (same slots as k_*), and what the length kernel worked
  // out per read for the writing one: LWR's denominator, --no-multi's choice
  uint32_t* s_se;
  double *s_d, *s_v, *s_c;
  double* rd_total;          // [nreads]
  uint32_t* rd_best;         // [nreads]
};

struct PlaceNum { // one "%.5f" number: its rounded magnitude and how it prints
  uint32_t nn;    // round(|v| * 1e5)
  uint32_t len;   // bytes
  uint8_t neg, nan;
};
// flags: kTextBadNum = not printable here (magnitude >= 1000, infinite); near_tie: the scaled value lies within 1e-8 of a rounding tie
__device__ __forceinline__ PlaceNum place_num_prep(double v, uint32_t& flags, bool& near_tie)
{
  PlaceNum p{0u, 0u, 0, 0};
  near_tie = false;
  if (v != v) { // "nan" / "-nan"
    p.nan = 1, p.neg = (uint8_t)((__double_as_longlong(v) >> 63) & 1);
    p.len = 3u + p.neg;
    return p;
  }
  p.neg = (uint8_t)((__double_as_longlong(v) >> 63) & 1);
  const double av = fabs(v);
  if (!kr::fixed5_exact(av, &p.nn)) {
    flags |= kTextBadNum;
    p.nn = 0;
  }
  const double sc = av * 100000.0, fr = sc - floor(sc);
  near_tie = fabs(fr - 0.5) < 1e-8;
  p.len = (uint32_t)p.neg + (p.nn < 1000000u ? 7u : (p.nn < 10000000u ? 8u : 9u));
  return p;
}
__device__ __forceinline__ char* place_num_put(char* q, const PlaceNum& p)
{
  if (p.neg) *q++ = '-';
  if (p.nan) {
    q[0] = 'n', q[1] = 'a', q[2] = 'n';
    return q + 3;
  }
  uint32_t ip = p.nn / 100000u, fp = p.nn - ip * 100000u;
  const uint32_t nd = ip >= 100u ? 3u : (ip >= 10u ? 2u : 1u);
  for (uint32_t x = nd; x-- > 0u;) q[x] = (char)('0' + ip % 10u), ip /= 10u;
  q[nd] = '.';
#pragma unroll
  for (int x = 4; x >= 0; --x) q[nd + 1u + (uint32_t)x] = (char)('0' + fp % 10u), fp /= 10u;
  return q + nd + 6u;
}
__device__ __forceinline__ uint32_t place_udigits(uint32_t v) { uint32_t n = 1; while (v >= 10u) v /= 10u, ++n; return n; }
__device__ __forceinline__ char* place_uput(char* q, uint32_t v)
{
  const uint32_t n = place_udigits(v);
  for (uint32_t x = n; x-- > 0u;) q[x] = (char)('0' + v % 10u), v /= 10u;
  return q + n;
}

// One read's kept candidates in ascending node number (the order the host path forms them in), written to the s_* arrays at the
// read's own slots (k_* sorted): rank by counting, 64 candidates of mine against all of the read's at a time -- a read keeps a
// handful of candidates, a few keep hundreds (those that reach every genome).  Then, in that order: the chi-square filter once
// more, LWR's denominator `total = total + lwr` as the host adds it, and --no-multi's choice.  Returns the number of candidates.
struct PlaceRow {
  uint32_t se;
  double pend, dist, negv, lwr, d;
};
__device__ __forceinline__ bool place_cand_keep(const PlaceTree& T, const PlaceText& tx, bool single, uint32_t i, uint32_t se, double c)
{
  if (single) return i == 0u; // a single placement: the read's first candidate as it is (src/query.cpp:233-244)
  return c < tx.chisq && T.parent[se] != 0u;
}
__device__ __forceinline__ uint32_t place_read_prepare(const PlaceOut& po, const PlaceTree& T, const PlaceText& tx, uint32_t r, double& total_out, uint32_t& best_out,
                                                       uint32_t& flags)
{
  const uint32_t lane = lane_id();
  const uint32_t info = po.rd_info[r];
  const uint32_t n = info & 0x3FFFFFFFu, c0 = po.rd_c0[r];
  const bool single = ((info >> 30) & 1u) != 0;
  // A node number taken from the kept-candidate arrays indexes the tree's arrays (parent, card, blen, label_off: pn + 1 entries) here
  // and in place_tile_rows, which reads it back from s_se: one that is not a node of the tree is replaced by node 0 and raises
  // kTextNoRange, so that nothing is indexed with it and the host formats the range.  (The compaction writes nodes of the tree
  // only; the check is what stands between a slot it did not write and a load far outside the arrays.)
  auto node_of = [&](uint32_t raw) -> uint32_t {
    if (raw == 0x7FFFFFFFu) return 0u; // (node 0 of a single placement: 0 itself marks an unused slot)
    if (raw > T.pn) {
      flags |= kTextNoRange;
      return 0u;
    }
    return raw;
  };
  // ---- sorted copy
  for (uint32_t a0 = 0; a0 < n; a0 += 64u) {
    const uint32_t i = a0 + lane;
    uint32_t se = 0xFFFFFFFFu;
    if (i < n) se = node_of(po.k_se[c0 + i]);
    uint32_t rank = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 64u) {
      uint32_t sb = 0xFFFFFFFFu;
      if (b0 + lane < n) sb = node_of(po.k_se[c0 + b0 + lane]);
      const uint32_t m = min(64u, n - b0);
      for (uint32_t j = 0; j < m; ++j) {
        const uint32_t sj = (uint32_t)__shfl((int)sb, (int)j);
        rank += (sj < se || (sj == se && b0 + j < i)) ? 1u : 0u;
      }
    }
    if (i < n) {
      tx.s_se[c0 + rank] = se;
      tx.s_d[c0 + rank] = po.k_d[c0 + i], tx.s_v[c0 + rank] = po.k_v[c0 + i], tx.s_c[c0 + rank] = po.k_chisq[c0 + i];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // this wave's own stores, read back below
  WAVE_SYNC();
  // ---- in node order: the sum of the kept candidates' exp(-chi2 / 2); --no-multi: the largest subtree, then the smallest d, then the last
  double total = 0;
  uint32_t best = 0xFFFFFFFFu, bc = 0;
  double bd = 0;
  if (!single)
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
      const uint32_t i = t0 + lane;
      uint32_t se = 0;
      double d = 0, c = 0;
      if (i < n) se = tx.s_se[c0 + i], d = tx.s_d[c0 + i], c = tx.s_c[c0 + i];
      const bool keep = i < n && place_cand_keep(T, tx, false, i, se, c);
      const double lw = keep ? exp(-c / 2) : 0.0;
      const uint32_t cd = keep ? tx.card[se] : 0u;
      for (uint64_t m = __ballot(keep); m != 0; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        total = total + __shfl(lw, j);
        if (!tx.multi) {
          const uint32_t cj = (uint32_t)__shfl((int)cd, j);
          const double dj = __shfl(d, j);
          if (best == 0xFFFFFFFFu || cj > bc || (cj == bc && dj <= bd)) best = t0 + (uint32_t)j, bc = cj, bd = dj;
        }
      }
    }
  total_out = total, best_out = best;
  return n;
}
// this lane's row of tile t0 of the read's SORTED candidates (if it has one); returns the rows of the tile as a lane mask
__device__ __forceinline__ uint64_t place_tile_rows(const PlaceOut& po, const PlaceTree& T, const PlaceText& tx, uint32_t r, uint32_t t0, double total, uint32_t best,
                                                    PlaceRow& row, bool& has_row)
{
  const uint32_t lane = lane_id();
  const uint32_t info = po.rd_info[r];
  const uint32_t n = info & 0x3FFFFFFFu, c0 = po.rd_c0[r];
  const bool single = ((info >> 30) & 1u) != 0;
  const uint32_t i = t0 + lane;
  uint32_t se = 0;
  double d = 0, v = 0, c = 0;
  if (i < n) se = tx.s_se[c0 + i], d = tx.s_d[c0 + i], v = tx.s_v[c0 + i], c = tx.s_c[c0 + i];
  bool keep = i < n && place_cand_keep(T, tx, single, i, se, c);
  if (!single && !tx.multi) keep = keep && i == best;
  has_row = keep;
  if (keep) {
    const double bl = tx.blen[se];
    const double mid = bl != bl ? 0.0 : bl / 2.0;
    row.se = se;
    row.pend = -0.75 * log(1 - 4.0 / 3.0 * d) - mid;
    row.dist = mid, row.negv = -v, row.d = d;
    row.lwr = single ? 1.0 : exp(-c / 2) / total;
  }
  return __ballot(keep);
}
// bytes of this lane's row, its numbers prepared; returns the row's length WITHOUT what stands between rows
__device__ __forceinline__ uint32_t place_row_len(const PlaceText& tx, const PlaceRow& row, uint32_t idl, PlaceNum (&pn)[5], uint32_t& flags)
{
  bool t0, t1, t2, t3, t4;
  const uint32_t edge = row.se - 1u;
  if (tx.tabular) {
    pn[0] = place_num_prep(row.lwr, flags, t0);
    pn[1] = place_num_prep(row.d, flags, t1);
    if (t0) flags |= kTextNearTie; // (LWR went through exp)
    const uint32_t ll = tx.label_off[row.se + 1] - tx.label_off[row.se];
    return idl + 1u + (ll ? ll : 2u) + 1u + place_udigits(edge) + 1u + pn[0].len + 1u + pn[1].len + 1u;
  }
  pn[0] = place_num_prep(row.pend, flags, t0);
  pn[1] = place_num_prep(row.dist, flags, t1);
  pn[2] = place_num_prep(row.negv, flags, t2);
  pn[3] = place_num_prep(row.lwr, flags, t3);
  pn[4] = place_num_prep(row.d, flags, t4);
  if (t0 || t3) flags |= kTextNearTie; // (pendant length through log, LWR through exp)
  return 1u + place_udigits(edge) + 2u + pn[0].len + 2u + pn[1].len + 2u + pn[2].len + 2u + pn[3].len + 2u + pn[4].len + 1u;
}
__device__ __forceinline__ char* place_row_put(char* q, const PlaceText& tx, const PlaceRow& row, const char* id, uint32_t idl, const PlaceNum (&pn)[5])
{
  const uint32_t edge = row.se - 1u;
  if (tx.tabular) {
    for (uint32_t x = 0; x < idl; ++x) q[x] = id[x];
    q += idl;
    *q++ = '\t';
    const uint32_t l0 = tx.label_off[row.se], ll = tx.label_off[row.se + 1] - l0;
    if (ll) {
      for (uint32_t x = 0; x < ll; ++x) q[x] = tx.labels[l0 + x];
      q += ll;
    } else {
      *q++ = 'N', *q++ = 'A';
    }
    *q++ = '\t';
    q = place_uput(q, edge);
    *q++ = '\t';
    q = place_num_put(q, pn[0]);
    *q++ = '\t';
    q = place_num_put(q, pn[1]);
    *q++ = '\n';
    return q;
  }
  *q++ = '[';
  q = place_uput(q, edge);
#pragma unroll
  for (int x = 0; x < 5; ++x) {
    *q++ = ',', *q++ = ' ';
    q = place_num_put(q, pn[x]);
  }
  *q++ = ']';
  return q;
}
// jplace framing: ",\n\t\t\t{\"n\" : [\"" ID "\"], \"p\" : ["  (14 + idl + 11 bytes), rows, closing
constexpr uint32_t kPlJpHead = 14u, kPlJpMid = 11u;
__device__ __forceinline__ uint32_t place_read_len(const PlaceText& tx, bool single, uint32_t nrows, uint32_t rows_len, uint32_t idl)
{
  if (tx.tabular) return rows_len;
  uint32_t len = kPlJpHead + idl + kPlJpMid + rows_len;
  if (single || !tx.multi)
    len += 2u; // "]}"
  else
    len += nrows * 5u + (nrows ? nrows - 1u : 0u) + 6u; // "\n\t\t\t\t" in front of every row, "," between rows, "]\n\t\t\t}"
  return len;
}

__global__ __launch_bounds__(256) void kr_place_text_len_kernel(PlaceOut po, PlaceTree T, PlaceText tx, uint32_t nreads)
{
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  // A range that ran out of candidate slots (kPlFlagCandCap) or of slots for the kept ones (kPlFlagKeepCap) is about to be run again
  // (place_device_finish), and its per-read words are not the compaction's: a read the compaction skipped for want of slots still
  // names its slots in the c_* arrays, where k_se holds the Brent list's slot numbers and 0xFFFFFFFF markers, not nodes.  Nothing of
  // such a range is read: every length is 0, so that kr_text_bscan_kernel finds its sums and total[0] defined, and kTextNoRange
  // in total[1] keeps the writing kernel out and the empty text from being taken for the range's.  (The flag word is final here:
  // these kernels are queued behind the compaction on the same stream.  The guard stands at the range and not in the compaction --
  // which could clear bit 31 of a read it skips -- because it also covers the reads that found no candidate slots, and saves the
  // sort and the logarithms of every other read of an attempt that is thrown away.)
  const bool discarded = (pl_cnt(po.cnt, kPlFlags) & (kPlFlagCandCap | kPlFlagKeepCap)) != 0;
  if (discarded && blockIdx.x == 0 && threadIdx.x == 0) atomicOr((unsigned long long*)&tx.total[1], (unsigned long long)kTextNoRange);
  for (uint32_t b = blockIdx.x; b * kPlTextBlock < nreads; b += gridDim.x) {
    const uint32_t rb = b * kPlTextBlock;
    uint32_t wsum = 0, flags = 0;
    for (uint32_t q = w; q < kPlTextBlock && rb + q < nreads; q += 4u) {
      const uint32_t r = rb + q;
      uint32_t len = 0;
      if (!discarded && (po.rd_info[r] >> 31)) {
        const uint32_t idl = tx.id_off[r + 1] - tx.id_off[r];
        double total;
        uint32_t best;
        const uint32_t n = place_read_prepare(po, T, tx, r, total, best, flags);
        if (lane == 0) tx.rd_total[r] = total, tx.rd_best[r] = best;
        uint32_t nrows = 0, rl = 0;
        for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
          PlaceRow row;
          bool has;
          nrows += (uint32_t)__popcll(place_tile_rows(po, T, tx, r, t0, total, best, row, has));
          PlaceNum pn[5];
          rl += has ? place_row_len(tx, row, idl, pn, flags) : 0u;
        }
        rl = wave_sum(rl);
        len = place_read_len(tx, ((po.rd_info[r] >> 30) & 1u) != 0, nrows, rl, idl);
      }
      if (lane == 0) tx.rd_tlen[r] = len;
      wsum += len;
    }
    flags = wave_or(flags);
    if (flags && lane == 0) atomicOr((unsigned long long*)&tx.total[1], (unsigned long long)flags);
    const uint64_t tot = block_sum_waves<uint64_t>(wsum);
    if (threadIdx.x == 0) tx.t_bsum[b] = tot;
  }
}

__global__ __launch_bounds__(256) void kr_place_text_write_kernel(PlaceOut po, PlaceTree T, PlaceText tx, uint32_t nreads)
{
  __shared__ uint32_t s_off[kPlTextBlock];
  if (tx.total[0] > tx.text_cap || (tx.total[1] & ~(unsigned long long)kTextOverCap) != 0) return; // (the host formats this range, or -- kTextNoRange -- it is run again)
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  for (uint32_t b = blockIdx.x; b * kPlTextBlock < nreads; b += gridDim.x) {
    const uint32_t rb = b * kPlTextBlock, q0 = 4u * threadIdx.x;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      c[q] = (q0 + q < kPlTextBlock && rb + q0 + q < nreads) ? tx.rd_tlen[rb + q0 + q] : 0u;
      tot += c[q];
    }
    uint32_t run = block_scan_excl(tot); // (64 reads: the first 16 threads own them, the totals of the others are 0)
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (q0 + q < kPlTextBlock) s_off[q0 + q] = run;
      run += c[q];
    }
    __syncthreads();
    char* const tb = tx.text + tx.t_bsum[b];
    for (uint32_t q = w; q < kPlTextBlock && rb + q < nreads; q += 4u) {
      const uint32_t r = rb + q;
      if (!(po.rd_info[r] >> 31)) continue; // (wave-uniform)
      const bool single = ((po.rd_info[r] >> 30) & 1u) != 0;
      const uint32_t id0 = tx.id_off[r], idl = tx.id_off[r + 1] - id0;
      const char* id = tx.ids + id0;
      const double total = tx.rd_total[r];
      const uint32_t best = tx.rd_best[r], n = po.rd_info[r] & 0x3FFFFFFFu;
      const bool listed = !tx.tabular && !single && tx.multi; // rows on lines of their own
      char* p = tb + s_off[q];
      if (!tx.tabular) { // head: ,\n\t\t\t{"n" : ["ID"], "p" : [
        const char h1[] = ",\n\t\t\t{\"n\" : [\"";
        const char h2[] = "\"], \"p\" : [";
        if (lane < kPlJpHead) p[lane] = h1[lane];
        for (uint32_t x = lane; x < idl; x += 64u) p[kPlJpHead + x] = id[x];
        if (lane < kPlJpMid) p[kPlJpHead + idl + lane] = h2[lane];
        p += kPlJpHead + idl + kPlJpMid;
      }
      uint32_t rows_before = 0; // rows of the tiles done (wave-uniform)
      for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        PlaceRow row;
        bool has;
        uint32_t flags = 0;
        const uint64_t hm = place_tile_rows(po, T, tx, r, t0, total, best, row, has);
        PlaceNum pn[5];
        const uint32_t rl = has ? place_row_len(tx, row, idl, pn, flags) : 0u;
        const uint32_t before = rows_before + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull)); // rows in front of mine
        const uint32_t comma = (has && listed && before) ? 1u : 0u;                              // "," between rows
        const uint32_t mine = rl + (has && listed ? 5u : 0u) + comma;                            // "\n\t\t\t\t" in front of a row
        const uint32_t incl = wave_scan_incl(mine);
        if (has) {
          char* o = p + (incl - mine);
          if (listed) {
            if (comma) *o++ = ',';
            *o++ = '\n', *o++ = '\t', *o++ = '\t', *o++ = '\t', *o++ = '\t';
          }
          place_row_put(o, tx, row, id, idl, pn);
        }
        p += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        rows_before += (uint32_t)__popcll(hm);
      }
      if (!tx.tabular) {
        if (listed) {
          const char t1[] = "]\n\t\t\t}";
          if (lane < 6u) p[lane] = t1[lane];
        } else if (lane < 2u) {
          p[lane] = lane ? '}' : ']';
        }
      }
    }
    __syncthreads();
  }
}
