// kr_build.cpp — index construction (`krepp index`, `krepp sketch`).  On the CPU by default; the leaf stage and the key stage
// can run on the GPU, and the groups' colour classes be found there (kr_build_params::gpu_minimizers, kr_minimizer.hip,
// kr_build_keys.hip), with identical files.  It exists
// because no index can be obtained any other way (the reference ships none).  Output files follow the reference's on-disk format
// byte for byte (src/krepp.cpp:18-29,206-246; src/table.cpp:77-83;
// src/record.cpp:213-219).
//
// Behaviour restated from:
//   set_nrows                         src/krepp.cpp:5-16
//   random LSH positions              src/lshf.cpp:126-147
//   minimizer extraction + rho        src/rqseq.cpp:51-144 (incl. the ring buffer that is
//                                     not reset at N / sequence ends, :67,108-114)
//   sort + unique per row             src/table.cpp:234-260
//   colour sets up the guide tree     src/table.cpp:182-232, src/record.cpp:5-107
//   compaction to colour ids          src/record.cpp:131-176
// Design differs from the reference (which materialises a row-vector table per tree
// node and unions them recursively): every genome yields a sorted list of
// (row, enc32) keys; equal keys are grouped across genomes and the colour of each
// group is folded up the guide tree.  The resulting leaf sets are identical; ids of
// colours that are not tree nodes depend on hash-map iteration order in the
// reference and on creation order here (set-level results unchanged).
#include "kr_common.h"
#include "kr_sdust.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <random>
#include <sstream>
#include <sys/stat.h>
#include <unordered_map>
#if defined(_OPENMP)
#include <omp.h>
#endif

namespace {

inline unsigned code_of(unsigned char c)
{ // seq_nt4_table, src/common.cpp:10-14
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
  }
}

} // namespace

namespace kr {

// HyperLogLog with b=12 as the reference instantiates it (src/rqseq.cpp:63-64,
// src/hyperloglog.hpp:98-135): index = top b bits of the 32-bit hash, rank =
// min(32-b, clz(hash << b)) + 1.
struct Hll {
  static constexpr int b = 12;
  std::vector<uint8_t> reg;
  Hll()
    : reg(1u << b, 0)
  {}
  void add(uint32_t hsh)
  {
    uint32_t ix = hsh >> (32 - b);
    uint32_t rest = hsh << b;
    int lz = rest ? __builtin_clz(rest) : 32;
    uint8_t rank = (uint8_t)(std::min(32 - b, lz) + 1);
    if (rank > reg[ix]) reg[ix] = rank;
  }
};

double hll12_estimate(const uint8_t* reg)
{
  const double mreg = 4096.0;
  const double alpha_mm = (0.7213 / (1.0 + 1.079 / mreg)) * mreg * mreg;
  double sum = 0.0;
  uint32_t zeros = 0;
  for (int i = 0; i < 4096; ++i) {
    sum += 1.0 / (double)(1u << reg[i]);
    zeros += reg[i] == 0;
  }
  double est = alpha_mm / sum;
  if (est <= 2.5 * mreg) {
    if (zeros) est = mreg * std::log(mreg / zeros);
  } else if (est > (1.0 / 30.0) * 4294967296.0) {
    est = -4294967296.0 * std::log(1.0 - est / 4294967296.0);
  }
  return est;
}

uint32_t LshPositions::rix(uint64_t bp) const
{
  uint32_t v = 0;
  for (uint32_t j = 0; j < h; ++j) v |= (uint32_t)((bp >> (2 * pasc[j])) & 3u) << (2 * j);
  return v;
}
uint32_t LshPositions::enc32(uint64_t bp) const
{
  uint32_t v = 0;
  for (uint32_t j = 0; j < k - h; ++j) {
    uint32_t c = (uint32_t)((bp >> (2 * npos[j])) & 3u);
    v |= (c & 1u) << j;
    v |= (c >> 1) << (16 + j);
  }
  return v;
}

bool make_positions(uint32_t k, uint32_t h, const uint8_t* ppos, LshPositions& lsh)
{
  lsh.k = k, lsh.h = h;
  lsh.ppos.assign(ppos, ppos + h);
  std::sort(lsh.ppos.begin(), lsh.ppos.end(), std::greater<uint8_t>());
  lsh.pasc.assign(lsh.ppos.rbegin(), lsh.ppos.rend());
  lsh.npos.clear();
  for (uint8_t p = 0; p < k; ++p)
    if (!std::count(lsh.ppos.begin(), lsh.ppos.end(), p)) lsh.npos.push_back(p);
  return lsh.pasc.size() == h && lsh.pasc.back() < k && lsh.npos.size() == k - h;
}

// RSeq::extract_mers (src/rqseq.cpp:51-144) for one contig.  rgs[0 .. mn): the contig's sdust intervals (start << 32 | finish),
// walked one at a time as :91-107 does; mn = 0: sdust off.
void extract_contig_cpu(const uint8_t* seq, uint64_t len, const BuildCfg& c, const LshPositions& lsh,
                        std::vector<uint64_t>& keys, double& n1, double& n2, const uint64_t* rgs, size_t mn)
{
  uint32_t k = c.k, w = c.w;
  uint32_t ldiff = w > k ? w - k + 1 : 1;
  if (w <= k) w = k;
  Hll c1, c2;
  struct Slot {
    uint64_t x, z;
  };
  std::vector<Slot> win(ldiff, Slot{0, 0});
  uint64_t kix = 0;
  const uint64_t mask_bp = ~0ull >> ((32 - k) * 2);
  uint64_t bp = 0;
  uint32_t l = 0;
  uint64_t mrs = 0, mre = len;
  size_t mi = 0;
  if (mn > 0) mre = (uint32_t)rgs[0], mrs = (uint32_t)(rgs[0] >> 32);
  for (uint64_t i = 0; i < len;) {
    unsigned cd = code_of(seq[i]);
    if (cd >= 4) {
      l = 0, i++;
      continue;
    }
    l++, i++;
    bp = (bp << 2) + cd; // compute/update_encoding give the same enc_bp once masked
    if (l < k) continue;
    uint64_t x = bp & mask_bp;
    if (mi < mn && i + k > mrs) { // src/rqseq.cpp:91-107: counted, kept out of the window; the interval ends with l = 0
      c1.add((uint32_t)fmix64(x));
      if (i < mre) continue;
      mi++;
      l = 0;
      if (mi < mn) mre = (uint32_t)rgs[mi], mrs = (uint32_t)(rgs[mi] >> 32);
      continue;
    }
    Slot s{x, fmix64(x)};
    win[kix % ldiff] = s;
    c1.add((uint32_t)s.z);
    kix++;
    if ((l < w) && (i != len)) continue;
    // std::min_element: first minimum in slot order (src/rqseq.cpp:115-116)
    size_t best = 0;
    for (size_t q = 1; q < win.size(); ++q)
      if (win[q].z < win[best].z) best = q;
    const Slot& mn_slot = win[best];
    c2.add((uint32_t)mn_slot.z);
    int64_t row = build_row(lsh.rix(mn_slot.x), c);
    if (row >= 0) keys.push_back(((uint64_t)row << 32) | lsh.enc32(mn_slot.x));
  }
  n1 += hll12_estimate(c1.reg.data());
  n2 += hll12_estimate(c2.reg.data());
}

// The interval walk of src/rqseq.cpp:91-107 as two bit strings over the contig (what the device's leaf stage reads):
//   skip[g]: the k-mer whose LAST base is g is counted for c1 but kept out of the window;
//   brk[b]:  l is set to 0 between bases b-1 and b (no k-mer spans that point).
// For interval j, skipping starts at the first valid k-mer end i (exclusive) with i + k > mrs_j and lasts up to and including the
// first valid one with i >= mre_j, i*_j, where the break falls.  "Valid" is l >= k, and l restarts at i*_(j-1): the chain runs over
// intervals.  Bits of invalid k-mers are set too; nobody reads them.
void resolve_mask(const uint8_t* seq, uint64_t len, uint32_t k, const uint64_t* rgs, size_t mn, std::vector<uint64_t>& skip,
                  std::vector<uint64_t>& brk)
{
  const size_t nw = (size_t)(len / 64) + 2;
  skip.assign(nw, 0);
  brk.assign(nw, 0);
  auto set_range = [&](uint64_t a, uint64_t b) { // bits [a, b)
    for (uint64_t q = a; q < b;) {
      if ((q & 63u) == 0 && b - q >= 64) {
        skip[q >> 6] = ~0ull, q += 64;
      } else {
        skip[q >> 6] |= 1ull << (q & 63u), ++q;
      }
    }
  };
  uint64_t last_break = 0;
  for (size_t j = 0; j < mn; ++j) {
    const uint64_t mrs = (uint32_t)(rgs[j] >> 32), mre = (uint32_t)rgs[j];
    const uint64_t from = mrs + 1 > k ? mrs + 1 - k : 0; // first end i with i + k > mrs
    // i*: the first i >= max(mre, last_break + k, from) with no non-base in [i - k, i)
    uint64_t i = std::max(std::max(mre, last_break + k), std::max<uint64_t>(from, k));
    bool found = false;
    while (i <= len) {
      uint64_t q = i;
      while (q > i - k && code_of(seq[q - 1]) < 4) --q;
      if (q == i - k) {
        found = true;
        break;
      }
      i = q + k; // q - 1 is no base: the next k-mer without it ends at q + k
    }
    if (!found) { // the contig ends while this interval is current
      if (from < len) set_range(from ? from - 1 : 0, len);
      return;
    }
    set_range(from ? from - 1 : 0, i); // ends from .. i  =  last bases from-1 .. i-1
    if (i < len) brk[i >> 6] |= 1ull << (i & 63u);
    last_break = i;
  }
}

bool contig_end_special(const uint8_t* seq, uint64_t len, const BuildCfg& c, uint64_t& x, uint64_t& z, const uint64_t* skip,
                        const uint64_t* brk)
{
  const uint32_t k = c.k, w = std::max(c.w, c.k), ldiff = w - k + 1;
  auto bit = [](const uint64_t* a, uint64_t q) { return a && ((a[q >> 6] >> (q & 63u)) & 1u); };
  // length of the final run of valid bases (behind the last non-base or the last break of the interval walk)
  uint64_t l = 0;
  while (l < len && code_of(seq[len - 1 - l]) < 4) {
    ++l;
    if (bit(brk, len - l)) break;
  }
  if (l < k || l >= w) return false; // no k-mer at the end, or the regular window rule applies
  if (bit(skip, len - 1)) return false; // the contig ends while skipping: src/rqseq.cpp:91-95 continues before :112
  // the ring buffer holds the last `ldiff` k-mers PUSHED anywhere in the contig (it is never reset; skipped k-mers are not
  // pushed), and zeros where fewer than ldiff have been pushed
  const uint64_t mask_bp = ~0ull >> ((32 - k) * 2);
  std::vector<uint64_t> xs; // most recent first
  uint64_t i = len;
  while (i > 0 && xs.size() < ldiff) {
    // k-mer ending at base i-1 is valid iff the k bases [i-k, i) are valid and no break lies strictly inside
    if (skip && i >= 64 && (i & 63u) == 0 && skip[(i >> 6) - 1] == ~0ull) {
      i -= 64; // 64 skipped ends at once
      continue;
    }
    if (i >= k && !bit(skip, i - 1)) {
      bool ok = true;
      uint64_t bp = 0;
      for (uint64_t q = i - k; q < i; ++q) {
        unsigned cd = code_of(seq[q]);
        if (cd >= 4 || (q > i - k && bit(brk, q))) {
          ok = false;
          break;
        }
        bp = (bp << 2) + cd;
      }
      if (ok) xs.push_back(bp & mask_bp);
    }
    --i;
  }
  bool have_zero = xs.size() < ldiff;
  x = 0, z = 0;
  bool first = true;
  for (uint64_t v : xs) {
    uint64_t hz = fmix64(v);
    if (first || hz < z) x = v, z = hz, first = false;
  }
  if (have_zero && (first || 0 < z)) x = 0, z = 0; // a never-written slot {0,0,0} wins unless some hash is 0
  return true;
}

// ---- sdust on the host (kr_sdust.h) ----
int sdust_check(uint32_t T, uint32_t W, const uint64_t* offsets, uint32_t ncontigs, const char* who)
{
  if (T == 0 || W < 4 || T > 0x7FFFFFFFu || W > 0x7FFFFFFFu) return fail(KR_ERR_ARG, std::string(who) + ": sdust needs T > 0 and W >= 4");
  for (uint32_t q = 0; q < ncontigs; ++q) {
    if (offsets[q + 1] < offsets[q]) return fail(KR_ERR_ARG, std::string(who) + ": offsets must not decrease");
    if (offsets[q + 1] - offsets[q] >= (1ull << 31))
      return fail(KR_ERR_ARG, std::string(who) + ": contig of 2^31 bases or more (the reference's sdust positions are int)");
  }
  return KR_OK;
}

namespace {
struct HostSdust { // a state with room for any W; P grows on demand (the contig is run again)
  std::vector<uint8_t> ring;
  std::vector<SdustPerf> P;
  SdustState<int32_t> S;
  HostSdust(uint32_t T, uint32_t W)
    : ring(W - 2)
    , P(256)
  {
    sdust_init(S, ring.data(), (int32_t)ring.size(), P.data(), (int32_t)P.size(), (int32_t)T, (int32_t)W);
  }
  void grow()
  {
    P.resize(P.size() * 2);
    sdust_init(S, ring.data(), (int32_t)ring.size(), P.data(), (int32_t)P.size(), S.T, S.W);
  }
};
} // namespace

// sdust(0, seq, -1, T, W, &n) for one contig: whole replay, the list merged as save_masked_regions does (src/sdust.h:117-122)
void sdust_contig_host(const uint8_t* seq, uint64_t len, uint32_t T, uint32_t W, std::vector<uint64_t>& out, uint32_t* pmax)
{
  HostSdust h(T, W);
  const size_t n0 = out.size();
  for (;;) {
    auto emit = [&](int32_t s, int32_t f) {
      if (out.size() > n0) {
        const int32_t ps = (int32_t)(out.back() >> 32), pf = (int32_t)(uint32_t)out.back();
        if (s <= pf) {
          out.back() = (uint64_t)(uint32_t)ps << 32 | (uint32_t)(pf > f ? pf : f);
          return;
        }
      }
      out.push_back((uint64_t)(uint32_t)s << 32 | (uint32_t)f);
    };
    sdust_scan(seq, len, W, [&](SdustEvent e) {
      if (!h.S.overflow) sdust_event(h.S, e, emit);
    });
    if (!h.S.overflow) break;
    out.resize(n0);
    h.grow();
  }
  if (pmax && (uint32_t)h.S.pmax > *pmax) *pmax = (uint32_t)h.S.pmax;
}

int sdust_lists_host(const uint8_t* bases, const uint64_t* offsets, uint32_t ncontigs, uint32_t T, uint32_t W, std::vector<uint64_t>& iv,
                     std::vector<uint64_t>& ioff)
{
  int rc = sdust_check(T, W, offsets, ncontigs, "sdust");
  if (rc) return rc;
  ioff.assign(1, 0);
  iv.clear();
  for (uint32_t q = 0; q < ncontigs; ++q) {
    sdust_contig_host(bases + offsets[q], offsets[q + 1] - offsets[q], T, W, iv, nullptr);
    ioff.push_back(iv.size());
  }
  return KR_OK;
}

int finish_sdust(const std::vector<uint64_t>& iv, const std::vector<uint64_t>& ioff, kr_sdust_result* out)
{
  out->ncontigs = (uint32_t)ioff.size() - 1;
  out->intervals = (uint64_t*)malloc(std::max<size_t>(1, iv.size()) * 8);
  out->offsets = (uint64_t*)malloc(ioff.size() * 8);
  if (!out->intervals || !out->offsets) {
    free(out->intervals), free(out->offsets);
    out->intervals = out->offsets = nullptr;
    return fail(KR_ERR_NOMEM, "kr_sdust: out of memory");
  }
  if (!iv.empty()) memcpy(out->intervals, iv.data(), iv.size() * 8);
  memcpy(out->offsets, ioff.data(), ioff.size() * 8);
  return KR_OK;
}

// ---- the key stage on the host ----
int key_groups_alloc(kr_key_groups* out, uint64_t nkeys, uint64_t npairs, uint32_t nrows)
{
  memset(out, 0, sizeof(*out));
  out->keys = (uint64_t*)malloc(std::max<uint64_t>(1, nkeys) * 8);
  out->goff = (uint64_t*)malloc((nkeys + 1) * 8);
  out->ranks = (uint32_t*)malloc(std::max<uint64_t>(1, npairs) * 4);
  out->inc = (uint64_t*)calloc(std::max<uint64_t>(1, nrows), 8);
  if (!out->keys || !out->goff || !out->ranks || !out->inc) {
    kr_key_groups_free(out);
    return fail(KR_ERR_NOMEM, "key stage: out of memory");
  }
  out->goff[0] = 0;
  out->nkeys = nkeys, out->npairs = npairs, out->nrows = nrows;
  return KR_OK;
}

int key_groups_host(std::vector<KeyRank>& all, uint32_t nrows, uint32_t nleaves, kr_key_groups* out)
{
  std::sort(all.begin(), all.end(), [](const KeyRank& a, const KeyRank& b) { return a.key != b.key ? a.key < b.key : a.rank < b.rank; });
  // runs of equal keys; within a run a rank counts once
  uint64_t nkeys = 0, npairs = 0;
  for (size_t a = 0; a < all.size(); ++a) {
    const bool head = a == 0 || all[a].key != all[a - 1].key;
    nkeys += head;
    npairs += head || all[a].rank != all[a - 1].rank;
    if ((uint32_t)(all[a].key >> 32) >= nrows) return fail(KR_ERR_FORMAT, "row out of range");
    if (all[a].rank >= nleaves) return fail(KR_ERR_ARG, "key stage: leaf rank out of range");
  }
  int rc = key_groups_alloc(out, nkeys, npairs, nrows);
  if (rc) return rc;
  uint64_t ik = 0, ip = 0;
  for (size_t a = 0; a < all.size();) {
    size_t b = a;
    out->keys[ik] = all[a].key, out->goff[ik] = ip;
    while (b < all.size() && all[b].key == all[a].key) {
      if (b == a || all[b].rank != all[b - 1].rank) out->ranks[ip++] = all[b].rank;
      ++b;
    }
    out->inc[(uint32_t)(all[a].key >> 32)]++;
    ++ik;
    a = b;
  }
  out->goff[nkeys] = npairs;
  for (uint32_t rr = 1; rr < nrows; ++rr) out->inc[rr] += out->inc[rr - 1];
  std::vector<KeyRank>().swap(all);
  return KR_OK;
}

// ---- the colour classes on the host ----
int colour_classes_alloc(kr_colour_classes* out, uint64_t nkeys, uint64_t cap)
{
  memset(out, 0, sizeof(*out));
  out->class_of = (uint32_t*)malloc(std::max<uint64_t>(1, nkeys) * 4);
  out->rep = (uint64_t*)malloc(std::max<uint64_t>(1, cap) * 8);
  if (!out->class_of || !out->rep) {
    kr_colour_classes_free(out);
    return fail(KR_ERR_NOMEM, "colour classes: out of memory");
  }
  memset(out->class_of, 0xFF, nkeys * 4);
  out->nkeys = nkeys;
  return KR_OK;
}

// One class per distinct rank sequence: a hash map from the sequence's hash to the newest class with it, classes of one hash chained
// through `next`; a group joins the class whose first group has its very ranks, or opens one.
int colour_classes_host(const uint64_t* goff, const uint32_t* ranks, uint64_t nkeys, kr_colour_classes* out)
{
  uint64_t multi = 0;
  for (uint64_t i = 0; i < nkeys; ++i) multi += goff[i + 1] - goff[i] >= 2;
  if (multi >= KR_NO_CLASS) return fail(KR_ERR_CAPACITY, "colour classes: 2^32 - 1 groups of several ranks or more");
  std::vector<uint64_t> rep;
  std::vector<uint32_t> next;
  std::unordered_map<uint64_t, uint32_t> newest;
  int rc = colour_classes_alloc(out, nkeys, 0);
  if (rc) return rc;
  for (uint64_t i = 0; i < nkeys; ++i) {
    const uint64_t a = goff[i], len = goff[i + 1] - a;
    if (len < 2) continue;
    uint64_t h = fmix64(len);
    for (uint64_t q = 0; q < len; ++q) h = fmix64(h ^ ranks[a + q]) + q;
    auto ins = newest.emplace(h, (uint32_t)rep.size());
    uint32_t c = ins.second ? KR_NO_CLASS : ins.first->second;
    for (; c != KR_NO_CLASS; c = next[c]) {
      const uint64_t b = goff[rep[c]];
      if (goff[rep[c] + 1] - b == len && !memcmp(ranks + a, ranks + b, len * 4)) break;
    }
    if (c == KR_NO_CLASS) {
      c = (uint32_t)rep.size();
      next.push_back(ins.second ? KR_NO_CLASS : ins.first->second);
      ins.first->second = c;
      rep.push_back(i);
    }
    out->class_of[i] = c;
  }
  free(out->rep);
  out->rep = (uint64_t*)malloc(std::max<size_t>(1, rep.size()) * 8);
  if (!out->rep) {
    kr_colour_classes_free(out);
    return fail(KR_ERR_NOMEM, "colour classes: out of memory");
  }
  if (!rep.empty()) memcpy(out->rep, rep.data(), rep.size() * 8);
  out->nclasses = rep.size();
  return KR_OK;
}

namespace {
std::atomic<uint64_t> g_colour_stat[8];
}
void colour_stats_note(uint64_t groups, uint64_t multi, uint64_t classes, uint64_t raised, uint64_t path, uint64_t passes)
{
  const uint64_t v[8] = {groups, multi, classes, raised, path, passes, 0, 0};
  for (int q = 0; q < 8; ++q) g_colour_stat[q].store(v[q]);
}

} // namespace kr

extern "C" int kr_colour_classes_cpu(const uint64_t* goff, const uint32_t* ranks, uint64_t nkeys, kr_colour_classes* out)
{
  kr::clear_error();
  if (!out || !goff) return kr::fail(KR_ERR_ARG, "kr_colour_classes_cpu: null argument");
  memset(out, 0, sizeof(*out));
  if (goff[0] != 0 || !std::is_sorted(goff, goff + nkeys + 1)) return kr::fail(KR_ERR_ARG, "kr_colour_classes_cpu: goff must ascend from 0");
  if (goff[nkeys] && !ranks) return kr::fail(KR_ERR_ARG, "kr_colour_classes_cpu: null argument");
  return kr::colour_classes_host(goff, ranks, nkeys, out);
}

extern "C" void kr_colour_classes_free(kr_colour_classes* c)
{
  if (!c) return;
  free(c->class_of), free(c->rep);
  memset(c, 0, sizeof(*c));
}

extern "C" void kr_debug_build_colours(uint64_t out[8])
{
  if (!out) return;
  for (int q = 0; q < 8; ++q) out[q] = kr::g_colour_stat[q].load();
}

extern "C" int kr_key_groups_cpu(const uint64_t* keys, const uint32_t* ranks, uint64_t n, uint32_t nrows, uint32_t nleaves, kr_key_groups* out)
{
  kr::clear_error();
  if (!out || (n && (!keys || !ranks))) return kr::fail(KR_ERR_ARG, "kr_key_groups_cpu: null argument");
  memset(out, 0, sizeof(*out));
  if (nleaves > 65536u) return kr::fail(KR_ERR_ARG, "kr_key_groups_cpu: more than 65536 leaves");
  std::vector<kr::KeyRank> all(n);
  for (uint64_t i = 0; i < n; ++i) all[i] = kr::KeyRank{keys[i], ranks[i]};
  return kr::key_groups_host(all, nrows, nleaves, out);
}

extern "C" void kr_key_groups_free(kr_key_groups* g)
{
  if (!g) return;
  free(g->keys), free(g->goff), free(g->ranks), free(g->inc);
  memset(g, 0, sizeof(*g));
}

namespace {
using kr::BuildCfg;
using kr::LshPositions;
using kr::fmix64;

struct Genome {
  std::string name, path;
  std::vector<uint64_t> keys; // (row << 32) | enc32, sorted unique
  double n1 = 0, n2 = 0;      // HLL sums over contigs
  bool present = false;
};

// Record / Subset (src/record.cpp:5-107): colour sets identified by the wrapping sum
// of their leaves' 64-bit name hashes.
struct SubsetRec {
  uint64_t ch;   // one of the two parts (the larger one)
  uint32_t card;
  uint64_t nonce;
  uint32_t se;
};

struct Colours {
  std::unordered_map<uint64_t, SubsetRec> by_sh;
  std::vector<uint64_t> created; // non-node subsets in creation order

  // Record::add_subset (src/record.cpp:82-107) with check_subset_collision (:119-130)
  uint64_t add(uint64_t sh1, uint64_t sh2)
  {
    const SubsetRec& s1 = by_sh.at(sh1);
    const SubsetRec& s2 = by_sh.at(sh2);
    uint64_t ch = s1.card > s2.card ? sh1 : sh2;
    uint32_t card = s1.card + s2.card;
    uint64_t sh = sh1 + sh2, nonce = 0;
    for (;;) {
      auto it = by_sh.find(sh + nonce);
      if (it == by_sh.end()) break;
      const SubsetRec& s = it->second;
      bool collision = (s.ch == 0 || (sh + nonce) == 0) ? true : !(s.ch == sh1 || s.ch == sh2);
      if (!collision) return sh + nonce;
      uint64_t t = nonce;
      nonce = kr::rehash64(t * sh1 * sh2); // nonce++ is post-increment: the old value is hashed
    }
    sh += nonce;
    by_sh[sh] = SubsetRec{ch, card, nonce, 0};
    created.push_back(sh);
    return sh;
  }
};

struct BuildTree {
  kr::HostTree t;
  std::vector<std::vector<uint32_t>> kids; // by se
  std::vector<uint64_t> sh;                // by se
  std::vector<uint32_t> lo, hi;            // leaf-rank interval of each subtree
  std::vector<uint32_t> leaf_rank;         // by se (leaves)
};

// Colour of a key present in the leaves ranks[a..b) (sorted leaf ranks), restricted to
// the subtree of `se`.  Children are folded LAST to FIRST so that a clade present in
// all children lands on the tree node's own id (Record(tree) registers each node with
// ch = its first child, src/record.cpp:5-33).
uint64_t colour_of(const BuildTree& bt, Colours& col, uint32_t se, const uint32_t* ranks, size_t a, size_t b)
{
  if (bt.t.nodes[se].kind == 1) return bt.sh[se];
  if (b - a == (size_t)(bt.hi[se] - bt.lo[se])) return bt.sh[se]; // whole clade
  uint64_t acc = 0;
  bool have = false;
  const auto& ch = bt.kids[se];
  for (size_t ci = ch.size(); ci-- > 0;) {
    uint32_t c = ch[ci];
    const uint32_t* p0 = std::lower_bound(ranks + a, ranks + b, bt.lo[c]);
    const uint32_t* p1 = std::lower_bound(ranks + a, ranks + b, bt.hi[c]);
    if (p0 == p1) continue;
    uint64_t s = colour_of(bt, col, c, ranks, (size_t)(p0 - ranks), (size_t)(p1 - ranks));
    acc = have ? col.add(acc, s) : s;
    have = true;
  }
  return acc;
}

// the given positions, or LSHF::get_random_positions (src/lshf.cpp:126-147) with the thread-local mt19937 `gen`
bool choose_positions(const kr_build_params* bp, const BuildCfg& c, LshPositions& lsh)
{
  lsh.k = c.k, lsh.h = c.h;
  if (bp->ppos) {
    lsh.ppos.assign(bp->ppos, bp->ppos + c.h);
    std::sort(lsh.ppos.begin(), lsh.ppos.end(), std::greater<uint8_t>());
  } else {
    std::mt19937 gen;
    if (bp->seed) gen.seed(bp->seed);
    std::uniform_int_distribution<uint8_t> distrib(0, (uint8_t)(c.k - 1));
    while (lsh.ppos.size() < c.h) {
      uint8_t n = distrib(gen);
      if (!std::count(lsh.ppos.begin(), lsh.ppos.end(), n)) lsh.ppos.push_back(n);
    }
    std::sort(lsh.ppos.begin(), lsh.ppos.end(), std::greater<uint8_t>());
  }
  lsh.pasc.assign(lsh.ppos.rbegin(), lsh.ppos.rend());
  for (uint8_t p = 0; p < c.k; ++p)
    if (!std::count(lsh.ppos.begin(), lsh.ppos.end(), p)) lsh.npos.push_back(p);
  return lsh.pasc.size() == c.h && lsh.pasc.back() < c.k;
}

// BaseLSH::set_nrows (src/krepp.cpp:5-16)
uint32_t nrows_of(const BuildCfg& c)
{
  uint32_t hash_size = 1u << (2 * c.h), full_res = hash_size % c.m, nrows;
  if (c.frac) {
    nrows = (hash_size / c.m) * (c.r + 1);
    nrows = full_res > c.r ? nrows + (c.r + 1) : nrows + full_res;
  } else {
    nrows = hash_size / c.m;
    nrows = full_res > c.r ? nrows + 1 : nrows;
  }
  return nrows;
}

// validate_configuration (src/krepp.hpp:59-90)
const char* bad_configuration(const BuildCfg& c)
{
  if (c.w < c.k) return "The minimum minimizer window size (-w) is k (-k).";
  if (c.h < 3 || c.h > 15) return "The number of LSH positions (-h) must be in [3,15].";
  if (c.k > 31 || c.k < 19) return "The k-mer length (-k) must be in [19,31].";
  if (c.k - c.h > 16) return "For compact k-mer encodings, h must be >= k-16.";
  if (c.m == 0 || c.r >= c.m) return "need 0 <= r < m";
  return nullptr;
}

bool write_file(const std::string& path, const void* hdr, size_t hdr_bytes, const void* data, size_t bytes)
{
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  bool ok = fwrite(hdr, 1, hdr_bytes, f) == hdr_bytes && (bytes == 0 || fwrite(data, 1, bytes, f) == bytes);
  return fclose(f) == 0 && ok;
}

// KR_BUILD_TIMING=1: the build's phases on stderr, one line each
struct PhaseClock {
  const bool on = getenv("KR_BUILD_TIMING") && atoi(getenv("KR_BUILD_TIMING")) != 0;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
  // less: seconds of the time since the last phase that belong to another phase (printed by span)
  void done(const char* phase, double less = 0)
  {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "build timing: %-24s %10.3f s\n", phase, std::chrono::duration<double>(now - last).count() - less);
    last = now;
  }
  void span(const char* phase, double seconds)
  {
    if (on) fprintf(stderr, "build timing: %-24s %10.3f s\n", phase, seconds);
  }
  void classes()
  {
    if (!on) return;
    uint64_t st[8] = {0};
    kr_debug_build_colours(st);
    fprintf(stderr, "build colours: groups %llu multi_rank_groups %llu classes %llu raised_by_compare %llu path %llu passes %llu\n",
            (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4],
            (unsigned long long)st[5]);
  }
  // the key stage's counts; pairs_in / passes: what the device path saw (0: the host path, whose input is unique per genome already)
  void keys(const kr_key_groups& g, bool device_pool)
  {
    if (!on) return;
    uint64_t st[8] = {0};
    if (device_pool) kr_debug_build_keys(st);
    fprintf(stderr, "build keys: pairs_in %llu pairs_out %llu keys %llu passes %llu pool_growths %llu path %llu\n", (unsigned long long)st[0],
            (unsigned long long)g.npairs, (unsigned long long)g.nkeys, (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[5]);
  }
  void total(const char* what)
  {
    if (on) fprintf(stderr, "build timing: %-24s %10.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
};
struct PoolOwner { // the device pool of a build, given back at every return
  kr::KeyPool* p = nullptr;
  ~PoolOwner() { kr::key_pool_free(p); }
};

// One contig through the leaf stage, masked when sdust is on.  Returns "" or what is wrong with the contig.
std::string masked_contig_cpu(const uint8_t* seq, uint64_t len, const BuildCfg& c, const LshPositions& lsh, uint32_t sdust_t,
                              uint32_t sdust_w, std::vector<uint64_t>& keys, double& n1, double& n2)
{
  if (!sdust_t) {
    kr::extract_contig_cpu(seq, len, c, lsh, keys, n1, n2);
    return "";
  }
  if (len >= (1ull << 31)) return "sdust: contig of 2^31 bases or more (the reference's sdust positions are int)";
  std::vector<uint64_t> iv;
  kr::sdust_contig_host(seq, len, sdust_t, sdust_w, iv, nullptr);
  kr::extract_contig_cpu(seq, len, c, lsh, keys, n1, n2, iv.data(), iv.size());
  return "";
}

} // namespace

extern "C" int kr_build_index(const char* input_tsv, const char* nwk_path, const char* out_dir,
                              const kr_build_params* bp)
{
  kr::clear_error();
  if (!input_tsv || !out_dir || !bp) return kr::fail(KR_ERR_ARG, "kr_build_index: null argument");
  BuildCfg c{bp->k, bp->w, bp->h, bp->m, bp->r, bp->frac != 0};
  if (const char* why = bad_configuration(c)) return kr::fail(KR_ERR_ARG, why);
  PhaseClock clk;

  // input map: name \t path (src/krepp.cpp:147-162)
  std::vector<Genome> genomes;
  {
    std::ifstream in(input_tsv);
    if (!in.good()) return kr::fail(KR_ERR_IO, std::string("Error opening ") + input_tsv);
    std::string line;
    while (std::getline(in, line)) {
      size_t tab = line.find('\t');
      if (tab == std::string::npos) return kr::fail(KR_ERR_FORMAT, "Failed to read the reference name to path/URL mapping!");
      Genome g;
      g.name = line.substr(0, tab);
      size_t tab2 = line.find('\t', tab + 1);
      g.path = line.substr(tab + 1, tab2 == std::string::npos ? std::string::npos : tab2 - tab - 1);
      genomes.push_back(g);
    }
  }
  if (genomes.empty()) return kr::fail(KR_ERR_FORMAT, "empty input map");

  // guide tree (src/krepp.cpp:131-145)
  BuildTree bt;
  std::string nwk_text;
  if (nwk_path && *nwk_path) {
    std::ifstream tf(nwk_path);
    if (!tf.good()) return kr::fail(KR_ERR_IO, std::string("Error opening ") + nwk_path);
    std::stringstream ss;
    ss << tf.rdbuf();
    nwk_text = ss.str();
    std::string err;
    if (!kr::parse_newick(nwk_text, bt.t, err)) return kr::fail(KR_ERR_FORMAT, err);
  } else {
    std::vector<std::string> names;
    for (auto& g : genomes) names.push_back(g.name);
    kr::balanced_tree(names, bt.t);
  }
  uint32_t nn = bt.t.nnodes();
  bt.kids.assign(nn + 1, {});
  bt.sh.assign(nn + 1, 0);
  bt.lo.assign(nn + 1, 0);
  bt.hi.assign(nn + 1, 0);
  bt.leaf_rank.assign(nn + 1, 0);
  for (uint32_t se = 1; se <= nn; ++se)
    if (bt.t.nodes[se].parent) bt.kids[bt.t.nodes[se].parent].push_back(se);
  // post-order numbering => a subtree is a contiguous se interval; leaf ranks follow se order
  std::map<std::string, uint32_t> leaf_by_name;
  uint32_t nleaves = 0;
  for (uint32_t se = 1; se <= nn; ++se) {
    if (bt.t.nodes[se].kind == 1) {
      bt.leaf_rank[se] = nleaves;
      bt.lo[se] = nleaves;
      bt.hi[se] = ++nleaves;
      uint64_t s = kr::leaf_name_hash(bt.t.nodes[se].label);
      while (!s) s = kr::rehash64(0x9e3779b97f4a7c15ull + se); // src/phytree.cpp:207-209 rehashes an address
      bt.sh[se] = s;
      leaf_by_name[bt.t.nodes[se].label] = se;
    } else {
      uint32_t lo = 0xFFFFFFFFu, hi = 0;
      uint64_t s = 0;
      for (uint32_t cse : bt.kids[se]) {
        lo = std::min(lo, bt.lo[cse]);
        hi = std::max(hi, bt.hi[cse]);
        s += bt.sh[cse]; // Node::add_children, src/phytree.hpp:107-116
      }
      bt.lo[se] = lo, bt.hi[se] = hi, bt.sh[se] = s;
    }
  }
  Colours col;
  col.by_sh[0] = SubsetRec{0, 0, 0, 0};
  for (uint32_t se = 1; se <= nn; ++se) {
    uint64_t ch = bt.t.nodes[se].kind == 1 ? 0 : bt.sh[bt.kids[se].front()];
    if (col.by_sh.count(bt.sh[se]))
      return kr::fail(KR_ERR_FORMAT, "node-name hash collision in the guide tree (Record::check_tree_collision)");
    col.by_sh[bt.sh[se]] = SubsetRec{ch, bt.hi[se] - bt.lo[se], 0, se};
  }

  // LSH positions
  LshPositions lsh;
  if (!choose_positions(bp, c, lsh)) return kr::fail(KR_ERR_ARG, "bad LSH positions");
  const uint32_t nrows = nrows_of(c);

  // leaves: minimizers of every contig (DynHT::fill_table, src/table.cpp:247-260)
  int nthreads = bp->num_threads ? (int)bp->num_threads : 1;
  (void)nthreads;
  std::string first_err;
  int first_rc = KR_ERR_IO;
  const uint32_t sdust_t = bp->sdust_t && bp->sdust_w ? bp->sdust_t : 0, sdust_w = sdust_t ? bp->sdust_w : 0; // either at 0: off
  if (sdust_t && sdust_w < 4) return kr::fail(KR_ERR_ARG, "--sdust-w must be at least 4");
  // KR_BUILD_GPU_KEYS: the genomes' raw keys stay on the device, in a pool that the key stage sorts and groups after the last genome
  PoolOwner pool;
  if (bp->gpu_minimizers & (KR_BUILD_GPU_KEYS | KR_BUILD_GPU_COLOURS)) {
    if (nleaves > 65536u)
      kr::key_stage_note_path(3); // two rank digits at most: this build keeps its keys on the host
    else if (int prc = kr::key_pool_create(bp->device, &pool.p))
      return prc;
  }
#if defined(_OPENMP)
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
#endif
  for (int64_t gi = 0; gi < (int64_t)genomes.size(); ++gi) {
    Genome& g = genomes[gi];
    if (!leaf_by_name.count(g.name)) continue; // genome not in the tree: never visited by build_for_subtree
    kr_fastx* fx = nullptr;
    if (kr_fastx_open(g.path.c_str(), &fx) != KR_OK) {
#if defined(_OPENMP)
#pragma omp critical
#endif
      if (first_err.empty()) first_err = "Failed to open the file at " + g.path;
      continue;
    }
    kr_fastx_batch b;
    std::vector<uint8_t> all_bases; // gpu_minimizers: the whole genome goes to the device at once
    std::vector<uint64_t> all_offs{0};
    do {
      kr_fastx_next(fx, 1, &b); // one record at a time keeps contigs separate
      for (uint32_t q = 0; q < b.nreads; ++q) {
        uint64_t len = b.offsets[q + 1] - b.offsets[q];
        if (bp->gpu_minimizers) {
          all_bases.insert(all_bases.end(), b.bases + b.offsets[q], b.bases + b.offsets[q + 1]);
          all_offs.push_back(all_bases.size());
        } else if (len >= c.w) {
          std::string why = masked_contig_cpu(b.bases + b.offsets[q], len, c, lsh, sdust_t, sdust_w, g.keys, g.n1, g.n2); // RSeq::set_curr_seq: len >= w
          if (!why.empty()) {
#if defined(_OPENMP)
#pragma omp critical
#endif
            if (first_err.empty()) first_err = why, first_rc = KR_ERR_ARG;
          }
        }
      }
    } while (b.more);
    kr_fastx_close(fx);
    if (bp->gpu_minimizers) {
      kr_build_params bq = *bp;
      bq.ppos = lsh.ppos.data();
      kr_minimizer_result mr;
      memset(&mr, 0, sizeof(mr));
      int mrc = KR_OK;
      // sdust: the host masker runs here, beside the other genomes' threads and outside the lock around the device; the device's
      // leaf stage reads the mask as uploaded bit strings
      std::vector<uint64_t> iv, ioff;
      const bool host_mask = sdust_t && sdust_w;
      if (host_mask) mrc = kr::sdust_lists_host(all_bases.data(), all_offs.data(), (uint32_t)all_offs.size() - 1, sdust_t, sdust_w, iv, ioff);
      const kr::MinSink sink{pool.p, pool.p ? bt.leaf_rank[leaf_by_name.at(g.name)] : 0u, 0.0, 0.0};
      if (mrc == KR_OK) {
#if defined(_OPENMP)
#pragma omp critical(kr_gpu_minimizers)
#endif
        mrc = kr::minimizers_device(bp->device, &bq, all_bases.data(), all_offs.data(), (uint32_t)all_offs.size() - 1,
                                    host_mask ? &iv : nullptr, host_mask ? &ioff : nullptr, &mr, &sink);
      }
      if (mrc != KR_OK) {
#if defined(_OPENMP)
#pragma omp critical
#endif
        if (first_err.empty()) first_err = std::string("GPU minimizers: ") + kr_last_error();
        continue;
      }
      g.keys.assign(mr.keys, mr.keys + mr.nkeys);
      g.n1 = mr.n1, g.n2 = mr.n2;
      kr_minimizers_free(&mr);
    }
    std::sort(g.keys.begin(), g.keys.end());
    g.keys.erase(std::unique(g.keys.begin(), g.keys.end()), g.keys.end());
    g.present = true;
  }
  if (!first_err.empty()) return kr::fail(first_rc, first_err);
  clk.done("read + leaf stage");

  // group equal keys across genomes: the key stage, on the device's pool or on the host
  struct Groups : kr_key_groups {
    Groups() { memset(static_cast<kr_key_groups*>(this), 0, sizeof(kr_key_groups)); }
    ~Groups() { kr_key_groups_free(this); }
  } grp;
  // KR_BUILD_GPU_COLOURS: the groups' colour classes with them, from the device while the groups are there or else from the host
  struct Classes : kr_colour_classes {
    Classes() { memset(static_cast<kr_colour_classes*>(this), 0, sizeof(kr_colour_classes)); }
    ~Classes() { kr_colour_classes_free(this); }
  } cls;
  const bool classed = (bp->gpu_minimizers & KR_BUILD_GPU_COLOURS) != 0;
  double cls_seconds = 0;
  const bool pooled = pool.p != nullptr;
  if (pooled) {
    int krc = kr::key_pool_finish(pool.p, nrows, nleaves, &grp, classed ? &cls : nullptr, &cls_seconds);
    kr::key_pool_free(pool.p), pool.p = nullptr;
    if (krc) return krc;
  } else {
    std::vector<kr::KeyRank> all;
    size_t tot = 0;
    for (auto& g : genomes) tot += g.keys.size();
    all.reserve(tot);
    for (auto& g : genomes) {
      if (!g.present) continue;
      uint32_t rank = bt.leaf_rank[leaf_by_name[g.name]];
      for (uint64_t key : g.keys) all.push_back(kr::KeyRank{key, rank});
      std::vector<uint64_t>().swap(g.keys);
    }
    if (all.empty()) return kr::fail(KR_ERR_FORMAT, "No k-mers to index!");
    if (int krc = kr::key_groups_host(all, nrows, nleaves, &grp)) return krc;
  }
  if (grp.nkeys == 0) return kr::fail(KR_ERR_FORMAT, "No k-mers to index!");
  clk.done("key sort + group", cls_seconds);
  clk.keys(grp, pooled);
  if (classed) {
    if (cls.class_of) {
      clk.span("colour classes", cls_seconds);
    } else { // the device did not make them: the canonical classes, from the host's copy of the groups
      if (int crc = kr::colour_classes_host(grp.goff, grp.ranks, grp.nkeys, &cls)) return crc;
      uint64_t multi = 0;
      for (uint64_t i = 0; i < grp.nkeys; ++i) multi += cls.class_of[i] != KR_NO_CLASS;
      kr::colour_stats_note(grp.nkeys, multi, cls.nclasses, 0, 2, 0);
      clk.done("colour classes");
    }
    clk.classes();
  } else {
    kr::colour_stats_note(0, 0, 0, 0, 0, 0);
  }

  // colours of the groups IN KEY ORDER: Colours::created's order fixes the ids of the colours that are no tree nodes
  std::vector<uint32_t> leaf_se(nleaves, 0);
  for (uint32_t se = 1; se <= nn; ++se)
    if (bt.t.nodes[se].kind == 1) leaf_se[bt.leaf_rank[se]] = se;
  std::vector<uint64_t> out_sh(classed ? 0 : grp.nkeys);
  uint32_t root_se = nn;
  for (uint64_t i = 0; i < out_sh.size(); ++i) {
    const uint64_t a = grp.goff[i], b = grp.goff[i + 1];
    // one leaf: colour_of would walk down to it and create nothing on the way
    out_sh[i] = b - a == 1 ? bt.sh[leaf_se[grp.ranks[a]]] : colour_of(bt, col, root_se, grp.ranks, (size_t)a, (size_t)b);
  }
  // ... or of the classes in the order of their first groups, which is the order in which the loop above meets each leaf set for
  // the first time; at every later group of a set colour_of finds what the first walk made and creates nothing
  std::vector<uint64_t> class_sh(cls.nclasses);
  for (uint64_t cc = 0; cc < cls.nclasses; ++cc) {
    const uint64_t i = cls.rep[cc];
    class_sh[cc] = colour_of(bt, col, root_se, grp.ranks, (size_t)grp.goff[i], (size_t)grp.goff[i + 1]);
  }

  // Record::make_compact + CRecord(record) (src/record.cpp:131-176)
  uint32_t next_se = nn + 1;
  for (uint64_t s : col.created) col.by_sh[s].se = next_se++;
  uint32_t nsubsets = next_se; // sh_to_se.size()+1 with the empty set at 0
  std::vector<uint32_t> pse((size_t)nsubsets * 2, 0);
  for (auto& kv : col.by_sh) {
    const SubsetRec& s = kv.second;
    if (kv.first == 0) continue;
    auto f1 = col.by_sh.find(s.ch);
    auto f2 = col.by_sh.find(kv.first - s.ch - s.nonce);
    pse[2 * (size_t)s.se] = f1 == col.by_sh.end() ? 0 : f1->second.se;
    pse[2 * (size_t)s.se + 1] = f2 == col.by_sh.end() ? 0 : f2->second.se; // operator[] default in the reference
  }
  std::vector<double> rho(nn + 1, 0.0);
  for (auto& g : genomes)
    if (g.present) rho[leaf_by_name[g.name]] = g.n1 > 0 ? g.n2 / g.n1 : 0.0; // RSeq::compute_rho, src/rqseq.hpp:79
  std::vector<uint32_t> cmer(grp.nkeys * 2);
  for (size_t i = 0; i < out_sh.size(); ++i) {
    cmer[2 * i] = (uint32_t)grp.keys[i];
    cmer[2 * i + 1] = col.by_sh[out_sh[i]].se;
  }
  if (classed) { // one look-up per class; a group of one leaf has the leaf's id, as bt.sh[leaf_se[rank]] looks up above
    std::vector<uint32_t> class_se(cls.nclasses);
    for (uint64_t cc = 0; cc < cls.nclasses; ++cc) class_se[cc] = col.by_sh.at(class_sh[cc]).se;
#if defined(_OPENMP)
#pragma omp parallel for schedule(static) num_threads(nthreads)
#endif
    for (int64_t i = 0; i < (int64_t)grp.nkeys; ++i) {
      cmer[2 * i] = (uint32_t)grp.keys[i];
      cmer[2 * i + 1] = cls.class_of[i] == KR_NO_CLASS ? leaf_se[grp.ranks[grp.goff[i]]] : class_se[cls.class_of[i]];
    }
  }
  clk.done("colours");

  // save_index (src/krepp.cpp:206-246)
  mkdir(out_dir, 0777);
  std::string sfx = "-m" + std::to_string(c.m) + "r" + std::to_string(c.r) + (c.frac ? "-frac" : "-no_frac");
  std::string dir = out_dir;
  uint64_t nk = grp.nkeys;
  uint32_t nn1 = nn + 1;
  bool ok = write_file(dir + "/cmer" + sfx, &nk, 8, cmer.data(), cmer.size() * 4);
  ok = ok && write_file(dir + "/inc" + sfx, &nrows, 4, grp.inc, (size_t)nrows * 8);
  {
    std::string blob;
    blob.append((const char*)&nn1, 4);
    blob.append((const char*)&nsubsets, 4);
    blob.append((const char*)pse.data(), pse.size() * 4);
    blob.append((const char*)rho.data(), rho.size() * 8);
    ok = ok && write_file(dir + "/crecord" + sfx, blob.data(), blob.size(), nullptr, 0);
  }
  {
    std::string names;
    for (auto& g : genomes) names += g.name + "\n";
    ok = ok && write_file(dir + "/reflist" + sfx, names.data(), names.size(), nullptr, 0);
  }
  if (!nwk_text.empty()) ok = ok && write_file(dir + "/tree" + sfx, nwk_text.data(), nwk_text.size(), nullptr, 0);
  {
    std::string md;
    uint8_t k8 = (uint8_t)c.k, w8 = (uint8_t)c.w, h8 = (uint8_t)c.h, f8 = c.frac ? 1 : 0;
    md.append((const char*)&k8, 1), md.append((const char*)&w8, 1), md.append((const char*)&h8, 1);
    md.append((const char*)&c.m, 4), md.append((const char*)&c.r, 4), md.append((const char*)&f8, 1);
    md.append((const char*)&nrows, 4);
    md.append((const char*)lsh.ppos.data(), lsh.ppos.size());
    md.append((const char*)lsh.npos.data(), lsh.npos.size());
    ok = ok && write_file(dir + "/metadata" + sfx, md.data(), md.size(), nullptr, 0);
  }
  {
    std::ostringstream info; // IndexMultiple::save_info (src/krepp.cpp:187-204); ignored by loaders
    info << "krepp version: v0.8.3-compatible (krepp-amd)\nseed: " << bp->seed << "\nk: " << c.k << "\nw: " << c.w
         << "\nh: " << c.h << "\nm: " << c.m << "\nfrac: " << (c.frac ? "true" : "false") << "\nnrows: " << nrows
         << "\ntotal_num_kmers: " << nk << "\n";
    if (sdust_t) info << "sdust-t: " << sdust_t << "\nsdust-w: " << sdust_w << "\n";
    std::string s = info.str();
    ok = ok && write_file(dir + "/metadata" + sfx + ".txt", s.data(), s.size(), nullptr, 0);
  }
  if (!ok) return kr::fail(KR_ERR_IO, std::string("failed to write index files under ") + out_dir);
  clk.done("write");
  clk.total("total");
  return KR_OK;
}

// ---------------------------------------------------------------------------
// Leaf stage on its own (CPU): the reference path for kr_minimizers_device.
// ---------------------------------------------------------------------------
namespace kr {
int check_minimizer_params(const kr_build_params* bp, BuildCfg& c, LshPositions& lsh)
{
  if (!bp || !bp->ppos) return fail(KR_ERR_ARG, "kr_minimizers: parameters with explicit ppos are required");
  c = BuildCfg{bp->k, bp->w, bp->h, bp->m, bp->r, bp->frac != 0};
  if (c.k > 31 || c.k < 3 || c.h == 0 || c.h >= c.k || c.k - c.h > 16 || c.h > 15 || c.m == 0 || c.r >= c.m || c.w > 255)
    return fail(KR_ERR_ARG, "kr_minimizers: unsupported k/w/h/m/r");
  if (!make_positions(c.k, c.h, bp->ppos, lsh)) return fail(KR_ERR_ARG, "kr_minimizers: bad LSH positions");
  return KR_OK;
}
int finish_minimizers(std::vector<uint64_t>& keys, double n1, double n2, kr_minimizer_result* out)
{
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  out->nkeys = keys.size();
  out->keys = (uint64_t*)malloc(std::max<size_t>(1, keys.size()) * 8);
  if (!out->keys) return fail(KR_ERR_NOMEM, "kr_minimizers: out of memory");
  if (!keys.empty()) memcpy(out->keys, keys.data(), keys.size() * 8);
  out->n1 = n1;
  out->n2 = n2;
  return KR_OK;
}
} // namespace kr

extern "C" int kr_minimizers_cpu(const kr_build_params* bp, const uint8_t* bases, const uint64_t* offsets, uint32_t ncontigs,
                                 kr_minimizer_result* out)
{
  kr::clear_error();
  if (!bases || !offsets || !out) return kr::fail(KR_ERR_ARG, "kr_minimizers_cpu: null argument");
  BuildCfg c;
  LshPositions lsh;
  int rc = kr::check_minimizer_params(bp, c, lsh);
  if (rc) return rc;
  std::vector<uint64_t> keys;
  double n1 = 0, n2 = 0;
  const uint32_t sdust_t = bp->sdust_t && bp->sdust_w ? bp->sdust_t : 0, sdust_w = sdust_t ? bp->sdust_w : 0;
  if (sdust_t && (rc = kr::sdust_check(sdust_t, sdust_w, offsets, ncontigs, "kr_minimizers_cpu"))) return rc;
  for (uint32_t q = 0; q < ncontigs; ++q) {
    uint64_t len = offsets[q + 1] - offsets[q];
    if (len >= c.w) masked_contig_cpu(bases + offsets[q], len, c, lsh, sdust_t, sdust_w, keys, n1, n2);
  }
  return kr::finish_minimizers(keys, n1, n2, out);
}

extern "C" int kr_sdust_cpu(const uint8_t* bases, const uint64_t* offsets, uint32_t ncontigs, uint32_t T, uint32_t W, kr_sdust_result* out)
{
  kr::clear_error();
  if (!bases || !offsets || !out) return kr::fail(KR_ERR_ARG, "kr_sdust_cpu: null argument");
  std::vector<uint64_t> iv, ioff;
  int rc = kr::sdust_lists_host(bases, offsets, ncontigs, T, W, iv, ioff);
  return rc ? rc : kr::finish_sdust(iv, ioff, out);
}

extern "C" void kr_sdust_free(kr_sdust_result* r)
{
  if (!r) return;
  free(r->intervals);
  free(r->offsets);
  r->intervals = r->offsets = nullptr;
  r->ncontigs = 0;
}

extern "C" void kr_minimizers_free(kr_minimizer_result* r)
{
  if (!r) return;
  free(r->keys);
  r->keys = nullptr;
  r->nkeys = 0;
}

// `krepp sketch` (SketchSingle::create_sketch / save_sketch, src/krepp.cpp:110-129): the minimizers of ONE
// FASTA/FASTQ file as a table without colours.  SDynHT::fill_table (src/table.cpp:234-246) = extract_mers of
// every record of length >= w, rows sorted by code, duplicates removed; file = SFlatHT::save
// (src/table.cpp:34-40: nkmers u64, codes u32[], nrows u32, cumulative row ends u64[]) + save_configuration
// (src/krepp.cpp:18-29) + rho f64.
extern "C" int kr_build_sketch(const char* input_path, const char* out_path, const kr_build_params* bp)
{
  kr::clear_error();
  if (!input_path || !out_path || !bp) return kr::fail(KR_ERR_ARG, "kr_build_sketch: null argument");
  BuildCfg c{bp->k, bp->w, bp->h, bp->m, bp->r, bp->frac != 0};
  if (const char* why = bad_configuration(c)) return kr::fail(KR_ERR_ARG, why);
  LshPositions lsh;
  if (!choose_positions(bp, c, lsh)) return kr::fail(KR_ERR_ARG, "bad LSH positions");
  const uint32_t nrows = nrows_of(c);
  const uint32_t sdust_t = bp->sdust_t && bp->sdust_w ? bp->sdust_t : 0, sdust_w = sdust_t ? bp->sdust_w : 0; // either at 0: off
  if (sdust_t && sdust_w < 4) return kr::fail(KR_ERR_ARG, "--sdust-w must be at least 4");
  PhaseClock clk;
  // gpu_minimizers, as in kr_build_index: the leaf stage of every batch of records on the device; KR_BUILD_GPU_KEYS: the keys stay
  // there, and the sort, the unique and the row counts are the key stage with one leaf.  One leaf has no colours to fold:
  // KR_BUILD_GPU_COLOURS is ignored.
  const bool gpu_leaf = (bp->gpu_minimizers & ~KR_BUILD_GPU_COLOURS) != 0;
  PoolOwner pool;
  if (bp->gpu_minimizers & KR_BUILD_GPU_KEYS)
    if (int prc = kr::key_pool_create(bp->device, &pool.p)) return prc;
  kr_build_params bq = *bp;
  bq.ppos = lsh.ppos.data();
  kr_fastx* fx = nullptr;
  if (kr_fastx_open(input_path, &fx) != KR_OK) return kr::fail(KR_ERR_IO, std::string("Failed to open the file at ") + input_path);
  std::vector<uint64_t> keys;
  double n1 = 0, n2 = 0;
  kr_fastx_batch b;
  do {
    if (kr_fastx_next(fx, 1u << 20, &b)) {
      kr_fastx_close(fx);
      return KR_ERR_IO;
    }
    if (gpu_leaf) {
      if (b.nreads == 0) continue;
      kr_minimizer_result mr;
      memset(&mr, 0, sizeof(mr));
      const kr::MinSink sink{pool.p, 0u, n1, n2}; // the contigs' estimates are added in file order, as on the host
      if (int mrc = kr::minimizers_device(bp->device, &bq, b.bases, b.offsets, b.nreads, nullptr, nullptr, &mr, &sink)) {
        kr_fastx_close(fx);
        return mrc;
      }
      keys.insert(keys.end(), mr.keys, mr.keys + mr.nkeys);
      n1 = mr.n1, n2 = mr.n2;
      kr_minimizers_free(&mr);
      continue;
    }
    for (uint32_t q = 0; q < b.nreads; ++q) {
      const uint64_t len = b.offsets[q + 1] - b.offsets[q];
      if (len < c.w) continue; // RSeq::set_curr_seq
      std::string why = masked_contig_cpu(b.bases + b.offsets[q], len, c, lsh, sdust_t, sdust_w, keys, n1, n2);
      if (!why.empty()) {
        kr_fastx_close(fx);
        return kr::fail(KR_ERR_ARG, why);
      }
    }
  } while (b.more);
  kr_fastx_close(fx);
  clk.done("read + leaf stage");
  std::vector<uint32_t> enc;
  std::vector<uint64_t> inc(nrows, 0);
  if (pool.p) {
    kr_key_groups grp;
    memset(&grp, 0, sizeof(grp));
    int krc = kr::key_pool_finish(pool.p, nrows, 1, &grp);
    kr::key_pool_free(pool.p), pool.p = nullptr;
    if (krc) return krc;
    enc.resize(grp.nkeys);
    for (uint64_t i = 0; i < grp.nkeys; ++i) enc[i] = (uint32_t)grp.keys[i];
    std::copy(grp.inc, grp.inc + nrows, inc.begin());
    kr_key_groups_free(&grp);
  } else {
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    enc.resize(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
      const uint32_t row = (uint32_t)(keys[i] >> 32);
      if (row >= nrows) return kr::fail(KR_ERR_STATE, "kr_build_sketch: row out of range");
      enc[i] = (uint32_t)keys[i];
      inc[row]++;
    }
    for (uint32_t r = 1; r < nrows; ++r) inc[r] += inc[r - 1];
  }
  clk.done("key sort + group");
  const double rho = n1 > 0 ? n2 / n1 : 0.0; // RSeq::compute_rho, src/rqseq.hpp:79
  std::string blob;
  const uint64_t nk = enc.size();
  blob.append((const char*)&nk, 8);
  blob.append((const char*)enc.data(), enc.size() * 4);
  blob.append((const char*)&nrows, 4);
  blob.append((const char*)inc.data(), inc.size() * 8);
  const uint8_t k8 = (uint8_t)c.k, w8 = (uint8_t)c.w, h8 = (uint8_t)c.h, f8 = c.frac ? 1 : 0;
  blob.append((const char*)&k8, 1), blob.append((const char*)&w8, 1), blob.append((const char*)&h8, 1);
  blob.append((const char*)&c.m, 4), blob.append((const char*)&c.r, 4), blob.append((const char*)&f8, 1);
  blob.append((const char*)&nrows, 4);
  blob.append((const char*)lsh.ppos.data(), lsh.ppos.size());
  blob.append((const char*)lsh.npos.data(), lsh.npos.size());
  blob.append((const char*)&rho, 8);
  if (!write_file(out_path, blob.data(), blob.size(), nullptr, 0)) return kr::fail(KR_ERR_IO, "Failed to write the sketch!");
  clk.done("write");
  clk.total("total");
  fprintf(stderr, "Total number of k-mers included in the sketch: %llu\nSubsampling rate (rho) is: %g\n", (unsigned long long)nk, rho);
  return KR_OK;
}
