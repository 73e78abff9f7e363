// kr_host_index.inc -- part of kr_device.hip (host side): kr_index, kr_index_upload / export / import / free, kr_index_broadcast (RCCL).

struct kr_index {
  int device = 0;
  uint32_t log_g = 0;           // lanes per probe in the bucket scan = 2^log_g (from the mean bucket length)
  uint32_t occ = 0;             // 1: the packed tables carry a row-occupancy bitmap (sparse tables)
  uint32_t slot_log2w = 0;      // slotted table copy: format code (slot_words(): 5 / 6 / 7 = 32 / 64 / 128 words, 8 = 48 words; 0: none)
  DevIndex dix;
  std::vector<DevLib> hlibs;    // host copy of the device DevLib array
  std::vector<void*> allocs;    // everything to hipFree
  std::vector<kr_index_buffer> bufs; // export order
  std::vector<uint8_t> desc;    // export descriptor
  uint64_t bytes = 0;
  // workspace of kr_llh_batch (grown on demand, reused across calls): one device buffer and one pinned host
  // buffer laid out [hist n*np | uc n | rho n | d_in n | d_out n | v n]
  // kernel chain: the kernels of every batch (every lane of every kr_stream) on this index run one batch after the
  // other, in submission order -- each batch's first kernel waits for the event recorded behind the previous batch's
  // last -- while the H2D copy in front of them and the D2H copy behind them overlap other batches' kernels.
  // Concurrent batches only slow each other down (DESIGN.md: measured), and a pipeline whose stages take turns
  // keeps the chip busy with two streams.
  mutable std::mutex chain_mu;
  static constexpr uint32_t kChainEvents = 16;
  mutable hipEvent_t chain_ev[kChainEvents] = {nullptr};
  mutable uint32_t chain_n = 0;
  mutable bool chain_off = false;
  mutable std::mutex llh_mu;
  mutable DevBuf<double> llh_dev; // (one capacity, in doubles)
  mutable PinBuf<double> llh_pin;
  // node names by colour id, for the device-side report text (kr_stream_text_enable; uploaded once, under chain_mu)
  mutable DevBuf<char> d_names;
  mutable DevBuf<uint32_t> d_name_off; // [tree_nnodes + 2]
};

namespace {

// One link of an index's kernel chain, as a scope around a batch's kernels on `st`: construction takes chain_mu and queues the wait for
// the previous batch's kernels (its result: `opened`), close() records the event the next batch waits for.  A scope that is left
// without close() -- a HIP call failed in between -- releases the lock and records no link.
struct ChainLink {
  const kr_index* ix;
  std::unique_lock<std::mutex> lock;
  hipError_t opened = hipSuccess;
  ChainLink(const kr_index* index, hipStream_t st) : ix(index), lock(index->chain_mu)
  {
    if (!ix->chain_off && ix->chain_n) opened = hipStreamWaitEvent(st, ix->chain_ev[(ix->chain_n - 1) % kr_index::kChainEvents], 0);
  }
  hipError_t close(hipStream_t st)
  {
    if (!ix->chain_off) {
      hipEvent_t& ce = ix->chain_ev[ix->chain_n % kr_index::kChainEvents];
      if (!ce)
        if (hipError_t e = hipEventCreateWithFlags(&ce, hipEventDisableTiming)) return e;
      if (hipError_t e = hipEventRecord(ce, st)) return e;
      ++ix->chain_n;
    }
    lock.unlock();
    return hipSuccess;
  }
};

struct DescHeader {
  uint32_t magic, k, h, m, nlibs, tree_nnodes, nleaves, log_g;
  uint32_t slot_log2w, occ; // format code of the slotted table copy (slot_words(); 0: none); 1: row-occupancy bitmaps
  uint64_t res_mask;
  uint8_t ppos[32], npos[32];
};
struct DescLib {
  uint64_t nkmers, nlist;
  uint32_t nrows, nsubsets, nnodes, numer;
};

int dev_alloc(kr_index* ix, void** p, uint64_t bytes)
{
  HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
  ix->allocs.push_back(*p);
  ix->bytes += bytes;
  return KR_OK;
}

// Allocate every device buffer of an index from its descriptor; fills ix->dix/hlibs/bufs.
int alloc_from_desc(kr_index* ix, const DescHeader& H, const std::vector<DescLib>& L)
{
  ix->hlibs.resize(H.nlibs);
  ix->bufs.clear();
  for (uint32_t i = 0; i < H.nlibs; ++i) {
    DevLib& d = ix->hlibs[i];
    memset(&d, 0, sizeof(d));
    d.nkmers = L[i].nkmers, d.nlist = L[i].nlist, d.nrows = L[i].nrows, d.nsubsets = L[i].nsubsets, d.nnodes = L[i].nnodes,
    d.numer = L[i].numer;
    void* p;
    int rc;
    uint64_t b;
    b = (uint64_t)d.nrows * 8;
    if ((rc = dev_alloc(ix, &p, b))) return rc;
    d.bkt = (const uint64_t*)p;
    ix->bufs.push_back({p, b});
    b = (d.nkmers + 16) * 4; // 16 entries of slack: 16-byte chunk loads may run past the end
    if ((rc = dev_alloc(ix, &p, b))) return rc;
    d.enc = (const uint32_t*)p;
    ix->bufs.push_back({p, b});
    b = (d.nkmers + 16) * 4;
    if ((rc = dev_alloc(ix, &p, b))) return rc;
    d.se = (const uint32_t*)p;
    ix->bufs.push_back({p, b});
    b = (uint64_t)d.nsubsets * 8;
    if ((rc = dev_alloc(ix, &p, b))) return rc;
    d.pse = (const uint2*)p;
    ix->bufs.push_back({p, b});
    b = (uint64_t)d.nnodes * 8;
    if ((rc = dev_alloc(ix, &p, b))) return rc;
    d.rho = (const double*)p;
    ix->bufs.push_back({p, b});
    b = d.nlist * 4;
    if ((rc = dev_alloc(ix, &p, b))) return rc;
    d.leaflist = (const uint32_t*)p;
    ix->bufs.push_back({p, b});
    if (H.occ) {
      b = (((uint64_t)d.nrows + 31) / 32) * 4;
      if ((rc = dev_alloc(ix, &p, b))) return rc;
      d.occ = (const uint32_t*)p;
      ix->bufs.push_back({p, b});
    }
    d.slot_log2w = H.slot_log2w;
    if (H.slot_log2w) {
      b = (uint64_t)d.nrows * slot_words(H.slot_log2w) * 4;
      if ((rc = dev_alloc(ix, &p, b))) return rc;
      d.slots = (const uint32_t*)p;
      ix->bufs.push_back({p, b});
    }
    if (H.slot_log2w == kSlotFilter) { // filter slots: the entries' colours and rest bits in slot order
      b = (uint64_t)d.nrows * kFiltSlotCodes * 8;
      if ((rc = dev_alloc(ix, &p, b))) return rc;
      d.sx = (const uint2*)p;
      ix->bufs.push_back({p, b});
    }
  }
  void* p;
  int rc;
  uint64_t b = ((uint64_t)H.tree_nnodes + 1) * 4;
  if ((rc = dev_alloc(ix, &p, b))) return rc;
  ix->dix.node_info = (const uint32_t*)p;
  ix->bufs.push_back({p, b});
  b = (uint64_t)std::max<uint32_t>(1u, H.nleaves) * 4;
  if ((rc = dev_alloc(ix, &p, b))) return rc;
  ix->dix.leaf_se = (const uint32_t*)p;
  ix->bufs.push_back({p, b});
  ix->dix.nleaves = H.nleaves;
  ix->log_g = H.log_g;
  ix->occ = H.occ;
  ix->slot_log2w = H.slot_log2w;
  b = (uint64_t)H.m * 4;
  if ((rc = dev_alloc(ix, &p, b))) return rc;
  ix->dix.res_lib = (const int32_t*)p;
  ix->bufs.push_back({p, b});
  b = (uint64_t)H.nlibs * sizeof(DevLib);
  if ((rc = dev_alloc(ix, &p, b))) return rc;
  ix->dix.libs = (const DevLib*)p;
  HIP_TRY(hipMemcpy(p, ix->hlibs.data(), b, hipMemcpyHostToDevice)); // pointers are per-device: never exported
  ix->dix.lib0 = ix->hlibs[0];
  ix->dix.res_mask = H.res_mask;

  ix->dix.k = H.k, ix->dix.h = H.h, ix->dix.m = H.m, ix->dix.nlibs = H.nlibs, ix->dix.tree_nnodes = H.tree_nnodes;
  ix->dix.m_shift = 0xFFFFFFFFu;
  if ((H.m & (H.m - 1)) == 0) {
    uint32_t s = 0;
    while ((1u << s) < H.m) ++s;
    ix->dix.m_shift = s;
  }
  std::vector<uint8_t> pasc(H.ppos, H.ppos + H.h), nasc(H.npos, H.npos + (H.k - H.h));
  ix->dix.pmask = make_pext(pasc);
  ix->dix.nmask = make_pext(nasc);
  std::sort(pasc.begin(), pasc.end());
  std::sort(nasc.begin(), nasc.end());
  auto pack_desc = [](const std::vector<uint8_t>& asc, uint64_t (&out)[2]) { // 5 bits each, 12 to a word, descending
    out[0] = out[1] = 0;
    for (size_t i = 0; i < asc.size(); ++i) out[i / 12] |= (uint64_t)asc[asc.size() - 1 - i] << (5 * (i % 12));
  };
  pack_desc(pasc, ix->dix.ppk);
  pack_desc(nasc, ix->dix.npk);
  { // byte tables of the table-driven front end (kr_dev_common.inc: front_end_tab): entry [b][v] = what byte b = v of the window
    // word contributes to {forward rix half, forward enc half, reverse rix half, reverse enc half}, spread and shifted into place
    std::vector<uint4> tab(4 * 256, make_uint4(0, 0, 0, 0));
    std::vector<int> p_of(32, -1), n_of(32, -1); // position -> index among the LSH / non-LSH positions (ascending)
    for (size_t t = 0; t < pasc.size(); ++t) p_of[pasc[t]] = (int)t;
    for (size_t t = 0; t < nasc.size(); ++t) n_of[nasc[t]] = (int)t;
    for (uint32_t b = 0; b < 4; ++b)
      for (uint32_t v = 0; v < 256; ++v) {
        uint4 e = make_uint4(0, 0, 0, 0);
        for (uint32_t q = 0; q < 8; ++q) {
          const uint32_t i = 8 * b + q; // bit of the window word = base at read position j + i
          if (i >= H.k || !((v >> q) & 1u)) continue;
          const uint32_t pf = H.k - 1 - i, pr = i; // forward: counted from the last base; reverse: order reversed
          if (p_of[pf] >= 0) e.x |= 1u << (2 * p_of[pf]);
          if (n_of[pf] >= 0) e.y |= 1u << n_of[pf];
          if (p_of[pr] >= 0) e.z |= 1u << (2 * p_of[pr]);
          if (n_of[pr] >= 0) e.w |= 1u << n_of[pr];
        }
        tab[b * 256 + v] = e;
      }
    void* pt = nullptr;
    if ((rc = dev_alloc(ix, &pt, tab.size() * sizeof(uint4)))) return rc;
    HIP_TRY(hipMemcpy(pt, tab.data(), tab.size() * sizeof(uint4), hipMemcpyHostToDevice));
    ix->dix.fe_tab = (const uint4*)pt;
  }
  ix->desc.resize(sizeof(DescHeader) + L.size() * sizeof(DescLib));
  memcpy(ix->desc.data(), &H, sizeof(H));
  memcpy(ix->desc.data() + sizeof(H), L.data(), L.size() * sizeof(DescLib));
  return KR_OK;
}

constexpr uint32_t kDescMagic = 0x4b524958u; // "KRIX"

// (The HIP runtime folds every stream after the third onto its last hardware queue -- GPU_MAX_HW_QUEUES, default 4 --
// where the copies of one kr_stream queue behind the kernels of another as blit kernels.  Raising it is the embedding
// application's choice, made before the runtime initialises: the `krepp` CLI and bench.py set it, INTEGRATION.md says
// why.  The library itself does not touch the process environment.)

} // namespace

extern "C" {

// Class of every colour id of a library, its se_to_pse table in the device form and the leaf lists (kr_dev_common.inc:
// 0 drop, 1 leaf rank, 2 walk, 3 flat).  One ascending pass: a colour's parts normally have smaller ids; a part that does
// not leaves the colour in class 2, which is always right.  A flat colour lists exactly the leaves that the walk through
// its parts (src/query.cpp:369-387) reaches: adjacent runs join into a run, anything else of at most kFlatMax leaves
// becomes a sorted list (a leaf reached through both parts is listed once: leaf updates are idempotent,
// src/query.hpp:153-176).  Tree nodes keep the classes they always had (null -> drop, leaf -> rank); every other colour
// keeps its id in the low bits.  KR_FLAT_MAX (default 64; 0: walk everything) bounds the lists, KR_RUN_MIN the runs.
constexpr uint32_t kFlatMax = 64;
constexpr bool kFilterByDefault = false; // filter slots where 256-byte slots would serve (KR_SLOT_FILTER=1 / 0 overrides)
static void colour_classes(std::vector<uint2>& pse, const std::vector<uint32_t>& node_info, uint32_t tree_nnodes, std::vector<uint32_t>& cls,
                           std::vector<uint32_t>& lists)
{
  const uint32_t n = (uint32_t)pse.size();
  uint32_t flat_max = kFlatMax, run_min = 2;
  if (const char* e = getenv("KR_FLAT_MAX")) flat_max = std::min<uint32_t>((uint32_t)atoi(e), 4096u);
  if (const char* e = getenv("KR_RUN_MIN")) run_min = (uint32_t)atoi(e);
  struct Info { uint32_t kind, lo, cnt; }; // kind 0: not known at upload, 1: run of cnt >= 0 ranks from lo, 2: lists[lo .. lo + cnt)
  std::vector<Info> inf(n, Info{0, 0, 0});
  cls.assign(n, 0u);
  lists.clear();
  std::vector<uint32_t> ta, tb2;
  auto ranks_of = [&](const Info& x, std::vector<uint32_t>& out) {
    out.clear();
    if (x.kind == 1)
      for (uint32_t t = 0; t < x.cnt; ++t) out.push_back(x.lo + t);
    else
      out.assign(lists.begin() + x.lo, lists.begin() + x.lo + x.cnt);
  };
  for (uint32_t se = 1; se < n; ++se) {
    const uint32_t kd = se <= tree_nnodes ? (node_info[se] & 3u) : 2u;
    if (kd == 0) { // null tree node
      inf[se] = Info{1, 0, 0};
      cls[se] = 0;
    } else if (kd == 1) {
      inf[se] = Info{1, node_info[se] >> 2, 1};
      cls[se] = (node_info[se] >> 2) | (1u << 30);
    } else {
      auto part = [&](uint32_t a) -> Info {
        if (a == 0 || a >= n) return Info{1, 0, 0}; // the empty set, or an id the crecord does not define: dropped
        return a < se ? inf[a] : Info{0, 0, 0};
      };
      const Info A = part(pse[se].x), B = part(pse[se].y);
      Info r{0, 0, 0};
      if (A.kind && B.kind) {
        if (A.cnt == 0) r = B;
        else if (B.cnt == 0) r = A;
        else if (A.kind == 1 && B.kind == 1 && (uint64_t)A.lo + A.cnt == B.lo) r = Info{1, A.lo, A.cnt + B.cnt};
        else if (A.kind == 1 && B.kind == 1 && (uint64_t)B.lo + B.cnt == A.lo) r = Info{1, B.lo, A.cnt + B.cnt};
        else if ((uint64_t)A.cnt + B.cnt <= flat_max && lists.size() + flat_max < (1ull << 31)) {
          ranks_of(A, ta), ranks_of(B, tb2);
          const uint32_t off = (uint32_t)lists.size();
          std::set_union(ta.begin(), ta.end(), tb2.begin(), tb2.end(), std::back_inserter(lists));
          r = Info{2, off, (uint32_t)lists.size() - off};
        }
      }
      if (r.kind == 1 && r.cnt >= 2 && r.cnt < run_min) r.kind = 0; // (experiments: short runs walked)
      if (r.kind && !flat_max) r.kind = 0;
      inf[se] = r;
      cls[se] = se | ((r.kind ? 3u : 2u) << 30);
    }
  }
  for (uint32_t se = 0; se < n; ++se) {
    if ((cls[se] >> 30) == 3u) {
      pse[se] = make_uint2(inf[se].lo | (inf[se].kind == 2 ? 0x80000000u : 0u), inf[se].cnt);
    } else {
      const uint32_t a = pse[se].x, b = pse[se].y;
      pse[se] = make_uint2(a < n ? cls[a] : 0u, b < n ? cls[b] : 0u);
    }
  }
}

int kr_debug_colour_classes(const uint32_t* pse_pairs, uint32_t nsubsets, const uint8_t* node_kind, uint32_t tree_nnodes,
                            uint32_t* cls_out, uint32_t* pse_out, uint32_t* lists_out, uint64_t* nlist)
{
  kr::clear_error();
  if (!pse_pairs || !node_kind || !cls_out || !pse_out || !nlist) return kr::fail(KR_ERR_ARG, "kr_debug_colour_classes: null argument");
  std::vector<uint32_t> node_info(tree_nnodes + 1, 0);
  uint32_t rank = 0;
  for (uint32_t se = 1; se <= tree_nnodes; ++se) { // as kr_index_upload numbers the leaves
    const uint32_t kd = node_kind[se] & 3u;
    node_info[se] = kd;
    if (kd == 1) node_info[se] |= rank++ << 2;
  }
  std::vector<uint2> pse(nsubsets);
  for (uint32_t i = 0; i < nsubsets; ++i) pse[i] = make_uint2(pse_pairs[2 * i], pse_pairs[2 * i + 1]);
  std::vector<uint32_t> cls, lists;
  colour_classes(pse, node_info, tree_nnodes, cls, lists);
  for (uint32_t i = 0; i < nsubsets; ++i) cls_out[i] = cls[i], pse_out[2 * i] = pse[i].x, pse_out[2 * i + 1] = pse[i].y;
  const uint64_t cap = *nlist;
  *nlist = lists.size();
  if (lists.size() > cap || (!lists_out && !lists.empty())) return kr::fail(KR_ERR_CAPACITY, "kr_debug_colour_classes: list buffer too small");
  if (!lists.empty()) memcpy(lists_out, lists.data(), lists.size() * 4);
  return KR_OK;
}

int kr_index_upload(const kr_index_view* v, int device, uint32_t flags, kr_index** out)
{
  kr::clear_error();
  if (!v || !out || !v->libs || !v->ppos || !v->npos || !v->node_kind) return kr::fail(KR_ERR_ARG, "kr_index_upload: null argument");
  *out = nullptr;
  if (v->k < 3 || v->k > 31 || v->h == 0 || v->h >= v->k || v->k - v->h > 16 || v->h > 15)
    return kr::fail(KR_ERR_ARG, "kr_index_upload: unsupported k/h (need k<=31, k-h<=16, h<=15)");
  if (v->nlibs == 0 || v->nlibs > (uint32_t)kMaxLibs) return kr::fail(KR_ERR_ARG, "kr_index_upload: 1..16 partial libraries supported");
  if (v->m == 0 || v->m > 65536) return kr::fail(KR_ERR_ARG, "kr_index_upload: m out of range");
  if (v->tree_nnodes >= (1u << 30)) return kr::fail(KR_ERR_ARG, "kr_index_upload: tree too large");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return kr::fail(KR_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return kr::fail(KR_ERR_ARG, "kr_index_upload: bad device ordinal");
  HIP_TRY(hipSetDevice(device));

  DescHeader H;
  memset(&H, 0, sizeof(H));
  H.magic = kDescMagic, H.k = v->k, H.h = v->h, H.m = v->m, H.nlibs = v->nlibs, H.tree_nnodes = v->tree_nnodes;
  memcpy(H.ppos, v->ppos, v->h);
  memcpy(H.npos, v->npos, v->k - v->h);
  std::vector<DescLib> L(v->nlibs);
  std::vector<int32_t> res_lib(v->m, -1);
  for (uint32_t i = 0; i < v->nlibs; ++i) {
    const kr_lib_view& lv = v->libs[i];
    if (lv.r >= v->m) return kr::fail(KR_ERR_FORMAT, "library residue r >= m");
    if (lv.nnodes != v->tree_nnodes + 1) return kr::fail(KR_ERR_FORMAT, "crecord nnodes does not match the tree");
    L[i] = DescLib{lv.nkmers, 0, lv.nrows, lv.nsubsets, lv.nnodes, lv.frac ? lv.r + 1 : 1u};
    // src/index.cpp:144-157
    if (lv.frac)
      for (uint32_t q = 0; q <= lv.r; ++q) res_lib[q] = (int32_t)i;
    else
      res_lib[lv.r] = (int32_t)i;
  }
  for (uint32_t q = 0; q < v->m && q < 64; ++q)
    if (res_lib[q] >= 0) H.res_mask |= 1ull << q;
  std::vector<uint32_t> node_info(v->tree_nnodes + 1, 0), leaf_se;
  for (uint32_t se = 1; se <= v->tree_nnodes; ++se) {
    uint32_t kd = v->node_kind[se] & 3u;
    node_info[se] = kd;
    if (kd == 1) {
      node_info[se] |= (uint32_t)leaf_se.size() << 2;
      leaf_se.push_back(se);
    }
  }
  H.nleaves = (uint32_t)leaf_se.size();
  // 2 key bits per leaf in the accumulate kernel's LDS bitmaps: 65,536 leaves = 45 KB of the 64 KB a workgroup may use
  if (2ull * H.nleaves > 131072) return kr::fail(KR_ERR_ARG, "kr_index_upload: more than 65536 reference leaves is not supported");
  { // lanes per probe: a bucket of L entries spans about (L + 4.5) / 4 aligned 16-byte chunks
    double nk = 0, nr = 0;
    for (uint32_t i = 0; i < v->nlibs; ++i) nk += (double)v->libs[i].nkmers, nr += (double)v->libs[i].nrows;
    double mean_len = nr > 0 ? nk / nr : 0; // empty buckets never reach the scan, so this underestimates slightly
    H.log_g = mean_len <= 3.0 ? 0u : (mean_len <= 44.0 ? 2u : 3u);
    if (const char* e = getenv("KR_LOG_G")) H.log_g = (uint32_t)atoi(e) > 3 ? 3u : (uint32_t)atoi(e);
    if (H.log_g == 1) H.log_g = 2;
    // dense tables get a slotted copy of the head of every bucket (see scan_group_slots): the smallest slot
    // of 32 / 64 / 128 words whose W-2 entries cover the mean bucket length + 3 sigma (Poisson)
    bool fits32 = true;
    for (uint32_t i = 0; i < v->nlibs; ++i) fits32 = fits32 && v->libs[i].nkmers < (1ull << 32);
    const double need = mean_len + 3.0 * std::sqrt(mean_len);
    if (mean_len >= 12.0 && fits32) H.slot_log2w = need <= 30.0 ? 5u : (need <= 62.0 ? 6u : (need <= 126.0 ? 7u : 0u));
    // where the 256-byte slot would serve (two lines per probe), FILTER slots do with one line for most probes
    // (kr_dev_common.inc; KR_SLOT_FILTER=1 / 0 overrides kFilterByDefault).  Costs nrows * 640 B for the slot-ordered colours.
    const bool want_filter = getenv("KR_SLOT_FILTER") ? atoi(getenv("KR_SLOT_FILTER")) != 0 : kFilterByDefault;
    if (H.slot_log2w == 6u && want_filter) H.slot_log2w = kSlotFilter;
    // sparse tables: a bit per row says whether its bucket holds anything (more than a third of the rows empty)
    H.occ = (mean_len < 1.0 && !H.slot_log2w) ? 1u : 0u;
    if (const char* e = getenv("KR_OCC_BITMAP")) H.occ = atoi(e) ? 1u : 0u; // tests / experiments
    if (const char* e = getenv("KR_SLOT_LOG2W")) { // tests / experiments: 0 (packed only), 5, 6, 7, 8 (48 words = 192 bytes), 9 (filter slots)
      const uint32_t w = (uint32_t)atoi(e);
      H.slot_log2w = (fits32 && w >= 5 && w <= 9) ? w : 0u;
    }
  }
  // colour classes, the se_to_pse table in its device form and the leaf lists, on the host: one pass over the colours
  std::vector<std::vector<uint2>> hpse(v->nlibs);
  std::vector<std::vector<uint32_t>> cls(v->nlibs), lists(v->nlibs);
  for (uint32_t i = 0; i < v->nlibs; ++i) {
    const kr_lib_view& lv = v->libs[i];
    if (lv.nsubsets > kColMask) return kr::fail(KR_ERR_ARG, "kr_index_upload: more than 2^30 colours is not supported");
    hpse[i].resize(lv.nsubsets);
    if (lv.nsubsets) {
      if (flags & KR_VIEW_DEVICE)
        HIP_TRY(hipMemcpy(hpse[i].data(), lv.pse, (uint64_t)lv.nsubsets * 8, hipMemcpyDeviceToHost));
      else
        memcpy(hpse[i].data(), lv.pse, (uint64_t)lv.nsubsets * 8);
    }
    colour_classes(hpse[i], node_info, v->tree_nnodes, cls[i], lists[i]);
    L[i].nlist = lists[i].size();
  }
  std::unique_ptr<kr_index> ix(new kr_index());
  ix->device = device;
  ix->chain_off = getenv("KR_NO_KERNEL_CHAIN") != nullptr;
  int rc = alloc_from_desc(ix.get(), H, L);
  if (rc) {
    kr_index_free(ix.release());
    return rc;
  }
  const hipMemcpyKind kind = (flags & KR_VIEW_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpy((void*)ix->dix.node_info, node_info.data(), node_info.size() * 4, hipMemcpyHostToDevice));
  if (!leaf_se.empty()) HIP_TRY(hipMemcpy((void*)ix->dix.leaf_se, leaf_se.data(), leaf_se.size() * 4, hipMemcpyHostToDevice));
  DevBuf<uint32_t> b_bad; // (this and the staging arrays below: freed at every return)
  if (!b_bad.reserve(1)) return alloc_failed("kr_index_upload");
  uint32_t* d_bad = b_bad.get();
  HIP_TRY(hipMemset(d_bad, 0, 4));
  for (uint32_t i = 0; i < v->nlibs; ++i) {
    const kr_lib_view& lv = v->libs[i];
    const DevLib& d = ix->hlibs[i];
    // stage the on-disk arrays, then re-lay them out on the device
    const uint32_t* src_cmer = lv.cmer;
    const uint64_t* src_inc = lv.inc;
    DevBuf<uint64_t> t_cmer, t_inc;
    if (!(flags & KR_VIEW_DEVICE)) {
      if (!t_cmer.reserve(lv.nkmers + 2)) return alloc_failed("kr_index_upload: staging");
      HIP_TRY(hipMemcpy(t_cmer.get(), lv.cmer, lv.nkmers * 8, hipMemcpyHostToDevice));
      if (!t_inc.reserve((uint64_t)lv.nrows + 2)) return alloc_failed("kr_index_upload: staging");
      HIP_TRY(hipMemcpy(t_inc.get(), lv.inc, (uint64_t)lv.nrows * 8, hipMemcpyHostToDevice));
      src_cmer = (const uint32_t*)t_cmer.get();
      src_inc = t_inc.get();
    }
    HIP_TRY(hipMemset((void*)d.enc, 0xFF, (d.nkmers + 16) * 4));
    HIP_TRY(hipMemset((void*)d.se, 0, (d.nkmers + 16) * 4));
    if (lv.nsubsets > kColMask) return kr::fail(KR_ERR_ARG, "kr_index_upload: more than 2^30 colours is not supported");
    DevBuf<uint32_t> b_cls;
    if (!b_cls.reserve((uint64_t)lv.nsubsets + 4)) return alloc_failed("kr_index_upload: staging");
    uint32_t* d_cls = b_cls.get();
    if (lv.nsubsets) HIP_TRY(hipMemcpy(d_cls, cls[i].data(), (uint64_t)lv.nsubsets * 4, hipMemcpyHostToDevice));
    if (!lists[i].empty()) HIP_TRY(hipMemcpy((void*)d.leaflist, lists[i].data(), lists[i].size() * 4, hipMemcpyHostToDevice));
    if (lv.nkmers)
      hipLaunchKernelGGL(kr_relayout_cmer, dim3(2048), dim3(256), 0, 0, src_cmer, lv.nkmers, (uint32_t*)d.enc, (uint32_t*)d.se, d_cls, lv.nsubsets);
    if (lv.nrows) hipLaunchKernelGGL(kr_relayout_inc, dim3(1024), dim3(256), 0, 0, src_inc, lv.nrows, (uint64_t*)d.bkt, d_bad);
    if (lv.nrows && H.occ) hipLaunchKernelGGL(kr_build_occ, dim3(1024), dim3(256), 0, 0, d.bkt, lv.nrows, (uint32_t*)d.occ);
    if (lv.nrows && H.slot_log2w == kSlotFilter) {
      hipLaunchKernelGGL(kr_build_fslots, dim3(8192), dim3(256), 0, 0, d.bkt, d.enc, lv.nrows, (uint4*)d.slots);
      hipLaunchKernelGGL(kr_build_sx, dim3(8192), dim3(256), 0, 0, d.bkt, d.enc, d.se, lv.nrows, (uint2*)d.sx);
    } else if (lv.nrows && H.slot_log2w)
      hipLaunchKernelGGL(kr_build_slots, dim3(8192), dim3(256), 0, 0, d.bkt, d.enc, lv.nrows, slot_words(H.slot_log2w), (uint32_t*)d.slots);
    HIP_TRY(hipDeviceSynchronize());
    t_cmer.reset(), t_inc.reset(), b_cls.reset(); // (before the copies below, as ever: hipFree synchronises)
    if (lv.nsubsets) HIP_TRY(hipMemcpy((void*)d.pse, hpse[i].data(), (uint64_t)lv.nsubsets * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((void*)d.rho, lv.rho, (uint64_t)lv.nnodes * 8, kind));
  }
  uint32_t bad = 0;
  HIP_TRY(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
  if (bad) {
    kr_index_free(ix.release());
    return kr::fail(KR_ERR_FORMAT, "inc-* is not monotone or a bucket exceeds 2^24 entries / 2^40 offset");
  }
  HIP_TRY(hipMemcpy((void*)ix->dix.res_lib, res_lib.data(), (uint64_t)v->m * 4, hipMemcpyHostToDevice));
  *out = ix.release();
  return KR_OK;
}

void kr_index_free(kr_index* ix)
{
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  for (void* p : ix->allocs) (void)hipFree(p);
  for (auto& e : ix->chain_ev)
    if (e) (void)hipEventDestroy(e);
  delete ix; // (the likelihood workspace and the node names free themselves: the device is set)
}

uint64_t kr_index_device_bytes(const kr_index* ix) { return ix ? ix->bytes : 0; }
uint32_t kr_index_slot_words(const kr_index* ix) { return ix && ix->slot_log2w ? slot_words(ix->slot_log2w) : 0; }
uint32_t kr_index_slot_format(const kr_index* ix) { return ix ? ix->slot_log2w : 0; }
uint32_t kr_index_log_g(const kr_index* ix) { return ix ? ix->log_g : 0; }
uint32_t kr_index_occ_bitmap(const kr_index* ix) { return ix ? ix->occ : 0; }

int kr_index_export(const kr_index* ix, void* desc, uint64_t* desc_bytes, kr_index_buffer* bufs, uint32_t* nbufs)
{
  if (!ix || !desc_bytes || !nbufs) return kr::fail(KR_ERR_ARG, "kr_index_export: null argument");
  uint64_t need = ix->desc.size();
  uint32_t nb = (uint32_t)ix->bufs.size();
  bool fits = desc && *desc_bytes >= need && bufs && *nbufs >= nb;
  *desc_bytes = need;
  *nbufs = nb;
  if (!fits) return (desc || bufs) ? kr::fail(KR_ERR_ARG, "kr_index_export: buffers too small") : KR_OK;
  memcpy(desc, ix->desc.data(), need);
  memcpy(bufs, ix->bufs.data(), nb * sizeof(kr_index_buffer));
  return KR_OK;
}

int kr_index_import(const void* desc, uint64_t desc_bytes, int device, kr_index** out, kr_index_buffer* bufs, uint32_t* nbufs)
{
  kr::clear_error();
  if (!desc || !out || !nbufs || desc_bytes < sizeof(DescHeader)) return kr::fail(KR_ERR_ARG, "kr_index_import: bad argument");
  DescHeader H;
  memcpy(&H, desc, sizeof(H));
  if (H.magic != kDescMagic || desc_bytes != sizeof(H) + (uint64_t)H.nlibs * sizeof(DescLib) || H.nlibs == 0 || H.nlibs > (uint32_t)kMaxLibs)
    return kr::fail(KR_ERR_FORMAT, "kr_index_import: bad descriptor");
  std::vector<DescLib> L(H.nlibs);
  memcpy(L.data(), (const uint8_t*)desc + sizeof(H), H.nlibs * sizeof(DescLib));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return kr::fail(KR_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return kr::fail(KR_ERR_ARG, "kr_index_import: bad device ordinal");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<kr_index> ix(new kr_index());
  ix->device = device;
  ix->chain_off = getenv("KR_NO_KERNEL_CHAIN") != nullptr;
  int rc = alloc_from_desc(ix.get(), H, L);
  if (rc) {
    kr_index_free(ix.release());
    return rc;
  }
  uint32_t nb = (uint32_t)ix->bufs.size();
  if (!bufs || *nbufs < nb) {
    *nbufs = nb;
    kr_index_free(ix.release());
    return kr::fail(KR_ERR_ARG, "kr_index_import: bufs too small");
  }
  memcpy(bufs, ix->bufs.data(), nb * sizeof(kr_index_buffer));
  *nbufs = nb;
  *out = ix.release();
  return KR_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------
// kr_index_broadcast: replicas over RCCL (xGMI), load time only
// ---------------------------------------------------------------------------
namespace {

// RCCL is loaded on first use: a process that never replicates an index (every single-GPU run, every rank of a
// one-process-per-GPU job that replicates through its own transport) neither maps nor initialises it.
struct Rccl {
  void* h = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclBroadcast) Broadcast = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string err;
  bool load()
  {
    if (h) return true;
    const char* names[] = {getenv("KR_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names)
      if (n && *n && (h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) {
      err = std::string("cannot load RCCL: ") + (dlerror() ? dlerror() : "librccl.so.1 not found");
      return false;
    }
#define KR_SYM(field, name)                                                            \
  if (!(field = reinterpret_cast<decltype(field)>(dlsym(h, name)))) {                  \
    err = std::string("RCCL lacks ") + name;                                           \
    dlclose(h), h = nullptr;                                                           \
    return false;                                                                      \
  }
    KR_SYM(CommInitAll, "ncclCommInitAll")
    KR_SYM(CommDestroy, "ncclCommDestroy")
    KR_SYM(Broadcast, "ncclBroadcast")
    KR_SYM(GroupStart, "ncclGroupStart")
    KR_SYM(GroupEnd, "ncclGroupEnd")
    KR_SYM(GetErrorString, "ncclGetErrorString")
#undef KR_SYM
    return true;
  }
};
Rccl g_rccl;
std::mutex g_rccl_mu;

} // namespace

extern "C" int kr_index_broadcast(const kr_index* root, int ndev, const int* devices, kr_index** replicas)
{
  kr::clear_error();
  if (!root || ndev < 0 || (ndev && (!devices || !replicas))) return kr::fail(KR_ERR_ARG, "kr_index_broadcast: bad argument");
  if (ndev == 0) return KR_OK;
  int have = 0;
  if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) return kr::fail(KR_ERR_NO_DEVICE, "no HIP device available");
  for (int i = 0; i < ndev; ++i) {
    replicas[i] = nullptr;
    if (devices[i] < 0 || devices[i] >= have) return kr::fail(KR_ERR_ARG, "kr_index_broadcast: bad device ordinal");
    for (int j = 0; j < i; ++j)
      if (devices[j] == devices[i]) return kr::fail(KR_ERR_ARG, "kr_index_broadcast: a device is listed twice");
  }
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (!g_rccl.load()) return kr::fail(KR_ERR_NO_DEVICE, g_rccl.err);
  Rccl& R = g_rccl;
  auto cleanup = [&](int rc) {
    for (int i = 0; i < ndev; ++i)
      if (replicas[i]) kr_index_free(replicas[i]), replicas[i] = nullptr;
    return rc;
  };
  // same buffers, same order, on every target device (kr_index_import's allocation)
  std::vector<std::vector<kr_index_buffer>> rb(ndev);
  for (int i = 0; i < ndev; ++i) {
    uint32_t nb = 0;
    rb[i].resize(root->bufs.size());
    nb = (uint32_t)rb[i].size();
    int rc = kr_index_import(root->desc.data(), root->desc.size(), devices[i], &replicas[i], rb[i].data(), &nb);
    if (rc) return cleanup(rc);
    if (nb != root->bufs.size()) return cleanup(kr::fail(KR_ERR_FORMAT, "kr_index_broadcast: replica layout differs from the root's"));
  }
  // one communicator over {root device} + the target devices that are not the root's; a target ON the root's device
  // (a second replica in the same HBM: tests, A/B runs) is served by a one-rank communicator, whose out-of-place
  // broadcast is a device copy
  std::vector<int> devlist{root->device};
  std::vector<int> rank_of(ndev, -1);
  for (int i = 0; i < ndev; ++i)
    if (devices[i] != root->device) rank_of[i] = (int)devlist.size(), devlist.push_back(devices[i]);
  const int nranks = (int)devlist.size();
  std::vector<ncclComm_t> comm(nranks, nullptr);
  std::vector<hipStream_t> strm(nranks, nullptr);
  auto nccl_fail = [&](ncclResult_t r, const char* what) {
    return kr::fail(KR_ERR_NO_DEVICE, std::string(what) + ": " + R.GetErrorString(r));
  };
  int rc = KR_OK;
  // RCCL may print a version banner on STDOUT when its first communicator is made.  The library leaves the process's file
  // descriptors alone (another thread may be writing report rows): an application whose stdout carries the report redirects
  // it around this call itself, before its writers start (krepp_main.cpp does; INTEGRATION.md), or runs with NCCL_DEBUG unset.
  ncclResult_t nr = R.CommInitAll(comm.data(), nranks, devlist.data());
  if (nr != ncclSuccess) return cleanup(nccl_fail(nr, "ncclCommInitAll"));
  for (int r = 0; r < nranks && rc == KR_OK; ++r) {
    if (hipSetDevice(devlist[r]) != hipSuccess || hipStreamCreateWithFlags(&strm[r], hipStreamNonBlocking) != hipSuccess)
      rc = kr::fail(KR_ERR_NO_DEVICE, "kr_index_broadcast: cannot create a stream");
  }
  // few, large buffers: one ring broadcast each (per-link bound over xGMI), all ranks of one buffer in one group
  for (size_t b = 0; b < root->bufs.size() && rc == KR_OK; ++b) {
    const uint64_t bytes = root->bufs[b].bytes;
    if (!bytes) continue;
    if ((nr = R.GroupStart()) != ncclSuccess) { rc = nccl_fail(nr, "ncclGroupStart"); break; }
    // rank 0 = the root: in place unless a same-device replica wants the bytes too
    void* root_recv = root->bufs[b].dptr;
    for (int i = 0; i < ndev; ++i)
      if (rank_of[i] < 0) root_recv = rb[i][b].dptr; // (at most one: devices are distinct)
    nr = R.Broadcast(root->bufs[b].dptr, root_recv, bytes, ncclUint8, 0, comm[0], strm[0]);
    for (int i = 0; i < ndev && nr == ncclSuccess; ++i)
      if (rank_of[i] > 0) nr = R.Broadcast(rb[i][b].dptr, rb[i][b].dptr, bytes, ncclUint8, 0, comm[rank_of[i]], strm[rank_of[i]]);
    ncclResult_t ge = R.GroupEnd();
    if (nr != ncclSuccess || ge != ncclSuccess) rc = nccl_fail(nr != ncclSuccess ? nr : ge, "ncclBroadcast");
  }
  for (int r = 0; r < nranks; ++r) {
    if (!strm[r]) continue;
    (void)hipSetDevice(devlist[r]);
    if (hipStreamSynchronize(strm[r]) != hipSuccess && rc == KR_OK) rc = kr::fail(KR_ERR_NO_DEVICE, "kr_index_broadcast: stream failed");
    (void)hipStreamDestroy(strm[r]);
  }
  for (auto c : comm)
    if (c) (void)R.CommDestroy(c);
  (void)hipSetDevice(root->device);
  return rc == KR_OK ? KR_OK : cleanup(rc);
}
