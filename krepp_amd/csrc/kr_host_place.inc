// kr_host_place.inc -- part of kr_device.hip (host side): kr::place_on_device, the launch of the place kernels for kr_place_stream
// and, for a batch the record finders queued, kr_place_stream_parsed (the _parsed entry points; kernels: kr_dev_place_parsed.inc).

namespace {
// Growth of the place workspace.  place_renew: a new block whatever the buffer holds; place_grow: when n exceeds its size;
// place_grow_all: a group with one capacity -- all of them at least n afterwards, or (a failed allocation) all of them empty, so that
// the next batch allocates again.  A new device block is poisoned under KR_DEBUG_POISON=all (as the stream's own buffers: salloc).
template <class T>
int place_fresh(DevBuf<T>& b) { return poison_fresh(b.get(), b.bytes()); }
template <class T>
int place_fresh(PinBuf<T>&) { return KR_OK; }
template <class B>
int place_renew(B& b, uint64_t n) { return b.renew(n) ? place_fresh(b) : alloc_failed("place workspace"); }
template <class B>
int place_grow(B& b, uint64_t n) { return n <= b.size() ? KR_OK : place_renew(b, n); }
template <class... B>
int place_grow_all(uint64_t n, B&... b)
{
  const bool fresh = ((n > b.size()) || ...);
  if (!reserve_all(n, b...)) return alloc_failed("place workspace");
  int rc = KR_OK;
  if (fresh) ((rc = rc ? rc : place_fresh(b)), ...);
  return rc;
}
// What the kernels are told the buffers hold: all of it, or what KR_DEBUG_PLACE_CAPS says (never more than there is)
uint64_t place_cand_slots(const kr_stream::PlaceWs& w) { return w.dbg_cand ? std::min<uint64_t>(w.dbg_cand, w.d_cse.size()) : w.d_cse.size(); }
uint64_t place_keep_slots(const kr_stream::PlaceWs& w) { return w.dbg_keep ? std::min<uint64_t>(w.dbg_keep, w.d_kse.size()) : w.d_kse.size(); }
uint64_t place_text_bytes(const kr_stream::PlaceWs& w)
{
  const uint64_t cap = w.d_text.size();
  if (!w.dbg_text) return cap;
  return std::min(cap, w.dbg_sticky ? w.dbg_text : std::max(w.dbg_text, w.text_want_min));
}
// candidate slots of a stream's place workspace: a read may need one per leaf and per distinct ancestor while it is worked on, and
// keeps what it emits; a range that runs out (large trees) is run again with as many as it asked for
int place_size_candidates(kr_stream* s, uint64_t want)
{
  kr_stream::PlaceWs& w = s->pw;
  int rc2 = 0;
  if ((rc2 = place_grow_all(want, w.d_cse, w.d_cread, w.d_cd, w.d_cv, w.d_cchi))) return rc2;
  const uint64_t cand_cap = w.d_cse.size();
  // every candidate, twice: a read that does not fit the rest of its wave's chunk takes a new one and leaves the rest unused (up to
  // total - 1 slots per read), + a partly used chunk per wave of the compaction; a range that still runs out is run again
  const uint64_t keep_want = w.dbg_keep ? w.dbg_keep : std::max<uint64_t>(w.keep_want_min, 2ull * cand_cap + 2048ull * 4ull * kPlKeepChunk);
  if ((rc2 = place_grow_all(keep_want, w.d_kse, w.d_kd, w.d_kv, w.d_kchi))) return rc2;
  // the sorted copy the text kernels work on (kr_dev_place.inc)
  if (w.text_on && (rc2 = place_grow_all(w.d_kse.size(), w.d_sse, w.d_sd, w.d_sv, w.d_sc))) return rc2;
  const uint64_t np_ = s->dp.np;
  if ((rc2 = place_grow(w.d_cprob, cand_cap * (np_ + 2))) || (rc2 = place_grow(w.d_rprob, w.d_len.size() * (np_ + 3)))) return rc2;
  return KR_OK;
}
} // namespace

// `place` back end for the batch last submitted on the stream (see kr_common.h).  Round 5: the batch can be worked through in read
// RANGES -- place_device_begin once, then per range place_device_launch (asynchronous) and place_device_finish (waits, copies the
// range's results back) -- so that the host's last phase of one range runs beside the kernels of the next (kr_place_stream).  The
// kernels do not know: they see the range's reads as reads 0 .. n through pointers moved by r0.
int kr::place_on_device(kr_stream* s, const void* tree_tag, const kr::PlaceTreeArrays& T, const uint32_t* read_len, uint32_t tau,
                        bool no_filter, double chisq, kr::PlaceDeviceResult* out)
{
  int rc = kr::place_device_begin(s, tree_tag, T, read_len);
  if (rc) return rc;
  if ((rc = kr::place_device_launch(s, T, 0, s->batch.nreads, tau, no_filter, chisq))) return rc;
  return kr::place_device_finish(s, T, 0, s->batch.nreads, tau, no_filter, chisq, 0, out);
}

namespace {
// What place_device_begin and place_device_begin_parsed share: the wait for the front end, the tree, the workspaces -- everything but
// the reads' lengths in d_len, which the caller queues behind it on lane 0's stream.
int place_begin_common(kr_stream* s, const void* tree_tag, const kr::PlaceTreeArrays& T)
{
  if (!s || !T.parent || !T.eff || !T.elig || !T.lo || !T.idx_to_pt || !T.depth) return kr::fail(KR_ERR_ARG, "place_on_device: null argument");
  if (!s->batch.submitted || !(s->batch.flags & KR_TAP_ACCS))
    return kr::fail(KR_ERR_STATE, "place: the batch must be submitted with KR_TAP_ACCS (the back end reads every record's histogram)");
  static const bool timing0 = getenv("KR_PLACE_TIMING") != nullptr;
  const auto t_w0 = std::chrono::steady_clock::now();
  int rc = kr_batch_wait(s);
  if (rc) return rc;
  if (timing0) fprintf(stderr, "[place/device]    front end: kr_batch_wait %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_w0).count());
  HIP_TRY(hipSetDevice(s->device));
  kr_stream::PlaceWs& w = s->pw;
  w.text_on = false; // (place_device_text_begin turns it on for this batch)
  hipStream_t st = s->lanes[0].stream;
  if (w.tree_tag != tree_tag || w.pn != T.pn || w.nidx != T.nidx) { // the tree as device arrays (once per tree)
    w.tree_tag = nullptr;
    const uint64_t n1 = (uint64_t)T.pn + 1, n2 = (uint64_t)T.nidx + 1;
    if ((rc = place_renew(w.d_parent, n1)) || (rc = place_renew(w.d_eff, n1)) || (rc = place_renew(w.d_lo, n1)) || (rc = place_renew(w.d_elig, n1)) ||
        (rc = place_renew(w.d_idx_to_pt, n2)) || (rc = place_renew(w.d_depth, n1)))
      return rc;
    HIP_TRY(hipMemcpy(w.d_parent.get(), T.parent, n1 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.d_eff.get(), T.eff, n1 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.d_lo.get(), T.lo, n1 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.d_elig.get(), T.elig, n1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.d_idx_to_pt.get(), T.idx_to_pt, n2 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.d_depth.get(), T.depth, n1 * 4, hipMemcpyHostToDevice));
    if ((rc = place_renew(w.d_node, n1))) return rc;
    {
      std::vector<uint4> nodes(n1);
      for (uint64_t i = 0; i < n1; ++i) nodes[i] = make_uint4(T.parent[i], T.lo[i], T.eff[i], T.depth[i]);
      HIP_TRY(hipMemcpy(w.d_node.get(), nodes.data(), n1 * sizeof(uint4), hipMemcpyHostToDevice));
    }
    w.tree_tag = tree_tag, w.pn = T.pn, w.nidx = T.nidx;
  }
  const uint32_t n = s->batch.nreads;
  if (n > w.d_len.size() && (rc = place_grow_all((uint64_t)n + n / 4, w.d_len, w.d_c0, w.d_info, w.h_len, w.h_c0, w.h_info))) return rc;
  if ((rc = place_grow_all(kPlCntCount * kPlCnt, w.d_cnt, w.h_cnt))) return rc;
  // candidate slots: a read may need one per leaf and per distinct ancestor while it is worked on, and keeps what it
  // emits; a batch that runs out (large trees) is run again with as many as it asked for
  // KR_DEBUG_PLACE_CAPS="c=SLOTS,k=SLOTS,t=BYTES,l=ENTRIES,sticky" (tests; read per batch, every field optional): the first attempt's
  // candidate slots, kept-candidate slots and text bytes in place of the floors here, in place_size_candidates and in
  // place_device_text_begin -- a new stream's buffers are made that small, a larger buffer is used up to there --, so that a small
  // batch runs out of each; l: what the internal candidates' list may take of the kept slots (a batch of a few hundred reads lists
  // fewer entries than its compaction takes slots: no kept cap cuts the one and not the other); "sticky": a range that is run
  // again gets no more than the first time (it ends at the host back end)
  w.dbg_cand = w.dbg_keep = w.dbg_text = w.dbg_list = 0, w.dbg_sticky = false;
  if (const char* e = getenv("KR_DEBUG_PLACE_CAPS")) {
    for (const char* q = e; *q;) {
      if (q[0] && q[1] == '=' && (q[0] == 'c' || q[0] == 'k' || q[0] == 't' || q[0] == 'l')) {
        const uint64_t v = std::max<uint64_t>(1, strtoull(q + 2, nullptr, 10));
        (q[0] == 'c' ? w.dbg_cand : q[0] == 'k' ? w.dbg_keep : q[0] == 't' ? w.dbg_text : w.dbg_list) = v;
      } else if (!strncmp(q, "sticky", 6)) {
        w.dbg_sticky = true;
      }
      while (*q && *q != ',') ++q;
      if (*q) ++q;
    }
    w.dbg_cand = std::min<uint64_t>(w.dbg_cand, 0x3FFFFFFFull);
  }
  if ((rc = place_size_candidates(s, w.dbg_cand ? w.dbg_cand : std::max<uint64_t>(1u << 20, (uint64_t)n * 24)))) return rc;
  // (the device's properties once per stream: the query is a millisecond-class call)
  if (!w.cu_count) {
    hipDeviceProp_t prop0;
    HIP_TRY(hipGetDeviceProperties(&prop0, s->device));
    w.cu_count = (uint32_t)prop0.multiProcessorCount;
  }
  struct { uint32_t multiProcessorCount; } prop{w.cu_count};
  static const bool timing = getenv("KR_PLACE_TIMING") != nullptr;
  auto wall = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_mark = wall();
  auto lap = [&](const char* what) {
    if (!timing) return;
    const double now = wall();
    fprintf(stderr, "[place/device]    %s %.2f ms\n", what, (now - t_mark) * 1e3);
    t_mark = now;
  };
  const uint32_t grid = std::min<uint32_t>(n, (uint32_t)prop.multiProcessorCount * 16u);
  { // heavy reads (more leaves / ancestors than kr_place_kernel's LDS arrays hold): list + per-wave global scratch of the second launch
    const uint64_t list = 2ull * n + 8ull * grid; // (the reads the first launch sets aside, in chunks of 8 per wave; behind them the reads it starts with)
    if (list > w.d_heavy.size() && (rc = place_grow(w.d_heavy, list + list / 4))) return rc;
    const uint32_t cwaves = std::max(grid, 1024u);
    if (!w.d_chain.get() || cwaves > w.chain_waves) { // the weights of every (leaf, ancestor) pair of a read: kPlChain doubles per wave of either launch
      // (+ a larger piece for each wave that may do an over-limit read itself: PlaceOut::chain_inline)
      if ((rc = place_renew(w.d_chain, (uint64_t)cwaves * kPlChain + 1024ull * kPlInlineChain * kPlChain))) return rc;
      w.chain_cap = kPlChain, w.chain_waves = cwaves;
    }
    const uint32_t hl = std::max<uint32_t>(kPlLeaves, s->ix->dix.nleaves), hn = std::max<uint32_t>(kPlNodes, T.pn);
    if (hl > w.heavy_leaves || hn > w.heavy_nodes || !w.d_heavy_u32.get() || !w.d_heavy_f64.get()) {
      const uint64_t per_wave = 32ull * hl + 4ull * hn; // bytes
      const uint32_t waves = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(1024, (1ull << 30) / per_wave)); // (<= 1024: the chain scratch above)
      if ((rc = place_renew(w.d_heavy_u32, (uint64_t)waves * (4ull * hl + hn))) || (rc = place_renew(w.d_heavy_f64, (uint64_t)waves * 2ull * hl))) return rc;
      w.heavy_leaves = hl, w.heavy_nodes = hn, w.heavy_waves = waves;
    }
  }
  lap("workspaces");
  return KR_OK;
}

// The batch a record finder queued last on the stream, as kr_place_stream_parsed needs it (krepp_amd.h: the state errors)
int place_parsed_state(const kr_stream* s)
{
  if (!s->fq.on || !s->parse.parsed) return kr::fail(KR_ERR_STATE, "kr_place_stream_parsed: the last submit on the stream was not kr_batch_submit_fastq / kr_batch_submit_fasta");
  if (!s->parse.nreads || !s->batch.submitted || !s->batch.from.parsed) return kr::fail(KR_ERR_STATE, "kr_place_stream_parsed: the last submit accepted no record (nothing was queued)");
  if (!(s->batch.flags & KR_TAP_ACCS)) return kr::fail(KR_ERR_STATE, "kr_place_stream_parsed: the batch must be submitted with KR_TAP_ACCS (the back end reads every record's histogram)");
  return KR_OK;
}

PlaceParsedIO place_parsed_io(kr_stream* s)
{
  kr_stream::PlaceWs& w = s->pw;
  return PlaceParsedIO{s->d_offsets, s->fq.d_raw, s->fq.d_npos, s->fq.d_nlen, s->batch.nreads, w.d_len.get(), w.d_idbsum.get(), w.d_id_off.get(), w.d_ids.get()};
}
} // namespace

int kr::place_device_begin(kr_stream* s, const void* tree_tag, const kr::PlaceTreeArrays& T, const uint32_t* read_len)
{
  if (!read_len) return kr::fail(KR_ERR_ARG, "place_on_device: null argument");
  if (s) s->pw.ids_queued = false, s->pw.ids_reads = 0; // (the ids of this batch, if any, are the host's staging)
  const int rc = place_begin_common(s, tree_tag, T);
  if (rc) return rc;
  kr_stream::PlaceWs& w = s->pw;
  const uint32_t n = s->batch.nreads;
  memcpy(w.h_len.get(), read_len, (uint64_t)n * 4);
  HIP_TRY(hipMemcpyAsync(w.d_len.get(), w.h_len.get(), (uint64_t)n * 4, hipMemcpyHostToDevice, s->lanes[0].stream));
  return KR_OK;
}

// The same for the batch that kr_batch_submit_fastq / kr_batch_submit_fasta queued last on the stream: the reads' lengths come from
// the record finder's offsets, on the device (kr_pp_len_kernel).  want_ids: the offsets of the reads' ids too (the three prefix-sum
// steps over the names' lengths), queued BEFORE the front end is waited for, so that their total is on the host when that wait
// returns -- place_device_text_begin_parsed sizes d_ids and d_text from it.
// Whose buffers: d_raw, d_npos and d_nlen (kr_stream::Fastq) are written by fq_begin's copy and the record finder's kernels only, and
// d_offsets by the record finder and by a host batch's copy in submit_batch only; build_tiles_device reads bases and offsets and
// writes the Tiles' own arrays, a batch that kr_batch_wait runs again is submitted from d_bases / d_offsets as they lie, and the
// place kernels touch none of the four: they hold the parsed batch until the stream's next submit.
int kr::place_device_begin_parsed(kr_stream* s, const void* tree_tag, const kr::PlaceTreeArrays& T, bool want_ids)
{
  if (!s) return kr::fail(KR_ERR_ARG, "place_on_device: null argument");
  int rc = place_parsed_state(s);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  kr_stream::PlaceWs& w = s->pw;
  hipStream_t st = s->lanes[0].stream;
  const uint32_t n = s->batch.nreads, nblk = n / kPpBlock + 1u;
  w.ids_queued = false, w.ids_reads = 0;
  if (want_ids) {
    if ((uint64_t)n + 1 > w.d_id_off.size() && (rc = place_grow_all((uint64_t)n + n / 4 + 16, w.d_id_off, w.h_id_off))) return rc;
    if ((rc = place_grow(w.d_idbsum, (uint64_t)nblk + nblk / 4 + 2)) || (rc = place_grow(w.h_idtot, 2))) return rc;
    const PlaceParsedIO io = place_parsed_io(s);
    hipLaunchKernelGGL(kr_pp_idsum_kernel, dim3(std::min<uint32_t>(nblk, 4096u)), dim3(256), 0, st, io);
    hipLaunchKernelGGL(kr_pp_idscan_kernel, dim3(1), dim3(1024), 0, st, io);
    hipLaunchKernelGGL(kr_pp_idoff_kernel, dim3(std::min<uint32_t>(nblk, 4096u)), dim3(256), 0, st, io);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w.h_idtot.get(), w.d_idbsum.get() + nblk, 8, hipMemcpyDeviceToHost, st));
    w.ids_queued = true;
  }
  if ((rc = place_begin_common(s, tree_tag, T))) return rc;
  hipLaunchKernelGGL(kr_pp_len_kernel, dim3(std::min<uint32_t>((n + 255u) / 256u, 4096u)), dim3(256), 0, st, place_parsed_io(s));
  HIP_TRY(hipGetLastError());
  return KR_OK;
}

// Queue the place kernels for reads [r0, r0 + n) of the batch and the copy of their counters (nothing waits here).
int kr::place_device_launch(kr_stream* s, const kr::PlaceTreeArrays& T, uint32_t r0, uint32_t n, uint32_t tau, bool no_filter, double chisq)
{
  kr_stream::PlaceWs& w = s->pw;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->lanes[0].stream;
  const uint32_t cus = w.cu_count;
  const uint32_t grid = std::min<uint32_t>(n, cus * 16u);
  BatchOut ro = result_out(s, s->out); // the range's reads as reads 0 .. n: the per-read arrays moved by r0 (records are named by rd_off)
  ro.rd_off += r0, ro.rd_cnt += r0, ro.rd_onmers += r0;
  const uint32_t* d_len = w.d_len.get() + r0;
  // the second launch's arrays in LDS where the tree allows it (KR_PLACE_HEAVY_GLOBAL=1: always global scratch, as for large trees)
  const uint32_t heavy_lds_bytes = 32u * w.heavy_leaves + 4u * w.heavy_nodes;
  const bool heavy_global = getenv("KR_PLACE_HEAVY_GLOBAL") != nullptr; // (read per call: tests switch it)
  const bool big_first = !getenv("KR_PLACE_BIG_FIRST") || atoi(getenv("KR_PLACE_BIG_FIRST")) != 0; // 0: every over-limit read through the second launch
  const bool heavy_lds = !heavy_global && (uint64_t)32 * w.heavy_leaves + 4ull * w.heavy_nodes <= 61440ull;
  PlaceTree PT{w.d_parent.get(), w.d_eff.get(), w.d_elig.get(), w.d_lo.get(), w.d_idx_to_pt.get(), w.d_depth.get(), w.d_node.get(), T.pn, T.nidx};
  HIP_TRY(hipMemsetAsync(w.d_cnt.get(), 0, kPlCntCount * kPlCnt * 4, st));
  HIP_TRY(hipMemsetAsync(w.d_cse.get(), 0, w.d_cse.size() * 4, st)); // 0 = unused slot: what the second kernel and the host skip
  PlaceOut PO{w.d_c0.get() + r0, w.d_info.get() + r0, w.d_cse.get(), w.d_cread.get(), w.d_cd.get(), w.d_cv.get(), w.d_cchi.get(), w.d_cprob.get(), w.d_rprob.get(), w.d_cnt.get(), (uint32_t)std::min<uint64_t>(place_cand_slots(w), 0x3FFFFFFFu),
              w.d_heavy.get(), w.d_heavy_u32.get(), w.d_heavy_f64.get(), w.heavy_leaves, w.heavy_nodes, kPlLeaves, kPlNodes,
              w.d_kse.get(), w.d_kd.get(), w.d_kv.get(), w.d_kchi.get(), (uint32_t)std::min<uint64_t>(place_keep_slots(w), 0xFFFFFFFFull), w.d_chain.get(), w.chain_cap,
              w.chain_cap * std::max<uint32_t>(1u, w.chain_waves / std::max<uint32_t>(1u, w.heavy_waves)), heavy_lds ? 1u : 0u,
              (uint32_t)((uint64_t)n + 8ull * grid), 0u, big_first ? std::min<uint32_t>(std::min<uint32_t>(w.heavy_waves, grid), 1024u) : 0u,
              w.d_chain.get() + (uint64_t)w.chain_waves * w.chain_cap, kPlInlineChain * w.chain_cap, 0u};
  const char* wit_env = getenv("KR_DEBUG_PLACE_PATHS"); // tests: the instantiations of kr_place_kernel that count their paths (read per call)
  const bool witness = wit_env && atoi(wit_env) != 0;
  PO.lcap = w.dbg_list ? (uint32_t)std::min<uint64_t>(w.dbg_list, PO.kcap) : PO.kcap;
  if (const char* e = getenv("KR_DEBUG_PLACE_LDS")) { // tests: "leaves,nodes" the LDS launch accepts, so that small trees have heavy reads
    unsigned a = kPlLeaves, b = kPlNodes;
    if (sscanf(e, "%u,%u", &a, &b) >= 1) PO.lds_leaves = std::max(1u, a), PO.lds_nodes = std::max(1u, b);
  }
  PO.big_min_records = PO.lds_leaves; // (a read with no more records than the LDS arrays have leaves cannot exceed them by its leaves)
  if (PO.inline_waves) hipLaunchKernelGGL(kr_place_big_first_kernel, dim3(std::min<uint32_t>((n + 255u) / 256u, 2048u)), dim3(256), 0, st, ro, n, PO);
  // (th = 4, the default: the instantiations whose histogram loops are unrolled, kr_dev_place.inc.  Second launch: the heavy reads the
  //  first one listed -- their number is final at the kernel boundary; usually none: the waves leave at once)
#define KR_PLACE_LAUNCH(NPV, W)  \
  do {  \
      hipLaunchKernelGGL((kr_place_kernel<false, NPV, W>), dim3(grid), dim3(kWave), 0, st, s->llh, s->ix->dix, ro, n, d_len, PT, PO, tau, no_filter ? 1u : 0u);  \
      hipLaunchKernelGGL((kr_place_kernel<true, NPV, W>), dim3(w.heavy_waves), dim3(kWave), heavy_lds ? heavy_lds_bytes : 0u, st, s->llh, s->ix->dix, ro, n, d_len, PT, PO, tau, no_filter ? 1u : 0u);  \
      hipLaunchKernelGGL((kr_place_brent_kernel<NPV>), dim3(cus * 8u), dim3(256), 0, st, s->llh, PO);  \
      hipLaunchKernelGGL((kr_place_llh_kernel<NPV>), dim3(cus * 8u), dim3(256), 0, st, s->llh, PO);  \
  } while (0)
  if (s->llh.th == 4 && !witness)
    KR_PLACE_LAUNCH(5, false);
  else if (!witness)
    KR_PLACE_LAUNCH(0, false);
  else if (s->llh.th == 4)
    KR_PLACE_LAUNCH(5, true);
  else
    KR_PLACE_LAUNCH(0, true);
#undef KR_PLACE_LAUNCH
  // (a wave of the compaction takes kept-candidate slots in chunks of kPlKeepChunk and leaves part of its last one unused, and what
  //  is copied back is every slot handed out: at least 64 reads to a wave, so that a 65,536-read batch does not copy 2 M slots back
  //  for its 200,000 candidates)
  hipLaunchKernelGGL(kr_place_compact_kernel, dim3(std::max<uint32_t>(16u, std::min<uint32_t>(2048u, (n + 255u) / 256u))), dim3(256), 0, st, PO, PT, n, chisq);
  if (w.text_on) { // the range's rows as text (kr_dev_place.inc): lengths, the blocks' first bytes, bytes
    PlaceText TX{w.d_ids.get(), w.d_id_off.get() + r0, w.d_blen.get(), w.d_card.get(), w.d_labels.get(), w.d_label_off.get(), w.d_tlen.get() + r0, w.d_tbsum.get(), w.d_text.get(), place_text_bytes(w), w.d_ttotal.get(),
                 w.text_tabular, w.text_multi, chisq, w.d_sse.get(), w.d_sd.get(), w.d_sv.get(), w.d_sc.get(), w.d_rtotal.get() + r0, w.d_rbest.get() + r0};
    const uint32_t nblk = (n + kPlTextBlock - 1) / kPlTextBlock;
    HIP_TRY(hipMemsetAsync(w.d_ttotal.get(), 0, 16, st));
    hipLaunchKernelGGL(kr_place_text_len_kernel, dim3(std::min<uint32_t>(nblk, 16384u)), dim3(256), 0, st, PO, PT, TX, n);
    hipLaunchKernelGGL(kr_text_bscan_kernel, dim3(1), dim3(1024), 0, st, TX.t_bsum, nblk, TX.text_cap, TX.total);
    hipLaunchKernelGGL(kr_place_text_write_kernel, dim3(std::min<uint32_t>(nblk, 16384u)), dim3(256), 0, st, PO, PT, TX, n);
    HIP_TRY(hipMemcpyAsync(w.h_ttotal.get(), w.d_ttotal.get(), 16, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(w.h_cnt.get(), w.d_cnt.get(), kPlCntCount * kPlCnt * 4, hipMemcpyDeviceToHost, st));
  return KR_OK;
}

// Wait for the range's kernels; a range that ran out of candidate slots is run again with as many as it asked for; then its
// per-read results (at their places in the batch's arrays) and its kept candidates come back -- the candidates behind the
// `kept_base` entries earlier ranges of this batch left in the host arrays (their reads' rd_c0 are moved accordingly).
int kr::place_device_finish(kr_stream* s, const kr::PlaceTreeArrays& T, uint32_t r0, uint32_t n, uint32_t tau, bool no_filter, double chisq,
                            uint64_t kept_base, kr::PlaceDeviceResult* out, bool first_of_file)
{
  if (!out) return kr::fail(KR_ERR_ARG, "place_device_finish: null argument");
  kr_stream::PlaceWs& w = s->pw;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->lanes[0].stream;
  int rc = 0;
  static const bool timing = getenv("KR_PLACE_TIMING") != nullptr;
  auto wall = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_mark = wall();
  auto lap = [&](const char* what) {
    if (!timing) return;
    const double now = wall();
    fprintf(stderr, "[place/device]    reads %u..%u: %s %.2f ms\n", r0, r0 + n, what, (now - t_mark) * 1e3);
    t_mark = now;
  };
  const uint32_t grid = std::min<uint32_t>(n, w.cu_count * 16u);
  int attempt = 0;
  for (;; ++attempt) {
    HIP_TRY(hipStreamSynchronize(st));
    if (!(pl_cnt(w.h_cnt.get(), kPlFlags) & (kPlFlagCandCap | kPlFlagKeepCap)) || attempt >= 2) break;
    // out of candidate slots (kPlFlagCandCap: kPlCandSlots went on counting what the reads asked for) or out of slots for the kept ones
    // (kPlFlagKeepCap: kPlKept went on counting what the compaction handed out)
    const uint64_t asked = (pl_cnt(w.h_cnt.get(), kPlFlags) & kPlFlagCandCap) ? (uint64_t)pl_cnt(w.h_cnt.get(), kPlCandSlots) + pl_cnt(w.h_cnt.get(), kPlCandSlots) / 8 + (uint64_t)grid * kPlChunk : place_cand_slots(w);
    if (asked > 0x3FFFFFFFull) break; // beyond what a slot index can name: the host back end takes the batch
    if (pl_cnt(w.h_cnt.get(), kPlFlags) & kPlFlagCandCap) kr::g_place_paths[kr::kPathRerunCand].fetch_add(1, std::memory_order_relaxed);
    if (pl_cnt(w.h_cnt.get(), kPlFlags) & kPlFlagKeepCap) {
      kr::g_place_paths[kr::kPathRerunKeep].fetch_add(1, std::memory_order_relaxed);
      w.keep_want_min = (uint64_t)pl_cnt(w.h_cnt.get(), kPlKept) + pl_cnt(w.h_cnt.get(), kPlKept) / 8 + 2048ull * 4ull * kPlKeepChunk;
    }
    if (!w.dbg_sticky) { // (KR_DEBUG_PLACE_CAPS: the rerun gets what it asked for, as it does from the real sizes)
      if (w.dbg_cand) w.dbg_cand = std::max(w.dbg_cand, asked);
      if (w.dbg_keep && (pl_cnt(w.h_cnt.get(), kPlFlags) & kPlFlagKeepCap)) w.dbg_keep = std::max(w.dbg_keep, w.keep_want_min);
    }
    if ((rc = place_size_candidates(s, asked))) return rc;
    if ((rc = kr::place_device_launch(s, T, r0, n, tau, no_filter, chisq))) return rc;
  }
  { // which paths this range took, and what it asked for (kr_place_path_counters)
    auto set = [](uint32_t k, uint64_t v) { kr::g_place_paths[k].store(v, std::memory_order_relaxed); };
    kr::g_place_paths[kr::kPathRanges].fetch_add(1, std::memory_order_relaxed);
    if (pl_cnt(w.h_cnt.get(), kPlFlags) & kPlFlagListCut) kr::g_place_paths[kr::kPathListCut].fetch_add(1, std::memory_order_relaxed);
    set(kr::kPathLastCnt0, pl_cnt(w.h_cnt.get(), kPlCandSlots)), set(kr::kPathLastCnt3, pl_cnt(w.h_cnt.get(), kPlKept)), set(kr::kPathLastCnt12, pl_cnt(w.h_cnt.get(), kPlListSlots));
    set(kr::kPathLastText, w.text_on ? w.h_ttotal.get()[0] : 0), set(kr::kPathLastCandCap, place_cand_slots(w)), set(kr::kPathLastKeepCap, place_keep_slots(w));
    set(kr::kPathLastTextCap, w.text_on ? place_text_bytes(w) : 0), set(kr::kPathLastFlags, pl_cnt(w.h_cnt.get(), kPlFlags));
    set(kr::kPathLastTextFlags, w.text_on ? w.h_ttotal.get()[1] : 0), set(kr::kPathLastAttempts, (uint64_t)attempt + 1);
    // place_read's path witnesses of the range's last attempt (all 0 without KR_DEBUG_PLACE_PATHS=1): kr_debug_place_paths
    static_assert(kPlWitEnd - kPlWitChained == kr::kPlaceWitCount && kPlWitEnd <= kPlCntCount, "kr_debug_place_paths: the names in krepp_amd/capi.py (PLACE_WITNESSES) follow PlaceCnt");
    for (uint32_t k = 0; k < kr::kPlaceWitCount; ++k)
      if (const uint32_t c = pl_cnt(w.h_cnt.get(), kPlWitChained + k)) kr::g_place_wit[k].fetch_add(c, std::memory_order_relaxed);
  }
  lap("place kernels (both launches, likelihoods, compaction) to their counters on the host");
  HIP_TRY(hipMemcpyAsync(w.h_c0.get() + r0, w.d_c0.get() + r0, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(w.h_info.get() + r0, w.d_info.get() + r0, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  out->nreads = n;
#if KR_PLACE_PROF
  fprintf(stderr, "[kr place prof] cycles/256 per phase: gather %u, sort %u, ancestors %u, weights %u, leaves %u, accumulate %u\n", pl_cnt(w.h_cnt.get(), kPlProf0), pl_cnt(w.h_cnt.get(), kPlProf0 + 1), pl_cnt(w.h_cnt.get(), kPlProf0 + 2),
          pl_cnt(w.h_cnt.get(), kPlProf0 + 3), pl_cnt(w.h_cnt.get(), kPlProf0 + 4), pl_cnt(w.h_cnt.get(), kPlProf0 + 5));
#endif
  out->overflow = (pl_cnt(w.h_cnt.get(), kPlFlags) & ~kPlFlagListCut) != 0; // (kPlFlagListCut: the internal candidates' list was incomplete -- the likelihood kernel did their minimisations itself)
  out->heavy_reads = pl_cnt(w.h_cnt.get(), kPlHeavySlots) + pl_cnt(w.h_cnt.get(), kPlInlineReads); // (list slots handed out, in chunks of 8: an upper bound, 0 when there was none; + reads done in global scratch by the first launch)
  if (out->overflow) return KR_OK;
  out->text = nullptr, out->text_len = 0, out->text_flags = 0, out->text_bgzf = false, out->text_plain = 0;
  if (w.text_on) {
    out->text_flags = w.h_ttotal.get()[1];
    const uint64_t tcap = place_text_bytes(w); // (what the kernels were told)
    if (w.h_ttotal.get()[0] > tcap) w.text_want_min = w.h_ttotal.get()[0] + w.h_ttotal.get()[0] / 4; // (this range goes to the host; the next batch gets the room)
    if (w.h_ttotal.get()[1] == 0 && w.h_ttotal.get()[0] <= tcap) { // the range's text is complete: it comes back, the candidates stay
      const uint64_t tl = w.h_ttotal.get()[0];
      if (s->bgzf_out.place_level) { // kr_stream_place_bgzf: deflated behind the text kernels, only the members come back
        // (jplace: every reported read begins with ",\n"; the first one of a file loses it -- kr_place_stream's rule, applied here
        //  to where the deflate starts)
        const uint64_t skip = (first_of_file && w.text_tabular == 0 && tl >= 2) ? 2 : 0;
        const char* comp = "";
        uint64_t clen = 0;
        if (tl > skip && (rc = kr::place_text_deflate(s, (const uint8_t*)w.d_text.get() + skip, tl - skip, &comp, &clen))) return rc;
        out->text = comp, out->text_len = clen, out->text_bgzf = true, out->text_plain = tl;
        out->kept = 0;
        out->rd_c0 = w.h_c0.get(), out->rd_info = w.h_info.get();
        lap("the range's rows as BGZF members, back on the host");
        return KR_OK;
      }
      if (tl > w.h_text.size() && (rc = place_grow(w.h_text, tl + tl / 4 + (1u << 20)))) return rc;
      if (tl) {
        HIP_TRY(hipMemcpyAsync(w.h_text.get(), w.d_text.get(), tl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
      out->text = w.h_text.get() ? w.h_text.get() : "", out->text_len = tl;
      out->kept = 0;
      out->rd_c0 = w.h_c0.get(), out->rd_info = w.h_info.get();
      lap("the range's rows as text, back on the host");
      return KR_OK;
    }
  }
  const uint64_t used = std::min<uint64_t>(pl_cnt(w.h_cnt.get(), kPlKept), place_keep_slots(w)); // the candidates kept (compacted)
  // (an earlier range's candidates have been consumed by the time a later one is finished: nothing to carry over)
  if (kept_base + used > w.h_cse.size() && (rc = place_grow_all(kept_base + used + used / 4 + 1024, w.h_cse, w.h_cd, w.h_cv, w.h_cchi))) return rc;
  if (used) {
    HIP_TRY(hipMemcpyAsync(w.h_cse.get() + kept_base, w.d_kse.get(), used * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(w.h_cd.get() + kept_base, w.d_kd.get(), used * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(w.h_cv.get() + kept_base, w.d_kv.get(), used * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(w.h_cchi.get() + kept_base, w.d_kchi.get(), used * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (kept_base)
    for (uint32_t r = r0; r < r0 + n; ++r) w.h_c0.get()[r] += (uint32_t)kept_base;
  out->kept = used;
  lap("candidates kept, back on the host");
  out->rd_c0 = w.h_c0.get(), out->rd_info = w.h_info.get(), out->c_se = w.h_cse.get(), out->c_d = w.h_cd.get(), out->c_v = w.h_cv.get(), out->c_chisq = w.h_cchi.get();
  return KR_OK;
}

uint32_t kr::place_stream_nreads(const kr_stream* s) { return s ? s->batch.nreads : 0; }

namespace {
// What place_device_text_begin and place_device_text_begin_parsed share.  place_text_tree: the tree's part of the text on the device;
// place_text_rooms: what is sized by the batch once its ids (`total` bytes of them) are placed, and the switch itself.
int place_text_tree(kr_stream* s, const kr::PlaceTreeArrays& T)
{
  kr_stream::PlaceWs& w = s->pw;
  int rc = 0;
  if (w.text_tree_tag != w.tree_tag || !w.d_blen.get()) { // the tree's branch lengths, subtree sizes and labels (once per tree)
    const uint64_t n1 = (uint64_t)T.pn + 1;
    const uint64_t lb = T.label_off[T.pn + 1];
    w.text_tree_tag = nullptr;
    if ((rc = place_renew(w.d_blen, n1)) || (rc = place_renew(w.d_card, n1)) || (rc = place_renew(w.d_label_off, n1 + 1)) || (rc = place_renew(w.d_labels, lb + 16))) return rc;
    HIP_TRY(hipMemcpy(w.d_blen.get(), T.blen, n1 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.d_card.get(), T.card, n1 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(w.d_label_off.get(), T.label_off, (n1 + 1) * 4, hipMemcpyHostToDevice));
    if (lb) HIP_TRY(hipMemcpy(w.d_labels.get(), T.labels, lb, hipMemcpyHostToDevice));
    w.text_tree_tag = w.tree_tag;
  }
  return KR_OK;
}
int place_text_rooms(kr_stream* s, uint32_t nreads, uint64_t total, int tabular, bool multi)
{
  kr_stream::PlaceWs& w = s->pw;
  int rc = 0;
  // per-read lengths, block sums, the text itself: room for the ids and 512 bytes of rows a read (a range with more comes back
  // with flag 2 and is formatted by the host)
  if (nreads > w.d_tlen.size() && (rc = place_grow(w.d_tlen, (uint64_t)nreads + nreads / 4 + 16))) return rc;
  if ((rc = place_grow(w.d_tbsum, w.d_tlen.size() / kPlTextBlock + 4)) || (rc = place_grow_all(2, w.d_ttotal, w.h_ttotal))) return rc; // (the block sums: sized by the lengths' array)
  const uint64_t want = std::max<uint64_t>(w.dbg_text ? w.dbg_text : total + (uint64_t)nreads * 512ull + (1u << 20), w.text_want_min); // (text_want_min: what a range that outgrew the buffer asked for)
  if ((rc = place_grow(w.d_text, want))) return rc;
  if (nreads > w.d_rtotal.size() && (rc = place_grow_all((uint64_t)nreads + nreads / 4 + 16, w.d_rtotal, w.d_rbest))) return rc;
  w.text_tabular = tabular ? 1u : 0u, w.text_multi = multi ? 1u : 0u;
  w.text_on = true;
  return place_size_candidates(s, w.d_cse.size()); // (the sorted copy of the kept candidates: sized with them, now and when a range is run again)
}
} // namespace

int kr::place_device_text_begin(kr_stream* s, const kr::PlaceTreeArrays& T, const char* const* names, uint32_t nreads, int tabular, bool multi)
{
  if (!s || !names || !T.blen || !T.card || !T.labels || !T.label_off) return kr::fail(KR_ERR_ARG, "place_device_text_begin: null argument");
  kr_stream::PlaceWs& w = s->pw;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->lanes[0].stream;
  int rc = place_text_tree(s, T);
  if (rc) return rc;
  // the reads' ids back to back (lengths and copies by the host pool: 400,000 names are 400,000 pointers to chase)
  if ((uint64_t)nreads + 1 > w.d_id_off.size() && (rc = place_grow_all((uint64_t)nreads + nreads / 4 + 16, w.d_id_off, w.h_id_off))) return rc;
  const int nt = std::max(1, std::min(std::min(kr::parallel_width(), 16), (int)(nreads / 8192)));
  std::vector<uint64_t> part((size_t)nt + 1, 0);
  kr::parallel_for(nt, [&](int t) {
    uint64_t sum = 0;
    for (size_t r = (size_t)nreads * t / nt; r < (size_t)nreads * (t + 1) / nt; ++r) {
      const uint32_t l = (uint32_t)strlen(names[r]);
      w.h_id_off.get()[r + 1] = l; // (lengths first; offsets below)
      sum += l;
    }
    part[(size_t)t + 1] = sum;
  });
  for (int t = 0; t < nt; ++t) part[(size_t)t + 1] += part[(size_t)t];
  const uint64_t total = part[(size_t)nt];
  if (total >= 0xFFFFFFF0ull) return kr::fail(KR_ERR_CAPACITY, "place: more than 4 GB of read ids in one batch");
  // (the smaller of the two: a parsed batch grows d_ids alone)
  if (total + 16 > std::min(w.d_ids.size(), w.h_ids.size()) && (rc = place_grow_all(total + total / 4 + 4096, w.d_ids, w.h_ids))) return rc;
  w.h_id_off.get()[0] = 0;
  kr::parallel_for(nt, [&](int t) {
    uint64_t at = part[(size_t)t];
    for (size_t r = (size_t)nreads * t / nt; r < (size_t)nreads * (t + 1) / nt; ++r) {
      const uint32_t l = w.h_id_off.get()[r + 1];
      memcpy(w.h_ids.get() + at, names[r], l);
      at += l;
      w.h_id_off.get()[r + 1] = (uint32_t)at;
    }
  });
  HIP_TRY(hipMemcpyAsync(w.d_id_off.get(), w.h_id_off.get(), ((uint64_t)nreads + 1) * 4, hipMemcpyHostToDevice, st));
  if (total) HIP_TRY(hipMemcpyAsync(w.d_ids.get(), w.h_ids.get(), total, hipMemcpyHostToDevice, st));
  return place_text_rooms(s, nreads, total, tabular, multi);
}

// The same for a batch begun with place_device_begin_parsed(want_ids): the ids' offsets are in d_id_off already and their total is on
// the host (the front end has been waited for behind them); d_ids and d_text are sized from it, and the copy kernel is queued.
int kr::place_device_text_begin_parsed(kr_stream* s, const kr::PlaceTreeArrays& T, int tabular, bool multi)
{
  if (!s || !T.blen || !T.card || !T.labels || !T.label_off) return kr::fail(KR_ERR_ARG, "place_device_text_begin: null argument");
  int rc = place_parsed_state(s);
  if (rc) return rc;
  kr_stream::PlaceWs& w = s->pw;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->lanes[0].stream;
  if (!w.ids_queued) return kr::fail(KR_ERR_STATE, "place_device_text_begin: place_device_begin_parsed did not lay out the ids");
  if ((rc = place_text_tree(s, T))) return rc;
  HIP_TRY(hipStreamSynchronize(st)); // (at once as a rule: kr_batch_wait has waited for this stream behind the total's copy)
  const uint32_t nreads = s->batch.nreads;
  const uint64_t total = w.h_idtot.get()[0];
  if (total >= 0xFFFFFFF0ull) return kr::fail(KR_ERR_CAPACITY, "place: more than 4 GB of read ids in one batch");
  if (total + 16 > w.d_ids.size() && (rc = place_grow(w.d_ids, total + total / 4 + 4096))) return rc; // (d_ids alone: no id is staged on the host, nothing is page-locked for them)
  hipLaunchKernelGGL(kr_pp_idcopy_kernel, dim3(std::max<uint32_t>(1u, std::min<uint32_t>((nreads + 15u) / 16u, 8192u))), dim3(256), 0, st, place_parsed_io(s));
  HIP_TRY(hipGetLastError());
  w.ids_reads = nreads;
  return place_text_rooms(s, nreads, total, tabular, multi);
}

// The host's side of a parsed batch, asked for only by the paths that format on the host: the caller's offsets, and the accepted
// records' names as (position in the chunk, length) -- kr_batch_fastq_names.
int kr::place_parsed_offsets(kr_stream* s, uint64_t* offsets)
{
  if (!s || !offsets) return kr::fail(KR_ERR_ARG, "place_parsed_offsets: null argument");
  const int rc = place_parsed_state(s);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->lanes[0].stream;
  HIP_TRY(hipMemcpyAsync(offsets, s->d_offsets, ((uint64_t)s->batch.nreads + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return KR_OK;
}
void kr::place_call_begin(kr_stream* s)
{
  if (s) s->pw.ids_queued = false, s->pw.ids_reads = 0;
}
uint32_t kr::place_parsed_nreads(const kr_stream* s) { return s && s->fq.on && s->parse.parsed && s->batch.submitted && s->batch.from.parsed ? s->parse.nreads : 0; }
int kr::place_parsed_check(const kr_stream* s) { return s ? place_parsed_state(s) : kr::fail(KR_ERR_ARG, "kr_place_stream_parsed: null argument"); }

extern "C" int kr_debug_place_layout(uint32_t* out8)
{ // (krepp_amd.h: the order of the values; no device is touched)
  kr::clear_error();
  if (!out8) return kr::fail(KR_ERR_ARG, "kr_debug_place_layout: null argument");
  const uint32_t v[8] = {kPlLeaves, kPlNodes, kPlBlock, kPlChain, kPlChunk, kPlChainFactor, kPlRunsLeaves, kPlInlineChain};
  memcpy(out8, v, sizeof(v));
  return KR_OK;
}

extern "C" int kr_debug_place_ids(kr_stream* s, char* ids, uint32_t* id_off)
{
  kr::clear_error();
  if (!s || !ids || !id_off) return kr::fail(KR_ERR_ARG, "kr_debug_place_ids: null argument");
  kr_stream::PlaceWs& w = s->pw;
  if (!w.ids_reads) return kr::fail(KR_ERR_STATE, "kr_debug_place_ids: the stream's last place call was not a kr_place_stream_parsed that laid out ids on the device");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->lanes[0].stream;
  HIP_TRY(hipMemcpyAsync(id_off, w.d_id_off.get(), ((uint64_t)w.ids_reads + 1) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (id_off[w.ids_reads]) HIP_TRY(hipMemcpyAsync(ids, w.d_ids.get(), id_off[w.ids_reads], hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return KR_OK;
}
void kr::place_device_abort(kr_stream* s)
{
  if (!s) return;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->lanes[0].stream);
}
