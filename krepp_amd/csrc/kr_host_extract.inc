// kr_host_extract.inc -- part of kr_device.hip (host side): kr_stream_extract_enable, kr_stream_extract_max, kr_stream_extract_defer,
// kr_batch_extract_pair, kr_batch_collect_extract, kr_batch_collect_extract_bgzf, kr_debug_extract_ms.  Kernels: kr_dev_extract.inc.
// A seek batch that a record finder queued (kr_batch_submit_fastq / _fasta / _bgzf with KR_SEEK) on a stream with extract enabled
// has the extract kernels queued behind its solve and text kernels, on the same stream and inside the same link of the index's
// kernel chain (seek_queue, kr_host_seek.inc): the chunk's accepted bytes [0, consumed) land in d_out as the matched reads followed
// by the unmatched reads.  The collect calls copy back the parts asked for, plain or deflated into BGZF members by the kernels of
// kr_dev_deflate.inc; nothing else of the batch is touched, so kr_batch_collect_text / _seek give what they give without extract.

namespace {

// the four extract kernels on `st` with the verdict taken from d[0 .. n): the reads' own distances (extract_queue) or the pair
// values (kr_batch_extract_pair); the chunk is the stream's last record finder call's
int extract_launch(kr_stream* s, hipStream_t st, const double* d)
{
  kr_stream::Extract& e = s->extract;
  const kr_stream::Fastq& f = s->fq;
  ExIO x;
  x.raw = f.d_raw, x.sum = f.d_sum;
  x.nl = f.last_fasta ? nullptr : f.d_nl, x.nl_cap = 4u * s->max_reads;
  x.hs = f.d_hs, x.max_reads = s->max_reads, x.raw_cap = f.raw_cap;
  if (f.last_fasta && !f.d_hs) return kr::fail(KR_ERR_STATE, "extract: the FASTA record finder's start list is missing");
  x.d = d, x.max_dist = e.max_dist;
  x.rec_start = e.d_start, x.mpre = e.d_mpre, x.bsum = e.d_bsum, x.out = e.d_out, x.res = e.d_res;
  static const bool bytes_only = getenv("KR_EXTRACT_STORE") && atoi(getenv("KR_EXTRACT_STORE")) == 1; // (measurements: byte stores only)
  x.wide = bytes_only ? 0u : 1u;
  // Two sources for the same numbers, on purpose: the kernels take the record count and `consumed` from the record finder's DEVICE
  // summary (x.sum) and bound every index by them; the host's copy (fq_finish waited for it before the batch was queued) only sizes
  // the grids.  Every kernel strides over its blocks / tiles, so a grid that differed from the device's counts would change how
  // the work is shared out, never what is computed.
  const uint32_t bgrid = std::min<uint32_t>(s->batch.nreads / kRowBlock + 1u, 4096u);
  const uint32_t tgrid = std::min<uint32_t>((uint32_t)((f.h_sum->consumed + kFqTile - 1) / kFqTile) + 1u, 65536u);
  hipLaunchKernelGGL(kr_ex_len_kernel, dim3(bgrid), dim3(256), 0, st, x);
  hipLaunchKernelGGL(kr_ex_scan_kernel, dim3(1), dim3(1024), 0, st, x);
  hipLaunchKernelGGL(kr_ex_pre_kernel, dim3(bgrid), dim3(256), 0, st, x);
  hipLaunchKernelGGL(kr_ex_copy_kernel, dim3(tgrid), dim3(256), 0, st, x);
  return KR_OK;
}

// queued by seek_queue behind the batch's last kernel
int extract_queue(kr_stream* s, hipStream_t st)
{
  kr_stream::Extract& e = s->extract;
  HIP_TRY(hipEventRecord(e.ev[0], st));
  if (int rc = extract_launch(s, st, s->seek.d_d)) return rc;
  HIP_TRY(hipEventRecord(e.ev[1], st));
  e.timed = true;
  HIP_TRY(hipMemcpyAsync(e.h_res, e.d_res, 32, hipMemcpyDeviceToHost, st));
  return KR_OK;
}

// the states both collect calls refuse; behind it the batch has been waited for and h_res holds its summary
int extract_ready(kr_stream* s, uint32_t which, kr_extract_view* out, const char* who)
{
  const std::string w = std::string(who) + ": ";
  if (!s || !out) return kr::fail(KR_ERR_ARG, w + "null argument");
  if (which == 0 || (which & ~(KR_EXTRACT_MATCHED | KR_EXTRACT_UNMATCHED))) return kr::fail(KR_ERR_ARG, w + "which: KR_EXTRACT_MATCHED, KR_EXTRACT_UNMATCHED or both");
  memset(out, 0, sizeof(*out));
  if (!s->extract.on) return kr::fail(KR_ERR_STATE, w + "kr_stream_extract_enable first");
  if (!s->batch.submitted || !s->batch.seek) return kr::fail(KR_ERR_STATE, w + "the last batch was not submitted with KR_SEEK");
  if (s->parse.parsed && s->batch.extract_deferred && !s->batch.extract)
    return kr::fail(KR_ERR_STATE, w + "the stream defers its split (kr_stream_extract_defer): kr_batch_extract_pair first");
  if (!s->parse.parsed || !s->batch.extract)
    return kr::fail(KR_ERR_STATE, w + "the last submit was not a seek batch of raw bytes (kr_batch_submit_fastq / _fasta / _bgzf with KR_SEEK)");
  if (s->parse.nreads == 0) return kr::fail(KR_ERR_STATE, w + "the last submit accepted no record");
  if (int rc = kr_batch_wait(s)) return rc;
  const unsigned long long* r = s->extract.h_res;
  if (r[0] > r[3] || r[3] > s->fq.raw_cap || r[1] > r[2]) return kr::fail(KR_ERR_NO_DEVICE, w + "the extract kernels left an impossible summary");
  out->nreads = (uint32_t)r[2], out->nmatched = (uint32_t)r[1];
  out->matched_bytes = r[0], out->unmatched_bytes = r[3] - r[0];
  return KR_OK;
}

} // namespace

extern "C" {

int kr_stream_extract_enable(kr_stream* s, double max_dist)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_stream_extract_enable: null argument");
  if (max_dist == max_dist && (max_dist < 0 || std::isinf(max_dist))) return kr::fail(KR_ERR_ARG, "kr_stream_extract_enable: max_dist is negative or infinite (NaN: no threshold)");
  if (!s->seek.on || !s->fq.on) return kr::fail(KR_ERR_STATE, "kr_stream_extract_enable: kr_stream_seek_enable and kr_stream_fastq_enable first");
  if (s->extract.on) return kr::fail(KR_ERR_STATE, "kr_stream_extract_enable: already enabled");
  HIP_TRY(hipSetDevice(s->ix->device));
  kr_stream::Extract& e = s->extract;
  const uint64_t nr = s->max_reads, out_pad = ((s->fq.raw_cap + 15) & ~15ull) + 16;
  int rc = 0;
  if ((rc = salloc(s, &e.d_start, nr + 1)) || (rc = salloc(s, &e.d_mpre, nr + 1)) || (rc = salloc(s, &e.d_bsum, nr / kRowBlock + 2)) ||
      (rc = salloc(s, &e.d_out, out_pad)) || (rc = salloc(s, &e.d_res, 4)) || (rc = halloc(s, &e.h_res, 4)) || (rc = halloc(s, &e.h_out, out_pad)))
    return rc;
  for (auto& ev : e.ev) HIP_TRY(hipEventCreate(&ev));
  e.max_dist = max_dist;
  e.on = true;
  return KR_OK;
}

int kr_stream_extract_max(kr_stream* s, double max_dist)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_stream_extract_max: null argument");
  if (max_dist == max_dist && (max_dist < 0 || std::isinf(max_dist))) return kr::fail(KR_ERR_ARG, "kr_stream_extract_max: max_dist is negative or infinite (NaN: no threshold)");
  if (!s->extract.on) return kr::fail(KR_ERR_STATE, "kr_stream_extract_max: kr_stream_extract_enable first");
  s->extract.max_dist = max_dist; // (read when the next batch is queued: the batch in flight keeps its rule)
  return KR_OK;
}

int kr_stream_extract_defer(kr_stream* s, uint32_t on)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_stream_extract_defer: null argument");
  if (!s->extract.on) return kr::fail(KR_ERR_STATE, "kr_stream_extract_defer: kr_stream_extract_enable first");
  kr_stream::Extract& e = s->extract;
  if (on && !e.ev_x[0]) {
    HIP_TRY(hipSetDevice(s->ix->device));
    for (auto& ev : e.ev_x) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  e.defer = on != 0; // (read when the next batch is queued: the batch in flight stays what it is)
  return KR_OK;
}

// The mates of a pair are split together.  Everything is queued on A's lane: it waits for B's lane as it stands now (B's solve and
// text kernels are behind that event), runs the pair kernel, the four extract kernels of A, those of B, and both summary copies; B's
// lane then waits for the event behind them, so kr_batch_wait(b) and B's next drain_batch cover the lot.  Every event is recorded
// before the wait on it is queued -- there is no cycle --, and the order holds without the index's kernel chain (chain_off): the
// ChainLink only keeps other batches' kernels out from between these.
int kr_batch_extract_pair(kr_stream* a, kr_stream* b, uint32_t rule)
{
  kr::clear_error();
  const std::string w = "kr_batch_extract_pair: ";
  if (!a || !b) return kr::fail(KR_ERR_ARG, w + "null argument");
  if (rule != KR_PAIR_ANY && rule != KR_PAIR_BOTH) return kr::fail(KR_ERR_ARG, w + "rule " + std::to_string(rule) + " (KR_PAIR_ANY or KR_PAIR_BOTH)");
  const bool inter = a == b;
  if (a->ix != b->ix) return kr::fail(KR_ERR_STATE, w + "the two streams are on different indexes");
  for (kr_stream* s : {a, b}) {
    if (!s->extract.on) return kr::fail(KR_ERR_STATE, w + "kr_stream_extract_enable first");
    if (!s->extract.defer) return kr::fail(KR_ERR_STATE, w + "kr_stream_extract_defer first: the stream splits every batch by its own reads");
    const Batch& q = s->batch;
    if (!q.submitted || !q.seek || !s->parse.parsed || !q.from.parsed || !q.extract_deferred) // (deferred: also a batch that a pair call has split)
      return kr::fail(KR_ERR_STATE, w + "the last submit was not a seek batch of raw bytes (kr_batch_submit_fastq / _fasta / _bgzf with KR_SEEK) on a deferring stream");
    if (q.rc) return kr::fail(KR_ERR_STATE, w + "the batch failed: " + q.msg);
    if (s->parse.nreads == 0) return kr::fail(KR_ERR_STATE, w + "the last submit accepted no record");
  }
  const uint32_t n = a->parse.nreads;
  if (b->parse.nreads != n)
    return kr::fail(KR_ERR_STATE, w + "the two batches hold " + std::to_string(n) + " and " + std::to_string(b->parse.nreads) + " records: mates must be the same records of both");
  if (inter && (n & 1u)) return kr::fail(KR_ERR_STATE, w + "an interleaved batch of " + std::to_string(n) + " records: the last one has no mate");
  const double ta = a->extract.max_dist, tb = b->extract.max_dist;
  if (!((ta != ta && tb != tb) || memcmp(&ta, &tb, sizeof(ta)) == 0)) return kr::fail(KR_ERR_STATE, w + "the two streams have different thresholds (kr_stream_extract_max)");
  HIP_TRY(hipSetDevice(a->ix->device));
  (void)hipGetLastError();
  for (kr_stream* s : {a, b})
    if (!s->extract.d_pair)
      if (int rc = salloc(s, &s->extract.d_pair, (uint64_t)s->max_reads)) return rc;
  kr_stream::Extract &ea = a->extract, &eb = b->extract;
  hipStream_t sa = a->lanes[0].stream, sb = b->lanes[0].stream;
  if (!inter) {
    HIP_TRY(hipEventRecord(eb.ev_x[0], sb));
    HIP_TRY(hipStreamWaitEvent(sa, eb.ev_x[0], 0));
  }
  ChainLink chain(a->ix, sa);
  HIP_TRY(chain.opened);
  HIP_TRY(hipEventRecord(ea.ev[0], sa));
  if (!inter) HIP_TRY(hipEventRecord(eb.ev[0], sa));
  ExPairIO p;
  p.sum_a = a->fq.d_sum, p.sum_b = b->fq.d_sum, p.max_a = a->max_reads, p.max_b = b->max_reads;
  p.d_a = a->seek.d_d, p.d_b = b->seek.d_d, p.pv_a = ea.d_pair, p.pv_b = eb.d_pair;
  p.rule = rule, p.interleaved = inter ? 1u : 0u;
  hipLaunchKernelGGL(kr_ex_pair_kernel, dim3(std::min<uint32_t>(n / 256u + 1u, 4096u)), dim3(256), 0, sa, p);
  if (int rc = extract_launch(a, sa, ea.d_pair)) return rc;
  if (!inter)
    if (int rc = extract_launch(b, sa, eb.d_pair)) return rc;
  HIP_TRY(hipEventRecord(ea.ev[1], sa));
  if (!inter) HIP_TRY(hipEventRecord(eb.ev[1], sa));
  HIP_TRY(hipMemcpyAsync(ea.h_res, ea.d_res, 32, hipMemcpyDeviceToHost, sa));
  if (!inter) HIP_TRY(hipMemcpyAsync(eb.h_res, eb.d_res, 32, hipMemcpyDeviceToHost, sa));
  HIP_TRY(chain.close(sa));
  if (!inter) {
    HIP_TRY(hipEventRecord(ea.ev_x[1], sa));
    HIP_TRY(hipStreamWaitEvent(sb, ea.ev_x[1], 0));
  }
  HIP_TRY(hipGetLastError());
  for (kr_stream* s : {a, b}) { // the parts are new: the batches are waited for again, nothing of the split is in the mirrors
    s->extract.timed = true;
    s->batch.extract = true, s->batch.extract_have = 0, s->batch.waited = false;
  }
  return KR_OK;
}

int kr_batch_collect_extract(kr_stream* s, uint32_t which, kr_extract_view* out)
{
  kr::clear_error();
  if (int rc = extract_ready(s, which, out, "kr_batch_collect_extract")) return rc;
  kr_stream::Extract& e = s->extract;
  const uint64_t M = out->matched_bytes, U = out->unmatched_bytes;
  const uint32_t need = which & ~s->batch.extract_have;
  if (need) { // each part goes where it lies in d_out: both pointers stay good whatever is asked for later
    HIP_TRY(hipSetDevice(s->ix->device));
    hipStream_t st = s->lanes[0].stream;
    if ((need & KR_EXTRACT_MATCHED) && M) HIP_TRY(hipMemcpyAsync(e.h_out, e.d_out, M, hipMemcpyDeviceToHost, st));
    if ((need & KR_EXTRACT_UNMATCHED) && U) HIP_TRY(hipMemcpyAsync(e.h_out + M, e.d_out + M, U, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    s->batch.extract_have |= need;
  }
  if (which & KR_EXTRACT_MATCHED) out->matched = e.h_out, out->matched_len = M;
  if (which & KR_EXTRACT_UNMATCHED) out->unmatched = e.h_out + M, out->unmatched_len = U;
  return KR_OK;
}

int kr_batch_collect_extract_bgzf(kr_stream* s, uint32_t which, uint32_t level, kr_extract_view* out)
{
  kr::clear_error();
  if (s && out && level != 1 && level != 2)
    return kr::fail(KR_ERR_ARG, "kr_batch_collect_extract_bgzf: level " + std::to_string(level) + " (1: fixed codes, 2: dynamic codes)");
  if (int rc = extract_ready(s, which, out, "kr_batch_collect_extract_bgzf")) return rc;
  kr_stream::Extract& e = s->extract;
  kr_stream::BgzfOut& o = s->bgzf_out;
  HIP_TRY(hipSetDevice(s->ix->device));
  hipStream_t st = s->lanes[0].stream;
  const uint64_t M = out->matched_bytes, U = out->unmatched_bytes;
  // room for both parts' members in the page-locked buffer, whatever is asked for: a later call for the other part moves nothing
  const uint64_t bound_m = kr::bgzf_deflate_bound(M, o.member_in), bound_u = kr::bgzf_deflate_bound(U, o.member_in);
  if (bound_m + bound_u > e.h_members.size() && !e.h_members.reserve(bound_m + bound_u + (bound_m + bound_u) / 4 + (1u << 20)))
    return alloc_failed("kr_batch_collect_extract_bgzf: the members' page-locked buffer");
  const uint32_t level_before = o.level;
  o.level = level;
  int rc = KR_OK;
  auto part = [&](const uint8_t* d_part, uint64_t n, uint8_t* h_at, uint64_t* len) -> int { // one part after the other through the stream's deflate buffers
    *len = 0;
    if (n == 0) return KR_OK; // an empty part writes no member
    const uint64_t bound = kr::bgzf_deflate_bound(n, o.member_in), nm = kr::bgzf_deflate_members(n, o.member_in);
    const bool room = nm * kr::bgzf_slot_stride(o.member_in) <= o.d_slots.size() && nm + 1 <= o.d_off.size() && bound <= o.d_out.size() &&
                      o.h_total.size() >= 1 && (o.level != 2 || nm * o.member_in <= o.d_tokens.size());
    if (!room) // (nothing of this stream's deflate is in flight: every deflate_run waits)
      if (int r = deflate_reserve(s, n + n / 4 + (1u << 20))) return r;
    uint64_t total = 0;
    if (int r = deflate_run(s, st, d_part, n, &total)) return r;
    HIP_TRY(hipMemcpyAsync(h_at, o.d_out.get(), total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *len = total;
    return KR_OK;
  };
  uint64_t len_m = 0, len_u = 0;
  if (which & KR_EXTRACT_MATCHED) rc = part(e.d_out, M, e.h_members.get(), &len_m);
  if (!rc && (which & KR_EXTRACT_UNMATCHED)) rc = part(e.d_out + M, U, e.h_members.get() + bound_m, &len_u);
  o.level = level_before;
  if (rc) return rc;
  if (which & KR_EXTRACT_MATCHED) out->matched = e.h_members.get(), out->matched_len = len_m;
  if (which & KR_EXTRACT_UNMATCHED) out->unmatched = e.h_members.get() + bound_m, out->unmatched_len = len_u;
  return KR_OK;
}

int kr_debug_extract_ms(kr_stream* s, float* ms)
{
  kr::clear_error();
  if (!s || !ms) return kr::fail(KR_ERR_ARG, "kr_debug_extract_ms: null argument");
  if (!s->extract.on || !s->extract.timed) return kr::fail(KR_ERR_STATE, "kr_debug_extract_ms: no extract batch on this stream yet");
  HIP_TRY(hipSetDevice(s->ix->device));
  HIP_TRY(hipEventSynchronize(s->extract.ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, s->extract.ev[0], s->extract.ev[1]));
  return KR_OK;
}

} // extern "C"
