// kr_host_seek.inc -- part of kr_device.hip (host side): kr_stream_seek_enable, the submit / wait of a batch flagged KR_SEEK,
// kr_batch_collect_seek, kr_debug_seek_layout, kr_debug_seek_ms.  Kernels: kr_dev_seek.inc.
// A seek batch is one lane's work on the stream's first lane: the bases' copy, the unit count, kr_seek_hist_kernel,
// kr_seek_solve_kernel and, for a batch with ids, the text kernels -- ordered by the index's kernel chain like any batch.  It uses
// the stream's base / offset staging, the text buffers and its own counters; none of the item list, record slots or accumulate scratch.

// the same test kr_format_seek applies to the host index: one library, the root and one leaf
static bool seek_is_sketch(const kr_index* ix) { return ix->dix.nlibs == 1 && ix->hlibs.size() == 1 && ix->hlibs[0].nnodes == 2; }

// Is `flags` a seek batch this stream can take?  tile_ok: the raw-bytes submits, where KR_TILE_DEVICE lets long records through
static int seek_check(const kr_stream* s, uint32_t flags, bool tile_ok, const char* who)
{
  const std::string w = std::string(who) + ": ";
  if (flags & (KR_TAP_ACCS | KR_TAP_HITS | KR_ROWS_ONLY | KR_ROWS_INDEXED | KR_TILE_ROWS))
    return kr::fail(KR_ERR_ARG, w + "KR_SEEK goes with none of KR_TAP_ACCS, KR_TAP_HITS, KR_ROWS_ONLY, KR_ROWS_INDEXED, KR_TILE_ROWS");
  if (!tile_ok && (flags & KR_TILE_DEVICE)) return kr::fail(KR_ERR_ARG, w + "KR_TILE_DEVICE means nothing for a seek batch here: it takes a sequence of any length");
  if (!seek_is_sketch(s->ix)) return kr::fail(KR_ERR_ARG, w + "KR_SEEK: not a sketch index");
  if (!s->seek.on) return kr::fail(KR_ERR_STATE, w + "KR_SEEK: kr_stream_seek_enable first");
  return KR_OK;
}

static SeekIO seek_io(const kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads)
{
  const kr_stream::Seek& k = s->seek;
  SeekIO io;
  io.bases = bases, io.offsets = offsets, io.nreads = nreads, io.np = k.np;
  io.first = k.d_first, io.bsum = k.d_bsum;
  io.hist = k.d_cnt, io.onmers = k.d_cnt + (uint64_t)nreads * 2u * k.np;
  io.d = k.d_d, io.d_strand = k.d_d + nreads;
  return io;
}

static int seek_queue(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags)
{
  kr_stream::Seek& k = s->seek;
  Lane& L = s->lanes[0];
  if (!L.stream) HIP_TRY(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
  hipStream_t st = L.stream;
  L.read0 = 0, L.nreads = nreads, L.nrecs = 0, L.nrows = 0;
  const uint8_t* d_bases = bases;
  const uint64_t* d_offsets = offsets;
  if (!(flags & KR_BASES_DEVICE)) { // as a dist batch's first lane
    if (int rc = stage_reads(s, st, bases, offsets, 0, nreads, 0, flags)) return rc;
    d_bases = s->d_bases, d_offsets = s->d_offsets;
  }
  kr_stream::Text& tx = s->text;
  const Batch& b = s->batch;
  if (b.from.ids == kIdsHost)
    if (int rc = upload_ids(s, st)) return rc;
  const SeekIO io = seek_io(s, d_bases, d_offsets, nreads);
  HIP_TRY(hipMemsetAsync(k.d_cnt, 0, (uint64_t)nreads * (2u * k.np + 1u) * 4, st)); // the batch's counters
  // the kernel chain of the index (see kr_index): wait for the previous batch's kernels, record behind ours
  const DevIndex& dix = s->ix->dix;
  ChainLink chain(s->ix, st);
  HIP_TRY(chain.opened);
  HIP_TRY(hipEventRecord(k.ev[0], st));
  const uint32_t nblk = (nreads + kRowBlock - 1) / kRowBlock, bgrid = std::min<uint32_t>(nblk, 4096u);
  hipLaunchKernelGGL(kr_seek_count_kernel, dim3(bgrid), dim3(256), 0, st, io, dix.k);
  hipLaunchKernelGGL(kr_seek_uscan_kernel, dim3(1), dim3(1024), 0, st, io);
  hipLaunchKernelGGL(kr_seek_first_kernel, dim3(bgrid), dim3(256), 0, st, io, dix.k);
  // (the number of units stays on the device: a grid that fills the chip strides over them)
  const uint32_t hgrid = 2048u; // 8,192 waves: what 256 CUs hold
  static const bool fe_tab = !getenv("KR_SEEK_FE") || atoi(getenv("KR_SEEK_FE")) != 0; // (experiments: 0 = the windows + software PEXT front end)
  with_bools([&](auto SL, auto TAB) {
    hipLaunchKernelGGL((kr_seek_hist_kernel<SL.value, TAB.value>), dim3(hgrid), dim3(kSeekHistWaves * kWave), 0, st, dix, io, s->llh.th);
  }, dix.m <= 64, fe_tab);
  HIP_TRY(hipEventRecord(k.ev[1], st));
  const uint32_t sgrid = (uint32_t)std::min<uint64_t>((2ull * nreads + 255) / 256, 8192u);
  with_bools([&](auto NP5) {
    constexpr int NPV = NP5.value ? 5 : 0; // the instantiation kr_llh_kernel runs for this threshold
    hipLaunchKernelGGL(kr_seek_solve_kernel<NPV>, dim3(sgrid), dim3(256), 0, st, s->llh, dix, io);
  }, s->llh.th == 4);
  HIP_TRY(hipEventRecord(k.ev[2], st));
  if (b.has_ids()) {
    TextIO t{tx.d_ids, tx.d_id_off, b.from.id_sep, nullptr, nullptr, tx.d_tlen, tx.d_bsum, tx.d_text, tx.text_cap, tx.d_total};
    HIP_TRY(hipMemsetAsync(tx.d_total, 0, 16, st));
    hipLaunchKernelGGL(kr_seek_text_len_kernel, dim3(std::min<uint32_t>(nblk, 8192u)), dim3(256), 0, st, io, t);
    hipLaunchKernelGGL(kr_text_bscan_kernel, dim3(1), dim3(1024), 0, st, t.t_bsum, nblk, t.text_cap, t.total);
    hipLaunchKernelGGL(kr_seek_text_write_kernel, dim3(std::min<uint32_t>(nblk, 8192u)), dim3(256), 0, st, io, t);
    HIP_TRY(hipMemcpyAsync(tx.h_total, tx.d_total, 16, hipMemcpyDeviceToHost, st));
    s->batch.text_made = true;
  }
  HIP_TRY(hipEventRecord(k.ev[3], st));
  k.timed = true;
  if (s->extract.on && b.from.parsed) { // the chunk is in fq.d_raw, the record finder's lists beside it: split it by d
    if (s->extract.defer) // (paired reads: kr_batch_extract_pair splits it, by the pair's verdict)
      s->batch.extract_deferred = true;
    else {
      if (int rc = extract_queue(s, st)) return rc;
      s->batch.extract = true;
    }
  }
  HIP_TRY(chain.close(st));
  HIP_TRY(hipGetLastError());
  return KR_OK;
}

// (the arguments were checked by the caller: submit_batch, or the raw-bytes submits behind their record finder)
static int seek_submit(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags, const BatchOrigin& from)
{
  HIP_TRY(hipSetDevice(s->ix->device));
  (void)hipGetLastError(); // a stale error of an earlier, unrelated call on this thread is not this batch's
  if (int rc = drain_batch(s)) return rc;
  Batch& b = begin_batch(s, bases, offsets, nreads, flags, from);
  b.seek = true, b.nlanes = 1;
  if (int rc = seek_queue(s, bases, offsets, nreads, flags)) return fail_submit(s, rc, 1);
  return KR_OK;
}

static int seek_wait(kr_stream* s)
{
  HIP_TRY(hipSetDevice(s->ix->device));
  HIP_TRY(hipStreamSynchronize(s->lanes[0].stream));
  s->batch.waited = true;
  return KR_OK;
}

extern "C" {

int kr_stream_seek_enable(kr_stream* s, uint64_t max_text_bytes, uint64_t max_id_bytes)
{
  kr::clear_error();
  if (!s || (max_text_bytes == 0) != (max_id_bytes == 0)) return kr::fail(KR_ERR_ARG, "kr_stream_seek_enable: bad argument (text and id bytes: both or neither)");
  if (!seek_is_sketch(s->ix)) return kr::fail(KR_ERR_ARG, "kr_stream_seek_enable: not a sketch index");
  if (s->seek.on) return kr::fail(KR_ERR_STATE, "kr_stream_seek_enable: already enabled");
  if (max_id_bytes >= (1ull << 32)) return kr::fail(KR_ERR_ARG, "kr_stream_seek_enable: the ids of one batch must stay below 4 GB");
  if (max_text_bytes && s->text.on && (max_text_bytes > s->text.text_cap || max_id_bytes > s->text.id_cap))
    return kr::fail(KR_ERR_STATE, "kr_stream_seek_enable: the stream's text buffers (kr_stream_text_enable) are smaller than asked for");
  HIP_TRY(hipSetDevice(s->ix->device));
  kr_stream::Seek& k = s->seek;
  k.np = s->llh.th + 1;
  const uint64_t nr = s->max_reads;
  int rc = 0;
  if ((rc = salloc(s, &k.d_first, nr + 1)) || (rc = salloc(s, &k.d_bsum, nr / kRowBlock + 2)) || (rc = salloc(s, &k.d_cnt, nr * (2u * k.np + 1u))) ||
      (rc = salloc(s, &k.d_d, 3 * nr)) || (rc = halloc(s, &k.h_cnt, nr * (2u * k.np + 1u))) || (rc = halloc(s, &k.h_d, 3 * nr)))
    return rc;
  for (auto& e : k.ev) HIP_TRY(hipEventCreate(&e));
  if (max_text_bytes && !s->text.on) {
    if ((rc = text_buffers(s, max_text_bytes, max_id_bytes))) return rc;
    s->text.seek_only = true;
  }
  k.on = true;
  return KR_OK;
}

int kr_batch_collect_seek(kr_stream* s, kr_seek_view* out)
{
  kr::clear_error();
  if (!s || !out) return kr::fail(KR_ERR_ARG, "kr_batch_collect_seek: null argument");
  if (!s->seek.on) return kr::fail(KR_ERR_STATE, "kr_batch_collect_seek: kr_stream_seek_enable first");
  if (!s->batch.submitted || !s->batch.seek) return kr::fail(KR_ERR_STATE, "kr_batch_collect_seek: the last batch was not submitted with KR_SEEK");
  const int rc = kr_batch_wait(s);
  if (rc) return rc;
  kr_stream::Seek& k = s->seek;
  const uint64_t n = s->batch.nreads;
  if (!s->batch.seek_view) {
    HIP_TRY(hipSetDevice(s->ix->device));
    hipStream_t st = s->lanes[0].stream;
    HIP_TRY(hipMemcpyAsync(k.h_cnt, k.d_cnt, n * (2u * k.np + 1u) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(k.h_d, k.d_d, 3 * n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    s->batch.seek_view = true;
  }
  out->nreads = s->batch.nreads, out->np = k.np;
  out->d = k.h_d, out->d_strand = k.h_d + n;
  out->hist = k.h_cnt, out->onmers = k.h_cnt + n * 2u * k.np;
  s->batch.collected = true;
  return KR_OK;
}

int kr_debug_seek_layout(uint32_t* out4)
{
  kr::clear_error();
  if (!out4) return kr::fail(KR_ERR_ARG, "kr_debug_seek_layout: null argument");
  out4[0] = kSeekUnit, out4[1] = kSegPos, out4[2] = kSeekHistWaves, out4[3] = kRowBlock;
  return KR_OK;
}

int kr_debug_seek_ms(kr_stream* s, float* ms3)
{
  kr::clear_error();
  if (!s || !ms3) return kr::fail(KR_ERR_ARG, "kr_debug_seek_ms: null argument");
  if (!s->seek.on || !s->seek.timed) return kr::fail(KR_ERR_STATE, "kr_debug_seek_ms: no seek batch on this stream yet");
  HIP_TRY(hipSetDevice(s->ix->device));
  kr_stream::Seek& k = s->seek;
  HIP_TRY(hipEventSynchronize(k.ev[3]));
  for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms3[i], k.ev[i], k.ev[i + 1]));
  return KR_OK;
}

} // extern "C"
