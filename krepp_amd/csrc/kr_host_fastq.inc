// kr_host_fastq.inc -- part of kr_device.hip (host side): kr_stream_fastq_enable, kr_batch_submit_fastq, kr_batch_fastq_names.
// A batch given as the raw bytes of a plain FASTQ file; the records are found by the kernels of kr_dev_fastq.inc, then the batch
// runs on the submit_batch path with its bases already in HBM (with KR_TILE_DEVICE: long records too, tiled by build_tiles_device;
// with KR_TILE_ROWS as well, such a batch's rows and text are the device's: submit_batch reads the flag, the ids are in HBM already).
// kr_batch_submit_fasta (kr_host_fasta.inc) shares everything but the record finder's kernels: fq_begin / fq_finish.

namespace {

// What kr_batch_submit_fastq and kr_batch_submit_fasta (kr_host_fasta.inc) share.  fq_begin: the argument checks, the wait for the
// batch in flight, the kernels' arguments that do not depend on the format, and the chunk's copy to d_raw; nbytes == 0 is accepted
// here (nothing is queued: the caller returns).  fq_finish: the wait for the summary, and the accepted prefix queued as a batch.
// FqHooks (kr_batch_submit_bgzf, kr_host_bgzf.inc): `fill` queues what writes the chunk into d_raw in place of the copy, `check`
// runs behind the wait for the summary and in front of the queueing -- when it fails nothing is queued.
struct FqHooks {
  int (*fill)(kr_stream*, hipStream_t, void*);
  int (*check)(kr_stream*, void*);
  void* arg;
};

int fq_begin(kr_stream* s, const char* fn, const uint8_t* raw, uint64_t nbytes, uint32_t flags, uint32_t at_eof, kr_fastq_parse* out, FqIO& io,
             bool& text, const FqHooks* hooks = nullptr)
{
  const std::string who = std::string(fn) + ": ";
  if (!s || !raw || !out) return kr::fail(KR_ERR_ARG, who + "null argument");
  if (nbytes >= (1ull << 32)) return kr::fail(KR_ERR_ARG, who + "a chunk must stay below 4 GB (positions are 32-bit)");
  if (!s->fq.on) return kr::fail(KR_ERR_STATE, who + "kr_stream_fastq_enable first");
  if (nbytes > s->fq.raw_cap) return kr::fail(KR_ERR_ARG, who + "more bytes than kr_stream_fastq_enable sized the stream for");
  if (flags & (KR_BASES_DEVICE | KR_BASES_PINNED)) return kr::fail(KR_ERR_ARG, who + "the bases are the record finder's: no KR_BASES_* flags");
  if (flags & KR_SEEK) // (a seek batch: with KR_TILE_DEVICE long records are accepted and the seek units do the splitting)
    if (int rc = seek_check(s, flags, true, fn)) return rc;
  memset(out, 0, sizeof(*out));
  out->at_eof = at_eof ? 1u : 0u;
  kr_stream::Fastq& f = s->fq;
  if (nbytes == 0) { // (a parse of no record: the batch in flight stays as it is)
    s->parse = LastParse{true, false, 0};
    return KR_OK;
  }
  text = s->text.on && !(flags & (KR_TAP_ACCS | KR_TAP_HITS)) && ((flags & KR_SEEK) || !s->text.seek_only);
  HIP_TRY(hipSetDevice(s->ix->device));
  (void)hipGetLastError();
  if (int rc = drain_batch(s)) return rc; // d_bases, d_offsets and the ids belong to the batch in flight
  s->parse = LastParse{}; // (d_raw is overwritten: the last parse's names are gone)
  hipStream_t st = s->lanes[0].stream; // (the lane of a device-input batch: the parse and the batch are ordered on it)
  io.raw = f.d_raw, io.nbytes = nbytes;
  io.tile_nl = f.d_tile_nl, io.nl = nullptr, io.nl_cap = 0, io.rec_lines = 0;
  io.rec_slen = f.d_slen, io.rec_npos = f.d_npos, io.rec_nlen = f.d_nlen;
  io.bsum_b = f.d_bsum_b, io.bsum_n = f.d_bsum_n, io.ctl = f.d_ctl;
  io.bases = s->d_bases, io.offsets = s->d_offsets;
  io.ids = text ? s->text.d_ids : nullptr;
  io.id_off = text ? s->text.d_id_off : f.d_id_off;
  io.max_reads = s->max_reads, io.max_bases = s->max_bases, io.id_cap = text ? s->text.id_cap : ~0ull;
  // KR_TILE_DEVICE: a long record is accepted like any other (no k-mer count exceeds the bound) and tiled on the device below
  io.k = s->ix->dix.k, io.tile_min_pos = (flags & KR_TILE_DEVICE) ? 0xFFFFFFFFu : s->tile_min_pos;
  io.sum = f.d_sum;
  // queued before the index's kernel chain is waited for (launch_lane): the copy and the parse overlap other streams' batches
  if (hooks) {
    if (int rc = hooks->fill(s, st, hooks->arg)) return rc;
  } else
    HIP_TRY(hipMemcpyAsync(f.d_raw, raw, nbytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(f.d_ctl, 0xFF, 32, st));
  return KR_OK;
}

// in front of the record finder's first kernel: where kr_debug_fastq_parse_ms, once asked, starts the kernels' time
int fq_mark(kr_stream* s)
{
  if (s->fq.ev_parse0) HIP_TRY(hipEventRecord(s->fq.ev_parse0, s->lanes[0].stream));
  return KR_OK;
}

int fq_finish(kr_stream* s, uint32_t flags, uint32_t at_eof, bool text, kr_fastq_parse* out, const FqHooks* hooks = nullptr)
{
  kr_stream::Fastq& f = s->fq;
  hipStream_t st = s->lanes[0].stream;
  HIP_TRY(hipGetLastError());
  if (f.ev_parse0) {
    HIP_TRY(hipEventRecord(f.ev_parse1, st));
    f.ev_set = true;
  }
  HIP_TRY(hipMemcpyAsync(f.h_sum, f.d_sum, sizeof(kr_fastq_parse), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (hooks)
    if (int rc = hooks->check(s, hooks->arg)) return rc; // (parse.parsed stays false: the stream serves the next submit)
  *out = *f.h_sum;
  out->at_eof = at_eof ? 1u : 0u;
  s->parse = LastParse{true, false, out->nreads};
  if (out->nreads == 0) return KR_OK; // (nothing to queue: the batch in flight stays as it is)
  BatchOrigin from;
  from.parsed = true;
  if (text) from.ids = kIdsDevice, from.id_bytes = out->id_bytes; // (the record finder wrote them into text.d_ids / d_id_off)
  if (flags & KR_SEEK) // no dist tile layout: the batch as the record finder left it
    return seek_submit(s, s->d_bases, s->d_offsets, out->nreads, KR_SEEK | KR_BASES_DEVICE, from);
  return submit_batch(s, s->d_bases, s->d_offsets, out->nreads, flags | KR_BASES_DEVICE | (text ? KR_ROWS_ONLY : 0u), from);
}

// kr_batch_submit_fastq; with hooks: the same for bytes that a kernel writes into d_raw (`raw` is then only checked for NULL)
int submit_fastq(kr_stream* s, const char* fn, const uint8_t* raw, uint64_t nbytes, uint32_t flags, uint32_t at_eof, kr_fastq_parse* out,
                 const FqHooks* hooks)
{
  FqIO io;
  bool text = false;
  int rc = fq_begin(s, fn, raw, nbytes, flags, at_eof, out, io, text, hooks);
  if (rc || nbytes == 0) return rc;
  kr_stream::Fastq& f = s->fq;
  hipStream_t st = s->lanes[0].stream;
  io.nl = f.d_nl, io.nl_cap = 4u * s->max_reads, io.rec_lines = 4;
  f.last_fasta = false;
  const uint32_t ntiles = (uint32_t)((nbytes + kFqTile - 1) / kFqTile);
  const uint32_t rgrid = std::min<uint32_t>((s->max_reads + 3) / 4, 8192u), bgrid = std::min<uint32_t>(s->max_reads / kFqRecBlock + 1, 4096u);
  if ((rc = fq_mark(s))) return rc;
  hipLaunchKernelGGL(kr_fq_nl_count_kernel, dim3(std::min<uint32_t>(ntiles, 16384u)), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fq_nl_scan_kernel, dim3(1), dim3(1024), 0, st, io);
  hipLaunchKernelGGL(kr_fq_nl_write_kernel, dim3(std::min<uint32_t>(ntiles, 16384u)), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fq_rec_kernel, dim3(rgrid), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fq_bsum_kernel, dim3(bgrid), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fq_bscan_kernel, dim3(1), dim3(1024), 0, st, io);
  hipLaunchKernelGGL(kr_fq_off_kernel, dim3(bgrid), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fq_copy_kernel, dim3(rgrid), dim3(256), 0, st, io);
  return fq_finish(s, flags, at_eof, text, out, hooks);
}

} // namespace

extern "C" {

int kr_stream_fastq_enable(kr_stream* s, uint64_t max_raw_bytes)
{
  kr::clear_error();
  if (!s || max_raw_bytes == 0) return kr::fail(KR_ERR_ARG, "kr_stream_fastq_enable: bad argument");
  if (max_raw_bytes >= (1ull << 32)) return kr::fail(KR_ERR_ARG, "kr_stream_fastq_enable: a chunk must stay below 4 GB (positions are 32-bit)");
  if (s->fq.on) return kr::fail(KR_ERR_STATE, "kr_stream_fastq_enable: already enabled");
  if (s->max_reads > (1u << 30)) return kr::fail(KR_ERR_ARG, "kr_stream_fastq_enable: more than 2^30 reads per batch (the newline list is indexed by 32 bits)");
  HIP_TRY(hipSetDevice(s->ix->device));
  kr_stream::Fastq& f = s->fq;
  const uint64_t raw_pad = ((max_raw_bytes + 15) & ~15ull) + 16; // (16-byte loads of the last bytes stay inside)
  const uint64_t ntiles = (max_raw_bytes + kFqTile - 1) / kFqTile + 1, nblk = (uint64_t)s->max_reads / kFqRecBlock + 2;
  int rc = 0;
  if ((rc = salloc(s, &f.d_raw, raw_pad)) || (rc = salloc(s, &f.d_tile_nl, ntiles)) || (rc = salloc(s, &f.d_nl, 4ull * s->max_reads)) ||
      (rc = salloc(s, &f.d_slen, (uint64_t)s->max_reads)) || (rc = salloc(s, &f.d_npos, (uint64_t)s->max_reads)) ||
      (rc = salloc(s, &f.d_nlen, (uint64_t)s->max_reads)) || (rc = salloc(s, &f.d_id_off, (uint64_t)s->max_reads + 1)) ||
      (rc = salloc(s, &f.d_bsum_b, nblk)) || (rc = salloc(s, &f.d_bsum_n, nblk)) || (rc = salloc(s, &f.d_ctl, 4)) ||
      (rc = salloc(s, &f.d_sum, 1)) || (rc = halloc(s, &f.h_sum, 1)))
    return rc;
  f.raw_cap = max_raw_bytes;
  f.on = true;
  return KR_OK;
}

int kr_batch_submit_fastq(kr_stream* s, const uint8_t* raw, uint64_t nbytes, uint32_t flags, uint32_t at_eof, kr_fastq_parse* out)
{
  kr::clear_error();
  return submit_fastq(s, "kr_batch_submit_fastq", raw, nbytes, flags, at_eof, out, nullptr);
}

int kr_batch_fastq_names(kr_stream* s, const uint64_t** name_pos, const uint32_t** name_len)
{
  kr::clear_error();
  if (!s || !name_pos || !name_len) return kr::fail(KR_ERR_ARG, "kr_batch_fastq_names: null argument");
  if (!s->fq.on || !s->parse.parsed) return kr::fail(KR_ERR_STATE, "kr_batch_fastq_names: the last submit was not kr_batch_submit_fastq");
  kr_stream::Fastq& f = s->fq;
  const uint32_t n = s->parse.nreads;
  if (!s->parse.have_names && n) {
    HIP_TRY(hipSetDevice(s->ix->device));
    if (!f.h_npos) { // page-locked mirrors, made on first use
      int rc = 0;
      if ((rc = halloc(s, &f.h_npos, (uint64_t)s->max_reads)) || (rc = halloc(s, &f.h_nlen, (uint64_t)s->max_reads))) return rc;
    }
    hipStream_t st = s->lanes[0].stream;
    HIP_TRY(hipMemcpyAsync(f.h_npos, f.d_npos, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(f.h_nlen, f.d_nlen, (uint64_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    f.name_pos.assign(f.h_npos, f.h_npos + n);
  }
  if (!n) f.name_pos.clear();
  s->parse.have_names = true;
  *name_pos = f.name_pos.data();
  *name_len = f.h_nlen;
  return KR_OK;
}

// (tests) the bases and offsets the record finder wrote for the last kr_batch_submit_fastq: offsets [nreads + 1], bases [nbases]
int kr_debug_fastq_batch(kr_stream* s, uint8_t* bases, uint64_t* offsets)
{
  kr::clear_error();
  if (!s || !bases || !offsets) return kr::fail(KR_ERR_ARG, "kr_debug_fastq_batch: null argument");
  if (!s->fq.on || !s->parse.parsed) return kr::fail(KR_ERR_STATE, "kr_debug_fastq_batch: the last submit was not kr_batch_submit_fastq");
  const uint32_t n = s->parse.nreads;
  offsets[0] = 0;
  if (!n) return KR_OK;
  HIP_TRY(hipSetDevice(s->ix->device));
  hipStream_t st = s->lanes[0].stream;
  HIP_TRY(hipMemcpyAsync(offsets, s->d_offsets, ((uint64_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (offsets[n]) HIP_TRY(hipMemcpyAsync(bases, s->d_bases, offsets[n], hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return KR_OK;
}

// (measurements) the device time of the record finder's kernels in the stream's last kr_batch_submit_fastq / _fasta, behind the
// chunk's copy and in front of the summary's.  The first call makes the events and gives *ms = -1: the next parse is the first measured.
int kr_debug_fastq_parse_ms(kr_stream* s, float* ms)
{
  kr::clear_error();
  if (!s || !ms) return kr::fail(KR_ERR_ARG, "kr_debug_fastq_parse_ms: null argument");
  if (!s->fq.on) return kr::fail(KR_ERR_STATE, "kr_debug_fastq_parse_ms: kr_stream_fastq_enable first");
  kr_stream::Fastq& f = s->fq;
  *ms = -1.0f;
  HIP_TRY(hipSetDevice(s->ix->device));
  if (!f.ev_parse0) {
    HIP_TRY(hipEventCreate(&f.ev_parse0));
    HIP_TRY(hipEventCreate(&f.ev_parse1));
    return KR_OK;
  }
  if (!f.ev_set) return KR_OK;
  HIP_TRY(hipEventSynchronize(f.ev_parse1));
  HIP_TRY(hipEventElapsedTime(ms, f.ev_parse0, f.ev_parse1));
  return KR_OK;
}

} // extern "C"
