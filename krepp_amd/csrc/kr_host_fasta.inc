// kr_host_fasta.inc -- part of kr_device.hip (host side): kr_batch_submit_fasta.
// A batch given as the raw bytes of a plain FASTA file; the records are found by the kernels of kr_dev_fasta.inc, then the accepted
// prefix is queued exactly as kr_batch_submit_fastq queues its own (fq_begin / fq_finish, kr_host_fastq.inc), and
// kr_batch_fastq_names / kr_debug_fastq_batch serve it unchanged.  (kr_fasta_chunk_cut needs no device: kr_host.cpp.)

namespace {

// kr_batch_submit_fasta; with hooks: the same for bytes that a kernel writes into d_raw (kr_batch_submit_bgzf)
int submit_fasta(kr_stream* s, const char* fn, const uint8_t* raw, uint64_t nbytes, uint32_t flags, uint32_t closed, kr_fastq_parse* out,
                 const FqHooks* hooks)
{
  FaIO io;
  bool text = false;
  int rc = fq_begin(s, fn, raw, nbytes, flags, closed, out, io.q, text, hooks);
  if (rc || nbytes == 0) return rc;
  kr_stream::Fastq& f = s->fq;
  if (!f.fa_on) { // what only FASTA needs, on the stream's first FASTA chunk (after a failed attempt: the buffers still missing)
    const uint64_t ntiles = (f.raw_cap + kFqTile - 1) / kFqTile + 1, nr = s->max_reads;
    auto need = [&](uint32_t** p, uint64_t n) { return *p ? KR_OK : salloc(s, p, n); };
    if ((rc = need(&f.d_tile_st, ntiles)) || (rc = need(&f.d_tile_gr, ntiles)) || (rc = need(&f.d_hs, nr + 2)) || (rc = need(&f.d_ga, nr + 2)) ||
        (rc = need(&f.d_hg, nr)) || (rc = need(&f.d_he, nr)))
      return rc;
    f.fa_on = true;
  }
  hipStream_t st = s->lanes[0].stream;
  io.tile_st = f.d_tile_st, io.tile_gr = f.d_tile_gr, io.hs = f.d_hs, io.ga = f.d_ga, io.rec_hg = f.d_hg, io.rec_he = f.d_he;
  io.closed = closed ? 1u : 0u;
  f.last_fasta = true;
  const uint32_t tgrid = std::min<uint32_t>((uint32_t)((nbytes + kFqTile - 1) / kFqTile), 16384u);
  const uint32_t rgrid = std::min<uint32_t>((s->max_reads + 3) / 4, 8192u), bgrid = std::min<uint32_t>(s->max_reads / kFqRecBlock + 1, 4096u);
  if ((rc = fq_mark(s))) return rc;
  hipLaunchKernelGGL(kr_fa_count_kernel, dim3(tgrid), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fa_scan_kernel, dim3(1), dim3(1024), 0, st, io);
  hipLaunchKernelGGL(kr_fa_write_kernel, dim3(tgrid), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fa_rec_kernel, dim3(rgrid), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fa_check_kernel, dim3(tgrid), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_fq_bsum_kernel, dim3(bgrid), dim3(256), 0, st, io.q);
  hipLaunchKernelGGL(kr_fq_bscan_kernel, dim3(1), dim3(1024), 0, st, io.q);
  hipLaunchKernelGGL(kr_fq_off_kernel, dim3(bgrid), dim3(256), 0, st, io.q);
  hipLaunchKernelGGL(kr_fa_copy_kernel, dim3(std::max(tgrid, std::min(rgrid, 1024u))), dim3(256), 0, st, io);
  return fq_finish(s, flags, closed, text, out, hooks);
}

} // namespace

extern "C" {

int kr_batch_submit_fasta(kr_stream* s, const uint8_t* raw, uint64_t nbytes, uint32_t flags, uint32_t closed, kr_fastq_parse* out)
{
  kr::clear_error();
  return submit_fasta(s, "kr_batch_submit_fasta", raw, nbytes, flags, closed, out, nullptr);
}

} // extern "C"
