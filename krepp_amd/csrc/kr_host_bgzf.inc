// kr_host_bgzf.inc -- part of kr_device.hip (host side): kr_stream_bgzf_enable, kr_batch_submit_bgzf, kr_debug_bgzf_inflate, kr_debug_bgzf_ms.
// A batch given as the WHOLE MEMBERS of a block-gzipped FASTQ / FASTA file: the host walks the members' headers and trailers, the
// kernel of kr_dev_bgzf.inc inflates them into the stream's d_raw in place of the chunk's copy, and from there on the submit is
// kr_batch_submit_fastq / _fasta (submit_fastq / submit_fasta with hooks: kr_host_fastq.inc).

namespace {

// The member table of comp[0 .. ncomp) in b.h_tab.  The chunk is bytes [skip, skip + nbytes) of the members' inflated bytes
// (whole: all of them, *nbytes is set).  Every bound the kernel relies on is checked here.
int bgzf_table(kr_stream* s, const uint8_t* comp, uint64_t ncomp, uint32_t skip, uint64_t* nbytes, bool whole, uint32_t* nmembers, uint64_t* total)
{
  kr_stream::Bgzf& b = s->bgzf;
  if (ncomp > b.comp_cap) return kr::fail(KR_ERR_ARG, "bgzf: more compressed bytes than kr_stream_bgzf_enable sized the stream for");
  b.member_off.clear();
  uint64_t off = 0, U = 0;
  uint32_t k = 0;
  while (off < ncomp) {
    kr::BgzfMember m;
    uint32_t ms = 0;
    if (const char* why = kr::bgzf_member_at(comp, ncomp, off, &m, &ms))
      return kr::fail(KR_ERR_FORMAT, "bgzf: BGZF member at offset " + std::to_string(off) + ": " + why);
    if (k >= b.max_members) return kr::fail(KR_ERR_ARG, "bgzf: more members than the table holds"); // (cannot be: a member has 28 bytes at least)
    m.out_pos = (int64_t)U - (int64_t)skip;
    b.h_tab[k++] = m;
    b.member_off.push_back(off);
    U += m.isize, off += ms;
  }
  if (whole) *nbytes = U;
  if (k && skip && skip >= b.h_tab[0].isize) return kr::fail(KR_ERR_ARG, "bgzf: skip must lie inside the first member");
  if ((uint64_t)skip + *nbytes > U) return kr::fail(KR_ERR_ARG, "bgzf: the chunk reaches past the members' inflated bytes");
  if (*nbytes > s->fq.raw_cap) return kr::fail(KR_ERR_ARG, "bgzf: more bytes than kr_stream_fastq_enable sized the stream for");
  for (uint32_t i = 0; i < k; ++i) { // only the first and the last member may reach outside the chunk: they go through a scratch window
    kr::BgzfMember& m = b.h_tab[i];
    const bool inside = m.out_pos >= 0 && (uint64_t)m.out_pos + m.isize <= *nbytes;
    if (inside) continue;
    if (i == 0) m.window = 1;
    else if (i + 1 == k) m.window = 2;
    else return kr::fail(KR_ERR_ARG, "bgzf: only the first and the last member may reach outside the chunk (member at offset " + std::to_string(b.member_off[i]) + ")");
  }
  *nmembers = k, *total = U;
  return KR_OK;
}

// The copies and the kernel, queued on st: comp and the table to the device, the members inflated into d_raw
int bgzf_queue(kr_stream* s, hipStream_t st, const uint8_t* comp, uint64_t ncomp, uint32_t nmembers, uint64_t nbytes)
{
  kr_stream::Bgzf& b = s->bgzf;
  HIP_TRY(hipMemsetAsync(b.d_sum, 0, sizeof(BgzfSum), st));
  HIP_TRY(hipMemsetAsync(&b.d_sum->first_bad, 0xFF, 4, st));
  if (nmembers) {
    HIP_TRY(hipMemcpyAsync(b.d_comp, comp, ncomp, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.d_tab, b.h_tab, (uint64_t)nmembers * sizeof(kr::BgzfMember), hipMemcpyHostToDevice, st));
  }
  if (b.ev0) HIP_TRY(hipEventRecord(b.ev0, st));
  if (nmembers) {
    BgzfIO io{b.d_comp, b.d_tab, nmembers, s->fq.d_raw, nbytes, b.d_scratch, b.d_status, b.d_sum};
    hipLaunchKernelGGL(kr_bgzf_inflate_kernel, dim3((nmembers + 3) / 4), dim3(256), 0, st, io);
    HIP_TRY(hipGetLastError());
  }
  if (b.ev0) {
    HIP_TRY(hipEventRecord(b.ev1, st));
    b.ev_set = true;
  }
  HIP_TRY(hipMemcpyAsync(b.h_sum, b.d_sum, sizeof(BgzfSum), hipMemcpyDeviceToHost, st));
  return KR_OK;
}

// behind the wait: the kernel's summary; the first member that broke a rule is named with its offset in comp
int bgzf_verdict(kr_stream* s, uint32_t nmembers)
{
  kr_stream::Bgzf& b = s->bgzf;
  if (b.h_sum->first_bad == 0xFFFFFFFFu && b.h_sum->done == nmembers) return KR_OK;
  const uint32_t m = b.h_sum->first_bad;
  if (m >= nmembers) return kr::fail(KR_ERR_NO_DEVICE, "bgzf: the inflate kernel finished " + std::to_string(b.h_sum->done) + " of " + std::to_string(nmembers) + " members");
  uint32_t status = 0;
  HIP_TRY(hipMemcpy(&status, b.d_status + m, 4, hipMemcpyDeviceToHost));
  return kr::fail(KR_ERR_FORMAT, kr::bgzf_member_message("bgzf", b.member_off[m], status >> 24, status & 0xFFFFFFu));
}

struct BgzfSubmit {
  const uint8_t* comp;
  uint64_t ncomp, nbytes;
  uint32_t nmembers;
  uint8_t* raw_out;
};
int bgzf_fill(kr_stream* s, hipStream_t st, void* arg)
{
  const BgzfSubmit& a = *(const BgzfSubmit*)arg;
  if (int rc = bgzf_queue(s, st, a.comp, a.ncomp, a.nmembers, a.nbytes)) return rc;
  if (a.raw_out) HIP_TRY(hipMemcpyAsync(a.raw_out, s->fq.d_raw, a.nbytes, hipMemcpyDeviceToHost, st));
  return KR_OK;
}
int bgzf_check(kr_stream* s, void* arg) { return bgzf_verdict(s, ((const BgzfSubmit*)arg)->nmembers); }

} // namespace

extern "C" {

int kr_stream_bgzf_enable(kr_stream* s, uint64_t max_comp_bytes)
{
  kr::clear_error();
  if (!s || max_comp_bytes == 0) return kr::fail(KR_ERR_ARG, "kr_stream_bgzf_enable: bad argument");
  if (max_comp_bytes >= (1ull << 32)) return kr::fail(KR_ERR_ARG, "kr_stream_bgzf_enable: a chunk must stay below 4 GB (positions are 32-bit)");
  if (!s->fq.on) return kr::fail(KR_ERR_STATE, "kr_stream_bgzf_enable: kr_stream_fastq_enable first");
  if (s->bgzf.on) return kr::fail(KR_ERR_STATE, "kr_stream_bgzf_enable: already enabled");
  HIP_TRY(hipSetDevice(s->ix->device));
  kr_stream::Bgzf& b = s->bgzf;
  const uint64_t nm = max_comp_bytes / 28 + 1; // a member has 18 bytes of header, 2 of payload and 8 of trailer at least
  int rc = 0;
  if ((rc = salloc(s, &b.d_comp, max_comp_bytes + 16)) || (rc = salloc(s, &b.d_scratch, 2ull * kr::kBgzfMaxIsize)) || (rc = salloc(s, &b.d_tab, nm)) ||
      (rc = halloc(s, &b.h_tab, nm)) || (rc = salloc(s, &b.d_status, nm)) || (rc = salloc(s, &b.d_sum, 1)) || (rc = halloc(s, &b.h_sum, 1)))
    return rc;
  b.comp_cap = max_comp_bytes, b.max_members = (uint32_t)nm;
  b.on = true;
  return KR_OK;
}

int kr_batch_submit_bgzf(kr_stream* s, const uint8_t* comp, uint64_t ncomp, uint32_t skip, uint64_t nbytes, uint8_t* raw_out, uint32_t flags,
                         uint32_t fasta, uint32_t at_eof_or_closed, kr_fastq_parse* out)
{
  kr::clear_error();
  if (!s || !comp || !out) return kr::fail(KR_ERR_ARG, "kr_batch_submit_bgzf: null argument");
  if (!s->bgzf.on) return kr::fail(KR_ERR_STATE, "kr_batch_submit_bgzf: kr_stream_bgzf_enable first");
  BgzfSubmit a{comp, ncomp, nbytes, 0, raw_out};
  uint64_t total = 0;
  if (int rc = bgzf_table(s, comp, ncomp, skip, &a.nbytes, false, &a.nmembers, &total)) return rc;
  const FqHooks hooks{bgzf_fill, bgzf_check, &a};
  return fasta ? submit_fasta(s, "kr_batch_submit_bgzf", comp, nbytes, flags, at_eof_or_closed, out, &hooks)
               : submit_fastq(s, "kr_batch_submit_bgzf", comp, nbytes, flags, at_eof_or_closed, out, &hooks);
}

// (tests) the kernel alone: every member of comp inflated, all their bytes back
int kr_debug_bgzf_inflate(kr_stream* s, const uint8_t* comp, uint64_t ncomp, uint8_t* out, uint64_t cap, uint64_t* len)
{
  kr::clear_error();
  if (!s || !comp || !out || !len) return kr::fail(KR_ERR_ARG, "bgzf: null argument");
  *len = 0;
  if (!s->bgzf.on) return kr::fail(KR_ERR_STATE, "kr_debug_bgzf_inflate: kr_stream_bgzf_enable first");
  uint64_t nbytes = 0, total = 0;
  uint32_t nm = 0;
  if (int rc = bgzf_table(s, comp, ncomp, 0, &nbytes, true, &nm, &total)) return rc;
  if (nbytes > cap) return kr::fail(KR_ERR_ARG, "bgzf: the members inflate to more bytes than the buffer holds");
  HIP_TRY(hipSetDevice(s->ix->device));
  (void)hipGetLastError();
  if (int rc = drain_batch(s)) return rc; // d_raw may still be read by the batch in flight
  s->parse = LastParse{}; // (... and is overwritten: the last parse's names are gone)
  hipStream_t st = s->lanes[0].stream;
  if (int rc = bgzf_queue(s, st, comp, ncomp, nm, nbytes)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (int rc = bgzf_verdict(s, nm)) return rc;
  if (nbytes) HIP_TRY(hipMemcpy(out, s->fq.d_raw, nbytes, hipMemcpyDeviceToHost));
  *len = nbytes;
  return KR_OK;
}

// (measurements) the device time of the inflate kernel in the stream's last kr_batch_submit_bgzf / kr_debug_bgzf_inflate.  The first
// call makes the events and gives *ms = -1: the next chunk is the first measured (as kr_debug_fastq_parse_ms).
int kr_debug_bgzf_ms(kr_stream* s, float* ms)
{
  kr::clear_error();
  if (!s || !ms) return kr::fail(KR_ERR_ARG, "kr_debug_bgzf_ms: null argument");
  if (!s->bgzf.on) return kr::fail(KR_ERR_STATE, "kr_debug_bgzf_ms: kr_stream_bgzf_enable first");
  kr_stream::Bgzf& b = s->bgzf;
  *ms = -1.0f;
  HIP_TRY(hipSetDevice(s->ix->device));
  if (!b.ev0) {
    HIP_TRY(hipEventCreate(&b.ev0));
    HIP_TRY(hipEventCreate(&b.ev1));
    return KR_OK;
  }
  if (!b.ev_set) return KR_OK;
  HIP_TRY(hipEventSynchronize(b.ev1));
  HIP_TRY(hipEventElapsedTime(ms, b.ev0, b.ev1));
  return KR_OK;
}

} // extern "C"
