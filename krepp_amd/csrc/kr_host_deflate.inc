// kr_host_deflate.inc -- part of kr_device.hip (host side): kr_stream_bgzf_out_enable, kr_stream_bgzf_out_level,
// kr_stream_bgzf_member, kr_stream_place_bgzf, kr_batch_collect_text_bgzf, kr_debug_bgzf_deflate, kr_debug_bgzf_deflate_at,
// kr_debug_bgzf_deflate_ms, kr_debug_huffman_lengths_device.  Report text that lies in device memory is deflated into BGZF members
// there (kernels: kr_dev_deflate.inc, encoder: kr_deflate.h) and only the members cross to the host.  kr::place_text_deflate is
// the same for a range of `place` rows (kr_host_place.inc: place_device_finish).

namespace {

// Room for the members of n text bytes at the stream's member length and level.  Every buffer is in hand before the first kernel
// is queued.
int deflate_reserve(kr_stream* s, uint64_t n)
{
  kr_stream::BgzfOut& o = s->bgzf_out;
  const uint64_t nm = kr::bgzf_deflate_members(n, o.member_in);
  if (!o.d_slots.reserve(nm * kr::bgzf_slot_stride(o.member_in)) || !o.d_off.reserve(nm + 1) || !o.d_out.reserve(kr::bgzf_deflate_bound(n, o.member_in)) || !o.h_total.reserve(1))
    return alloc_failed("bgzf out: device buffers");
  if (o.level == 2 && !o.d_tokens.reserve(nm * o.member_in)) return alloc_failed("bgzf out: the token buffer of level 2");
  return KR_OK;
}

// d_text[0 .. n), n > 0, deflated on st; behind the wait *total is the members' bytes, back to back in d_out
int deflate_run(kr_stream* s, hipStream_t st, const uint8_t* d_text, uint64_t n, uint64_t* total)
{
  kr_stream::BgzfOut& o = s->bgzf_out;
  const uint64_t nm = kr::bgzf_deflate_members(n, o.member_in);
  // (a grid dimension and scan_block_sums' count; at the least member length, 256, that is half a terabyte of text)
  if (nm >= (1ull << 31)) return kr::fail(KR_ERR_ARG, "bgzf out: too many members");
  DeflateIO io{d_text, n, (uint32_t)nm, o.d_slots.get(), o.d_off.get(), o.d_out.get(), o.member_in, kr::bgzf_slot_stride(o.member_in)};
  if (o.ev0) HIP_TRY(hipEventRecord(o.ev0, st));
  if (o.level == 2) hipLaunchKernelGGL(kr_bgzf_deflate_dyn_kernel, dim3((uint32_t)((nm + 3) / 4)), dim3(256), 0, st, io, o.d_tokens.get());
  else hipLaunchKernelGGL(kr_bgzf_deflate_kernel, dim3((uint32_t)((nm + 3) / 4)), dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_bgzf_deflate_scan_kernel, dim3(1), dim3(1024), 0, st, io.off, io.nmembers);
  hipLaunchKernelGGL(kr_bgzf_deflate_copy_kernel, dim3(io.nmembers), dim3(256), 0, st, io);
  HIP_TRY(hipGetLastError());
  if (o.ev0) {
    HIP_TRY(hipEventRecord(o.ev1, st));
    o.ev_set = true;
  }
  HIP_TRY(hipMemcpyAsync(o.h_total.get(), io.off + nm, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *total = *o.h_total.get();
  if (*total < nm * 28 || *total > kr::bgzf_deflate_bound(n, o.member_in)) return kr::fail(KR_ERR_NO_DEVICE, "bgzf out: the deflate kernels left an impossible size");
  return KR_OK;
}

} // namespace

// A range's `place` rows d_text[0 .. n), n > 0, written on lane 0's stream by the text kernels, deflated behind them at the
// stream's place level and member length; the members come back in the stream's page-locked buffer.  The buffers grow with the
// text, with headroom as the place workspace's h_text gets: a place stream has no max_text_bytes to size them by.
int kr::place_text_deflate(kr_stream* s, const uint8_t* d_text, uint64_t n, const char** comp, uint64_t* len)
{
  kr_stream::BgzfOut& o = s->bgzf_out;
  hipStream_t st = s->lanes[0].stream;
  const uint32_t level_before = o.level;
  o.level = o.place_level;
  int rc = KR_OK;
  const uint64_t bound = kr::bgzf_deflate_bound(n, o.member_in), nm = kr::bgzf_deflate_members(n, o.member_in);
  const bool room = nm * kr::bgzf_slot_stride(o.member_in) <= o.d_slots.size() && nm + 1 <= o.d_off.size() && bound <= o.d_out.size() &&
                    o.h_total.size() >= 1 && (o.level != 2 || nm * o.member_in <= o.d_tokens.size());
  if (!room) rc = deflate_reserve(s, n + n / 4 + (1u << 20)); // (nothing of this stream's deflate is in flight: every deflate_run waits)
  if (!rc && bound > o.h_comp.size() && !o.h_comp.reserve(bound + bound / 4 + (1u << 20))) rc = alloc_failed("place: the members' page-locked buffer");
  uint64_t total = 0;
  if (!rc) rc = deflate_run(s, st, d_text, n, &total);
  o.level = level_before;
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(o.h_comp.get(), o.d_out.get(), total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *comp = (const char*)o.h_comp.get(), *len = total;
  return KR_OK;
}
uint32_t kr::place_bgzf_level(const kr_stream* s) { return s ? s->bgzf_out.place_level : 0; }
uint32_t kr::place_bgzf_member(const kr_stream* s) { return s ? s->bgzf_out.member_in : kr::kDefMemberIn; }

extern "C" {

int kr_stream_bgzf_out_enable(kr_stream* s)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_stream_bgzf_out_enable: null argument");
  if (!s->text.on) return kr::fail(KR_ERR_STATE, "kr_stream_bgzf_out_enable: kr_stream_text_enable or kr_stream_seek_enable (with text buffers) first");
  if (s->bgzf_out.on) return kr::fail(KR_ERR_STATE, "kr_stream_bgzf_out_enable: already enabled");
  HIP_TRY(hipSetDevice(s->ix->device));
  if (int rc = deflate_reserve(s, s->text.text_cap)) return rc;
  s->bgzf_out.on = true;
  return KR_OK;
}

int kr_stream_bgzf_out_level(kr_stream* s, uint32_t level)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_stream_bgzf_out_level: null argument");
  if (!s->bgzf_out.on) return kr::fail(KR_ERR_STATE, "kr_stream_bgzf_out_level: kr_stream_bgzf_out_enable first");
  if (level != 1 && level != 2) return kr::fail(KR_ERR_ARG, "kr_stream_bgzf_out_level: level " + std::to_string(level) + " (1: fixed codes, 2: dynamic codes)");
  HIP_TRY(hipSetDevice(s->ix->device));
  const uint32_t before = s->bgzf_out.level;
  s->bgzf_out.level = level;
  if (int rc = deflate_reserve(s, s->text.text_cap)) { // (level 2: the token buffer, in hand before a kernel is queued)
    s->bgzf_out.level = before;
    return rc;
  }
  return KR_OK;
}

int kr_stream_bgzf_member(kr_stream* s, uint32_t member_bytes)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_stream_bgzf_member: null argument");
  if (!kr::bgzf_member_in_ok(member_bytes))
    return kr::fail(KR_ERR_ARG, "kr_stream_bgzf_member: " + std::to_string(member_bytes) + " bytes a member (256 to 65280)");
  kr_stream::BgzfOut& o = s->bgzf_out;
  if (member_bytes == o.member_in) return KR_OK;
  const uint32_t before = o.member_in;
  o.member_in = member_bytes;
  if (o.on) { // (a dist / seek stream: room for max_text_bytes at the new member count, in hand before a kernel is queued; a place
              //  stream's buffers grow with the ranges' text: kr::place_text_deflate)
    HIP_TRY(hipSetDevice(s->ix->device));
    int rc = drain_batch(s); // (growing a buffer frees the old one)
    if (!rc) rc = deflate_reserve(s, s->text.text_cap);
    if (rc) {
      o.member_in = before;
      return rc;
    }
  }
  return KR_OK;
}

int kr_stream_place_bgzf(kr_stream* s, uint32_t level)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_stream_place_bgzf: null argument");
  if (level > 2) return kr::fail(KR_ERR_ARG, "kr_stream_place_bgzf: level " + std::to_string(level) + " (0: off, 1: fixed codes, 2: dynamic codes)");
  s->bgzf_out.place_level = level;
  return KR_OK;
}

int kr_batch_collect_text_bgzf(kr_stream* s, const uint8_t** comp, uint64_t* len, uint64_t* text_len)
{
  kr::clear_error();
  if (!s || !comp || !len || !text_len) return kr::fail(KR_ERR_ARG, "kr_batch_collect_text_bgzf: null argument");
  *comp = (const uint8_t*)"", *len = 0, *text_len = 0;
  if (!s->bgzf_out.on) return kr::fail(KR_ERR_STATE, "kr_batch_collect_text_bgzf: kr_stream_bgzf_out_enable first");
  if (!s->batch.submitted || !s->batch.has_ids()) return kr::fail(KR_ERR_STATE, "kr_batch_collect_text_bgzf: no batch submitted with kr_batch_submit_text");
  if (int rc = kr_batch_wait(s)) return rc;
  kr_stream::Text& t = s->text;
  kr_stream::BgzfOut& o = s->bgzf_out;
  // (the statuses of kr_batch_collect_text, for the same reasons)
  if (!s->batch.text_made) return kr::fail(KR_ERR_UNSUPPORTED, "kr_batch_collect_text_bgzf: the batch left the device as record slots (long sequences; submit with KR_TILE_ROWS for device text): kr_batch_collect + kr_format_dist");
  if (t.h_total[1] & kTextOverCap) return kr::fail(KR_ERR_CAPACITY, "the batch's report text exceeds max_text_bytes: submit fewer reads per batch");
  if (t.h_total[1] & kTextBadNum) return kr::fail(KR_ERR_UNSUPPORTED, "kr_batch_collect_text_bgzf: a DIST outside [0, 1000): kr_batch_collect + kr_format_dist");
  HIP_TRY(hipSetDevice(s->ix->device));
  const uint64_t n = t.h_total[0];
  if (n == 0) return KR_OK;
  if (n > t.text_cap) return kr::fail(KR_ERR_CAPACITY, "the batch's report text exceeds max_text_bytes: submit fewer reads per batch"); // (cannot be: the kernels flag it)
  const uint64_t bound = kr::bgzf_deflate_bound(n, o.member_in);
  if (int rc = deflate_reserve(s, n)) return rc; // (in hand since kr_stream_bgzf_out_enable: n <= max_text_bytes)
  if (bound > o.h_comp.size() && !o.h_comp.reserve(std::min<uint64_t>(kr::bgzf_deflate_bound(t.text_cap, o.member_in), bound + bound / 4 + (1u << 20))))
    return alloc_failed("kr_batch_collect_text_bgzf");
  hipStream_t st = s->lanes[0].stream;
  uint64_t total = 0;
  if (int rc = deflate_run(s, st, (const uint8_t*)t.d_text, n, &total)) return rc;
  HIP_TRY(hipMemcpyAsync(o.h_comp.get(), o.d_out.get(), total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *comp = o.h_comp.get(), *len = total, *text_len = n;
  return KR_OK;
}

// (tests) any host bytes through the kernels: bytes[0 .. n) go to the device, [skip, n) is deflated from the device address
// d_in + skip (d_in: the start of an allocation), so that a text that begins at any byte can be tried
static int debug_deflate_at(const char* who, kr_stream* s, const uint8_t* bytes, uint64_t n, uint64_t skip, uint8_t* out, uint64_t cap, uint64_t* len)
{
  kr::clear_error();
  if (!s || !len || (n && !bytes) || (cap && !out)) return kr::fail(KR_ERR_ARG, std::string(who) + ": null argument");
  *len = 0;
  if (!s->bgzf_out.on) return kr::fail(KR_ERR_STATE, std::string(who) + ": kr_stream_bgzf_out_enable first");
  if (skip > n) return kr::fail(KR_ERR_ARG, std::string(who) + ": skip exceeds the bytes given");
  if (n == skip) return KR_OK;
  HIP_TRY(hipSetDevice(s->ix->device));
  (void)hipGetLastError();
  if (int rc = drain_batch(s)) return rc; // (growing a buffer frees the old one)
  kr_stream::BgzfOut& o = s->bgzf_out;
  if (int rc = deflate_reserve(s, n - skip)) return rc;
  if (!o.d_in.reserve(n)) return alloc_failed(who);
  hipStream_t st = s->lanes[0].stream;
  HIP_TRY(hipMemcpyAsync(o.d_in.get(), bytes, n, hipMemcpyHostToDevice, st));
  uint64_t total = 0;
  if (int rc = deflate_run(s, st, o.d_in.get() + skip, n - skip, &total)) return rc;
  if (total > cap) return kr::fail(KR_ERR_CAPACITY, std::string(who) + ": the members take " + std::to_string(total) + " bytes, the buffer holds " + std::to_string(cap));
  HIP_TRY(hipMemcpy(out, o.d_out.get(), total, hipMemcpyDeviceToHost));
  *len = total;
  return KR_OK;
}

int kr_debug_bgzf_deflate(kr_stream* s, const uint8_t* bytes, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* len)
{
  return debug_deflate_at("kr_debug_bgzf_deflate", s, bytes, n, 0, out, cap, len);
}

int kr_debug_bgzf_deflate_at(kr_stream* s, const uint8_t* bytes, uint64_t n, uint64_t skip, uint8_t* out, uint64_t cap, uint64_t* len)
{
  return debug_deflate_at("kr_debug_bgzf_deflate_at", s, bytes, n, skip, out, cap, len);
}

// (measurements) the device time of the deflate, scan and copy kernels of the stream's last kr_batch_collect_text_bgzf /
// kr_debug_bgzf_deflate.  The first call makes the events and gives *ms = -1: the next deflate is the first measured.
int kr_debug_bgzf_deflate_ms(kr_stream* s, float* ms)
{
  kr::clear_error();
  if (!s || !ms) return kr::fail(KR_ERR_ARG, "kr_debug_bgzf_deflate_ms: null argument");
  if (!s->bgzf_out.on) return kr::fail(KR_ERR_STATE, "kr_debug_bgzf_deflate_ms: kr_stream_bgzf_out_enable first");
  kr_stream::BgzfOut& o = s->bgzf_out;
  *ms = -1.0f;
  HIP_TRY(hipSetDevice(s->ix->device));
  if (!o.ev0) {
    HIP_TRY(hipEventCreate(&o.ev0));
    HIP_TRY(hipEventCreate(&o.ev1));
    return KR_OK;
  }
  if (!o.ev_set) return KR_OK;
  HIP_TRY(hipEventSynchronize(o.ev1));
  HIP_TRY(hipEventElapsedTime(ms, o.ev0, o.ev1));
  return KR_OK;
}

// (tests) def_build_lengths through kr_huffman_lengths_kernel
int kr_debug_huffman_lengths_device(kr_stream* s, const uint32_t* freq, uint32_t nsym, uint32_t maxbits, uint8_t* lens, uint32_t* limited)
{
  kr::clear_error();
  if (!s || !freq || !lens || !limited) return kr::fail(KR_ERR_ARG, "kr_debug_huffman_lengths_device: null argument");
  if (!kr::def_build_args_ok(freq, nsym, maxbits))
    return kr::fail(KR_ERR_ARG, "kr_debug_huffman_lengths_device: 1 to 286 symbols, 1 to 15 bits with room for every counted symbol, counts below 2^22");
  HIP_TRY(hipSetDevice(s->ix->device));
  (void)hipGetLastError();
  kr_stream::BgzfOut& o = s->bgzf_out;
  const uint32_t lens_at = kr::kDefLL, flag_at = lens_at + (kr::kDefLL + 3u) / 4u; // in words: counts | lengths | the flag
  if (!o.d_huff.reserve(flag_at + 1u)) return alloc_failed("kr_debug_huffman_lengths_device");
  uint32_t* d = o.d_huff.get();
  hipStream_t st = s->lanes[0].stream;
  HIP_TRY(hipMemcpyAsync(d, freq, nsym * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(kr_huffman_lengths_kernel, dim3(1), dim3(64), 0, st, d, nsym, maxbits, (uint8_t*)(d + lens_at), d + flag_at);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(lens, d + lens_at, nsym, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(limited, d + flag_at, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return KR_OK;
}

} // extern "C"
