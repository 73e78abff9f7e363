// asan_gzip_sym.cpp -- the serial twin of the device gzip inflater (krepp_amd/csrc/kr_inflate_sym.h, kr_gzip_super.h) under
// AddressSanitizer and UBSan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -Ikrepp_amd/csrc scripts/asan_gzip_sym.cpp -lz -o asan_gzip_sym
//   ./asan_gzip_sym
//
// A stand-alone program: it runs on the CPU and needs no device.  The twin keeps the compressed input, the symbol buffer, every
// table and the output in heap blocks of exactly their sizes (GzHostBackend), and the file handed to it here is such a block too, so
// one byte read or written outside any of them is reported.  Corpus: the inputs of tests/test_gzip_sym_host.py in kind (FASTQ-shaped
// text at several levels, strategies, memory levels, flushes, members, header fields, sub-chunk and super-chunk sizes, a run of one
// letter under ratio_cap 4, binary content, a decoy block start inside a stored block), every single-bit flip and every truncation of the first 4 KB of fixture B, and 2,000
// random byte strings behind a gzip header.  zlib's verdict (inflate with a gzip wrapper, member after member, as gzread reads) is
// taken beside each run: the twin must accept what zlib accepts, with the same bytes, and refuse what zlib refuses, having handed
// out only bytes zlib produced too.  Left out: the hand-assembled fixed-Huffman streams of tests/gzip_cases.py (seam_cases: a copy of
// distance exactly 32,768 as a chunk's first token, a source that straddles window and output, chunks of 32,767 .. 32,769 symbols); they
// need that file's bit writer and run through the same twin in tests/test_gzip_sym_host.py, without the sanitizer.  Prints a summary line and exits 0 when nothing differs.
#include "kr_gzip_super.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <thread>

typedef std::vector<uint8_t> Bytes;

static Bytes fastq_text(uint32_t records, uint64_t seed)
{
  std::mt19937_64 rng(seed);
  Bytes t;
  for (uint32_t i = 0; i < records; ++i) {
    char name[64];
    const int n = snprintf(name, sizeof(name), "@read%u/1 run=%u\n", i, (unsigned)(seed % 1000));
    t.insert(t.end(), name, name + n);
    for (int k = 0; k < 150; ++k) t.push_back("ACGT"[rng() & 3]);
    t.push_back('\n'), t.push_back('+'), t.push_back('\n');
    for (int k = 0; k < 150; ++k) t.push_back((uint8_t)(33 + rng() % 41));
    t.push_back('\n');
  }
  return t;
}

// one gzip member; flush_at: a Z_SYNC_FLUSH (1) or Z_FULL_FLUSH (2) after that many bytes
static Bytes gzip_member(const Bytes& data, int level, int strategy, int mem_level, size_t flush_at = 0, int flush_kind = 0)
{
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (deflateInit2(&zs, level, Z_DEFLATED, 31, mem_level, strategy) != Z_OK) abort();
  Bytes out(deflateBound(&zs, (uLong)data.size()) + 64);
  zs.next_out = out.data(), zs.avail_out = (uInt)out.size();
  zs.next_in = const_cast<Bytef*>(data.data());
  if (flush_kind && flush_at < data.size()) {
    zs.avail_in = (uInt)flush_at;
    if (deflate(&zs, flush_kind == 1 ? Z_SYNC_FLUSH : Z_FULL_FLUSH) != Z_OK) abort();
    zs.avail_in = (uInt)(data.size() - flush_at);
  } else
    zs.avail_in = (uInt)data.size();
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
  out.resize(zs.total_out);
  deflateEnd(&zs);
  return out;
}

// zlib, member after member as gzread reads: true and all bytes, or false and the bytes in front of the error
static bool zlib_reads(const Bytes& file, Bytes& out)
{
  out.clear();
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, 31) != Z_OK) abort();
  zs.next_in = const_cast<Bytef*>(file.data()), zs.avail_in = (uInt)file.size();
  bool ok = false;
  for (;;) {
    out.resize(out.size() + (1u << 16));
    zs.next_out = out.data() + zs.total_out, zs.avail_out = (uInt)(out.size() - zs.total_out);
    const int rc = inflate(&zs, Z_NO_FLUSH);
    if (rc == Z_STREAM_END) {
      if (zs.avail_in >= 2 && zs.next_in[0] == 0x1f && zs.next_in[1] == 0x8b) {
        const uLong done = zs.total_out;
        if (inflateReset(&zs) != Z_OK) abort();
        zs.total_out = done;
        continue;
      }
      ok = true; // the end, or bytes that are no gzip member
      break;
    }
    if (rc == Z_OK && (zs.avail_in || zs.avail_out == 0)) continue;
    if (rc == Z_BUF_ERROR && zs.avail_out == 0) continue;
    break; // an error, or the file ends inside a member
  }
  out.resize(zs.total_out);
  inflateEnd(&zs);
  return ok;
}

// a raw deflate stream in parts: data[0] deflated and full-flushed (byte-aligned, history forgotten), `stored` as stored blocks that
// are not the last, data[1] deflated to the end -- and the bytes the whole inflates to
static Bytes raw_parts(const Bytes& first, const Bytes& stored, const Bytes& last, int mem_level, Bytes& inflated)
{
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (deflateInit2(&zs, 6, Z_DEFLATED, -15, mem_level, Z_DEFAULT_STRATEGY) != Z_OK) abort();
  Bytes out(deflateBound(&zs, (uLong)(first.size() + last.size())) + stored.size() + 1024), mid;
  zs.next_out = out.data(), zs.avail_out = (uInt)out.size();
  zs.next_in = const_cast<Bytef*>(first.data()), zs.avail_in = (uInt)first.size();
  if (!stored.empty()) {
    if (deflate(&zs, Z_FULL_FLUSH) != Z_OK) abort();
    for (size_t i = 0; i < stored.size(); i += 60000) {
      const size_t n = std::min<size_t>(60000, stored.size() - i);
      const uint8_t h[5] = {0, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
      mid.insert(mid.end(), h, h + 5);
      mid.insert(mid.end(), stored.begin() + i, stored.begin() + i + n);
    }
  }
  const size_t cut = zs.total_out;
  zs.next_in = const_cast<Bytef*>(last.data()), zs.avail_in = (uInt)last.size();
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
  out.resize(zs.total_out);
  deflateEnd(&zs);
  out.insert(out.begin() + cut, mid.begin(), mid.end());
  inflated = first;
  inflated.insert(inflated.end(), stored.begin(), stored.end());
  inflated.insert(inflated.end(), last.begin(), last.end());
  return out;
}
// a gzip member around a raw deflate stream; flags: FEXTRA 4, FNAME 8, FCOMMENT 16, FHCRC 2
static Bytes wrap(const Bytes& raw, const Bytes& data, unsigned flags)
{
  Bytes h = {0x1f, 0x8b, 8, (uint8_t)flags, 0, 0, 0, 0, 0, 3};
  if (flags & 4) h.insert(h.end(), {6, 0, 'a', 'b', 2, 0, 'x', 'y'});
  if (flags & 8) h.insert(h.end(), {'r', '.', 'f', 'q', 0});
  if (flags & 16) h.insert(h.end(), {'n', 'o', 't', 'e', 0});
  if (flags & 2) {
    const uint32_t c = (uint32_t)crc32(crc32(0L, Z_NULL, 0), h.data(), (uInt)h.size());
    h.push_back((uint8_t)c), h.push_back((uint8_t)(c >> 8));
  }
  h.insert(h.end(), raw.begin(), raw.end());
  const uint32_t t[2] = {(uint32_t)crc32(crc32(0L, Z_NULL, 0), data.data(), (uInt)data.size()), (uint32_t)data.size()};
  for (uint32_t v : t)
    for (int k = 0; k < 4; ++k) h.push_back((uint8_t)(v >> (8 * k)));
  return h;
}

static std::atomic<uint64_t> n_cases{0}, n_accept{0}, n_diff{0}, n_host_ranges{0}, n_super{0};
static std::mutex print_mu;

// returns the twin's counters through c[6] (null: not wanted)
static void one(const Bytes& file, uint32_t sub, uint32_t ratio, uint64_t max_comp, const char* what, uint64_t* c = nullptr)
{
  std::unique_ptr<uint8_t[]> in(new uint8_t[file.size() ? file.size() : 1]);
  if (!file.empty()) memcpy(in.get(), file.data(), file.size());
  Bytes ref;
  const bool z = zlib_reads(file, ref);
  std::unique_ptr<uint8_t[]> out(new uint8_t[ref.size() + 1]);
  kr::GzParams prm;
  prm.sub = sub, prm.ratio = ratio, prm.max_comp = max_comp;
  kr::GzHostBackend be;
  const uint64_t tab_cap = (file.size() / sub + 2) * 64 + 64;
  std::vector<uint32_t> S(tab_cap), E(tab_cap), St(tab_cap), Lk(tab_cap), Ln(tab_cap), Cr(tab_cap);
  uint64_t len = 0, ntab = 0, ctr[6] = {0, 0, 0, 0, 0, 0};
  std::string msg;
  const int rc = kr::gz_debug_run(be, in.get(), file.size(), prm, out.get(), ref.size() + 1, &len, tab_cap, S.data(), E.data(), St.data(), Lk.data(), Ln.data(), Cr.data(),
                                  &ntab, ctr, msg);
  ++n_cases;
  n_host_ranges += ctr[4], n_super += ctr[0];
  if (c) memcpy(c, ctr, sizeof(ctr));
  bool same;
  if (z) same = rc == 0 && len == ref.size() && memcmp(out.get(), ref.data(), len) == 0;
  else same = rc == -2 && len <= ref.size() && memcmp(out.get(), ref.data(), len) == 0;
  if (rc == 0) ++n_accept;
  if (!same) {
    ++n_diff;
    std::lock_guard<std::mutex> lk(print_mu);
    fprintf(stderr, "DIFFERENT (%s): %zu bytes, sub %u, ratio %u, super %llu: twin rc %d, %llu bytes (%s); zlib %s, %zu bytes\n", what, file.size(), sub, ratio,
            (unsigned long long)max_comp, rc, (unsigned long long)len, msg.c_str(), z ? "accepts" : "refuses", ref.size());
  }
}

template <class F>
static void parallel(size_t n, F f)
{
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&] {
      for (size_t i; (i = next++) < n;) f(i);
    });
  for (auto& t : th) t.join();
}

int main()
{
  const uint64_t big = 1u << 20;
  const Bytes A = gzip_member(fastq_text(600, 1), 6, Z_DEFAULT_STRATEGY, 3), B = gzip_member(fastq_text(300, 2), 6, Z_DEFAULT_STRATEGY, 8);
  uint64_t c[6];
  one(A, 1024, 16, big, "fixture A", c);
  if (c[4] != 0 || c[3] != 0 || c[1] < 100) ++n_diff, fprintf(stderr, "fixture A: linked %llu, dropped %llu, host ranges %llu\n", (unsigned long long)c[1], (unsigned long long)c[3], (unsigned long long)c[4]);
  one(B, 4096, 16, big, "fixture B", c);
  if (c[4] != 0 || c[2] < 10) ++n_diff, fprintf(stderr, "fixture B: without start %llu, host ranges %llu\n", (unsigned long long)c[2], (unsigned long long)c[4]);
  for (uint32_t sub : {512u, 1024u, 4096u, 65536u}) one(A, sub, 16, big, "fixture A, sub"), one(B, sub, 16, big, "fixture B, sub");
  one(A, 1024, 16, A.size() / 5 + 1024, "fixture A, five super-chunks", c);
  if (c[0] < 5) ++n_diff, fprintf(stderr, "fixture A: %llu super-chunks\n", (unsigned long long)c[0]);
  const Bytes text = fastq_text(400, 3);
  for (int level : {1, 9}) one(gzip_member(text, level, Z_DEFAULT_STRATEGY, 3), 1024, 16, big, "level");
  for (int st : {Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE}) one(gzip_member(text, 6, st, 3), 1024, 16, big, "strategy");
  one(gzip_member(text, 0, Z_DEFAULT_STRATEGY, 8), 1024, 16, big, "level 0");
  for (int kind : {1, 2}) one(gzip_member(text, 6, Z_DEFAULT_STRATEGY, 3, text.size() / 2, kind), 1024, 16, big, "flush");
  { // members: two and three, one ending inside a super-chunk and one exactly at its end; bytes that are no member behind them
    const Bytes m1 = gzip_member(fastq_text(100, 4), 6, Z_DEFAULT_STRATEGY, 3), m2 = gzip_member(fastq_text(120, 5), 6, Z_DEFAULT_STRATEGY, 3), m3 = gzip_member(fastq_text(50, 6), 9, Z_DEFAULT_STRATEGY, 3);
    Bytes two = m1, three = m1;
    two.insert(two.end(), m2.begin(), m2.end());
    three.insert(three.end(), m2.begin(), m2.end()), three.insert(three.end(), m3.begin(), m3.end());
    one(two, 1024, 16, big, "two members");
    one(three, 1024, 16, big, "three members");
    one(three, 1024, 16, m1.size(), "a member ending at the super-chunk's end");
    one(three, 512, 16, m1.size() - 9, "a trailer across super-chunks");
    Bytes junk = two;
    for (int i = 0; i < 100; ++i) junk.push_back((uint8_t)i);
    one(junk, 1024, 16, big, "junk behind the last member");
  }
  { // header fields (gz_member_header), one by one and together; a header CRC that is wrong
    Bytes data;
    const Bytes raw = raw_parts(Bytes(), Bytes(), text, 3, data);
    for (unsigned flags : {4u, 8u, 16u, 2u, 30u}) one(wrap(raw, data, flags), 1024, 16, big, "header fields");
    Bytes bad = wrap(raw, data, 30u);
    bad[10 + 8 + 5 + 5] ^= 1; // the FHCRC's first byte
    one(bad, 1024, 16, big, "a wrong header CRC");
  }
  { // a decoy block start inside a stored block: the stored data are a deflate stream of other text
    Bytes inner_text, data;
    const Bytes inner = raw_parts(Bytes(), Bytes(), fastq_text(150, 12), 3, inner_text);
    const Bytes raw = raw_parts(fastq_text(120, 11), inner, fastq_text(120, 13), 3, data);
    one(wrap(raw, data, 0), 1024, 16, big, "a decoy start in a stored block", c);
    if (c[3] == 0 || c[4] == 0) ++n_diff, fprintf(stderr, "the decoy: dropped %llu, host ranges %llu\n", (unsigned long long)c[3], (unsigned long long)c[4]);
  }
  { // a run of one letter: a ratio above ratio_cap, inflated by the host
    Bytes run = fastq_text(50, 7);
    run.insert(run.end(), 100000, 'A');
    const Bytes tail = fastq_text(200, 8);
    run.insert(run.end(), tail.begin(), tail.end());
    one(gzip_member(run, 6, Z_DEFAULT_STRATEGY, 3), 1024, 4, big, "100,000 As under ratio_cap 4", c);
    if (c[4] == 0) ++n_diff, fprintf(stderr, "the run of As: no host range\n");
  }
  { // binary content: no start anywhere
    std::mt19937_64 rng(9);
    Bytes bin(60000);
    for (auto& b : bin) b = (uint8_t)(rng() % 7 ? rng() : 0);
    one(gzip_member(bin, 6, Z_DEFAULT_STRATEGY, 8), 1024, 16, 8192, "binary content", c);
    if (c[4] == 0) ++n_diff, fprintf(stderr, "binary content: no host range\n");
  }
  // every bit flip and every truncation of fixture B's first 4 KB
  parallel(4096 * 8, [&](size_t bit) {
    Bytes f = B;
    f[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
    one(f, 4096, 16, big, "bit flip");
  });
  parallel(4096, [&](size_t n) { one(Bytes(B.begin(), B.begin() + n), 4096, 16, big, "truncation"); });
  parallel(64, [&](size_t k) { one(Bytes(B.begin(), B.end() - 1 - k), 4096, 16, big, "truncation at the end"); });
  // random byte strings behind a gzip header
  parallel(2000, [&](size_t i) {
    std::mt19937_64 rng(1000 + i);
    Bytes f = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    const size_t n = 18 + rng() % 3000;
    while (f.size() < n) f.push_back((uint8_t)rng());
    if (i % 2) f[10] = (uint8_t)((f[10] & ~7u) | 4u); // a dynamic block that is not the last: the header rules get their share
    one(f, i % 3 ? 512 : 64, 16, i % 5 ? big : 1024, "random bytes");
  });
  printf("asan_gzip_sym: %llu inputs, %llu accepted, %llu super-chunks, %llu host ranges, %llu differences from zlib\n", (unsigned long long)n_cases.load(),
         (unsigned long long)n_accept.load(), (unsigned long long)n_super.load(), (unsigned long long)n_host_ranges.load(), (unsigned long long)n_diff.load());
  return n_diff ? 1 : 0;
}
