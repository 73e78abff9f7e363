// asan_bgzf.cpp -- the BGZF member decoder's host instantiation (krepp_amd/csrc/kr_inflate.h) under AddressSanitizer and UBSan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ikrepp_amd/csrc scripts/asan_bgzf.cpp -lz -o asan_bgzf
//   ./asan_bgzf
//
// A stand-alone program: it runs on the CPU and needs no device.  Every payload is copied into a heap block of exactly its size and
// every output into a block of exactly ISIZE bytes, so that one byte read or written outside either is reported.  Corpus: every
// single-bit flip and every truncation of a dynamic-Huffman and of a fixed-Huffman payload, 200 random members (random levels,
// strategies and contents), 2000 payloads of random bytes.  Each verdict is compared with zlib's inflate(); the sliced CRC (the
// form a wave computes) is compared with zlib's crc32.  Prints a summary line and exits 0 when nothing differs.
#include "kr_inflate.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t>& data, int level, int strategy, int mem_level = 8)
{
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (deflateInit2(&zs, level, Z_DEFLATED, -15, mem_level, strategy) != Z_OK) abort();
  std::vector<uint8_t> out(deflateBound(&zs, (uLong)data.size()) + 16);
  zs.next_in = const_cast<Bytef*>(data.data()), zs.avail_in = (uInt)data.size();
  zs.next_out = out.data(), zs.avail_out = (uInt)out.size();
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
  out.resize(zs.total_out);
  deflateEnd(&zs);
  return out;
}

// zlib's verdict on a payload that must inflate to exactly isize bytes and use up the payload
static bool zlib_accepts(const std::vector<uint8_t>& payload, uint32_t isize, std::vector<uint8_t>& out)
{
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, -15) != Z_OK) abort();
  out.assign(isize + 1, 0);
  zs.next_in = const_cast<Bytef*>(payload.data()), zs.avail_in = (uInt)payload.size();
  zs.next_out = out.data(), zs.avail_out = isize;
  const int rc = inflate(&zs, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && zs.avail_out == 0 && zs.avail_in == 0;
  inflateEnd(&zs);
  out.resize(isize);
  return ok;
}

static uint64_t n_cases = 0, n_accept = 0, n_diff = 0;

static void one(const std::vector<uint8_t>& payload, uint32_t isize)
{
  std::unique_ptr<uint8_t[]> in(new uint8_t[payload.size() ? payload.size() : 1]); // exact blocks: the sanitizer sees the first byte outside
  if (!payload.empty()) memcpy(in.get(), payload.data(), payload.size());
  std::unique_ptr<uint8_t[]> out(new uint8_t[isize ? isize : 1]);
  std::unique_ptr<kr::InfTables> T(new kr::InfTables);
  kr::InfSerial L;
  uint32_t pos = 0;
  const uint32_t rule = kr::inflate_member(in.get(), (uint32_t)payload.size(), out.get(), isize, *T, L, &pos);
  std::vector<uint8_t> ref;
  const bool z = zlib_accepts(payload, isize, ref);
  ++n_cases;
  if ((rule == 0) != z || pos > isize || (z && memcmp(ref.data(), out.get(), isize) != 0)) {
    ++n_diff;
    fprintf(stderr, "DIFFERENT: payload of %zu bytes, isize %u: rule %u (%s) at %u, zlib %s\n", payload.size(), isize, rule, kr::inf_rule_name(rule), pos,
            z ? "accepts" : "rejects");
  }
  if (rule == 0) {
    ++n_accept;
    const uint32_t a = ~kr::crc_raw(kr::crc_host_table(), 0xFFFFFFFFu, out.get(), isize), b = kr::crc_sliced_host(kr::crc_host_table(), out.get(), isize);
    const uint32_t c = (uint32_t)crc32(crc32(0L, Z_NULL, 0), out.get(), isize);
    if (a != c || b != c) {
      ++n_diff;
      fprintf(stderr, "DIFFERENT CRC: %u bytes: byte loop %08x, sliced %08x, zlib %08x\n", isize, a, b, c);
    }
  }
}

static void flips_and_cuts(const std::vector<uint8_t>& payload, uint32_t isize)
{
  one(payload, isize);
  for (size_t bit = 0; bit < payload.size() * 8; ++bit) {
    std::vector<uint8_t> p = payload;
    p[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
    one(p, isize);
  }
  for (size_t n = 0; n < payload.size(); ++n) one(std::vector<uint8_t>(payload.begin(), payload.begin() + n), isize);
  one(payload, isize + 1);
  if (isize) one(payload, isize - 1);
}

int main()
{
  std::mt19937_64 rng(20240611);
  std::vector<uint8_t> text;
  for (int i = 0; text.size() < 700; ++i) {
    char rec[256];
    const int n = snprintf(rec, sizeof(rec), "@read%d/1\nACGTTGCA%dGGATCCATTAGACCA\n+\nIIIIHHHH%dFFFFFFFFFFFFFFF\n", i, i * 7919 % 1000, i * 104729 % 1000);
    text.insert(text.end(), rec, rec + n);
  }
  flips_and_cuts(deflate_raw(text, 6, Z_DEFAULT_STRATEGY), (uint32_t)text.size());
  flips_and_cuts(deflate_raw(text, 6, Z_FIXED), (uint32_t)text.size());
  flips_and_cuts(deflate_raw(text, 0, Z_DEFAULT_STRATEGY), (uint32_t)text.size());
  for (int i = 0; i < 200; ++i) { // random members: contents from one symbol to all 256, runs, every strategy
    const uint32_t n = (uint32_t)(rng() % (i < 150 ? 5000 : 65537));
    const uint32_t alphabet = 1u + (uint32_t)(rng() % 256), run = 1u + (uint32_t)(rng() % 40);
    std::vector<uint8_t> d(n);
    for (uint32_t j = 0; j < n;) {
      const uint8_t b = (uint8_t)(rng() % alphabet);
      for (uint32_t r = 1 + (uint32_t)(rng() % run); r && j < n; --r) d[j++] = b;
    }
    const int strategies[5] = {Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED};
    const std::vector<uint8_t> p = deflate_raw(d, (int)(rng() % 10), strategies[rng() % 5], 1 + (int)(rng() % 9));
    one(p, n);
    std::vector<uint8_t> q = p; // and one damaged form of each
    if (!q.empty()) q[rng() % q.size()] ^= (uint8_t)(1u << (rng() % 8));
    one(q, n);
  }
  for (int i = 0; i < 2000; ++i) { // bytes that were never a deflate stream
    std::vector<uint8_t> p(rng() % 200);
    for (auto& b : p) b = (uint8_t)rng();
    if (!p.empty() && i % 2) p[0] = (uint8_t)((p[0] & ~7u) | 5u); // a last, dynamic block: the code-length rules get their share
    one(p, (uint32_t)(rng() % 3000));
  }
  printf("asan_bgzf: %llu payloads, %llu accepted, %llu differences from zlib\n", (unsigned long long)n_cases, (unsigned long long)n_accept,
         (unsigned long long)n_diff);
  return n_diff ? 1 : 0;
}
