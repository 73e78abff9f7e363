// asan_bgzf_deflate_dyn.cpp -- level 2 (dynamic Huffman codes) of the BGZF member encoder's host instantiation
// (krepp_amd/csrc/kr_deflate.h, deflate_member_dyn) under AddressSanitizer and UBSan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ikrepp_amd/csrc scripts/asan_bgzf_deflate_dyn.cpp -lz -o asan_bgzf_deflate_dyn
//   ./asan_bgzf_deflate_dyn
//
// A stand-alone program: it runs on the CPU and needs no device.  Every input is copied into a heap block of exactly its size, every
// member is written into a block of exactly n + 31 bytes and its tokens into a block of exactly n tokens, so that one byte read or
// written outside any of them is reported.  Corpus: that of asan_bgzf_deflate.cpp (random, periodic, copied, report-shaped and
// one-byte inputs of every length 1 .. 600 and 65,270 .. 65,280), and members of mostly literals whose literal code must be limited
// to 15 bits (32,770 fillers from 32 bytes, sixteen rare bytes with the counts 1, 2, 4, 7, 12, ..., 2,583).  Each member is
// inflated with zlib (as a gzip member: header, CRC-32 and ISIZE are checked too) and with kr_inflate.h's inflate_member; BSIZE
// must be the member's size; a level-2 member must not be larger than the level-1 member and must equal it where it kept the
// fixed codes or the stored block.  The code-length builder also runs alone on random counts of all three alphabets and its
// result is checked (Kraft sum 1, the limit kept, zero count <=> zero length).  Prints a summary line and exits 0 when nothing differs.
#include "kr_deflate.h"
#include "kr_inflate.h"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

static uint64_t n_cases = 0, n_diff = 0, n_in = 0, n_out = 0, n_builder = 0;
static kr::DefStats total;

static void differs(const char* what, const char* kind, uint32_t n)
{
  ++n_diff;
  fprintf(stderr, "DIFFERENT: %s input of %u bytes: %s\n", kind, n, what);
}

static void one(const std::vector<uint8_t>& data, const char* kind)
{
  const uint32_t n = (uint32_t)data.size();
  std::unique_ptr<uint8_t[]> in(new uint8_t[n]); // exact blocks: the sanitizer sees the first byte outside
  memcpy(in.get(), data.data(), n);
  std::unique_ptr<uint8_t[]> slot(new uint8_t[n + kr::kDefOverhead]), slot1(new uint8_t[n + kr::kDefOverhead]);
  std::unique_ptr<uint32_t[]> tok(new uint32_t[n]);
  std::unique_ptr<kr::DefDynState> S(new kr::DefDynState);
  std::unique_ptr<kr::DefState> S1(new kr::DefState);
  const uint32_t size = kr::bgzf_deflate_member_host_dyn(in.get(), n, 0, slot.get(), *S, tok.get(), &total);
  const uint32_t size1 = kr::bgzf_deflate_member_host(in.get(), n, 0, slot1.get(), *S1, nullptr);
  ++n_cases, n_in += n, n_out += size;
  if (size > n + kr::kDefOverhead || size > kr::bgzf_deflate_bound(n)) return differs("larger than the bound", kind, n);
  if (size > size1) return differs("larger than the level-1 member", kind, n);
  if (((slot[18] >> 1) & 3u) != S->btype) return differs("the block type is not the one the state names", kind, n);
  if (S->btype != 2u && (size != size1 || memcmp(slot.get(), slot1.get(), size) != 0)) return differs("a fixed or stored member that is not level 1's", kind, n);
  if (kr::bgzf_member_size(slot.get(), size) != size) return differs("BSIZE is not the member's size", kind, n);
  { // zlib, as a gzip member
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 31) != Z_OK) abort();
    std::vector<uint8_t> out(n + 1);
    zs.next_in = slot.get(), zs.avail_in = size;
    zs.next_out = out.data(), zs.avail_out = n + 1;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == n && zs.avail_in == 0 && memcmp(out.data(), in.get(), n) == 0;
    inflateEnd(&zs);
    if (!ok) return differs("zlib does not inflate the member to the input", kind, n);
  }
  { // our decoder
    kr::BgzfMember m;
    uint32_t ms = 0, pos = 0;
    if (kr::bgzf_member_at(slot.get(), size, 0, &m, &ms) || ms != size || m.isize != n) return differs("bgzf_member_at refuses the member", kind, n);
    std::unique_ptr<uint8_t[]> out(new uint8_t[n]);
    std::unique_ptr<kr::InfTables> T(new kr::InfTables);
    kr::InfSerial L;
    const uint32_t rule = kr::inflate_member(slot.get() + m.in_off, m.in_size, out.get(), n, *T, L, &pos);
    if (rule || memcmp(out.get(), in.get(), n) != 0) return differs("inflate_member does not return the input", kind, n);
    if (~kr::crc_raw(kr::crc_host_table(), 0xFFFFFFFFu, out.get(), n) != m.crc) return differs("wrong CRC-32", kind, n);
  }
}

static std::vector<uint8_t> report_text(uint32_t n, std::mt19937_64& rng)
{
  std::vector<uint8_t> t;
  for (uint32_t r = (uint32_t)(rng() % 1000); t.size() < n; ++r)
    for (int row = 0; row < 33 && t.size() < n; ++row) {
      char rec[96];
      const int k = snprintf(rec, sizeof(rec), "SRR1234567.%u\tG%09u\t0.%05u\n", r, (unsigned)(rng() % 500) * 7919u, (unsigned)(rng() % 100000));
      t.insert(t.end(), rec, rec + k);
    }
  t.resize(n);
  return t;
}

// mostly literals with very unequal counts: 32,770 fillers drawn from 32 bytes, the rare bytes 1 .. 16 (1, 2, 4, 7, 12, ..., 2,583 times,
// shuffled) behind every fourth of them: where no match takes literals away the literal code is deeper than 15 bits until it is limited
static std::vector<uint8_t> limiter(std::mt19937_64& rng)
{
  std::vector<uint8_t> rare;
  uint32_t a = 1, b = 2;
  for (uint32_t s = 1; s <= 16; ++s) {
    rare.insert(rare.end(), a, (uint8_t)s);
    const uint32_t c = a + b + 1;
    a = b, b = c;
  }
  std::shuffle(rare.begin(), rare.end(), rng);
  std::vector<uint8_t> out;
  for (uint32_t i = 0; i < 32770; ++i) {
    out.push_back((uint8_t)(64u + rng() % 32u));
    if (i % 4 == 2 && i / 4 < rare.size()) out.push_back(rare[i / 4]);
  }
  return out;
}

static void builder(const std::vector<uint32_t>& freq, uint32_t maxbits)
{
  const uint32_t nsym = (uint32_t)freq.size();
  std::unique_ptr<uint32_t[]> f(new uint32_t[nsym]);
  std::unique_ptr<uint8_t[]> lens(new uint8_t[nsym]);
  memcpy(f.get(), freq.data(), nsym * sizeof(uint32_t));
  std::unique_ptr<kr::DefBuild> B(new kr::DefBuild);
  if (!kr::def_build_args_ok(f.get(), nsym, maxbits)) return;
  (void)kr::def_build_lengths(f.get(), nsym, maxbits, lens.get(), *B);
  ++n_builder;
  uint64_t kraft = 0;
  uint32_t counted = 0;
  for (uint32_t i = 0; i < nsym; ++i) {
    if ((f[i] == 0) != (lens[i] == 0) || lens[i] > maxbits) return differs("a length that breaks the builder's contract", "counts", nsym);
    if (lens[i]) kraft += 1ull << (maxbits - lens[i]), ++counted;
  }
  if (counted >= 2 && kraft != 1ull << maxbits) differs("the Kraft sum is not 1", "counts", nsym);
}

int main()
{
  std::mt19937_64 rng(20240702);
  std::vector<uint32_t> lengths;
  for (uint32_t n = 1; n <= 600; ++n) lengths.push_back(n);
  for (uint32_t n = kr::kDefMemberIn - 10; n <= kr::kDefMemberIn; ++n) lengths.push_back(n);
  for (uint32_t n : lengths) {
    std::vector<uint8_t> d(n);
    for (auto& b : d) b = (uint8_t)rng();
    one(d, "random");
    const uint32_t period = 1u + (uint32_t)(rng() % 300), alphabet = 1u + (uint32_t)(rng() % 256);
    for (uint32_t i = 0; i < n; ++i) d[i] = i < period ? (uint8_t)(rng() % alphabet) : d[i - period];
    one(d, "periodic");
    for (uint32_t i = 0; i < n; ++i) // few symbols, runs: matches of every length, and the far ones of the long inputs
      d[i] = (uint8_t)("ACGT"[rng() % 4]);
    for (uint32_t i = 300; i + 300 < n; i += 1 + (uint32_t)(rng() % 40000)) memcpy(d.data() + i, d.data(), 100 + rng() % 200);
    one(d, "copies");
    one(report_text(n, rng), "report");
    one(std::vector<uint8_t>(n, (uint8_t)(n * 37u)), "one byte");
  }
  const uint64_t limited_before = total.limited;
  for (int i = 0; i < 3; ++i) one(limiter(rng), "limiter");
  if (total.limited == limited_before) differs("none of the limiter inputs needed the limit", "limiter", 0);
  for (int i = 0; i < 3000; ++i) {
    const uint32_t nsym = i % 3 == 0 ? kr::kDefLL : i % 3 == 1 ? kr::kDefD : kr::kDefCL, maxbits = nsym == kr::kDefCL ? 7u : 15u;
    std::vector<uint32_t> f(nsym);
    const uint32_t shape = (uint32_t)(rng() % 4);
    for (uint32_t s = 0; s < nsym; ++s) {
      const uint64_t r = rng();
      f[s] = shape == 0 ? (uint32_t)(r % 65281) : shape == 1 ? (uint32_t)(r % 3) : shape == 2 ? (uint32_t)(1u << (r % 22)) : (r % 7 ? 0u : (uint32_t)(r % 1000));
    }
    builder(f, maxbits);
  }
  printf("asan_bgzf_deflate_dyn: %llu members (%llu stored, %llu fixed, %llu dynamic, %llu with a limited code), %llu bytes in, %llu out, "
         "%llu builder runs, %llu differences\n", (unsigned long long)n_cases, (unsigned long long)total.stored, (unsigned long long)total.fixed,
         (unsigned long long)total.dynamic, (unsigned long long)total.limited, (unsigned long long)n_in, (unsigned long long)n_out,
         (unsigned long long)n_builder, (unsigned long long)n_diff);
  return n_diff ? 1 : 0;
}
