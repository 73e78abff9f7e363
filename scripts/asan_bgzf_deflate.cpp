// asan_bgzf_deflate.cpp -- the BGZF member encoder's host instantiation (krepp_amd/csrc/kr_deflate.h) under AddressSanitizer and UBSan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ikrepp_amd/csrc scripts/asan_bgzf_deflate.cpp -lz -o asan_bgzf_deflate
//   ./asan_bgzf_deflate
//
// A stand-alone program: it runs on the CPU and needs no device.  Every input is copied into a heap block of exactly its size and
// every member is written into a block of exactly n + 31 bytes, so that one byte read or written outside either is reported.
// Corpus: random, periodic and report-shaped inputs of every length 1 .. 600 and 65,270 .. 65,280 (a member's most), and runs of one
// byte.  Each member is inflated with zlib (as a gzip member: header, CRC-32 and ISIZE are checked too) and with kr_inflate.h's
// inflate_member; BSIZE must be the member's size.  Length 0 is no member: the program checks that the bound is 0 there.  Prints a
// summary line and exits 0 when nothing differs.
#include "kr_deflate.h"
#include "kr_inflate.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

static uint64_t n_cases = 0, n_stored = 0, n_diff = 0, n_in = 0, n_out = 0;

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
  std::unique_ptr<uint8_t[]> slot(new uint8_t[n + kr::kDefOverhead]);
  std::unique_ptr<kr::DefState> S(new kr::DefState);
  kr::DefStats st;
  const uint32_t size = kr::bgzf_deflate_member_host(in.get(), n, 0, slot.get(), *S, &st);
  ++n_cases, n_stored += st.stored, n_in += n, n_out += size;
  if (size > n + kr::kDefOverhead || size > kr::bgzf_deflate_bound(n)) return differs("larger than the bound", kind, n);
  if (kr::bgzf_member_size(slot.get(), size) != size) return differs("BSIZE is not the member's size", kind, n);
  if (st.longest > kr::kDefMaxMatch || st.farthest > kr::kDefMaxDist) return differs("a match outside DEFLATE's limits", kind, n);
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

int main()
{
  std::mt19937_64 rng(20240702);
  if (kr::bgzf_deflate_bound(0) != 0 || kr::bgzf_deflate_members(0) != 0) differs("length 0 is no member", "empty", 0);
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
  printf("asan_bgzf_deflate: %llu members (%llu stored), %llu bytes in, %llu out, %llu differences\n", (unsigned long long)n_cases,
         (unsigned long long)n_stored, (unsigned long long)n_in, (unsigned long long)n_out, (unsigned long long)n_diff);
  return n_diff ? 1 : 0;
}
