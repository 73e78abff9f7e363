// asan_bgzf_member.cpp -- the member length as a parameter of the BGZF encoder's host instantiation (krepp_amd/csrc/kr_deflate.h:
// bgzf_deflate_member_host / bgzf_deflate_member_host_dyn with member_in) under AddressSanitizer and UBSan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ikrepp_amd/csrc scripts/asan_bgzf_member.cpp -lz -o asan_bgzf_member
//   ./asan_bgzf_member
//
// A stand-alone program: it runs on the CPU and needs no device.  Every (member length, text length) pair of
// tests/test_bgzf_member_host.py -- member lengths 256, 257, 4,099, 16,320 and 65,279, texts of k L - 1, k L and k L + 1 bytes for
// k = 1 and 3 -- in report-shaped, random and few-symbol bytes.  The text lies in a heap block of exactly its size; member m is cut
// out of it by the functions under test (text + m * member_in, at any alignment) and written into a block of exactly its own
// length + 31 bytes, its tokens (level 2) into a block of exactly its own length in tokens: one byte read or written outside any of
// them is reported.  Each member is inflated with zlib (as a gzip member: header, CRC-32 and ISIZE are checked too) and with
// kr_inflate.h's inflate_member, and must give its part of the text; a level-2 member must not be larger than the level-1 member.
// Prints a summary line and exits 0 when nothing differs.
#include "kr_deflate.h"
#include "kr_inflate.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

static uint64_t n_members = 0, n_diff = 0, n_in = 0, n_out = 0;

static void differs(const char* what, const char* kind, uint32_t L, uint64_t n, uint64_t m)
{
  ++n_diff;
  fprintf(stderr, "DIFFERENT: %s text of %llu bytes, member length %u, member %llu: %s\n", kind, (unsigned long long)n, L, (unsigned long long)m, what);
}

static bool inflates_to(const uint8_t* slot, uint32_t size, const uint8_t* part, uint32_t len, const char** why)
{
  { // zlib, as a gzip member
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 31) != Z_OK) abort();
    std::vector<uint8_t> out(len + 1);
    zs.next_in = const_cast<uint8_t*>(slot), zs.avail_in = size;
    zs.next_out = out.data(), zs.avail_out = len + 1;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == len && zs.avail_in == 0 && memcmp(out.data(), part, len) == 0;
    inflateEnd(&zs);
    if (!ok) return *why = "zlib does not inflate the member to its part of the text", false;
  }
  kr::BgzfMember bm;
  uint32_t ms = 0, pos = 0;
  if (kr::bgzf_member_at(slot, size, 0, &bm, &ms) || ms != size || bm.isize != len) return *why = "bgzf_member_at refuses the member", false;
  std::unique_ptr<uint8_t[]> out(new uint8_t[len]);
  std::unique_ptr<kr::InfTables> T(new kr::InfTables);
  kr::InfSerial Li;
  const uint32_t rule = kr::inflate_member(slot + bm.in_off, bm.in_size, out.get(), len, *T, Li, &pos);
  if (rule || memcmp(out.get(), part, len) != 0) return *why = "inflate_member does not return the member's part of the text", false;
  if (~kr::crc_raw(kr::crc_host_table(), 0xFFFFFFFFu, out.get(), len) != bm.crc) return *why = "wrong CRC-32", false;
  return true;
}

static void one(const std::vector<uint8_t>& data, uint32_t L, const char* kind)
{
  const uint64_t n = data.size();
  std::unique_ptr<uint8_t[]> text(new uint8_t[n]); // an exact block: the sanitizer sees the first byte outside
  memcpy(text.get(), data.data(), n);
  std::unique_ptr<kr::DefState> S1(new kr::DefState);
  std::unique_ptr<kr::DefDynState> S2(new kr::DefDynState);
  const uint64_t nm = kr::bgzf_deflate_members(n, L);
  if (nm != (n + L - 1) / L) return differs("the member count is not ceil(n / L)", kind, L, n, 0);
  uint64_t total1 = 0, total2 = 0;
  for (uint64_t m = 0; m < nm; ++m) {
    const uint32_t len = (uint32_t)(n - m * L < L ? n - m * L : L);
    std::unique_ptr<uint8_t[]> slot1(new uint8_t[len + kr::kDefOverhead]), slot2(new uint8_t[len + kr::kDefOverhead]);
    std::unique_ptr<uint32_t[]> tok(new uint32_t[len]);
    const uint32_t size1 = kr::bgzf_deflate_member_host(text.get(), n, m, slot1.get(), *S1, nullptr, L);
    const uint32_t size2 = kr::bgzf_deflate_member_host_dyn(text.get(), n, m, slot2.get(), *S2, tok.get(), nullptr, L);
    ++n_members, n_in += len, n_out += size1 + size2;
    total1 += size1, total2 += size2;
    if (size1 > len + kr::kDefOverhead || size2 > size1) return differs("larger than its bound", kind, L, n, m);
    const char* why = "";
    if (!inflates_to(slot1.get(), size1, text.get() + m * L, len, &why)) return differs(why, kind, L, n, m);
    if (!inflates_to(slot2.get(), size2, text.get() + m * L, len, &why)) return differs(why, kind, L, n, m);
  }
  if (total1 > kr::bgzf_deflate_bound(n, L) || total2 > kr::bgzf_deflate_bound(n, L)) differs("larger than bgzf_deflate_bound", kind, L, n, nm);
}

static std::vector<uint8_t> report_text(uint64_t n, std::mt19937_64& rng)
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
  std::mt19937_64 rng(20241021);
  const uint32_t lengths[] = {256, 257, 4099, 16320, 65279};
  for (uint32_t L : lengths) {
    if (!kr::bgzf_member_in_ok(L) || kr::bgzf_slot_stride(L) < L + kr::kDefOverhead || kr::bgzf_slot_stride(L) % 32u) return fprintf(stderr, "member length %u: no slot stride\n", L), 1;
    for (uint32_t k : {1u, 3u})
      for (int d = -1; d <= 1; ++d) {
        const uint64_t n = (uint64_t)k * L + d;
        one(report_text(n, rng), L, "report");
        std::vector<uint8_t> v(n);
        for (auto& b : v) b = (uint8_t)rng();
        one(v, L, "random");
        for (auto& b : v) b = (uint8_t)("ACGT"[rng() % 4]); // few symbols: matches that reach the member's last byte, and across where the cut is
        one(v, L, "few symbols");
      }
  }
  if (kr::bgzf_member_in_ok(255) || kr::bgzf_member_in_ok(65281) || kr::bgzf_slot_stride(kr::kDefMemberIn) != kr::kDefSlot) return fprintf(stderr, "the limits of the member length are not 256 and 65,280\n"), 1;
  printf("asan_bgzf_member: %llu members at levels 1 and 2, %llu bytes in, %llu out, %llu differences\n", (unsigned long long)n_members,
         (unsigned long long)n_in, (unsigned long long)n_out, (unsigned long long)n_diff);
  return n_diff ? 1 : 0;
}
