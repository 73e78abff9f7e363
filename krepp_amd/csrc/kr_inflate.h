// kr_inflate.h — raw DEFLATE (RFC 1951) for ONE BGZF member, as one piece of code for the host and the device, and the walk over
// the members of a block-gzipped buffer (host only).
//
// A BGZF member is an independent gzip member of at most 64 KB of inflated bytes that announces its compressed size ("BC" extra
// field) and its inflated size (ISIZE, trailer).  inflate_member() decodes one member's payload into [out, out + isize): the window
// of every match is the member's own output, nothing is shared between members.  On the host it is a plain serial function
// (kr_debug_bgzf_inflate_host, the sanitizer program scripts/asan_bgzf.cpp); on the device it is the body of kr_bgzf_inflate_kernel
// (kr_dev_bgzf.inc): one wave per member, every lane running the same symbol loop on the same bit buffer, the decode tables in LDS.
// What a wave does with all its lanes sits behind the `Lanes` argument, which has a serial form (InfSerial):
//   table fill   the direct-lookup tables are cleared and filled in strides of nlanes()
//   literals     a wave keeps up to 64 pending literals, one per lane, and stores them together
//   match copy   dst[i] = src[i % distance] in strides of nlanes() (distance < length is the periodic pattern)
//   CRC          crc_raw / crc_mulmod / crc_xpow8: lanes take contiguous slices, the partial registers are combined by x^(8n) mod P
//
// Bounds, for ANY input bytes: no read outside [in, in + in_size) -- a refill past the end yields zero bits and sets an error --, no
// write outside [out, out + isize); every loop is bounded by the remaining input bits or the remaining output bytes.  Members are
// accepted and rejected where zlib's inflate() does (tests/test_bgzf_host.py compares the two): over-subscribed code-length sets,
// incomplete sets other than a single code of length 1 (distance sets may be empty; the code-length code must be complete), a
// missing end-of-block code, a repeat without a previous length or across HLIT + HDIST, more than 286 / 30 symbols, block type 3,
// LEN != ~NLEN, a distance in front of the member's output, codes 286 / 287 and distance codes 30 / 31.
#ifndef KR_INFLATE_H
#define KR_INFLATE_H

#include <cstdint>
#include <cstring>
#include <string>

#if defined(__HIPCC__)
#define KR_INF_HD __host__ __device__
#else
#define KR_INF_HD
#endif

namespace kr {

// The first rule a member broke (a status word is rule << 24 | output position)
enum InfRule : uint32_t {
  INF_OK = 0,
  INF_INPUT_END = 1,     // the payload ends inside a block
  INF_BLOCK_TYPE = 2,    // block type 3
  INF_STORED_LEN = 3,    // stored block: LEN != ~NLEN
  INF_SYMBOL_COUNT = 4,  // more than 286 literal/length or 30 distance symbols
  INF_CODELEN_SET = 5,   // the code-length code is over-subscribed or incomplete
  INF_REPEAT = 6,        // a length repeat without a previous length, or across HLIT + HDIST
  INF_NO_END_CODE = 7,   // no end-of-block code
  INF_LITLEN_SET = 8,    // literal/length lengths over-subscribed or incomplete
  INF_DIST_SET = 9,      // distance lengths over-subscribed or incomplete
  INF_LITLEN_CODE = 10,  // a bit pattern that is no literal/length code, or code 286 / 287
  INF_DIST_CODE = 11,    // a bit pattern that is no distance code, or code 30 / 31
  INF_DIST_FAR = 12,     // a distance that reaches in front of the member's output
  INF_OUT_LONG = 13,     // more output than ISIZE
  INF_OUT_SHORT = 14,    // less output than ISIZE
  INF_INPUT_LEFT = 15,   // input left over before the trailer
  INF_CRC = 16,          // the inflated bytes do not have the trailer's CRC-32
  INF_RULES = 17
};

inline const char* inf_rule_name(uint32_t rule)
{
  static const char* const names[INF_RULES] = {"ok",
                                               "the payload ends inside a block",
                                               "block type 3",
                                               "stored block with LEN != ~NLEN",
                                               "too many length or distance symbols",
                                               "invalid code-length code",
                                               "invalid length repeat",
                                               "no end-of-block code",
                                               "invalid literal/length code lengths",
                                               "invalid distance code lengths",
                                               "invalid literal/length code",
                                               "invalid distance code",
                                               "distance in front of the member's output",
                                               "more output than ISIZE",
                                               "less output than ISIZE",
                                               "input left over before the trailer",
                                               "wrong CRC-32"};
  return rule < INF_RULES ? names[rule] : "unknown rule";
}

constexpr uint32_t kInfLitBits = 10, kInfDistBits = 8, kInfClBits = 7; // index bits of the direct-lookup tables
constexpr uint32_t kBgzfMaxIsize = 65536;

// Decode tables of one member: 3,648 bytes, fixed size (on the device: LDS, one per wave).  A code is looked up by its first bits
// in `fast` (entry: symbol << 4 | length, 0: longer than the index or no code) and otherwise walked length by length through the
// canonical form (cnt: codes per length, sym: symbols by code).
struct InfTables {
  uint16_t lit_fast[1u << kInfLitBits];
  uint16_t dist_fast[1u << kInfDistBits]; // the code-length code uses its first 128 entries while the lengths are read
  uint16_t lit_sym[288];
  uint16_t dist_sym[32];
  uint16_t lit_cnt[16], dist_cnt[16], offs[16];
  uint8_t lens[320];   // HLIT + HDIST <= 316 code lengths
  uint8_t cl_lens[32]; // 19 lengths of the code-length code
};

// ---- lanes --------------------------------------------------------------------------------------------------------------------
struct InfSerial {
  KR_INF_HD uint32_t lane() const { return 0; }
  KR_INF_HD uint32_t nlanes() const { return 1; }
  KR_INF_HD void sync() const {}
  KR_INF_HD void literal(uint8_t* out, uint32_t pos, uint8_t b) { out[pos] = b; }
  KR_INF_HD void flush(uint8_t*, uint32_t) {}
};

// ---- bits ---------------------------------------------------------------------------------------------------------------------
struct InfBits {
  const uint8_t* in;
  uint32_t ip, end; // next byte, end of the payload
  uint64_t bb;      // bits not yet taken, the next one lowest; zero above nb
  uint32_t nb;
  uint32_t over; // bits were taken that the payload does not have
  KR_INF_HD void refill()
  {
    while (nb <= 56 && ip < end) bb |= (uint64_t)in[ip++] << nb, nb += 8;
  }
  KR_INF_HD uint32_t peek(uint32_t n) const { return (uint32_t)bb & ((1u << n) - 1u); } // n <= 16
  KR_INF_HD void drop(uint32_t n)
  {
    if (n > nb) over = 1, bb = 0, nb = 0;
    else bb >>= n, nb -= n;
  }
  KR_INF_HD uint32_t take(uint32_t n)
  {
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
};

KR_INF_HD inline uint32_t inf_rev(uint32_t code, uint32_t len)
{
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r = (r << 1) | ((code >> i) & 1u);
  return r;
}

// Canonical tables of n code lengths.  kind 0: the code-length code (must be complete), 1: literal/length, 2: distance (1, 2: a
// single code of length 1 is accepted, 2: no code at all too).  0, or 1 for a set zlib's inflate_table rejects.
template <typename Lanes>
KR_INF_HD inline int inf_build(const uint8_t* lens, uint32_t n, uint16_t* cnt, uint16_t* offs, uint16_t* sym, uint16_t* fast, uint32_t fbits,
                               int kind, Lanes& L)
{
  for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
  for (uint32_t s = 0; s < n; ++s) cnt[lens[s] & 15u] = (uint16_t)(cnt[lens[s] & 15u] + 1);
  int32_t left = 1;
  uint32_t max = 0;
  for (uint32_t l = 1; l < 16; ++l) {
    left = (left << 1) - (int32_t)cnt[l];
    if (left < 0) return 1; // over-subscribed
    if (cnt[l]) max = l;
  }
  if (max == 0) {
    if (kind != 2) return 1;
  } else if (left > 0 && (kind == 0 || max != 1))
    return 1; // incomplete
  offs[1] = 0;
  for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lens[s] & 15u;
    if (l) {
      const uint32_t o = offs[l];
      sym[o] = (uint16_t)s; // (o < n: the counts sum to at most n)
      offs[l] = (uint16_t)(o + 1);
    }
  }
  const uint32_t total = n - cnt[0], fsize = 1u << fbits;
  L.sync();
  for (uint32_t i = L.lane(); i < fsize; i += L.nlanes()) fast[i] = 0;
  L.sync();
  for (uint32_t idx = L.lane(); idx < total; idx += L.nlanes()) {
    uint32_t first = 0, index = 0;
    for (uint32_t l = 1; l <= fbits; ++l) {
      const uint32_t c = cnt[l];
      if (idx - index < c) {
        const uint32_t r = inf_rev(first + (idx - index), l);
        const uint16_t e = (uint16_t)((uint32_t)sym[idx] << 4 | l);
        for (uint32_t k = r; k < fsize; k += 1u << l) fast[k] = e; // (a prefix code: no two symbols share an entry)
        break;
      }
      index += c;
      first = (first + c) << 1;
    }
  }
  L.sync();
  return 0;
}

// The next symbol: looked up by the code's first bits, else walked length by length (at most 15 steps); 0xFFFF: no code
KR_INF_HD inline uint32_t inf_symbol(InfBits& B, const uint16_t* cnt, const uint16_t* sym, const uint16_t* fast, uint32_t fbits)
{
  const uint32_t e = fast[B.peek(fbits)];
  if (e) {
    B.drop(e & 15u);
    return e >> 4;
  }
  uint32_t code = 0, first = 0, index = 0;
  const uint32_t bits = B.peek(15);
  for (uint32_t l = 1; l < 16; ++l) {
    code |= (bits >> (l - 1)) & 1u;
    const uint32_t c = cnt[l];
    if (code - first < c) {
      B.drop(l);
      return sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return 0xFFFFu;
}

// One member.  in[0 .. in_size): the raw deflate payload (between the gzip header and the 8-byte trailer); out[0 .. isize): where
// its bytes go.  Returns 0 or the first rule broken; *opos: the output position reached.  The CRC is the caller's.
template <typename Lanes>
KR_INF_HD inline uint32_t inflate_member(const uint8_t* in, uint32_t in_size, uint8_t* out, uint32_t isize, InfTables& T, Lanes& L, uint32_t* opos)
{
  InfBits B;
  B.in = in, B.ip = 0, B.end = in_size, B.bb = 0, B.nb = 0, B.over = 0;
  uint32_t pos = 0, rule = INF_OK, last = 0;
  const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  while (!last && !rule) { // a block takes at least 3 bits: bounded by the input
    B.refill();
    last = B.take(1);
    const uint32_t type = B.take(2);
    if (B.over) {
      rule = INF_INPUT_END;
      break;
    }
    if (type == 3) {
      rule = INF_BLOCK_TYPE;
      break;
    }
    if (type == 0) { // stored: to the byte boundary, LEN, NLEN, then LEN bytes as they are
      B.drop(B.nb & 7u);
      B.refill();
      const uint32_t len = B.take(16), nlen = B.take(16);
      if (B.over) {
        rule = INF_INPUT_END;
        break;
      }
      if (len != (nlen ^ 0xFFFFu)) {
        rule = INF_STORED_LEN;
        break;
      }
      B.ip -= B.nb >> 3, B.bb = 0, B.nb = 0; // (whole bytes only: the buffer was at a byte boundary)
      if (len > B.end - B.ip) {
        rule = INF_INPUT_END;
        break;
      }
      L.flush(out, pos);
      if (len > isize - pos) {
        rule = INF_OUT_LONG;
        break;
      }
      for (uint32_t i = L.lane(); i < len; i += L.nlanes()) out[pos + i] = in[B.ip + i];
      L.sync();
      B.ip += len, pos += len;
      continue;
    }
    uint32_t nlen = 288, ndist = 32;
    if (type == 1) { // fixed codes (RFC 1951 3.2.6); 286, 287 and distances 30, 31 have codes and are refused below
      for (uint32_t s = 0; s < 288; ++s) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
      for (uint32_t s = 0; s < 32; ++s) T.lens[288 + s] = 5;
    } else {
      nlen = B.take(5) + 257, ndist = B.take(5) + 1;
      const uint32_t ncode = B.take(4) + 4;
      if (B.over) {
        rule = INF_INPUT_END;
        break;
      }
      if (nlen > 286 || ndist > 30) {
        rule = INF_SYMBOL_COUNT;
        break;
      }
      for (uint32_t i = 0; i < 19; ++i) {
        if ((i & 15u) == 0) B.refill();
        T.cl_lens[cl_order[i]] = i < ncode ? (uint8_t)B.take(3) : (uint8_t)0;
      }
      if (B.over) {
        rule = INF_INPUT_END;
        break;
      }
      if (inf_build(T.cl_lens, 19, T.dist_cnt, T.offs, T.dist_sym, T.dist_fast, kInfClBits, 0, L)) {
        rule = INF_CODELEN_SET;
        break;
      }
      uint32_t have = 0;
      while (have < nlen + ndist) { // every step stores at least one length
        B.refill();
        const uint32_t s = inf_symbol(B, T.dist_cnt, T.dist_sym, T.dist_fast, kInfClBits);
        if (s == 0xFFFFu) { // (a complete code has no unused pattern: only when the input ended)
          rule = INF_CODELEN_SET;
          break;
        }
        if (s < 16) {
          if (B.over) break;
          T.lens[have++] = (uint8_t)s;
          continue;
        }
        uint32_t prev = 0, rep;
        if (s == 16) {
          if (B.over) break;
          if (have == 0) {
            rule = INF_REPEAT;
            break;
          }
          prev = T.lens[have - 1];
          rep = 3 + B.take(2);
        } else if (s == 17)
          rep = 3 + B.take(3);
        else
          rep = 11 + B.take(7);
        if (B.over) break;
        if (have + rep > nlen + ndist) {
          rule = INF_REPEAT;
          break;
        }
        for (uint32_t i = 0; i < rep; ++i) T.lens[have++] = (uint8_t)prev;
      }
      if (!rule && B.over) rule = INF_INPUT_END;
      if (rule) break;
      if (T.lens[256] == 0) {
        rule = INF_NO_END_CODE;
        break;
      }
    }
    if (inf_build(T.lens, nlen, T.lit_cnt, T.offs, T.lit_sym, T.lit_fast, kInfLitBits, 1, L)) {
      rule = INF_LITLEN_SET;
      break;
    }
    if (inf_build(T.lens + nlen, ndist, T.dist_cnt, T.offs, T.dist_sym, T.dist_fast, kInfDistBits, 2, L)) {
      rule = INF_DIST_SET;
      break;
    }
    for (;;) { // a symbol takes at least one bit: bounded by the input (B.over ends it)
      B.refill(); // >= 57 bits unless the payload ends: a length / distance pair takes at most 15 + 5 + 15 + 13
      uint32_t s = inf_symbol(B, T.lit_cnt, T.lit_sym, T.lit_fast, kInfLitBits);
      if (B.over) {
        rule = INF_INPUT_END;
        break;
      }
      if (s < 256) {
        if (pos >= isize) {
          rule = INF_OUT_LONG;
          break;
        }
        L.literal(out, pos, (uint8_t)s);
        ++pos;
        continue;
      }
      if (s == 256) break;
      if (s >= 286) { // 0xFFFF too
        rule = INF_LITLEN_CODE;
        break;
      }
      s -= 257;
      uint32_t len;
      if (s < 8) len = 3 + s;
      else if (s == 28) len = 258;
      else {
        const uint32_t eb = (s >> 2) - 1;
        len = 3 + ((4 + (s & 3u)) << eb) + B.take(eb);
      }
      const uint32_t d = inf_symbol(B, T.dist_cnt, T.dist_sym, T.dist_fast, kInfDistBits);
      if (B.over) {
        rule = INF_INPUT_END;
        break;
      }
      if (d >= 30) {
        rule = INF_DIST_CODE;
        break;
      }
      uint32_t dist;
      if (d < 4) dist = 1 + d;
      else {
        const uint32_t eb = (d >> 1) - 1;
        dist = 1 + ((2 + (d & 1u)) << eb) + B.take(eb);
      }
      if (B.over) {
        rule = INF_INPUT_END;
        break;
      }
      if (dist > pos) {
        rule = INF_DIST_FAR;
        break;
      }
      if (len > isize - pos) {
        rule = INF_OUT_LONG;
        break;
      }
      L.flush(out, pos);
      const uint8_t* src = out + (pos - dist); // [pos - dist, pos) was written before this match: no lane reads what another writes now
      if (dist >= len)
        for (uint32_t i = L.lane(); i < len; i += L.nlanes()) out[pos + i] = src[i];
      else
        for (uint32_t i = L.lane(); i < len; i += L.nlanes()) out[pos + i] = src[i % dist];
      L.sync();
      pos += len;
    }
  }
  L.flush(out, pos);
  if (!rule && pos != isize) rule = INF_OUT_SHORT;
  if (!rule && (B.end - B.ip) + (B.nb >> 3) != 0) rule = INF_INPUT_LEFT;
  *opos = pos;
  return rule;
}

// ---- CRC-32 (zlib's: reflected 0xEDB88320) ----------------------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
KR_INF_HD inline uint32_t crc_table_entry(uint32_t i)
{
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}
// the CRC register r after n more bytes (no conditioning: crc32(p, n) = ~crc_raw(tab, ~0, p, n))
KR_INF_HD inline uint32_t crc_raw(const uint32_t* tab, uint32_t r, const uint8_t* p, uint32_t n)
{
  for (uint32_t i = 0; i < n; ++i) r = tab[(r ^ p[i]) & 0xFFu] ^ (r >> 8);
  return r;
}
// a * b mod P over GF(2), bit 31 = x^0
KR_INF_HD inline uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// x^(8 n) mod P: what n zero bytes do to a register
KR_INF_HD inline uint32_t crc_xpow8(uint32_t n)
{
  uint32_t p = 1u << 31, sq = 1u << 23; // x^0, x^8
  for (; n; n >>= 1) {
    if (n & 1u) p = crc_mulmod(sq, p);
    sq = crc_mulmod(sq, sq);
  }
  return p;
}
// Slices for `nl` lanes: the bytes are thought of as right-aligned in nl slices of `per` bytes each, zeros in front (zeros do
// nothing to a zero register).  Lane l takes [a, b); its register is crc_raw(tab, 0, p + a, b - a).  A pair of neighbouring
// runs A, B of s slices each combines to crc_mulmod(x^(8 s per), A) ^ B; the whole: ~(crc_mulmod(x^(8 n), ~0) ^ all).
KR_INF_HD inline void crc_slice(uint32_t n, uint32_t nl, uint32_t l, uint32_t* per, uint32_t* a, uint32_t* b)
{
  const uint32_t p = (n + nl - 1) / nl, pad = p * nl - n;
  const uint32_t lo = l * p, hi = lo + p;
  *per = p;
  *a = lo > pad ? lo - pad : 0;
  *b = hi > pad ? hi - pad : 0;
}
// the serial form of what a wave does: 64 slices, combined pairwise
inline uint32_t crc_sliced_host(const uint32_t* tab, const uint8_t* p, uint32_t n)
{
  uint32_t part[64], per = 0;
  for (uint32_t l = 0; l < 64; ++l) {
    uint32_t a, b;
    crc_slice(n, 64, l, &per, &a, &b);
    part[l] = crc_raw(tab, 0, p + a, b - a);
  }
  uint32_t op = crc_xpow8(per);
  for (uint32_t s = 1; s < 64; s <<= 1) {
    for (uint32_t l = 0; l < 64; l += 2 * s) part[l] = crc_mulmod(op, part[l]) ^ part[l + s];
    op = crc_mulmod(op, op);
  }
  return ~(crc_mulmod(crc_xpow8(n), 0xFFFFFFFFu) ^ part[0]);
}
inline const uint32_t* crc_host_table()
{
  static const struct Tab {
    uint32_t t[256];
    Tab()
    {
      for (uint32_t i = 0; i < 256; ++i) t[i] = crc_table_entry(i);
    }
  } tab;
  return tab.t;
}

// ---- the members of a block-gzipped buffer (host) -----------------------------------------------------------------------------
// size of the BGZF member that starts at h (0: these bytes are not the start of one)
inline uint32_t bgzf_member_size(const uint8_t* h, uint64_t avail)
{
  if (avail < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return 0;
  const uint32_t xlen = h[10] | (h[11] << 8);
  if (avail < 12 + (uint64_t)xlen) return 0;
  for (uint32_t p = 12; p + 4 <= 12 + xlen;) {
    const uint32_t slen = h[p + 2] | (h[p + 3] << 8);
    if (h[p] == 'B' && h[p + 1] == 'C' && slen == 2 && p + 6 <= 12 + xlen) return (uint32_t)(h[p + 4] | (h[p + 5] << 8)) + 1u;
    p += 4 + slen;
  }
  return 0;
}

struct BgzfMember { // one entry of the kernel's member table: 32 bytes
  uint32_t in_off, in_size; // the deflate payload in the compressed chunk
  uint32_t isize, crc;      // the trailer
  int64_t out_pos;          // of the member's first byte in the chunk (negative: the front belongs to the chunk before)
  uint32_t window;          // 0: the member lies inside the chunk and is inflated in place; 1, 2: into that scratch window first
  uint32_t pad;
};

inline uint32_t bgzf_le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// The member at buf[off ..): its table entry but for out_pos / window.  0, or why these bytes are no whole, well-formed member.
inline const char* bgzf_member_at(const uint8_t* buf, uint64_t n, uint64_t off, BgzfMember* m, uint32_t* msize)
{
  const uint32_t ms = off < n ? bgzf_member_size(buf + off, n - off) : 0;
  if (ms == 0) return "not a BGZF member";
  if (ms > n - off) return "the member is cut short";
  const uint8_t* h = buf + off;
  if (h[3] & ~4u) return "gzip header flags other than FEXTRA"; // (a name, comment or header CRC would sit in front of the payload)
  const uint32_t xlen = h[10] | (h[11] << 8);
  if (12ull + xlen + 8 > ms) return "the extra field is larger than the member";
  m->in_off = (uint32_t)(off + 12 + xlen), m->in_size = ms - 12 - xlen - 8;
  m->crc = bgzf_le32(h + ms - 8), m->isize = bgzf_le32(h + ms - 4);
  m->out_pos = 0, m->window = 0, m->pad = 0;
  if (m->isize > kBgzfMaxIsize) return "ISIZE above 65,536";
  *msize = ms;
  return nullptr;
}

// the message of a rejected member, the same from the host decoder and from the kernel's status word
inline std::string bgzf_member_message(const char* who, uint64_t member_off, uint32_t rule, uint32_t pos)
{
  return std::string(who) + ": BGZF member at offset " + std::to_string(member_off) + ": " + inf_rule_name(rule) + " (at output byte " +
         std::to_string(pos) + ")";
}

} // namespace kr
#endif
