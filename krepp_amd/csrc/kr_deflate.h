// kr_deflate.h — DEFLATE (RFC 1951) into ONE BGZF member, as one piece of code for the host and the device: the encoder that goes
// with kr_inflate.h's decoder.  A member takes at most 65,280 input bytes (0xff00, where bgzip cuts) and is laid out as
//   18-byte gzip header with the "BC" extra field (BSIZE) | one DEFLATE block | CRC-32 | ISIZE
// deflate_member() writes it into a slot of n + 31 bytes.  On the host it is a plain serial function (kr_bgzf_deflate_host, the
// sanitizer program scripts/asan_bgzf_deflate.cpp); on the device it is the body of kr_bgzf_deflate_kernel (kr_dev_deflate.inc): one
// wave per member.  What a wave does with all its lanes sits behind the `Lanes` argument, which has a serial form (DefSerial).
//
// THE ALGORITHM IS DEFINED IN TILES OF 64 POSITIONS, whatever the number of lanes, so the two forms give the same bytes:
//   lookup   every position p of the tile with 4 bytes in front of it hashes them and reads its candidate from the head table
//            (DefState::head: position + 1 of the LARGEST position entered with that hash, 0: none).  The table holds positions of
//            EARLIER tiles only: the tile's own positions are entered after every lookup of the tile.
//   verify   the position compares its candidate byte by byte: a match of 3 .. 258 bytes at a distance of 1 .. 32,768, or none.
//            A match never reaches past the member's input.
//   enter    the tile's positions are entered with a maximum (an LDS atomicMax on the device): the result does not depend on the
//            order of the lanes.
//   parse    greedy.  `next`, the first position not yet covered, is carried from tile to tile; inside the tile the token starts are
//            walked from it (start, start + max(1, its match length), ...): at most 64 steps, the same in every lane.
//   code     fixed Huffman codes (BTYPE 01).  A token is at most 31 bits (length code 8 + 5 extra, distance code 5 + 13 extra); an
//            exclusive prefix sum of the tokens' bit counts places them; the bits are ORed into a window of 32-bit words (atomicOr on
//            the device: OR commutes), the window's whole words go to the slot, the word that is left becomes the window's first.
//   stored   a coded block that would not be smaller than n + 5 bytes is given up -- no byte past n + 4 of the payload is ever
//            written -- and the member gets one stored block instead: a member is never larger than n + 31 bytes.
// Every step is a function of the input bytes and of the state the steps before left, none of the lane count or of timing.
//
// Bounds, for ANY input bytes: no read outside [in, in + n) (a hash is taken only where p + 4 <= n, a comparison stops at
// min(258, n - p)), no write outside [out, out + n + 31).
#ifndef KR_DEFLATE_H
#define KR_DEFLATE_H

#include "kr_inflate.h"

namespace kr {

constexpr uint32_t kDefMemberIn = 0xff00u;  // input bytes of a member
constexpr uint32_t kDefOverhead = 31u;      // header 18 + stored block 5 + trailer 8: a member of n bytes is at most n + 31
constexpr uint32_t kDefSlot = kDefMemberIn + 32u; // stride of the members' slots (a multiple of 32)
constexpr uint32_t kDefHashBits = 11u;
constexpr uint32_t kDefTile = 64u;
constexpr uint32_t kDefMinMatch = 3u, kDefMaxMatch = 258u, kDefMaxDist = 32768u;
constexpr uint32_t kDefWinWords = 66u; // carry (< 32 bits) + 64 tokens of at most 31 bits: 63 words, and room to spare

// State of one member: 8,712 bytes, fixed size (on the device: LDS, one per wave)
struct DefState {
  uint32_t head[1u << kDefHashBits]; // position + 1 of the largest position entered with this hash
  uint32_t win[kDefWinWords];        // the bits not yet written to the slot, the next one lowest in win[0]
  uint16_t len[kDefTile], dist[kDefTile]; // the tile's matches (len 0: none)
};

struct DefStats { // what the host form counts (kr_debug_bgzf_deflate_stats)
  uint64_t members = 0, stored = 0, literals = 0, matches = 0, longest = 0, farthest = 0;
};

// ---- lanes --------------------------------------------------------------------------------------------------------------------
// The serial form visits the positions of a tile in ascending order, so its prefix sum is a running total.
struct DefSerial {
  uint32_t run = 0;
  DefStats tok; // literals, matches, longest, farthest of the member in hand (coded or given up)
  KR_INF_HD uint32_t lane() const { return 0; }
  KR_INF_HD uint32_t nlanes() const { return 1; }
  KR_INF_HD void sync() const {}
  KR_INF_HD void head_max(uint32_t* p, uint32_t v) const
  {
    if (*p < v) *p = v;
  }
  KR_INF_HD void or_bits(uint32_t* p, uint32_t v) const { *p |= v; }
  KR_INF_HD void scan_begin() { run = 0; }
  KR_INF_HD uint32_t scan_excl(uint32_t v)
  {
    const uint32_t r = run;
    run += v;
    return r;
  }
  KR_INF_HD uint32_t scan_total() const { return run; }
  KR_INF_HD uint32_t crc(const uint32_t* tab, const uint8_t* p, uint32_t n) const { return ~crc_raw(tab, 0xFFFFFFFFu, p, n); }
  KR_INF_HD void token(uint32_t len, uint32_t dist)
  {
    if (!len) {
      ++tok.literals;
      return;
    }
    ++tok.matches;
    if (len > tok.longest) tok.longest = len;
    if (dist > tok.farthest) tok.farthest = dist;
  }
};

// ---- codes --------------------------------------------------------------------------------------------------------------------
KR_INF_HD inline uint32_t def_rev(uint32_t v, uint32_t nbits) // the low nbits of v, first bit last (Huffman codes go out first bit first)
{
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
  v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32u - nbits);
}
KR_INF_HD inline uint32_t def_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); } // v > 0

// One token in the fixed codes of RFC 1951 3.2.6, the first bit lowest.  len 0: the literal `byte`; else a match (3 <= len <= 258,
// 1 <= dist <= 32,768).  *nbits <= 31.
KR_INF_HD inline uint32_t def_token(uint32_t byte, uint32_t len, uint32_t dist, uint32_t* nbits)
{
  if (len == 0) {
    if (byte < 144u) {
      *nbits = 8;
      return def_rev(0x30u + byte, 8);
    }
    *nbits = 9;
    return def_rev(0x190u + (byte - 144u), 9);
  }
  uint32_t s, eb = 0, extra = 0; // length symbol 257 + s
  const uint32_t l = len - 3u;
  if (l < 8u) s = l;
  else if (len == 258u) s = 28u;
  else {
    eb = def_log2(l) - 2u;
    s = ((eb + 1u) << 2) | ((l >> eb) & 3u);
    extra = l & ((1u << eb) - 1u);
  }
  uint32_t bits, nb;
  if (s < 23u) bits = def_rev(s + 1u, 7), nb = 7; // symbols 256 .. 279: 7 bits from 0000000
  else bits = def_rev(0xC0u + (s - 23u), 8), nb = 8; // 280 .. 287: 8 bits from 11000000
  bits |= extra << nb, nb += eb;
  const uint32_t d = dist - 1u;
  uint32_t dc = d, deb = 0, dextra = 0;
  if (d >= 4u) {
    deb = def_log2(d) - 1u;
    dc = ((deb + 1u) << 1) | ((d >> deb) & 1u);
    dextra = d & ((1u << deb) - 1u);
  }
  bits |= def_rev(dc, 5) << nb, nb += 5u;
  bits |= dextra << nb, nb += deb;
  *nbits = nb;
  return bits;
}

KR_INF_HD inline uint32_t def_hash(const uint8_t* p) // of p[0 .. 4)
{
  const uint32_t v = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  return (v * 0x9E3779B1u) >> (32u - kDefHashBits);
}

// One member.  in[0 .. n), 1 <= n <= 65,280; out[0 .. n + 31): the member's slot.  Returns the member's size (<= n + 31).
// crc_tab: the 256 entries of crc_table_entry.
template <typename Lanes>
KR_INF_HD inline uint32_t deflate_member(const uint8_t* in, uint32_t n, uint8_t* out, DefState& S, const uint32_t* crc_tab, Lanes& L)
{
  const uint32_t nl = L.nlanes(), me = L.lane();
  for (uint32_t i = me; i < (1u << kDefHashBits); i += nl) S.head[i] = 0;
  for (uint32_t i = me; i < kDefWinWords; i += nl) S.win[i] = i ? 0u : 3u; // BFINAL = 1, BTYPE = 01
  L.sync();
  uint8_t* const pay = out + 18;
  const uint32_t limit = n + 4u; // the most payload bytes a coded block may take
  uint32_t nbits = 3, opos = 0, next = 0; // bits of the block so far; payload bytes written (= nbits / 32 * 4); first position not covered
  bool coded = true;
  for (uint32_t t0 = 0; t0 < n; t0 += kDefTile) {
    // lookup and verify
    for (uint32_t i = me; i < kDefTile; i += nl) {
      const uint32_t p = t0 + i;
      uint32_t len = 0, dist = 0;
      if (p + 4u <= n) {
        const uint32_t c = S.head[def_hash(in + p)]; // (c - 1 < t0 <= p)
        if (c && p + 1u - c <= kDefMaxDist) {
          const uint32_t cp = c - 1u, maxl = n - p < kDefMaxMatch ? n - p : kDefMaxMatch;
          uint32_t l = 0;
          while (l < maxl && in[cp + l] == in[p + l]) ++l;
          if (l >= kDefMinMatch) len = l, dist = p - cp;
        }
      }
      S.len[i] = (uint16_t)len, S.dist[i] = (uint16_t)dist; // (32,768 fits)
    }
    L.sync();
    // enter
    for (uint32_t i = me; i < kDefTile; i += nl) {
      const uint32_t p = t0 + i;
      if (p + 4u <= n) L.head_max(&S.head[def_hash(in + p)], p + 1u);
    }
    // parse: the same walk in every lane
    const uint32_t tend = n - t0 < kDefTile ? n : t0 + kDefTile;
    uint64_t starts = 0;
    uint32_t p = next > t0 ? next : t0;
    while (p < tend) {
      const uint32_t i = p - t0, l = S.len[i];
      starts |= 1ull << i;
      p += l ? l : 1u;
    }
    next = p;
    // code
    const uint32_t carry = nbits & 31u;
    L.scan_begin();
    for (uint32_t i = me; i < kDefTile; i += nl) {
      uint32_t bits = 0, nb = 0;
      if ((starts >> i) & 1u) {
        bits = def_token(in[t0 + i], S.len[i], S.dist[i], &nb);
        L.token(S.len[i], S.dist[i]);
      }
      const uint32_t o = carry + L.scan_excl(nb);
      if (nb) {
        L.or_bits(&S.win[o >> 5], bits << (o & 31u));
        if ((o & 31u) + nb > 32u) L.or_bits(&S.win[(o >> 5) + 1u], bits >> (32u - (o & 31u)));
      }
    }
    const uint32_t tile_bits = L.scan_total(), nw = (carry + tile_bits) >> 5;
    L.sync();
    // the window's whole words to the slot
    if (opos + nw * 4u > limit) {
      coded = false;
      break;
    }
    for (uint32_t b = me; b < nw * 4u; b += nl) pay[opos + b] = (uint8_t)(S.win[b >> 2] >> (8u * (b & 3u)));
    const uint32_t left = S.win[nw];
    L.sync();
    for (uint32_t i = me; i <= nw; i += nl) S.win[i] = i ? 0u : left;
    L.sync();
    opos += nw * 4u, nbits += tile_bits;
  }
  uint32_t cbytes = 0;
  if (coded) { // the end-of-block code: 7 zero bits, then zeros to the byte
    const uint32_t rem = ((nbits & 31u) + 7u + 7u) >> 3; // <= 5
    if (opos + rem > limit) coded = false;
    else {
      for (uint32_t b = me; b < rem; b += nl) pay[opos + b] = (uint8_t)(S.win[b >> 2] >> (8u * (b & 3u)));
      cbytes = opos + rem;
    }
  }
  if (!coded) { // one stored block: 00000001, LEN, NLEN, the bytes (over what the coded block left in the slot)
    L.sync();
    if (me == 0) {
      pay[0] = 1;
      pay[1] = (uint8_t)n, pay[2] = (uint8_t)(n >> 8);
      pay[3] = (uint8_t)~n, pay[4] = (uint8_t)(~n >> 8);
    }
    for (uint32_t i = me; i < n; i += nl) pay[5u + i] = in[i];
    cbytes = n + 5u;
  }
  const uint32_t crc = L.crc(crc_tab, in, n), size = 18u + cbytes + 8u;
  if (me == 0) {
    const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (uint32_t i = 0; i < 16; ++i) out[i] = h[i];
    out[16] = (uint8_t)(size - 1u), out[17] = (uint8_t)((size - 1u) >> 8);
    uint8_t* t = pay + cbytes;
    for (uint32_t i = 0; i < 4; ++i) t[i] = (uint8_t)(crc >> (8u * i)), t[4 + i] = (uint8_t)(n >> (8u * i));
  }
  L.sync();
  return size;
}

// members of n input bytes, and the most bytes they take
inline uint64_t bgzf_deflate_members(uint64_t n) { return (n + kDefMemberIn - 1) / kDefMemberIn; }
inline uint64_t bgzf_deflate_bound(uint64_t n) { return n + bgzf_deflate_members(n) * kDefOverhead; }

// the empty member that ends a BGZF file
inline void bgzf_eof(uint8_t* out28)
{
  const uint8_t e[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  memcpy(out28, e, 28);
}

// Host form: member m of text[0 .. n) into its slot; `st` (optional) is added to.  Returns the member's size.
inline uint32_t bgzf_deflate_member_host(const uint8_t* text, uint64_t n, uint64_t m, uint8_t* slot, DefState& S, DefStats* st)
{
  const uint64_t a = m * kDefMemberIn;
  const uint32_t len = (uint32_t)(n - a < kDefMemberIn ? n - a : kDefMemberIn);
  DefSerial L;
  const uint32_t size = deflate_member(text + a, len, slot, S, crc_host_table(), L);
  if (st) {
    ++st->members;
    if ((slot[18] & 6u) == 0) ++st->stored; // BTYPE 00
    else {
      st->literals += L.tok.literals, st->matches += L.tok.matches;
      if (L.tok.longest > st->longest) st->longest = L.tok.longest;
      if (L.tok.farthest > st->farthest) st->farthest = L.tok.farthest;
    }
  }
  return size;
}

} // namespace kr
#endif
