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
//
// LEVEL 2 (deflate_member_dyn; kr_bgzf_deflate_host_level, kr_bgzf_deflate_dyn_kernel) codes THE SAME TOKENS under dynamic Huffman
// codes (BTYPE 10), in two passes.  Level 1 is deflate_member above, untouched: the default, the same bytes as ever.
//   pass 1   lookup, verify, enter and parse as above, in tiles of 64 positions.  A tile's tokens are not coded: token k of the
//            member -- k = the tokens of the tiles before + the token starts below it in its tile -- goes to tok[k] (4 bytes:
//            length in the low half, 0 for a literal; the byte or the distance in the high half; global memory on the device,
//            kDefTokStride tokens a member) and is counted in a literal/length histogram of 286 and a distance histogram of 30
//            entries in the state (integer adds: an LDS atomic add on the device, so the order of the lanes does not matter).  The
//            end-of-block symbol counts once.
//   codes    ONE lane (def_dyn_plan).  As zlib does, a histogram with fewer than two counts gets its lowest symbols without a
//            count counted once until it has two (def_force_two): every code sent is complete.  def_build_lengths gives the code
//            lengths (at most 15 bits for the two alphabets, 7 for the code-length alphabet; its comment says how), def_canonical
//            the codes of RFC 1951 3.2.2.
//   header   HLIT (>= 257), HDIST, HCLEN and the code-length code's lengths in the RFC's order, then the HLIT + HDIST lengths as
//            ONE sequence, run-length coded by this rule: at position i with value v and r equal values from i on (counted up to
//            138): v = 0 and r >= 11: symbol 18 for all r; v = 0 and r >= 3: symbol 17 for r; v != 0, v the length sent last and
//            r >= 3: symbol 16 for min(r, 6); else v itself, for one position.  One lane writes the header straight into the
//            payload in whole words (def_dyn_header); the bits that are left (< 32) become the window's first word.  The header
//            is never held whole.
//   choice   all three sizes are known exactly after pass 1, from the histograms: S = n + 5 (stored), F (the fixed-code block of
//            these tokens), D (the dynamic block, header included).  min(F, D) >= S: stored; else dynamic if D < F; else fixed.
//            Level 1 codes with fixed codes exactly when F < S, so where level 2 picks fixed or stored it writes level 1's bytes,
//            and a level-2 member is never larger than the level-1 member.  A coded block is below n + 5 bytes before a bit of it
//            is written: nothing is given up half way, nothing is written past n + 31.
//   pass 2   tiles of 64 TOKENS, a lane each: the token's bits (at most 48: 15 + 5 extra, 15 + 13 extra, in 64 bits) are placed by
//            an exclusive prefix sum and ORed into up to three words of the window (kDefDynWinWords: 31 + 64 x 48 bits), whole
//            words go to the slot, as above; then the end-of-block code.
// The head table is dead behind pass 1: the builder's scratch and the code tables lie over it (DefDynState: 10,128 bytes).
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

// ---- level 2 (dynamic codes) ----
constexpr uint32_t kDefLL = 286u, kDefD = 30u, kDefCL = 19u; // symbols of the literal/length, distance and code-length alphabets
constexpr uint32_t kDefTokStride = kDefMemberIn; // tokens of 4 bytes a member has room for in the token list (one a byte at most)
constexpr uint32_t kDefDynWinWords = 100u; // carry (< 32 bits) + 64 tokens of at most 48 bits: 97 words, and room to spare
constexpr uint32_t kDefMaxFreq = (1u << 22) - 1u; // the largest count def_build_lengths takes (a member's are at most 65,281)

struct DefBuild { // scratch of def_build_lengths
  uint32_t a[kDefLL];    // sort keys, then the tree, then the depths
  uint16_t perm[kDefLL]; // the symbols with a count, by (count, symbol)
};

struct DefCodes { // what is made between the passes: alive while the head table is dead, and lies over it
  DefBuild build;
  uint16_t ll_code[kDefLL], d_code[kDefD], cl_code[kDefCL]; // the first bit lowest
  uint8_t ll_len[kDefLL], d_len[kDefD], cl_len[kDefCL];
  uint32_t cl_cnt[kDefCL];
  uint16_t next_code[16];       // def_canonical's
  uint16_t seq[kDefLL + kDefD]; // the run-length coded lengths: symbol | extra << 8
  uint32_t nseq, hlit, hdist, hclen;
};

// State of one member at level 2: 10,128 bytes, fixed size (on the device: LDS, one per wave)
struct DefDynState {
  union {
    uint32_t head[1u << kDefHashBits]; // pass 1
    DefCodes c;                        // between the passes and pass 2
  };
  uint32_t win[kDefDynWinWords];
  uint16_t len[kDefTile], dist[kDefTile];
  uint32_t ll_cnt[kDefLL], d_cnt[kDefD]; // what pass 1 counts
  uint32_t btype, limited, hdr_bits, pad; // what became of the member: 0 stored / 1 fixed / 2 dynamic; a code was limited; header bits
};

struct DefStats { // what the host form counts (kr_debug_bgzf_deflate_stats, kr_debug_bgzf_deflate_stats_level)
  uint64_t members = 0, stored = 0, literals = 0, matches = 0, longest = 0, farthest = 0;
  uint64_t fixed = 0, dynamic = 0, limited = 0, header_bits = 0;
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
  KR_INF_HD void add(uint32_t* p, uint32_t v) const { *p += v; }
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

// The three helpers below are level 2's: deflate_member keeps these steps in its own body, as it was written, so that level 1's
// kernel stays what it was instruction for instruction (78 VGPRs; with the steps shared it took 82).  A change to a step is made
// in both places, and tests/test_bgzf_deflate_dyn_host.py holds level 2's fixed-code members to level 1's bytes.
// One stored block in the payload: 00000001, LEN, NLEN, the bytes (over what a coded block left in the slot).  Returns n + 5.
template <typename Lanes>
KR_INF_HD inline uint32_t def_stored(const uint8_t* in, uint32_t n, uint8_t* pay, Lanes& L)
{
  const uint32_t nl = L.nlanes(), me = L.lane();
  L.sync();
  if (me == 0) {
    pay[0] = 1;
    pay[1] = (uint8_t)n, pay[2] = (uint8_t)(n >> 8);
    pay[3] = (uint8_t)~n, pay[4] = (uint8_t)(~n >> 8);
  }
  for (uint32_t i = me; i < n; i += nl) pay[5u + i] = in[i];
  return n + 5u;
}

// The gzip header with BSIZE in front of a payload of cbytes and the trailer behind it.  Returns the member's size.
template <typename Lanes>
KR_INF_HD inline uint32_t def_frame(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cbytes, const uint32_t* crc_tab, Lanes& L)
{
  const uint32_t crc = L.crc(crc_tab, in, n), size = 18u + cbytes + 8u;
  if (L.lane() == 0) {
    const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (uint32_t i = 0; i < 16; ++i) out[i] = h[i];
    out[16] = (uint8_t)(size - 1u), out[17] = (uint8_t)((size - 1u) >> 8);
    uint8_t* t = out + 18 + cbytes;
    for (uint32_t i = 0; i < 4; ++i) t[i] = (uint8_t)(crc >> (8u * i)), t[4 + i] = (uint8_t)(n >> (8u * i));
  }
  return size;
}

// Lookup, verify, enter and parse of the tile at t0 (the header comment): the tile's matches are left in S.len / S.dist, *next is
// carried on, and the result has bit i set where position t0 + i starts a token.  The same in every lane.
template <typename State, typename Lanes>
KR_INF_HD inline uint64_t def_tile_parse(const uint8_t* in, uint32_t n, uint32_t t0, State& S, Lanes& L, uint32_t* next)
{
  const uint32_t nl = L.nlanes(), me = L.lane();
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
  uint32_t p = *next > t0 ? *next : t0;
  while (p < tend) {
    const uint32_t i = p - t0, l = S.len[i];
    starts |= 1ull << i;
    p += l ? l : 1u;
  }
  *next = p;
  return starts;
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

// ---- level 2: the same tokens under dynamic Huffman codes (the header comment, LEVEL 2) ------------------------------------------
// length 3 .. 258 -> symbol 257 + the result, with *eb extra bits of value *extra
KR_INF_HD inline uint32_t def_len_sym(uint32_t len, uint32_t* eb, uint32_t* extra)
{
  const uint32_t l = len - 3u;
  *eb = 0, *extra = 0;
  if (l < 8u) return l;
  if (len == 258u) return 28u;
  *eb = def_log2(l) - 2u;
  *extra = l & ((1u << *eb) - 1u);
  return ((*eb + 1u) << 2) | ((l >> *eb) & 3u);
}
// distance 1 .. 32,768 -> its symbol, with *eb extra bits of value *extra
KR_INF_HD inline uint32_t def_dist_sym(uint32_t dist, uint32_t* eb, uint32_t* extra)
{
  const uint32_t d = dist - 1u;
  *eb = 0, *extra = 0;
  if (d < 4u) return d;
  *eb = def_log2(d) - 1u;
  *extra = d & ((1u << *eb) - 1u);
  return ((*eb + 1u) << 1) | ((d >> *eb) & 1u);
}
KR_INF_HD inline uint32_t def_ll_extra(uint32_t s) { return s < 265u || s == 285u ? 0u : ((s - 257u) >> 2) - 1u; } // extra bits of symbol s
KR_INF_HD inline uint32_t def_d_extra(uint32_t d) { return d < 4u ? 0u : (d >> 1) - 1u; }
KR_INF_HD inline uint32_t def_ll_fixed(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; } // RFC 1951 3.2.6

// Code lengths for the counts freq[0 .. nsym) (nsym <= 286, every count <= kDefMaxFreq, 2^maxbits >= the symbols with a count),
// none longer than maxbits; returns whether the limit was needed.  Scalar, deterministic, no allocation, no recursion.
//   The symbols with a count are sorted by (count, symbol) -- a shell sort over keys count << 9 | symbol -- and the in-place
//   algorithm of Moffat and Katajainen builds a minimum-redundancy code over the sorted counts; where two weights are equal it
//   takes the leaf before the inner node, which gives the Huffman code of the least depth.  If that is deeper than maxbits, all
//   counts are halved, rounding up (round r: ceil(count / 2^r), so the order stands and no count becomes 0), and the code is
//   built again: after 22 rounds at the latest all counts are 1 and the depth is ceil(log2(symbols)).
// Result: zero count <=> zero length; with two counts or more the Kraft sum is exactly 1; a larger count never has a longer code
// (lengths fall along the sorted order); cost = the Huffman optimum whenever no round was needed.  A single count gets length 1.
KR_INF_HD inline bool def_build_lengths(const uint32_t* freq, uint32_t nsym, uint32_t maxbits, uint8_t* lens, DefBuild& B)
{
  uint32_t* const A = B.a;
  uint32_t m = 0;
  for (uint32_t i = 0; i < nsym; ++i) {
    lens[i] = 0;
    if (freq[i]) A[m++] = (freq[i] << 9) | i;
  }
  if (m == 0) return false;
  if (m == 1) {
    lens[A[0] & 511u] = 1;
    return false;
  }
  for (uint32_t gap = 121; gap; gap /= 3) // 121, 40, 13, 4, 1
    for (uint32_t i = gap; i < m; ++i) {
      const uint32_t k = A[i];
      uint32_t j = i;
      while (j >= gap && A[j - gap] > k) A[j] = A[j - gap], j -= gap;
      A[j] = k;
    }
  for (uint32_t i = 0; i < m; ++i) B.perm[i] = (uint16_t)(A[i] & 511u);
  bool limited = false;
  for (uint32_t shift = 0; shift < 23; ++shift) {
    const uint32_t round = (1u << shift) - 1u;
    for (uint32_t i = 0; i < m; ++i) A[i] = (freq[B.perm[i]] + round) >> shift;
    // phase 1: the tree, inner node `next` made of the two least of what is left; A[root .. next) weights, below root parents
    A[0] += A[1];
    uint32_t root = 0, leaf = 2;
    for (uint32_t next = 1; next + 1 < m; ++next) {
      if (leaf >= m || A[root] < A[leaf]) A[next] = A[root], A[root++] = next;
      else A[next] = A[leaf++];
      if (leaf >= m || (root < next && A[root] < A[leaf])) A[next] += A[root], A[root++] = next;
      else A[next] += A[leaf++];
    }
    // phase 2: the inner nodes' depths
    A[m - 2] = 0;
    for (uint32_t next = m - 2; next-- > 0;) A[next] = A[A[next]] + 1u;
    // phase 3: the leaves' depths, the deepest first in A
    int32_t avbl = 1, used = 0, r = (int32_t)m - 2, nx = (int32_t)m - 1;
    for (uint32_t dpth = 0; avbl > 0; ++dpth) {
      while (r >= 0 && A[r] == dpth) ++used, --r;
      while (avbl > used) A[nx--] = dpth, --avbl;
      avbl = 2 * used, used = 0;
    }
    if (A[0] <= maxbits) break;
    limited = true;
  }
  for (uint32_t i = 0; i < m; ++i) lens[B.perm[i]] = (uint8_t)A[i];
  return limited;
}

// what def_build_lengths asks of its arguments (the debug calls check it; the encoder's own counts meet it)
inline bool def_build_args_ok(const uint32_t* freq, uint32_t nsym, uint32_t maxbits)
{
  if (nsym < 1u || nsym > kDefLL || maxbits < 1u || maxbits > 15u) return false;
  uint32_t counted = 0;
  for (uint32_t i = 0; i < nsym; ++i) {
    if (freq[i] > kDefMaxFreq) return false;
    counted += freq[i] != 0;
  }
  return counted <= (1u << maxbits);
}

// The canonical codes of RFC 1951 3.2.2 for lens[0 .. nsym) (each <= 15), the first bit lowest.  next: 16 entries of scratch.
KR_INF_HD inline void def_canonical(const uint8_t* lens, uint32_t nsym, uint16_t* codes, uint16_t* next)
{
  for (uint32_t b = 0; b < 16; ++b) next[b] = 0;
  for (uint32_t i = 0; i < nsym; ++i)
    if (lens[i]) ++next[lens[i]];
  uint32_t code = 0, before = 0; // `before`: the codes one bit shorter
  for (uint32_t b = 1; b < 16; ++b) {
    code = (code + before) << 1;
    before = next[b], next[b] = (uint16_t)code;
  }
  for (uint32_t i = 0; i < nsym; ++i) codes[i] = lens[i] ? (uint16_t)def_rev(next[lens[i]]++, lens[i]) : (uint16_t)0;
}

// As zlib does: a histogram with fewer than two counts gets its lowest symbols without one counted once until it has two, so
// that the code sent is complete and any inflater accepts it.  *f0, *f1: the symbols so counted (nsym: none).
KR_INF_HD inline void def_force_two(uint32_t* cnt, uint32_t nsym, uint32_t* f0, uint32_t* f1)
{
  uint32_t nz = 0;
  for (uint32_t i = 0; i < nsym; ++i) nz += cnt[i] != 0;
  *f0 = *f1 = nsym;
  for (uint32_t i = 0; i < nsym && nz < 2u; ++i)
    if (!cnt[i]) {
      cnt[i] = 1, ++nz;
      if (*f0 == nsym) *f0 = i;
      else *f1 = i;
    }
}

// One lane, between the passes: the three codes of the member from S.ll_cnt / S.d_cnt, and the header's plan (S.c.seq, hlit,
// hdist, hclen, S.hdr_bits).  The counts are left as pass 1 made them, with the end-of-block symbol counted once.
KR_INF_HD inline void def_dyn_plan(DefDynState& S)
{
  DefCodes& C = S.c;
  S.ll_cnt[256] = 1;
  uint32_t f0, f1, g0, g1;
  def_force_two(S.ll_cnt, kDefLL, &f0, &f1); // (never needed: a token and the end of the block)
  def_force_two(S.d_cnt, kDefD, &g0, &g1);
  bool limited = def_build_lengths(S.ll_cnt, kDefLL, 15, C.ll_len, C.build);
  limited |= def_build_lengths(S.d_cnt, kDefD, 15, C.d_len, C.build);
  if (f0 < kDefLL) S.ll_cnt[f0] = 0;
  if (f1 < kDefLL) S.ll_cnt[f1] = 0;
  if (g0 < kDefD) S.d_cnt[g0] = 0;
  if (g1 < kDefD) S.d_cnt[g1] = 0;
  def_canonical(C.ll_len, kDefLL, C.ll_code, C.next_code);
  def_canonical(C.d_len, kDefD, C.d_code, C.next_code);
  uint32_t hlit = kDefLL, hdist = kDefD;
  while (hlit > 257u && !C.ll_len[hlit - 1u]) --hlit;
  while (hdist > 1u && !C.d_len[hdist - 1u]) --hdist;
  C.hlit = hlit, C.hdist = hdist;
  // the hlit + hdist lengths as one sequence, run-length coded (the header comment's rule)
  for (uint32_t i = 0; i < kDefCL; ++i) C.cl_cnt[i] = 0;
  const uint32_t total = hlit + hdist;
  uint32_t nseq = 0, prev = 0, extra_bits = 0;
  for (uint32_t i = 0; i < total;) {
    const uint32_t v = i < hlit ? C.ll_len[i] : C.d_len[i - hlit];
    uint32_t r = 1;
    while (r < 138u && i + r < total && (i + r < hlit ? C.ll_len[i + r] : C.d_len[i + r - hlit]) == v) ++r;
    uint32_t sym = v, extra = 0, step = 1;
    if (v == 0 && r >= 11u) sym = 18, extra = r - 11u, step = r, extra_bits += 7u;
    else if (v == 0 && r >= 3u) sym = 17, extra = r - 3u, step = r, extra_bits += 3u;
    else if (v != 0 && v == prev && r >= 3u) sym = 16, step = r < 6u ? r : 6u, extra = step - 3u, extra_bits += 2u;
    prev = v;
    C.seq[nseq++] = (uint16_t)(sym | (extra << 8));
    ++C.cl_cnt[sym];
    i += step;
  }
  C.nseq = nseq;
  def_force_two(C.cl_cnt, kDefCL, &f0, &f1);
  limited |= def_build_lengths(C.cl_cnt, kDefCL, 7, C.cl_len, C.build);
  if (f0 < kDefCL) C.cl_cnt[f0] = 0;
  if (f1 < kDefCL) C.cl_cnt[f1] = 0;
  def_canonical(C.cl_len, kDefCL, C.cl_code, C.next_code);
  const uint8_t cl_order[kDefCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t hclen = kDefCL;
  while (hclen > 4u && !C.cl_len[cl_order[hclen - 1u]]) --hclen;
  C.hclen = hclen;
  uint32_t bits = 3u + 5u + 5u + 4u + 3u * hclen + extra_bits;
  for (uint32_t i = 0; i < kDefCL; ++i) bits += C.cl_cnt[i] * C.cl_len[i];
  S.hdr_bits = bits, S.limited = limited ? 1u : 0u;
}

// One lane: the dynamic block's header into the payload in whole words, the bits that are left (< 32) into S.win[0]
KR_INF_HD inline void def_dyn_header(DefDynState& S, uint8_t* pay)
{
  const DefCodes& C = S.c;
  const uint8_t cl_order[kDefCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint64_t acc = 0;
  uint32_t na = 0, opos = 0;
#define KR_DEF_PUT(v, nb)                                                                      \
  do {                                                                                         \
    acc |= (uint64_t)(v) << na, na += (nb);                                                    \
    if (na >= 32u) {                                                                           \
      for (uint32_t b_ = 0; b_ < 4u; ++b_) pay[opos + b_] = (uint8_t)(acc >> (8u * b_));       \
      opos += 4u, acc >>= 32, na -= 32u;                                                       \
    }                                                                                          \
  } while (0)
  KR_DEF_PUT(5u, 3u); // BFINAL = 1, BTYPE = 10
  KR_DEF_PUT(C.hlit - 257u, 5u);
  KR_DEF_PUT(C.hdist - 1u, 5u);
  KR_DEF_PUT(C.hclen - 4u, 4u);
  for (uint32_t i = 0; i < C.hclen; ++i) KR_DEF_PUT((uint32_t)C.cl_len[cl_order[i]], 3u);
  for (uint32_t i = 0; i < C.nseq; ++i) {
    const uint32_t sym = C.seq[i] & 255u, extra = C.seq[i] >> 8;
    KR_DEF_PUT((uint32_t)C.cl_code[sym], (uint32_t)C.cl_len[sym]);
    if (sym >= 16u) KR_DEF_PUT(extra, sym == 16u ? 2u : sym == 17u ? 3u : 7u);
  }
#undef KR_DEF_PUT
  S.win[0] = (uint32_t)acc;
}

// One token of the list under the member's dynamic codes, the first bit lowest.  *nbits <= 48 (15 + 5 extra, 15 + 13 extra).
KR_INF_HD inline uint64_t def_token_dyn(const DefCodes& C, uint32_t tok, uint32_t* nbits)
{
  const uint32_t len = tok & 0xffffu, hi = tok >> 16; // literal: the byte; match: the distance
  if (len == 0) {
    *nbits = C.ll_len[hi];
    return C.ll_code[hi];
  }
  uint32_t eb, extra, deb, dextra;
  const uint32_t s = 257u + def_len_sym(len, &eb, &extra), dc = def_dist_sym(hi, &deb, &dextra);
  uint32_t nb = C.ll_len[s];
  uint64_t bits = C.ll_code[s] | ((uint64_t)extra << nb);
  nb += eb;
  bits |= (uint64_t)C.d_code[dc] << nb, nb += C.d_len[dc];
  bits |= (uint64_t)dextra << nb, nb += deb;
  *nbits = nb;
  return bits;
}

// One member at level 2.  As deflate_member; tok[0 .. n): the member's part of the token list (global memory on the device).
// Afterwards S.btype, S.limited and S.hdr_bits say what became of it.
template <typename Lanes>
KR_INF_HD inline uint32_t deflate_member_dyn(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t* tok, DefDynState& S, const uint32_t* crc_tab, Lanes& L)
{
  const uint32_t nl = L.nlanes(), me = L.lane();
  for (uint32_t i = me; i < (1u << kDefHashBits); i += nl) S.head[i] = 0;
  for (uint32_t i = me; i < kDefLL; i += nl) S.ll_cnt[i] = 0;
  for (uint32_t i = me; i < kDefD; i += nl) S.d_cnt[i] = 0;
  L.sync();
  // pass 1: the tokens of level 1, listed and counted
  uint32_t ntok = 0, next = 0;
  for (uint32_t t0 = 0; t0 < n; t0 += kDefTile) {
    const uint64_t starts = def_tile_parse(in, n, t0, S, L, &next);
    for (uint32_t i = me; i < kDefTile; i += nl) {
      if (!((starts >> i) & 1u)) continue;
      const uint32_t at = ntok + (uint32_t)__builtin_popcountll(starts & ((1ull << i) - 1ull)); // (< n: a token covers a byte at least)
      const uint32_t len = S.len[i], dist = S.dist[i];
      if (len == 0) {
        const uint32_t b = in[t0 + i];
        tok[at] = b << 16;
        L.add(&S.ll_cnt[b], 1u);
      } else {
        uint32_t eb, extra;
        tok[at] = len | (dist << 16);
        L.add(&S.ll_cnt[257u + def_len_sym(len, &eb, &extra)], 1u);
        L.add(&S.d_cnt[def_dist_sym(dist, &eb, &extra)], 1u);
      }
      L.token(len, dist);
    }
    ntok += (uint32_t)__builtin_popcountll(starts);
    L.sync(); // (the tile's lengths are read before the next tile's are written)
  }
  // the codes, and the three sizes
  if (me == 0) def_dyn_plan(S);
  L.sync();
  uint32_t fbits = 0, dbits = 0;
  for (uint32_t s = me; s < kDefLL; s += nl) {
    const uint32_t c = S.ll_cnt[s], x = def_ll_extra(s);
    fbits += c * (def_ll_fixed(s) + x), dbits += c * (S.c.ll_len[s] + x);
  }
  for (uint32_t d = me; d < kDefD; d += nl) {
    const uint32_t c = S.d_cnt[d], x = def_d_extra(d);
    fbits += c * (5u + x), dbits += c * (S.c.d_len[d] + x);
  }
  L.scan_begin();
  (void)L.scan_excl(fbits);
  fbits = 3u + L.scan_total();
  L.scan_begin();
  (void)L.scan_excl(dbits);
  dbits = S.hdr_bits + L.scan_total();
  const uint32_t sbytes = n + 5u, fbytes = (fbits + 7u) >> 3, dbytes = (dbits + 7u) >> 3;
  const uint32_t btype = (fbytes < dbytes ? fbytes : dbytes) >= sbytes ? 0u : dbytes < fbytes ? 2u : 1u;
  uint8_t* const pay = out + 18;
  uint32_t cbytes;
  if (btype == 0) cbytes = def_stored(in, n, pay, L);
  else {
    // pass 2: tiles of 64 tokens, a lane each; level 1's bits where the codes are the fixed ones
    const bool dyn = btype == 2u;
    for (uint32_t i = me; i < kDefDynWinWords; i += nl) S.win[i] = i ? 0u : 3u; // BFINAL = 1, BTYPE = 01
    L.sync();
    if (dyn && me == 0) def_dyn_header(S, pay);
    L.sync();
    uint32_t nbits = dyn ? S.hdr_bits : 3u, opos = (nbits >> 5) * 4u; // as in deflate_member
    for (uint32_t t0 = 0; t0 < ntok; t0 += kDefTile) {
      const uint32_t carry = nbits & 31u;
      L.scan_begin();
      for (uint32_t i = me; i < kDefTile; i += nl) {
        uint64_t bits = 0;
        uint32_t nb = 0;
        if (t0 + i < ntok) {
          const uint32_t t = tok[t0 + i];
          bits = dyn ? def_token_dyn(S.c, t, &nb) : (uint64_t)def_token(t >> 16, t & 0xffffu, t >> 16, &nb);
        }
        const uint32_t o = carry + L.scan_excl(nb);
        if (nb) {
          const uint32_t w = o >> 5, sh = o & 31u;
          L.or_bits(&S.win[w], (uint32_t)(bits << sh));
          if (sh + nb > 32u) L.or_bits(&S.win[w + 1u], (uint32_t)(bits >> (32u - sh)));
          if (sh + nb > 64u) L.or_bits(&S.win[w + 2u], (uint32_t)(bits >> (64u - sh)));
        }
      }
      const uint32_t tile_bits = L.scan_total(), nw = (carry + tile_bits) >> 5;
      L.sync();
      for (uint32_t b = me; b < nw * 4u; b += nl) pay[opos + b] = (uint8_t)(S.win[b >> 2] >> (8u * (b & 3u)));
      const uint32_t left = S.win[nw];
      L.sync();
      for (uint32_t i = me; i <= nw; i += nl) S.win[i] = i ? 0u : left;
      L.sync();
      opos += nw * 4u, nbits += tile_bits;
    }
    // the end-of-block code, then zeros to the byte
    const uint32_t sh = nbits & 31u, eob_len = dyn ? S.c.ll_len[256] : 7u;
    if (me == 0 && dyn) {
      const uint64_t eob = (uint64_t)S.c.ll_code[256] << sh;
      L.or_bits(&S.win[0], (uint32_t)eob);
      L.or_bits(&S.win[1], (uint32_t)(eob >> 32));
    }
    L.sync();
    const uint32_t rem = (sh + eob_len + 7u) >> 3; // <= 6
    for (uint32_t b = me; b < rem; b += nl) pay[opos + b] = (uint8_t)(S.win[b >> 2] >> (8u * (b & 3u)));
    cbytes = opos + rem; // = dbytes or fbytes, below n + 5
  }
  const uint32_t size = def_frame(in, n, out, cbytes, crc_tab, L);
  if (me == 0) S.btype = btype;
  L.sync();
  return size;
}

// The member length (input bytes a member takes) is the caller's: the cut is made outside deflate_member.  kDefMemberIn is the
// default and the most; kDefMinMemberIn the least (kr_bgzf_deflate_host_member, kr_stream_bgzf_member, `--bgzf-member`).
constexpr uint32_t kDefMinMemberIn = 256u;
inline bool bgzf_member_in_ok(uint64_t member_in) { return member_in >= kDefMinMemberIn && member_in <= kDefMemberIn; }
// the stride of the members' slots for a member length: room for member_in + 31 bytes, a multiple of 32 (kDefSlot at the default)
KR_INF_HD inline uint32_t bgzf_slot_stride(uint32_t member_in) { return (member_in + 32u + 31u) & ~31u; }

// members of n input bytes, and the most bytes they take
inline uint64_t bgzf_deflate_members(uint64_t n, uint32_t member_in = kDefMemberIn) { return (n + member_in - 1) / member_in; }
inline uint64_t bgzf_deflate_bound(uint64_t n, uint32_t member_in = kDefMemberIn) { return n + bgzf_deflate_members(n, member_in) * kDefOverhead; }

// the empty member that ends a BGZF file
inline void bgzf_eof(uint8_t* out28)
{
  const uint8_t e[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  memcpy(out28, e, 28);
}

// Host form: member m (of member_in input bytes) of text[0 .. n) into its slot; `st` (optional) is added to.  Returns the member's size.
inline uint32_t bgzf_deflate_member_host(const uint8_t* text, uint64_t n, uint64_t m, uint8_t* slot, DefState& S, DefStats* st,
                                         uint32_t member_in = kDefMemberIn)
{
  const uint64_t a = m * member_in;
  const uint32_t len = (uint32_t)(n - a < member_in ? n - a : member_in);
  DefSerial L;
  const uint32_t size = deflate_member(text + a, len, slot, S, crc_host_table(), L);
  if (st) {
    ++st->members;
    if ((slot[18] & 6u) == 0) ++st->stored; // BTYPE 00
    else {
      ++st->fixed;
      st->literals += L.tok.literals, st->matches += L.tok.matches;
      if (L.tok.longest > st->longest) st->longest = L.tok.longest;
      if (L.tok.farthest > st->farthest) st->farthest = L.tok.farthest;
    }
  }
  return size;
}

// The same at level 2.  tok: room for member_in tokens (kDefTokStride at the most).
inline uint32_t bgzf_deflate_member_host_dyn(const uint8_t* text, uint64_t n, uint64_t m, uint8_t* slot, DefDynState& S, uint32_t* tok, DefStats* st,
                                             uint32_t member_in = kDefMemberIn)
{
  const uint64_t a = m * member_in;
  const uint32_t len = (uint32_t)(n - a < member_in ? n - a : member_in);
  DefSerial L;
  const uint32_t size = deflate_member_dyn(text + a, len, slot, tok, S, crc_host_table(), L);
  if (st) {
    ++st->members;
    st->limited += S.limited;
    if (S.btype == 0) ++st->stored;
    else {
      if (S.btype == 2u) ++st->dynamic, st->header_bits += S.hdr_bits;
      else ++st->fixed;
      st->literals += L.tok.literals, st->matches += L.tok.matches;
      if (L.tok.longest > st->longest) st->longest = L.tok.longest;
      if (L.tok.farthest > st->farthest) st->farthest = L.tok.farthest;
    }
  }
  return size;
}

} // namespace kr
#endif
