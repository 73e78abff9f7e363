// kr_inflate_sym.h — DEFLATE decoded SYMBOLICALLY from an arbitrary block start of an ordinary gzip stream, as one piece of code for
// the host and the device (the stages of kr_pgz.inc, restated in kr_inflate.h's `Lanes` idiom).
//
// A gzip member is one dependent stream: a block's matches reach up to 32 KB back into what earlier blocks produced.  A SUPER-CHUNK
// of compressed bytes that starts at a known bit P is cut into SUB-CHUNKS of `sub` bytes.  Four stages, each parallel over sub-chunks:
//   search   (gz_search_sub)  the first bit in the sub-chunk's range at which a dynamic block starts (gz_candidate + gz_verify_start:
//            pgz::Source::sync's predicate); sub-chunk 0 starts at P
//   decode   (gz_decode_sub)  block after block from that start into the sub-chunk's SLOT of the symbol buffer, until a block ends
//            exactly where a later sub-chunk starts.  A symbol is a byte (0..255) or 256 + i: "byte i of the 32 KB window in front of
//            this chunk" (pgz::SymDecoder::block's formula; copies propagate symbols)
//   chain    (gz_chain_window) the sub-chunks the verified stream passes through, in order; the window behind each: its last 32 K symbols
//            resolved against the window in front of it
//   resolve  (gz_resolve_symbol) symbols to bytes, and their CRC-32
// What a wave does with its lanes sits behind `Lanes` (SymSerial here, SymWave in kr_dev_gzip.inc): table fill, pending literals,
// match copies.  Every lane decodes the same symbols; every branch is wave-uniform.
//
// Bounds, for ANY input bytes: no read outside [comp, comp + ncomp) -- a refill past the end yields zero bits and sets `over` --; no
// write outside the sub-chunk's slot; every loop is bounded by the remaining input bits or the slot's room; every index comes from bit
// positions and counts, never from a decoded symbol's value (a window symbol is an index only in gz_resolve_symbol, behind a range check).
#ifndef KR_INFLATE_SYM_H
#define KR_INFLATE_SYM_H

#include "kr_inflate.h"

namespace kr {

constexpr uint32_t kGzWin = 32768;
constexpr uint32_t kGzSearchMin = 256, kGzSearchCap = 4u << 20; // a block start is accepted with this many symbols (pgz::Source::sync's)
constexpr uint32_t kGzNone = 0xFFFFFFFFu;                       // S: no start found; link: none

enum GzStatus : uint32_t {
  GZ_IDLE = 0,       // no start: the sub-chunk decoded nothing
  GZ_LINKED = 1,     // a block ended exactly at the start of sub-chunk `link`
  GZ_MEMBER_END = 2, // the member's final block ended
  GZ_INPUT_END = 3,  // the last block that lies wholly inside the super-chunk ended
  GZ_OVERFLOW = 4,   // the slot is full (a false start stepped over, or a ratio above ratio_cap)
  GZ_BAD = 5         // a block broke a rule (`link` holds the InfRule)
};

// One super-chunk, as the stages see it.  Bit positions are relative to comp[0]; the stream continues at bit pbit (< 8).
struct GzSuper {
  const uint8_t* comp;
  uint32_t ncomp; // < 2^29: bit positions are 32-bit
  uint32_t pbit, sub, nsub, ratio;
  uint16_t* sym; // [ratio * ncomp + 1]
  // per sub-chunk
  uint32_t *S, *end, *status, *link, *len;
};
KR_INF_HD inline uint64_t gz_slot_base(const GzSuper& G, uint32_t bit) { return (uint64_t)G.ratio * (bit - G.pbit) / 8u; }

// ---- lanes (the serial form) ------------------------------------------------------------------------------------------------------
struct SymSerial {
  KR_INF_HD uint32_t lane() const { return 0; }
  KR_INF_HD uint32_t nlanes() const { return 1; }
  KR_INF_HD void sync() const {}
  KR_INF_HD void literal(uint16_t* out, uint32_t pos, uint32_t b) { out[pos] = (uint16_t)b; }
  KR_INF_HD void flush(uint16_t*, uint32_t) {}
};

KR_INF_HD inline void gz_bits_at(InfBits& B, const uint8_t* in, uint32_t nbytes, uint32_t bit)
{
  B.in = in, B.ip = bit >> 3 < nbytes ? bit >> 3 : nbytes, B.end = nbytes, B.bb = 0, B.nb = 0, B.over = 0;
  B.refill();
  B.drop(bit & 7u);
}
KR_INF_HD inline uint32_t gz_bitpos(const InfBits& B) { return B.ip * 8u - B.nb; } // (meaningful while !B.over)

KR_INF_HD inline bool gz_texty(uint32_t c) { return c == '\n' || c == '\r' || c == '\t' || (c >= 32 && c < 127); }

// 64 bits from bit `bit` on, zeros behind the end
KR_INF_HD inline uint64_t gz_peek64(const uint8_t* in, uint32_t nbytes, uint32_t bit)
{
  const uint32_t by = bit >> 3, sh = bit & 7u;
  uint64_t lo = 0;
  uint32_t hi = 0;
  for (uint32_t i = 0; i < 8; ++i)
    if (by + i < nbytes) lo |= (uint64_t)in[by + i] << (8 * i);
  if (by + 8 < nbytes) hi = in[by + 8];
  return sh ? (lo >> sh) | ((uint64_t)hi << (64 - sh)) : lo;
}

// The part of the predicate a lane tests on its own: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29 (raw fields), and the
// code-length code complete (sum of 2^(7 - length) == 128: what inf_build(kind 0) asks, tested before any table is built).
KR_INF_HD inline bool gz_candidate(const uint8_t* in, uint32_t nbytes, uint32_t bit)
{
  const uint64_t v = gz_peek64(in, nbytes, bit);
  if ((v & 7u) != 4u) return false;
  if ((uint32_t)((v >> 3) & 31u) > 29u || (uint32_t)((v >> 8) & 31u) > 29u) return false;
  const uint32_t ncode = (uint32_t)((v >> 13) & 15u) + 4u;
  if (bit + 17u + 3u * ncode > nbytes * 8u) return false; // the header runs out of input
  uint32_t kraft = 0;
  uint64_t w = v >> 17; // 47 bits: 15 lengths; the rest from a second load
  for (uint32_t i = 0; i < ncode; ++i) {
    if (i == 15) w = gz_peek64(in, nbytes, bit + 17u + 45u);
    const uint32_t l = (uint32_t)(w & 7u);
    w >>= 3;
    if (l) kraft += 128u >> l;
  }
  return kraft == 128u;
}

// The code lengths of a dynamic block (B stands behind BFINAL / BTYPE, refilled) into T.lens: pgz's dynamic_lengths, the rules and
// their order inflate_member's.  0 or the rule broken.
template <typename Lanes>
KR_INF_HD inline uint32_t gz_dynamic_lengths(InfBits& B, InfTables& T, Lanes& L, uint32_t* pnlen, uint32_t* pndist)
{
  const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  const uint32_t nlen = B.take(5) + 257, ndist = B.take(5) + 1, ncode = B.take(4) + 4;
  *pnlen = nlen, *pndist = ndist;
  if (B.over) return INF_INPUT_END;
  if (nlen > 286 || ndist > 30) return INF_SYMBOL_COUNT;
  for (uint32_t i = 0; i < 19; ++i) {
    if ((i & 15u) == 0) B.refill();
    T.cl_lens[cl_order[i]] = i < ncode ? (uint8_t)B.take(3) : (uint8_t)0;
  }
  if (B.over) return INF_INPUT_END;
  if (inf_build(T.cl_lens, 19, T.dist_cnt, T.offs, T.dist_sym, T.dist_fast, kInfClBits, 0, L)) return INF_CODELEN_SET;
  uint32_t have = 0;
  while (have < nlen + ndist) { // every step stores at least one length
    B.refill();
    const uint32_t s = inf_symbol(B, T.dist_cnt, T.dist_sym, T.dist_fast, kInfClBits);
    if (s == 0xFFFFu) return INF_CODELEN_SET;
    if (B.over) return INF_INPUT_END;
    if (s < 16) {
      T.lens[have++] = (uint8_t)s;
      continue;
    }
    uint32_t prev = 0, rep;
    if (s == 16) {
      if (have == 0) return INF_REPEAT;
      prev = T.lens[have - 1];
      rep = 3 + B.take(2);
    } else if (s == 17)
      rep = 3 + B.take(3);
    else
      rep = 11 + B.take(7);
    if (B.over) return INF_INPUT_END;
    if (have + rep > nlen + ndist) return INF_REPEAT;
    for (uint32_t i = 0; i < rep; ++i) T.lens[have++] = (uint8_t)prev;
  }
  if (T.lens[256] == 0) return INF_NO_END_CODE;
  return INF_OK;
}

// One block at B, symbolically.  kStore: its symbols go to out[*ppos ..), at most `cap` in all (INF_OUT_LONG: no room; what was written
// lies inside the slot).  !kStore (a search trial): nothing is written, the symbols are counted up to `cap` and every literal must
// be `texty` (INF_LITLEN_CODE if not).  0: the block has ended, *plast = BFINAL; INF_INPUT_END: the input ends inside it.
template <bool kStore, typename Lanes>
KR_INF_HD inline uint32_t gz_sym_block(InfBits& B, InfTables& T, Lanes& L, uint16_t* out, uint32_t cap, uint32_t* ppos, uint32_t* plast)
{
  uint32_t pos = *ppos, rule = INF_OK;
  B.refill();
  *plast = B.take(1);
  const uint32_t type = B.take(2);
  if (B.over) return INF_INPUT_END;
  if (type == 3) return INF_BLOCK_TYPE;
  if (type == 0) { // stored: to the byte boundary, LEN, NLEN, then LEN bytes as they are
    B.drop(B.nb & 7u);
    B.refill();
    const uint32_t len = B.take(16), nlen = B.take(16);
    if (B.over) return INF_INPUT_END;
    if (len != (nlen ^ 0xFFFFu)) return INF_STORED_LEN;
    B.ip -= B.nb >> 3, B.bb = 0, B.nb = 0; // (whole bytes only: the buffer was at a byte boundary)
    if (len > B.end - B.ip) return INF_INPUT_END;
    if (len > cap - pos) return INF_OUT_LONG;
    if (kStore) {
      for (uint32_t i = L.lane(); i < len; i += L.nlanes()) out[pos + i] = B.in[B.ip + i];
      L.sync();
    }
    B.ip += len, *ppos = pos + len;
    return INF_OK;
  }
  uint32_t nlen = 288, ndist = 32;
  if (type == 1) {
    for (uint32_t s = 0; s < 288; ++s) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    for (uint32_t s = 0; s < 32; ++s) T.lens[288 + s] = 5;
  } else if ((rule = gz_dynamic_lengths(B, T, L, &nlen, &ndist)))
    return rule;
  if (inf_build(T.lens, nlen, T.lit_cnt, T.offs, T.lit_sym, T.lit_fast, kInfLitBits, 1, L)) return INF_LITLEN_SET;
  if (inf_build(T.lens + nlen, ndist, T.dist_cnt, T.offs, T.dist_sym, T.dist_fast, kInfDistBits, 2, L)) return INF_DIST_SET;
  for (;;) { // a symbol takes at least one bit: bounded by the input (B.over ends it)
    B.refill();
    uint32_t s = inf_symbol(B, T.lit_cnt, T.lit_sym, T.lit_fast, kInfLitBits);
    if (B.over) {
      rule = INF_INPUT_END;
      break;
    }
    if (s < 256) {
      if (pos >= cap) {
        rule = INF_OUT_LONG;
        break;
      }
      if (kStore) L.literal(out, pos, s);
      else if (!gz_texty(s)) {
        rule = INF_LITLEN_CODE;
        break;
      }
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
    if (dist > pos + kGzWin) { // further back than any window reaches
      rule = INF_DIST_FAR;
      break;
    }
    if (len > cap - pos) {
      rule = INF_OUT_LONG;
      break;
    }
    if (kStore) {
      L.flush(out, pos);
      // element i is what stands `dist` in front of it: own output (written before this match: no lane reads what another writes
      // now), or position kGzWin - (dist - p) of the window in front of the chunk.  dist < len: the periodic pattern.
      for (uint32_t i = L.lane(); i < len; i += L.nlanes()) {
        const uint32_t p = pos + (dist >= len ? i : i % dist);
        out[pos + i] = p >= dist ? out[p - dist] : (uint16_t)(256u + (kGzWin - (dist - p)));
      }
      L.sync();
    }
    pos += len;
  }
  if (kStore) L.flush(out, pos);
  *ppos = pos;
  return rule;
}

// pgz::Source::sync's verdict on bit `at` (a gz_candidate): the block decodes as text to 256 .. kGzSearchCap symbols, is not final,
// and the next block's header holds water (not type 3; dynamic: its lengths parse).  Writes nothing but T.
template <typename Lanes>
KR_INF_HD inline bool gz_verify_start(const uint8_t* in, uint32_t nbytes, uint32_t at, InfTables& T, Lanes& L)
{
  InfBits B;
  gz_bits_at(B, in, nbytes, at);
  uint32_t n = 0, last = 0;
  if (gz_sym_block<false>(B, T, L, nullptr, kGzSearchCap, &n, &last) || last || n < kGzSearchMin) return false;
  B.refill();
  B.take(1);
  const uint32_t t = B.take(2);
  if (B.over || t == 3) return false;
  if (t == 2) {
    uint32_t a, b;
    if (gz_dynamic_lengths(B, T, L, &a, &b)) return false;
  }
  return true;
}

// Search stage of sub-chunk i (serial form; the wave tests 64 candidates at a time, kr_dev_gzip.inc, and verifies in the same order)
inline void gz_search_sub(const GzSuper& G, uint32_t i, InfTables& T)
{
  SymSerial L;
  if (i == 0) {
    G.S[0] = G.pbit;
    return;
  }
  uint32_t found = kGzNone;
  const uint32_t lo = i * G.sub * 8u, hi = (i + 1 < G.nsub ? (i + 1) * G.sub : G.ncomp) * 8u;
  for (uint32_t at = lo; at < hi; ++at)
    if (gz_candidate(G.comp, G.ncomp, at) && gz_verify_start(G.comp, G.ncomp, at, T, L)) {
      found = at;
      break;
    }
  G.S[i] = found;
}

// Decode stage of sub-chunk i: block after block from S[i] into its slot [base(S[i]), base(next found start)).
template <typename Lanes>
KR_INF_HD inline void gz_decode_sub(const GzSuper& G, uint32_t i, InfTables& T, Lanes& L)
{
  const uint32_t s0 = G.S[i], end_bit = G.ncomp * 8u;
  uint32_t status = GZ_IDLE, link = kGzNone, pos = 0, end = s0;
  if (s0 != kGzNone) {
    uint32_t j = i + 1;
    while (j < G.nsub && G.S[j] == kGzNone) ++j; // the slot ends where the next found start's begins
    const uint64_t base = gz_slot_base(G, s0), room = gz_slot_base(G, j < G.nsub ? G.S[j] : end_bit) - base;
    const uint32_t cap = room < 0x7FFFFFFFu ? (uint32_t)room : 0x7FFFFFFFu;
    uint16_t* out = G.sym + base;
    InfBits B;
    gz_bits_at(B, G.comp, G.ncomp, s0);
    j = i + 1;
    for (;;) { // a block takes at least 3 bits: bounded by the input
      const uint32_t pos0 = pos;
      uint32_t last = 0;
      const uint32_t rule = gz_sym_block<true>(B, T, L, out, cap, &pos, &last);
      if (rule) { // the block in flight is discarded: the chunk ends where it began
        pos = pos0;
        // within the super-chunk's last bits a code may be cut short and read as no code at all: that is the input's end, not
        // damage (if the file ends there too, zlib says so: the host range)
        const bool at_end = B.ip >= B.end && B.nb < 48u;
        status = rule == INF_OUT_LONG ? GZ_OVERFLOW : (rule == INF_INPUT_END || at_end) ? GZ_INPUT_END : GZ_BAD;
        if (status == GZ_BAD) link = rule;
        break;
      }
      end = gz_bitpos(B);
      if (last) {
        status = GZ_MEMBER_END;
        break;
      }
      while (j < G.nsub && (G.S[j] == kGzNone || G.S[j] < end)) ++j; // S is sorted: a forward cursor
      if (j < G.nsub && G.S[j] == end) {
        status = GZ_LINKED, link = j;
        break;
      }
      if (end >= end_bit) {
        status = GZ_INPUT_END;
        break;
      }
    }
  }
  if (L.lane() == 0) G.end[i] = end, G.status[i] = status, G.link[i] = link, G.len[i] = pos;
}

// A symbol as a byte, against the window in front of its chunk: win[0 .. kGzWin), of which the last wlen bytes exist.
// *bad is set for a symbol that points in front of the member's first byte (INF_DIST_FAR) or is no symbol at all.
KR_INF_HD inline uint8_t gz_resolve_symbol(uint32_t s, const uint8_t* win, uint32_t wlen, uint32_t* bad)
{
  if (s < 256u) return (uint8_t)s;
  const uint32_t i = s - 256u;
  if (i >= kGzWin || i < kGzWin - wlen) {
    *bad = 1;
    return 0;
  }
  return win[i];
}
// Byte t of the window behind a chunk of `len` symbols
KR_INF_HD inline uint8_t gz_chain_window(const uint16_t* sym, uint32_t len, const uint8_t* win, uint32_t wlen, uint32_t t, uint32_t* bad)
{
  if (len >= kGzWin) return gz_resolve_symbol(sym[len - kGzWin + t], win, wlen, bad);
  if (t + len < kGzWin) return win[t + len];
  return gz_resolve_symbol(sym[t + len - kGzWin], win, wlen, bad);
}

// What the chain stage writes
struct GzChainSum {
  uint32_t nchain;     // chain chunks
  uint32_t end_bit;    // where the verified stream stands behind them
  uint32_t end_status; // the last chain chunk's status
  uint32_t bad_at;     // first chain chunk with a symbol in front of the member's output (kGzNone: none)
  uint64_t total;      // bytes
};

// crc32(A ++ B) from crc32(A), crc32(B) and B's length (zlib's crc32_combine)
inline uint32_t gz_crc_combine(uint32_t a, uint32_t b, uint64_t nb)
{
  uint32_t op = 1u << 31; // x^(8 nb) mod P
  for (uint64_t n = nb; n;) {
    const uint32_t k = (uint32_t)(n < 0x40000000u ? n : 0x40000000u);
    op = crc_mulmod(crc_xpow8(k), op);
    n -= k;
  }
  return crc_mulmod(op, a) ^ b;
}

} // namespace kr
#endif
