// kr_gzip_super.h — an ordinary gzip file inflated super-chunk by super-chunk (host only): what happens between the runs of the four
// stages of kr_inflate_sym.h.  The stages themselves sit behind GzBackend: the kernels (kr_host_gzip.inc) or their serial twin
// (GzHostBackend below: kr_debug_gzdev_inflate_host, scripts/asan_gzip_sym.cpp).  Everything here is the same code for both, so the two
// hand out the same bytes, tables, counters and messages.
//
// The verified stream stands at bit P of the file, with its last <= 32 KB (the window), the member's running CRC-32 and length.  A
// super-chunk is the next max_comp bytes from P's byte on.  Its chain (the sub-chunks the stream passes through) gives the bytes up
// to a verified end bit; then, by the chain's end status:
//   MEMBER_END   CRC-32 and length are compared with the trailer as gzread would; the next member's header is parsed with
//                pgz::member_header's rules (bytes that are no gzip member end the stream, as for gzread)
//   INPUT_END / OVERFLOW / a start nobody linked to   not damage: the next super-chunk begins at the end bit with its window.  If
//                the chain did not get past its first block (a ratio above ratio_cap, a block larger than the super-chunk), the host
//                inflates the super-chunk's byte range with zlib primed at (P, window) -- pgz::ZSeq's way -- and the stages go on behind it
//   BAD, a symbol in front of the member's first byte, a wrong trailer   damage: an error AFTER the bytes in front of it were handed out
// Correctness never rests on the search: a sub-chunk counts only from a bit the verified stream reaches, decoding from there is
// deterministic, and every member's CRC-32 and length are checked.
#ifndef KR_GZIP_SUPER_H
#define KR_GZIP_SUPER_H

#include "kr_inflate_sym.h"

#include <zlib.h>

#include <algorithm>
#include <deque>
#include <memory>
#include <string>
#include <vector>

namespace kr {

struct GzParams {
  uint32_t sub = 32768, ratio = 16;
  uint64_t max_comp = 64ull << 20;
};
inline const char* gz_params_check(const GzParams& p)
{
  if (p.sub < 64 || p.ratio < 1 || p.ratio > 1024 || p.max_comp < p.sub) return "sub_bytes >= 64, 1 <= ratio_cap <= 1024 and max_comp_bytes >= sub_bytes are required";
  if (p.max_comp >= (1ull << 29)) return "a super-chunk must stay below 512 MB (bit positions are 32-bit)";
  if ((uint64_t)p.ratio * p.max_comp >= (1ull << 31)) return "ratio_cap * max_comp_bytes must stay below 2^31 symbols";
  return nullptr;
}
struct GzCounters {
  uint64_t super_chunks = 0, linked = 0, without_start = 0, dropped = 0, host_ranges = 0;
  uint64_t redone_bytes = 0; // compressed bytes that super-chunks took in behind their verified end: copied, searched and decoded again by the next
};
struct GzSubRow { // one sub-chunk of one super-chunk (tests)
  uint32_t S, end, status, link, len, crc;
};
// Where the stream can be taken up again (kr_gzip_point's content)
struct GzPoint {
  uint64_t bit = 0;          // compressed bit position in the file
  uint64_t inflated_off = 0; // of the first byte inflated from there
  uint32_t crc = 0;          // the member's CRC-32 so far
  uint64_t mlen = 0;         // ... and length
  uint32_t wlen = 0;
  uint8_t win[kGzWin];       // the last wlen bytes in front, at win[kGzWin - wlen ..)
};

struct GzBackend {
  virtual ~GzBackend() {}
  // The four stages over comp[0 .. nc), the stream at bit pbit, win[kGzWin - wlen ..) in front of it.  rows: [nsub]; chain: the
  // chain's sub-chunks in order; win_out: the window behind the chain.  The bytes stay with the backend (fetch).  0 or a KR_ERR code.
  virtual int run(const uint8_t* comp, uint32_t nc, uint32_t pbit, uint32_t sub, uint32_t nsub, uint32_t ratio, const uint8_t* win, uint32_t wlen,
                  std::vector<GzSubRow>& rows, std::vector<uint32_t>& chain, GzChainSum& sum, uint8_t* win_out, std::string& err) = 0;
  virtual int fetch(uint8_t* dst, uint64_t off, uint64_t n, std::string& err) = 0;
};

// gzip member header at byte `at` (pgz::member_header's rules): the byte offset of its deflate data, 0 if it is no header
inline uint64_t gz_member_header(const uint8_t* p, uint64_t n, uint64_t at)
{
  if (at + 18 > n || p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8 || (p[at + 3] & 0xE0)) return 0;
  const unsigned flg = p[at + 3];
  uint64_t q = at + 10;
  if (flg & 4) {
    if (q + 2 > n) return 0;
    q += 2 + (p[q] | (p[q + 1] << 8));
  }
  for (unsigned bit : {8u, 16u})
    if (flg & bit) {
      while (q < n && p[q]) ++q;
      ++q;
    }
  if (flg & 2) { // FHCRC: the low 16 bits of the CRC-32 of the header so far
    if (q + 2 > n) return 0;
    const uint32_t hc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), p + at, (uInt)(q - at)) & 0xFFFFu;
    if (hc != (uint32_t)(p[q] | (p[q + 1] << 8))) return 0;
    q += 2;
  }
  return q < n ? q : 0;
}

// zlib primed in mid-stream (pgz::ZSeq): raw inflate from bit `bitpos` of file[0 .. nb) with a known window
struct GzZlib {
  z_stream zs;
  bool live = false;
  const uint8_t* p = nullptr;
  uint64_t nbytes = 0;
  GzZlib() = default;
  GzZlib(const GzZlib&) = delete;
  GzZlib& operator=(const GzZlib&) = delete;
  ~GzZlib()
  {
    if (live) inflateEnd(&zs);
  }
  bool start(const uint8_t* file, uint64_t nb, uint64_t bitpos, const uint8_t* win, uint32_t wlen)
  {
    if (live) inflateEnd(&zs);
    live = false;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    live = true;
    p = file, nbytes = nb;
    if (wlen && inflateSetDictionary(&zs, win, wlen) != Z_OK) return false;
    uint64_t by = bitpos >> 3;
    const unsigned sh = (unsigned)(bitpos & 7u);
    if (sh) {
      if (by >= nb || inflatePrime(&zs, (int)(8 - sh), p[by] >> sh) != Z_OK) return false;
      ++by;
    }
    if (by > nb) return false;
    zs.next_in = const_cast<Bytef*>(p + by);
    zs.avail_in = 0;
    return true;
  }
  uint64_t bitpos() const { return (uint64_t)(zs.next_in - p) * 8ull - (uint64_t)(zs.data_type & 7); }
  // Inflate (appending to dst) to a block boundary at or beyond until_bit, or to the end of the deflate stream.
  // 0: error (what came out in front of it is in dst), 1: at a block boundary, 2: the final block has ended, 3: more than max_out bytes
  int run(std::vector<uint8_t>& dst, uint64_t until_bit, uint64_t max_out)
  {
    size_t n = dst.size();
    int res = -1;
    while (res < 0) {
      if (n > max_out) {
        res = 3;
        break;
      }
      if (zs.avail_in == 0) zs.avail_in = (uInt)std::min<uint64_t>(nbytes - (uint64_t)(zs.next_in - p), 1u << 30);
      if (dst.size() - n < (1u << 16)) dst.resize(std::max<size_t>(dst.size() * 2, n + (1u << 20)));
      zs.next_out = dst.data() + n;
      zs.avail_out = (uInt)std::min<size_t>(dst.size() - n, 1u << 30);
      const uInt gave = zs.avail_out;
      const int rc = inflate(&zs, Z_BLOCK);
      n += gave - zs.avail_out;
      if (rc == Z_STREAM_END) res = 2;
      else if (rc != Z_OK && rc != Z_BUF_ERROR) res = 0;
      else if ((zs.data_type & 128) && !(zs.data_type & 64) && bitpos() >= until_bit) res = 1;
      else if (rc == Z_BUF_ERROR && zs.avail_in == 0 && (uint64_t)(zs.next_in - p) >= nbytes) res = 0; // the file ends inside the stream
    }
    dst.resize(n);
    return res;
  }
};

class GzInflater {
 public:
  GzCounters ctr;
  std::string msg;             // of the error returned
  bool keep_rows = false;      // (tests)
  std::vector<GzSubRow> rows_all;
  std::deque<GzPoint> points;  // the starts of the last `keep_points` super-chunks and host ranges
  size_t keep_points = 4;

  GzInflater(GzBackend* be, const uint8_t* file, uint64_t size, const GzParams& p, std::string name)
      : be_(be), file_(file), size_(size), prm_(p), name_(std::move(name))
  {
  }
  // 0, or -2 (KR_ERR_IO): not a gzip file
  int open()
  {
    const uint64_t d = gz_member_header(file_, size_, 0);
    if (!d) return damaged("not a gzip member header", 0);
    P_ = d * 8, crc_ = 0, mlen_ = 0, wlen_ = 0;
    return 0;
  }
  // The next inflated bytes in file order, at most cap; *n == 0: the end.  0, -2 (KR_ERR_IO: damage, after the bytes in front of it), or
  // a backend's error code
  int read(uint8_t* dst, uint64_t cap, uint64_t* n)
  {
    *n = 0;
    while (pend_off_ == pend_end_) {
      if (err_) return deliver_error();
      if (done_) return 0;
      if (int rc = advance()) return rc;
    }
    const uint64_t k = std::min(cap, pend_end_ - pend_off_);
    if (pend_host_) memcpy(dst, hv_.data() + pend_off_, k);
    else if (int rc = be_->fetch(dst, pend_off_, k, msg)) return rc;
    pend_off_ += k, *n = k;
    return 0;
  }
  uint64_t inflated() const { return out_off_; } // bytes the super-chunks so far inflate to

 private:
  GzBackend* be_;
  const uint8_t* file_;
  uint64_t size_;
  GzParams prm_;
  std::string name_;
  uint64_t P_ = 0, mlen_ = 0, out_off_ = 0;
  uint32_t crc_ = 0, wlen_ = 0;
  uint8_t win_[kGzWin] = {0}, win_new_[kGzWin] = {0};
  bool done_ = false, pend_host_ = false;
  int err_ = 0;
  std::string err_msg_;
  uint64_t pend_off_ = 0, pend_end_ = 0;
  std::vector<uint8_t> hv_;
  std::unique_ptr<GzZlib> hz_; // a host range under way
  uint64_t hz_until_ = 0;
  std::vector<GzSubRow> rows_;
  std::vector<uint32_t> chain_;

  int damaged(const std::string& why, uint64_t off)
  {
    msg = "damaged gzip file " + name_ + ": " + why + " (at compressed offset " + std::to_string(off) + ")";
    return -2;
  }
  void later(const std::string& why, uint64_t off)
  {
    if (err_) return;
    err_ = damaged(why, off), err_msg_ = msg;
  }
  int deliver_error()
  {
    msg = err_msg_;
    return err_;
  }
  void mark_point()
  {
    points.emplace_back();
    GzPoint& pt = points.back();
    pt.bit = P_, pt.inflated_off = out_off_, pt.crc = crc_, pt.mlen = mlen_, pt.wlen = wlen_;
    memcpy(pt.win, win_, kGzWin);
    while (points.size() > std::max<size_t>(keep_points, 1)) points.pop_front();
  }
  // the member's final block has ended at file bit `bit`: the trailer, then the next member or the end
  void member_end(uint64_t bit)
  {
    const uint64_t t = (bit + 7) >> 3;
    if (t + 8 > size_) return later("the member's trailer is cut short", t);
    const uint32_t want_crc = bgzf_le32(file_ + t), want_len = bgzf_le32(file_ + t + 4);
    if (want_crc != crc_) return later("wrong CRC-32 in the member's trailer", t);
    if (want_len != (uint32_t)mlen_) return later("wrong length in the member's trailer", t + 4);
    crc_ = 0, mlen_ = 0, wlen_ = 0;
    const uint64_t q = t + 8;
    if (q + 2 > size_ || file_[q] != 0x1f || file_[q + 1] != 0x8b) { // the end, or bytes that are no gzip member: ignored, as by gzread
      done_ = true;
      return;
    }
    const uint64_t d = gz_member_header(file_, size_, q);
    if (!d) return later("a member header cut short or of an unknown kind", q);
    P_ = d * 8;
  }
  // A stretch the stages could not take: zlib primed at (P, window) inflates up to a block boundary at or beyond until_bit (or the
  // member's end), in pieces of about kHostPiece bytes -- a piece each time the bytes handed out run dry -- so that no ratio makes the
  // host hold more than a piece
  static constexpr uint64_t kHostPiece = 64ull << 20;
  int host_range(uint64_t until_bit)
  {
    ++ctr.host_ranges;
    mark_point();
    hz_.reset(new GzZlib());
    hz_until_ = until_bit;
    if (!hz_->start(file_, size_, P_, win_ + (kGzWin - wlen_), wlen_)) {
      hz_.reset();
      later("the deflate stream ends", P_ >> 3);
      return 0;
    }
    return host_piece();
  }
  int host_piece()
  {
    GzZlib& z = *hz_;
    hv_.clear();
    const int r = z.run(hv_, hz_until_, kHostPiece); // 3: the piece is full, zlib stands inside a block and goes on from there
    const uint64_t n = hv_.size();
    pend_host_ = true, pend_off_ = 0, pend_end_ = n;
    if (n) {
      const uint32_t c = ~crc_raw(crc_host_table(), 0xFFFFFFFFu, hv_.data(), (uint32_t)n); // (a piece stays far below 4 GB)
      crc_ = gz_crc_combine(crc_, c, n), mlen_ += n, out_off_ += n;
      if (n >= kGzWin) memcpy(win_, hv_.data() + n - kGzWin, kGzWin), wlen_ = kGzWin;
      else {
        memmove(win_, win_ + n, kGzWin - n);
        memcpy(win_ + kGzWin - n, hv_.data(), n);
        wlen_ = (uint32_t)std::min<uint64_t>(kGzWin, wlen_ + n);
      }
    }
    if (r == 3) return 0;
    if (r == 0) later(z.zs.msg ? std::string("zlib: ") + z.zs.msg : std::string("the deflate stream ends inside a block"), (uint64_t)(z.zs.next_in - file_));
    else {
      P_ = z.bitpos();
      if (r == 2) member_end(P_);
    }
    hz_.reset();
    return 0;
  }
  int advance()
  {
    if (hz_) return host_piece();
    const uint64_t B0 = P_ >> 3;
    const uint32_t pbit = (uint32_t)(P_ & 7u);
    if (B0 >= size_) {
      later("the deflate stream ends", size_);
      return 0;
    }
    const uint32_t nc = (uint32_t)std::min<uint64_t>(size_ - B0, prm_.max_comp);
    const uint32_t nsub = (nc + prm_.sub - 1) / prm_.sub;
    GzChainSum sum{};
    if (int rc = be_->run(file_ + B0, nc, pbit, prm_.sub, nsub, prm_.ratio, win_, wlen_, rows_, chain_, sum, win_new_, msg)) return rc;
    ++ctr.super_chunks;
    if (keep_rows) rows_all.insert(rows_all.end(), rows_.begin(), rows_.end());
    if (sum.nchain > nsub || chain_.size() != sum.nchain) {
      msg = "gzip inflater: the chain stage returned an impossible chain";
      return -4;
    }
    if (sum.nchain == 0 && sum.bad_at == kGzNone) { // (cannot be: sub-chunk 0 always is on the chain)
      msg = "gzip inflater: the chain stage returned no chain";
      return -4;
    }
    mark_point();
    // what lies behind the verified end is the next super-chunk's again (many small members, a false start, an overflow: the cost shows here)
    struct Redo {
      GzInflater* g;
      uint64_t n;
      ~Redo()
      {
        if (!g->done_) g->ctr.redone_bytes += n;
      }
    } redo{this, nc - std::min<uint64_t>(nc, ((uint64_t)sum.end_bit + 7) >> 3)};
    uint64_t total = 0;
    std::vector<uint8_t> on_chain(nsub, 0);
    uint64_t all = 0;
    for (uint32_t k = 0; k < sum.nchain; ++k) {
      const GzSubRow& r = rows_[chain_[k]];
      on_chain[chain_[k]] = 1;
      all += r.len;
      if (sum.bad_at != kGzNone && chain_[k] >= sum.bad_at) continue; // what is handed out ends in front of the first bad chunk
      crc_ = gz_crc_combine(crc_, r.crc, r.len), mlen_ += r.len, total += r.len;
    }
    if (all != sum.total) {
      msg = "gzip inflater: the chain's lengths do not add up";
      return -4;
    }
    ctr.linked += sum.nchain ? sum.nchain - 1 : 0;
    for (uint32_t i = 1; i < nsub; ++i) { // (what lies behind the verified end is searched again by the next super-chunk, and counted again)
      if (rows_[i].S == kGzNone) ++ctr.without_start;
      else if (!on_chain[i]) ++ctr.dropped; // decoded, not used: a false start, or a start behind where the chain ended
    }
    pend_host_ = false, pend_off_ = 0, pend_end_ = total, out_off_ += total;
    memcpy(win_, win_new_, kGzWin);
    wlen_ = (uint32_t)std::min<uint64_t>(kGzWin, wlen_ + total);
    const uint64_t end_file_bit = B0 * 8 + sum.end_bit;
    if (sum.bad_at != kGzNone) {
      later(inf_rule_name(INF_DIST_FAR), (B0 * 8 + rows_[sum.bad_at < nsub ? sum.bad_at : 0].S) >> 3);
      return 0;
    }
    if (sum.end_status == GZ_MEMBER_END) {
      P_ = end_file_bit;
      member_end(end_file_bit);
      return 0;
    }
    if (sum.end_status == GZ_BAD) {
      const uint32_t c = chain_.back();
      later(inf_rule_name(rows_[c].link), end_file_bit >> 3);
      return 0;
    }
    if (sum.end_bit > pbit) { // the verified prefix is kept
      P_ = end_file_bit;
      return 0;
    }
    return host_range((B0 + nc) * 8); // the first sub-chunk could not finish a block
  }
};

// ---- the stages' serial twin --------------------------------------------------------------------------------------------------------
class GzHostBackend : public GzBackend {
 public:
  int run(const uint8_t* comp, uint32_t nc, uint32_t pbit, uint32_t sub, uint32_t nsub, uint32_t ratio, const uint8_t* win, uint32_t wlen,
          std::vector<GzSubRow>& rows, std::vector<uint32_t>& chain, GzChainSum& sum, uint8_t* win_out, std::string&) override
  {
    // every buffer is a heap block of exactly its size (the sanitizer program sees the first byte outside)
    std::unique_ptr<uint8_t[]> in(new uint8_t[nc]);
    memcpy(in.get(), comp, nc);
    const uint64_t nsym = (uint64_t)ratio * ((uint64_t)nc * 8u - pbit) / 8u;
    std::unique_ptr<uint16_t[]> sym(new uint16_t[nsym ? nsym : 1]);
    std::unique_ptr<uint32_t[]> S(new uint32_t[nsub]), end(new uint32_t[nsub]), status(new uint32_t[nsub]), link(new uint32_t[nsub]), len(new uint32_t[nsub]);
    std::unique_ptr<InfTables> T(new InfTables);
    GzSuper G{in.get(), nc, pbit, sub, nsub, ratio, sym.get(), S.get(), end.get(), status.get(), link.get(), len.get()};
    for (uint32_t i = 0; i < nsub; ++i) gz_search_sub(G, i, *T);
    SymSerial L;
    for (uint32_t i = 0; i < nsub; ++i) gz_decode_sub(G, i, *T, L);
    rows.resize(nsub);
    for (uint32_t i = 0; i < nsub; ++i) rows[i] = GzSubRow{S[i], end[i], status[i], link[i], len[i], 0};
    // chain
    chain.clear();
    std::vector<uint32_t> offs, wlens;
    std::unique_ptr<uint8_t[]> wins(new uint8_t[(size_t)kGzWin * 2]); // in front of / behind the current chain chunk
    uint8_t *w = wins.get(), *nw = wins.get() + kGzWin;
    memcpy(w, win, kGzWin);
    sum = GzChainSum{0, pbit, GZ_IDLE, kGzNone, 0};
    std::vector<std::vector<uint8_t>> chain_wins; // the window in front of every chain chunk (the resolve stage's)
    uint32_t c = 0, wl = wlen;
    uint64_t off = 0;
    for (;;) {
      const uint16_t* cs = sym.get() + gz_slot_base(G, S[c]);
      uint32_t bad = 0;
      for (uint32_t t = 0; t < kGzWin; ++t) nw[t] = gz_chain_window(cs, len[c], w, wl, t, &bad);
      if (bad) {
        sum.bad_at = c, sum.end_status = GZ_BAD;
        break;
      }
      chain.push_back(c), offs.push_back((uint32_t)off), wlens.push_back(wl);
      chain_wins.emplace_back(w, w + kGzWin);
      off += len[c], wl = std::min<uint32_t>(kGzWin, wl + len[c]);
      std::swap(w, nw);
      sum.end_bit = end[c], sum.end_status = status[c];
      if (status[c] != GZ_LINKED || link[c] <= c || link[c] >= nsub) break;
      c = link[c];
    }
    sum.nchain = (uint32_t)chain.size(), sum.total = off;
    memcpy(win_out, w, kGzWin);
    // resolve
    out_.reset(new uint8_t[off ? off : 1]);
    out_n_ = off;
    for (uint32_t k = 0; k < sum.nchain; ++k) {
      const uint32_t cc = chain[k];
      const uint16_t* cs = sym.get() + gz_slot_base(G, S[cc]);
      uint8_t* o = out_.get() + offs[k];
      uint32_t bad = 0;
      for (uint32_t i = 0; i < len[cc]; ++i) o[i] = gz_resolve_symbol(cs[i], chain_wins[k].data(), wlens[k], &bad);
      if (bad && (sum.bad_at == kGzNone || cc < sum.bad_at)) sum.bad_at = cc;
      rows[cc].crc = crc_sliced_host(crc_host_table(), o, len[cc]);
    }
    return 0;
  }
  int fetch(uint8_t* dst, uint64_t off, uint64_t n, std::string&) override
  {
    if (off + n > out_n_) return -1;
    memcpy(dst, out_.get() + off, n);
    return 0;
  }

 private:
  std::unique_ptr<uint8_t[]> out_;
  uint64_t out_n_ = 0;
};

// (tests) a whole gzip buffer through a backend: all its bytes, the rows of every super-chunk one after the other, the counters.
// 0, -1 (KR_ERR_ARG: out or the tables are too small), -2 (damage; *len bytes in front of it are in out), or a backend's code
inline int gz_debug_run(GzBackend& be, const uint8_t* comp, uint64_t n, const GzParams& prm, uint8_t* out, uint64_t cap, uint64_t* len, uint64_t tab_cap,
                        uint32_t* S, uint32_t* end, uint32_t* status, uint32_t* link, uint32_t* length, uint32_t* crc, uint64_t* ntab, uint64_t* counters,
                        std::string& msg)
{
  *len = 0, *ntab = 0;
  GzInflater g(&be, comp, n, prm, "(buffer)");
  g.keep_rows = true;
  int rc = g.open();
  while (!rc) {
    uint64_t k = 0;
    rc = g.read(out + *len, cap - *len, &k);
    if (rc || k == 0) break;
    *len += k;
    if (*len == cap) { // full: only the end may follow
      uint8_t one;
      rc = g.read(&one, 1, &k);
      if (!rc && k) {
        msg = "kr_debug_gzdev_inflate: the buffer inflates to more bytes than `cap`";
        return -1;
      }
      break;
    }
  }
  if (rc) msg = g.msg;
  const uint64_t nt = g.rows_all.size();
  if (nt > tab_cap) {
    msg = "kr_debug_gzdev_inflate: more sub-chunk rows than `tab_cap`";
    return -1;
  }
  for (uint64_t i = 0; i < nt; ++i) {
    const GzSubRow& r = g.rows_all[i];
    S[i] = r.S, end[i] = r.end, status[i] = r.status, link[i] = r.link, length[i] = r.len, crc[i] = r.crc;
  }
  *ntab = nt;
  counters[0] = g.ctr.super_chunks, counters[1] = g.ctr.linked, counters[2] = g.ctr.without_start, counters[3] = g.ctr.dropped, counters[4] = g.ctr.host_ranges, counters[5] = g.ctr.redone_bytes;
  return rc;
}

// (tests) the restart point at or in front of inflated_off, as an inflater over `be` that has read that far keeps it
inline int gz_debug_point(GzBackend& be, const uint8_t* comp, uint64_t n, const GzParams& prm, uint64_t inflated_off, GzPoint* out, std::string& msg)
{
  GzInflater g(&be, comp, n, prm, "(buffer)");
  int rc = g.open();
  std::vector<uint8_t> sink(1u << 16);
  uint64_t got = 0;
  while (!rc && g.inflated() <= inflated_off) {
    uint64_t k = 0;
    rc = g.read(sink.data(), sink.size(), &k);
    if (rc || k == 0) break;
    got += k;
  }
  if (rc) {
    msg = g.msg;
    return rc;
  }
  const GzPoint* best = nullptr;
  for (const GzPoint& p : g.points)
    if (p.inflated_off <= inflated_off && (!best || p.inflated_off >= best->inflated_off)) best = &p;
  if (!best) {
    msg = "no restart point is kept that far back";
    return -1;
  }
  *out = *best;
  return 0;
}

} // namespace kr
#endif
