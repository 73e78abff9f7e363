// kr_sdust.h — the symmetric DUST masker (`--sdust-t/-w`) as ONE piece of code for the host and the device.
//
// Behaviour restated from the reference's sdust_core (src/sdust.h:90-185): the result for a contig equals
// sdust(0, seq, -1, T, W, &n) element for element, including what that code does at an N: only `l` and `t` are
// reset there (:176-181), the word deque, cv, cw, L, rv and rw live on, so words from before an N run keep taking
// part behind it and an interval may cover N bases or reach past the end of the contig (finish <= start + W).
//
// The state machine does not read bases.  It replays EVENTS, one per base position at most:
//   word  (t, start): a 3-base word t was completed; start = first base of the current window (:170)
//   break (start):    the first non-base after a base, or the end of the contig; start as computed at :177
// (an N that follows an N, or opens the contig, finds the list P empty and does nothing).  sdust_scan() yields the
// events of a contig from its bases.
//
// All events of a contig go through one state; saved intervals are merged into the list as :111-126 does (kr_build.cpp).
// That merge looks at the LAST list element only, and it is not always a union: behind an N the stale ring places candidates
// at ring index + window start (:146), ahead of where their words lie, so a second N within W bases can flush an entry whose
// start lies beyond intervals found and saved afterwards; the list then keeps the LATER start and drops the bases in front
// of it (fixture entry "two_N_within_W").  P, the list of perfect intervals of a window, is not small either: a homopolymer
// fills (W-5)(W-6)/2 entries (1711 at W = 64), a stale ring twice that.  Both stand in the way of replaying a contig in
// independent chunks on the device (tried: docs/design/07_minimizers_build.md §3.6); the state machine is written with fixed-size
// state and __host__ __device__ so that such a path can use it.
#ifndef KR_SDUST_H
#define KR_SDUST_H

#include <cstdint>

#if defined(__HIPCC__)
#define KR_SD_HD __host__ __device__
#else
#define KR_SD_HD
#endif

namespace kr {

// seq2nt4 of src/sdust.h:53-60: bytes 0..3 and ACGTacgt are bases.  (The minimizers' seq_nt4_table differs: bytes 1..3 are no
// bases there.)
KR_SD_HD inline uint32_t sdust_code(uint8_t c)
{
  if (c < 4) return c;
  const uint32_t u = c | 0x20u;
  return u == 'a' ? 0u : u == 'c' ? 1u : u == 'g' ? 2u : u == 't' ? 3u : 4u;
}

struct SdustEvent {
  uint32_t start; // window start (word) / flush start (break)
  uint32_t tk;    // word: t (6 bits); break: kSdustBreak
};
constexpr uint32_t kSdustBreak = 64;

struct alignas(16) SdustPerf {
  int32_t start, finish, r, l;
};

// Cnt: type of the 2 x 64 word counters (a count never exceeds W-2)
template <typename Cnt>
struct SdustState {
  uint8_t* ring;  // [rcap], rcap >= W-2: the word deque
  SdustPerf* P;   // [pcap]: perfect intervals of the current window, by descending start, then ascending finish
  int32_t rcap, front, count;
  int32_t pcap, pn, pmax;
  int32_t L, rv, rw, T, W;
  int32_t overflow; // P needed more than pcap entries: the result is not to be used
  Cnt cv[64], cw[64];
};

template <typename Cnt>
KR_SD_HD inline void sdust_reset(SdustState<Cnt>& S)
{
  S.front = S.count = 0;
  S.pn = 0;
  S.L = S.rv = S.rw = 0;
  for (int q = 0; q < 64; ++q) S.cv[q] = 0, S.cw[q] = 0;
}
template <typename Cnt>
KR_SD_HD inline void sdust_init(SdustState<Cnt>& S, uint8_t* ring, int32_t rcap, SdustPerf* P, int32_t pcap, int32_t T, int32_t W)
{
  S.ring = ring, S.rcap = rcap, S.P = P, S.pcap = pcap, S.T = T, S.W = W;
  S.pmax = 0, S.overflow = 0;
  sdust_reset(S);
}
template <typename Cnt>
KR_SD_HD inline int32_t sdust_at(const SdustState<Cnt>& S, int32_t i)
{
  int32_t p = S.front + i;
  if (p >= S.rcap) p -= S.rcap;
  return S.ring[p];
}

// shift_window, src/sdust.h:90-109
template <typename Cnt>
KR_SD_HD inline void sdust_shift_window(SdustState<Cnt>& S, int32_t t)
{
  if (S.count >= S.W - 2) {
    const int32_t s = S.ring[S.front];
    if (++S.front == S.rcap) S.front = 0;
    --S.count;
    S.rw -= (int32_t)--S.cw[s];
    if (S.L > S.count) --S.L, S.rv -= (int32_t)--S.cv[s];
  }
  {
    int32_t p = S.front + S.count;
    if (p >= S.rcap) p -= S.rcap;
    S.ring[p] = (uint8_t)t;
    ++S.count;
  }
  ++S.L;
  S.rw += (int32_t)S.cw[t]++;
  S.rv += (int32_t)S.cv[t]++;
  if ((int64_t)S.cv[t] * 10 > ((int64_t)S.T << 1)) {
    int32_t s;
    do {
      s = sdust_at(S, S.count - S.L);
      S.rv -= (int32_t)--S.cv[s];
      --S.L;
    } while (s != t);
  }
}

// save_masked_regions, src/sdust.h:111-126, without the merge into the result list: emit(start, finish) gets the raw interval
template <typename Cnt, class Emit>
KR_SD_HD inline void sdust_save(SdustState<Cnt>& S, int32_t start, Emit& emit)
{
  if (S.pn == 0 || S.P[S.pn - 1].start >= start) return;
  emit(S.P[S.pn - 1].start, S.P[S.pn - 1].finish);
  int32_t i = S.pn - 1;
  while (i >= 0 && S.P[i].start < start) --i;
  S.pn = i + 1;
}

// find_perfect, src/sdust.h:128-151
template <typename Cnt>
KR_SD_HD inline void sdust_find_perfect(SdustState<Cnt>& S, int32_t start)
{
  Cnt c[64];
  for (int q = 0; q < 64; ++q) c[q] = S.cv[q];
  int32_t r = S.rv, max_r = 0, max_l = 0;
  for (int32_t i = S.count - S.L - 1; i >= 0; --i) {
    const int32_t t = sdust_at(S, i);
    r += (int32_t)c[t]++;
    const int32_t new_r = r, new_l = S.count - i - 1;
    if ((int64_t)new_r * 10 > (int64_t)S.T * new_l) {
      int32_t j = 0;
      for (; j < S.pn && S.P[j].start >= i + start; ++j) {
        const SdustPerf& p = S.P[j];
        if (max_r == 0 || (int64_t)p.r * max_l > (int64_t)max_r * p.l) max_r = p.r, max_l = p.l;
      }
      if (max_r == 0 || (int64_t)new_r * max_l >= (int64_t)max_r * new_l) {
        max_r = new_r, max_l = new_l;
        if (S.pn >= S.pcap) {
          S.overflow = 1;
          return;
        }
        for (int32_t q = S.pn; q > j; --q) S.P[q] = S.P[q - 1];
        ++S.pn;
        if (S.pn > S.pmax) S.pmax = S.pn;
        S.P[j].start = i + start, S.P[j].finish = S.count + 2 + start;
        S.P[j].r = new_r, S.P[j].l = new_l;
      }
    }
  }
}

// one event through the state (src/sdust.h:169-181)
template <typename Cnt, class Emit>
KR_SD_HD inline void sdust_event(SdustState<Cnt>& S, SdustEvent e, Emit& emit)
{
  int32_t start = (int32_t)e.start;
  if (e.tk < kSdustBreak) {
    sdust_save(S, start, emit);
    sdust_shift_window(S, (int32_t)e.tk);
    if ((int64_t)S.rw * 10 > (int64_t)S.L * S.T) sdust_find_perfect(S, start);
  } else {
    while (S.pn) sdust_save(S, start++, emit);
  }
}

// The events of one contig in order (src/sdust.h:165-181): f(SdustEvent) for each.
template <class F>
inline void sdust_scan(const uint8_t* seq, uint64_t len, uint32_t W, F&& f)
{
  int64_t l = 0;
  uint32_t t = 0;
  const int64_t Wl = (int64_t)W;
  for (int64_t i = 0; i <= (int64_t)len; ++i) {
    const uint32_t b = i < (int64_t)len ? sdust_code(seq[i]) : 4u;
    if (b < 4) {
      ++l, t = (t << 2 | b) & 63u;
      if (l >= 3) f(SdustEvent{(uint32_t)((l - Wl > 0 ? l - Wl : 0) + (i + 1 - l)), t});
    } else {
      if (l > 0) f(SdustEvent{(uint32_t)((l - Wl + 1 > 0 ? l - Wl + 1 : 0) + (i + 1 - l)), kSdustBreak});
      l = 0, t = 0;
    }
  }
}

} // namespace kr

#endif
