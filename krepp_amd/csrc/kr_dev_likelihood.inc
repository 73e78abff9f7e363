// kr_dev_likelihood.inc -- part of kr_device.hip (one translation unit, included in order): likelihood, Brent, de-duplication, selection kernels.

// ---------------------------------------------------------------------------
// Likelihood (HDistHistLLH::operator(), src/hdhistllh.hpp:71-89) and Brent
// ---------------------------------------------------------------------------
struct LlhProblem {
  double mc[kMaxPlanes];
  double uc, rho;
};

// x^n for a small positive integer n in double-double arithmetic (error-free products through fma).
// The chain carries ~100 bits, so the rounded result is the correctly rounded power except in
// near-tie cases: the contract of glibc's pow, which the reference calls at src/hdhistllh.hpp:74,
// and tighter (and ~3x cheaper) than the general-purpose device pow.
struct DD {
  double hi, lo;
};
__device__ __forceinline__ DD dd_mul(DD a, DD b)
{
  double p = a.hi * b.hi;
  double e = fma(a.hi, b.hi, -p);
  e = fma(a.hi, b.lo, e);
  e = fma(a.lo, b.hi, e);
  double s = p + e;
  return DD{s, e - (s - p)};
}
__device__ __forceinline__ double pown_dd(double x, uint32_t n)
{
  DD r{1.0, 0.0}, b{x, 0.0};
  while (n) {
    if (n & 1u) r = dd_mul(r, b);
    n >>= 1;
    if (n) b = dd_mul(b, b);
  }
  return r.hi + r.lo;
}

// Natural logarithm of a positive normal double, error < 1 ulp: the argument reduction and the degree-14
// minimax polynomial of the classic freely distributable libm `log` (x = 2^k (1+f), s = f/(2+f),
// log(1+f) = f - s (f - R(s^2)), k ln2 added in two pieces), restated without its special cases -- the
// likelihood only takes logs of numbers in (1e-300, 1].  40 instructions against the 75 of the general
// device `log`, and the objective takes three per evaluation (55 % of its instructions before).
__device__ __attribute__((noinline)) double kr_log_general(double x) { return log(x); }
__device__ __forceinline__ double kr_log(double x)
{
#ifdef KR_OCML_LOG
  return log(x);
#endif
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  if (!(x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308)) return kr_log_general(x); // zero, subnormal, negative, inf, nan
  int32_t hx = __double2hiint(x);
  const uint32_t lx = (uint32_t)__double2loint(x);
  int32_t k = (hx >> 20) - 1023;
  hx &= 0x000fffff;
  int32_t i = (hx + 0x95f64) & 0x100000;
  x = __hiloint2double(hx | (i ^ 0x3ff00000), (int32_t)lx); // normalise x or x/2
  k += i >> 20;
  const double f = x - 1.0;
  const double s = f / (2.0 + f);
  const double dk = (double)k;
  const double z = s * s;
  i = hx - 0x6147a;
  const double w = z * z;
  const int32_t j = 0x6b851 - hx;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  i |= j;
  const double R = t2 + t1;
  if (i > 0) {
    const double hfsq = 0.5 * f * f;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  }
  return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

typedef KR_LDS double lds_f64;
struct LlhTables { // per-workgroup copies of the binomial tables (uniform LDS reads, no scalar-load stalls)
  lds_f64* bk;  // [k+1]
  lds_f64* hnk; // [th+1]
};
__device__ __forceinline__ void llh_tables_init(const LlhConst& C, lds_f64* bk, lds_f64* hnk)
{
  for (uint32_t i = threadIdx.x; i <= C.k; i += blockDim.x) bk[i] = C.binom_k[i];
  for (uint32_t i = threadIdx.x; i <= C.th; i += blockDim.x) hnk[i] = C.binom_hnk[i];
  __syncthreads();
}

// HDistHistLLH::operator() (src/hdhistllh.hpp:71-89), same operation order.  NPT = th+1 when known
// at compile time (histogram in registers), 0 = any th.
// The objective splits into a part that depends on d alone -- (1-d)^k, two logs, the (k+1)-term sum lv_m:
// 85 % of the work -- and a cheap combination with the record's histogram.  Same operations, same order,
// as the single loop of the reference (the two accumulators never meet before the last line).
struct LlhShared {
  double logdn, logdp, lv_m; // k log(1-d), log(d) - log(1-d), sum of the likelihood weights
};
template <int NPT>
__device__ __forceinline__ LlhShared llh_dpart(const LlhConst& C, const LlhTables& T, double d)
{
  LlhShared g;
  double lv_m = 0.0;
  double powdc = (C.dbg & 1u) ? pow(1.0 - d, (double)C.k) : pown_dd(1.0 - d, C.k);
  g.logdn = kr_log(1.0 - d);
  g.logdp = kr_log(d) - g.logdn;
  g.logdn *= (double)C.k;
  const double dratio = d / (1.0 - d);
  if (NPT > 0) {
#pragma unroll
    for (int x = 0; x < NPT; ++x) {
      lv_m += T.hnk[x] * powdc;
      powdc *= dratio;
    }
  } else {
    for (uint32_t x = 0; x <= C.th; ++x) {
      lv_m += T.hnk[x] * powdc;
      powdc *= dratio;
    }
  }
  // (a fully unrolled k = 29 tail with the binomials in SGPRs was tried: 37 SGPR spills, 2 % slower)
#pragma unroll 4
  for (uint32_t x = C.th + 1; x <= C.k; ++x) {
    lv_m += powdc * T.bk[x];
    powdc *= dratio;
  }
  g.lv_m = lv_m;
  return g;
}
template <int NPT>
__device__ __forceinline__ double llh_combine(const LlhConst& C, const LlhShared& g, const LlhProblem& p)
{
  double sum = 0.0;
  if (NPT > 0) {
#pragma unroll
    for (int x = 0; x < NPT; ++x) sum -= (g.logdn + (double)x * g.logdp) * p.mc[x];
  } else {
    for (uint32_t x = 0; x <= C.th; ++x) sum -= (g.logdn + (double)x * g.logdp) * p.mc[x];
  }
  return sum - kr_log(p.rho * g.lv_m + 1.0 - p.rho) * p.uc;
}
template <int NPT>
__device__ __forceinline__ double llh_eval(const LlhConst& C, const LlhTables& T, const LlhProblem& p, double d)
{
  return llh_combine<NPT>(C, llh_dpart<NPT>(C, T, d), p);
}

// boost::math::tools::brent_find_minima(f, 1e-10, 0.5, 16) (src/query.cpp:430);
// published algorithm, see SURVEY.md Appendix B.  The minimisation is written as a resumable state
// machine -- one objective evaluation per step() -- so that the record kernel can hand a lane a new
// record the moment its minimisation converges (the number of evaluations varies 10..23 between
// records; a wave that waits for its slowest lane idles 40 % of its lanes).
struct BrentState {
  double x, w, v, fx, fw, fv, mn, mx, delta, delta2;
  int it;
};
constexpr double kBrentTol = 0x1p-15; // ldexp(1, 1 - min(53/2, 16))

// Before an evaluation: false if converged (result is x, fx), else the next abscissa in u.
__device__ __forceinline__ bool brent_next(BrentState& s, double& u)
{
  const double golden = 0.3819660f;
  const double mid = (s.mn + s.mx) / 2;
  const double fract1 = kBrentTol * fabs(s.x) + kBrentTol / 4;
  const double fract2 = 2 * fract1;
  if (s.it >= 1000 || fabs(s.x - mid) <= (fract2 - (s.mx - s.mn) / 2)) return false;
  ++s.it;
  if (fabs(s.delta2) > fract1) {
    double r = (s.x - s.w) * (s.fx - s.fv);
    double q = (s.x - s.v) * (s.fx - s.fw);
    double pp = (s.x - s.v) * q - (s.x - s.w) * r;
    q = 2 * (q - r);
    if (q > 0) pp = -pp;
    q = fabs(q);
    double td = s.delta2;
    s.delta2 = s.delta;
    if ((fabs(pp) >= fabs(q * td / 2)) || (pp <= q * (s.mn - s.x)) || (pp >= q * (s.mx - s.x))) {
      s.delta2 = (s.x >= mid) ? s.mn - s.x : s.mx - s.x;
      s.delta = golden * s.delta2;
    } else {
      s.delta = pp / q;
      u = s.x + s.delta;
      if (((u - s.mn) < fract2) || ((s.mx - u) < fract2)) s.delta = (mid - s.x) < 0 ? -fabs(fract1) : fabs(fract1);
    }
  } else {
    s.delta2 = (s.x >= mid) ? s.mn - s.x : s.mx - s.x;
    s.delta = golden * s.delta2;
  }
  u = (fabs(s.delta) >= fract1) ? (s.x + s.delta) : (s.delta > 0 ? (s.x + fabs(fract1)) : (s.x - fabs(fract1)));
  return true;
}
// First evaluation (at the upper bracket end).
__device__ __forceinline__ void brent_start(BrentState& s, double u, double fu)
{
  s.mn = 1e-10, s.mx = 0.5;
  s.x = s.w = s.v = u;
  s.fw = s.fv = s.fx = fu;
  s.delta2 = s.delta = 0;
  s.it = 0;
}
// After an evaluation at u.
__device__ __forceinline__ void brent_update(BrentState& s, double u, double fu)
{
  if (fu <= s.fx) {
    if (u >= s.x)
      s.mn = s.x;
    else
      s.mx = s.x;
    s.v = s.w, s.w = s.x, s.x = u;
    s.fv = s.fw, s.fw = s.fx, s.fx = fu;
  } else {
    if (u < s.x)
      s.mn = u;
    else
      s.mx = u;
    if ((fu <= s.fw) || (s.w == s.x)) {
      s.v = s.w, s.w = u;
      s.fv = s.fw, s.fw = fu;
    } else if ((fu <= s.fv) || (s.v == s.x) || (s.v == s.w)) {
      s.v = u;
      s.fv = fu;
    }
  }
}

template <int NPT>
__device__ __forceinline__ void brent_min(const LlhConst& C, const LlhTables& T, const LlhProblem& p, double& d_out, double& v_out)
{
  BrentState s;
  double u = 0.5;
  brent_start(s, u, llh_eval<NPT>(C, T, p, u));
  while (brent_next(s, u)) brent_update(s, u, llh_eval<NPT>(C, T, p, u));
  d_out = s.x;
  v_out = s.fx;
}

template <int NPT>
__device__ __forceinline__ void load_problem(const LlhConst& C, const uint32_t* hist, uint64_t stride, uint32_t onmers,
                                             double rho, LlhProblem& p)
{ // hist[x] of this record at hist[x * stride]
  uint32_t mc = 0;
  if (NPT > 0) {
#pragma unroll
    for (int x = 0; x < NPT; ++x) {
      uint32_t hv = hist[(uint64_t)x * stride];
      p.mc[x] = (double)hv;
      mc += hv;
    }
  } else {
    for (uint32_t x = 0; x <= C.th; ++x) {
      uint32_t hv = hist[(uint64_t)x * stride];
      p.mc[x] = (double)hv;
      mc += hv;
    }
  }
  p.uc = (double)onmers - (double)mc; // mismatch_count = onmers - match_count (src/query.cpp:104)
  p.rho = rho;
}

// The problem of record i: from its packed word where there is one (then the record has no planes unless the batch
// keeps histograms), else from its planes and its read's k-mer count.
template <int NPT>
__device__ __forceinline__ void load_record(const LlhConst& C, const BatchOut& out, uint32_t i, double rho, LlhProblem& p)
{
  const uint64_t w0 = out.rec_w0[i];
  if (w0 != 0ull) { // five 8-bit counts (th = 4), k-mers of the read in bits 40..55
    uint32_t mc = 0;
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      const uint32_t hv = (uint32_t)(w0 >> (8 * x)) & 255u;
      p.mc[x] = (double)hv;
      mc += hv;
    }
    p.uc = (double)((uint32_t)(w0 >> 40) & 0xFFFFu) - (double)mc;
    p.rho = rho;
    return;
  }
  load_problem<NPT>(C, out.rec_hist + i, out.rec_stride, out.rd_onmers[out.rec_read[i]], rho, p);
}
// match_count of record i (src/query.cpp:129-133)
__device__ __forceinline__ uint32_t record_matches(const LlhConst& C, const BatchOut& out, uint32_t i)
{
  const uint64_t w0 = out.rec_w0[i];
  uint32_t m = 0;
  if (w0 != 0ull) {
#pragma unroll
    for (int x = 0; x < 5; ++x) m += (uint32_t)(w0 >> (8 * x)) & 255u;
    return m;
  }
  for (uint32_t x = 0; x <= C.th; ++x) m += out.rec_hist[(uint64_t)x * out.rec_stride + i];
  return m;
}

// ---------------------------------------------------------------------------
// Likelihood de-duplication.  The ML distance of a record is a pure function of (leaf -> rho, histogram,
// number of k-mers of the read), and a batch repeats the same few problems over and over -- a reference
// reached by one k-mer at Hamming distance 1 from a 150-bp read is THE most common record.  kr_dedup_kernel
// finds the distinct problems of the batch with an open-addressing table in HBM (slot = 64-bit histogram
// word claimed by CAS + 64-bit {leaf, list position}), the likelihood kernels run on the distinct ones, and
// kr_select_kernel hands the result to the duplicates (rec_d / rec_v) as it reads the records.  Nothing is kept between batches.  Records the
// 64-bit word cannot describe (th != 4, a count above 255, more than 65535 k-mers) are their own problem.  The word is packed by kr_acc_kernel as it writes the record.
// ---------------------------------------------------------------------------
// List positions are handed out to waves in chunks: ONE shared counter serves ~90 M atomics/s, and with chunks of 16 the 6.5 M
// distinct problems of a 2 M-read batch on the 10,000-genome index cost 400,000 of them -- the kernel's whole run time (4.08 ms;
// 1.08 ms with chunks of 128, profiles/round5_*).  The chunk grows with the records a wave works through (1 / 16 of them, 16 ..
// kRepChunkMax): a small batch does not strew holes over its list (the unused tail of a wave's last chunk is marked as holes,
// which the likelihood kernels skip).
#ifndef KR_REP_CHUNK
#define KR_REP_CHUNK 256
#endif
constexpr uint32_t kRepChunk = 16, kRepChunkMax = KR_REP_CHUNK;
constexpr uint32_t kDedupBlocks = 4096;                      // grid of kr_dedup_kernel (256 threads a block)
constexpr uint32_t kRepSlack = kDedupBlocks * 4u * kRepChunkMax; // list positions its waves may leave unused
constexpr uint32_t kDdMinSlots = 1024;    // the fewest table slots a batch uses (dd_mask)
constexpr int kDdProbeRounds = 48;        // rounds of kr_dedup_kernel's retry loop; a record still unresolved then stands alone
constexpr uint32_t kDdOslotReads = 4096;  // reads per block of kr_dedup_oslot_kernel's grid (launch_likelihood)
constexpr uint64_t kDdHashWord = 0x9E3779B97F4A7C15ull; // first slot = (word * kDdHashWord) >> 32 ^ leaf * kDdHashLeaf, masked
constexpr uint32_t kDdHashLeaf = 0x85EBCA6Bu;
#ifndef KR_DEDUP_PROBE16
#define KR_DEDUP_PROBE16 1
#endif
__device__ __forceinline__ uint32_t dd_mask(const BatchOut& out)
{ // table slots used for this batch: a power of two >= (number of record slots) >> dd_shift, at most dd_slots
  const uint32_t n = min(out.counters[kCtRecSlots], out.rec_cap);
  uint32_t m = kDdMinSlots;
  while (m < out.dd_slots && m < (n >> out.dd_shift)) m <<= 1;
  return m - 1u;
}
#ifndef KR_DD_DIRECT
#define KR_DD_DIRECT 1
#endif
constexpr uint32_t kDdMaxEvents = 3, kDdClasses = 55 /* multisets of 1..3 out of 5 hd values */, kDdOslots = 8;
constexpr uint32_t kDdDirectFlag = 0x80000000u; // rec_rep: the low bits are a place in dd_direct (never 0x7FFFFFFF: 0xFFFFFFFF stays "hole")
__global__ __launch_bounds__(256) void kr_dedup_clear_kernel(BatchOut out)
{
  const uint32_t n = dd_mask(out) + 1u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out.dd_table[i] = make_ulonglong2(0, 0);
  if (out.dd_nodes) {
    const uint32_t nd = kDdOslots * kDdClasses * out.dd_nodes; // (a multiple of 4 words is allocated)
    u32x4* d4 = reinterpret_cast<u32x4*>(out.dd_direct);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < (nd + 3u) / 4u; i += gridDim.x * blockDim.x) d4[i] = u32x4{~0u, ~0u, ~0u, ~0u};
    if (blockIdx.x == 0)
      for (uint32_t i = threadIdx.x; i < 257u; i += blockDim.x) out.dd_ohist[i] = 0;
  }
}
// The kDdOslots most frequent k-mer counts among the batch's reads (a 150-bp read without N has L - k + 1; one N in a hundred reads
// adds a few neighbours) get a slot of the direct part; ties go to the larger count.  Last block out picks them (ticket).
__global__ __launch_bounds__(256) void kr_dedup_oslot_kernel(BatchOut out, uint32_t nreads)
{
  __shared__ uint32_t s_h[256];
  __shared__ uint32_t s_last;
  s_h[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += gridDim.x * blockDim.x) {
    const uint32_t om = out.rd_onmers[r];
    if (om < 256u && out.rd_cnt[r] != 0) atomicAdd(&s_h[om], 1u);
  }
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&out.dd_ohist[threadIdx.x], s_h[threadIdx.x]);
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(&out.dd_ohist[256], 1u) == gridDim.x - 1u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  s_h[threadIdx.x] = __hip_atomic_load(&out.dd_ohist[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  // rank of my count among the 256 (more reads first, then the larger count): the first kDdOslots get slots
  const uint32_t mine = s_h[threadIdx.x];
  uint32_t rank = 0;
  for (uint32_t j = 0; j < 256u; ++j) {
    const uint32_t o = s_h[j];
    rank += (o > mine || (o == mine && j > threadIdx.x)) ? 1u : 0u;
  }
  out.dd_oslot[threadIdx.x] = (mine != 0 && rank < kDdOslots) ? (uint8_t)rank : (uint8_t)0xFF;
}
__global__ __launch_bounds__(256) void kr_dedup_kernel(BatchOut out)
{
  const uint32_t nrec = min(out.counters[kCtRecSlots], out.rec_cap);
  const uint32_t mask = dd_mask(out);
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(out.dd_table);
  // Once the table is half full a wave stops inserting (look-ups only; new problems stand alone).  The wave learns
  // it from the list positions its own insertions get: a shared flag polled by every wave was measured at 3x the
  // kernel's run time -- one word read by the whole chip serialises on its L2 channel.
  bool crowded = false;
  uint32_t rep_chunk = kRepChunk; // per wave: 1 / 16 of the records it works through
  {
    const uint32_t rpw = nrec / max(1u, gridDim.x * (blockDim.x / kWave));
    while (rep_chunk < kRepChunkMax && rep_chunk * 16u < rpw) rep_chunk <<= 1;
  }
  // (list positions run ahead of the insertions by the chunks' unused parts, one chunk per wave at work at most: allowed for, so
  //  that a small batch is not declared crowded by its holes -- the table then fills to 3/4 at worst)
  const uint32_t crowded_at = (mask >> 1) + min(gridDim.x * (blockDim.x / kWave), (nrec + kWave - 1u) / kWave) * rep_chunk;
  // list positions come from wave-private chunks of kRepChunk (one shared-counter atomic per chunk: distinct
  // problems are ~5 % of the records, one winner per wave and round, and a single word serves ~90 M atomics/s);
  // the unused tail of a wave's last chunk is marked as holes
  uint32_t lp_next = 0, lp_end = 0;
  auto take_positions = [&](uint32_t n) -> uint32_t { // wave-uniform
    if (lp_next + n > lp_end) {
      for (uint32_t q = lp_next + lane_id(); q < lp_end; q += 64) out.rep_list[q] = 0xFFFFFFFFu;
      const uint32_t size = max(n, rep_chunk);
      uint32_t base = 0;
      if (lane_id() == 0) base = atomicAdd(&out.counters[kCtProblems], size);
      base = __shfl(base, 0);
      if ((uint64_t)base + size > out.rep_cap) { // (round-5 advice: the slack covers one unused chunk per wave, not every discarded tail)
        if (lane_id() == 0) atomicOr(&out.counters[kCtErr], kErrRecCap); // the batch is reported as over capacity; nothing is written past the slice
        // (what the request takes of the slice is nobody's now: holes, or the likelihood kernels -- which still run -- would take whatever
        //  an earlier batch, or the allocator, left there for record indices)
        for (uint64_t q = (uint64_t)base + lane_id(); q < out.rep_cap; q += 64) out.rep_list[q] = 0xFFFFFFFFu;
        base = 0;
      }
      lp_next = base, lp_end = base + size;
    }
    const uint32_t r = lp_next;
    lp_next += n;
    return r;
  };
  __shared__ uint8_t s_cls[1024], s_oslot[256];
  const bool direct_on = KR_DD_DIRECT && out.dd_nodes != 0;
  if (direct_on) {
    for (uint32_t q = threadIdx.x; q < 1024u; q += blockDim.x) s_cls[q] = out.dd_cls[q];
    s_oslot[threadIdx.x] = out.dd_oslot[threadIdx.x];
    __syncthreads();
  }
  for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < nrec; i0 += gridDim.x * blockDim.x) { // wave-uniform trip count
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t key = i < nrec ? out.rec_key[i] : 0u;
    bool todo = key != 0; // 0 = hole at the end of a wave's record chunk
    bool own = false;     // becomes its own problem without the table
    uint64_t w0 = 0;
    uint32_t pos = 0xFFFFFFFFu;
    const uint32_t se = key >> 1;
    if (todo) {
      w0 = out.rec_w0[i];
      own = w0 == 0;
    }
    if (direct_on && todo && !own) { // few events: no probe -- the problem has a place of its own
      const uint32_t lo = (uint32_t)w0, c4 = (uint32_t)(w0 >> 32) & 255u, om = (uint32_t)(w0 >> 40) & 0xFFFFu;
      // every count <= 3 (bits 2..7 of each byte clear), then the code c0 | c1 << 2 | c2 << 4 | c3 << 6 | c4 << 8
      if (((lo & 0xFCFCFCFCu) | (c4 & 0xFCu)) == 0u && om < 256u) {
        const uint32_t code = (lo & 3u) | ((lo >> 6) & 0xCu) | ((lo >> 12) & 0x30u) | ((lo >> 18) & 0xC0u) | (c4 << 8);
        const uint32_t cls = s_cls[code], sl = s_oslot[om];
        if (cls != 0xFFu && sl != 0xFFu && se < out.dd_nodes) {
          const uint32_t at = (sl * kDdClasses + cls) * out.dd_nodes + se;
          out.dd_direct[at] = i; // (a plain store: every record stored here is the same problem; the last one represents it)
          pos = kDdDirectFlag | at;
          todo = false;
        }
      }
    }
    uint32_t slot = (uint32_t)((w0 * kDdHashWord) >> 32) ^ (se * kDdHashLeaf);
    // Retry loop without an inner spin: a lane that finds its histogram word in a slot whose second word is not
    // published yet simply comes round again (the publishing lane may be in this very wave).
    const uint64_t lt = (1ull << lane_id()) - 1ull;
    for (int it = 0; it < kDdProbeRounds && __ballot(todo && !own) != 0; ++it) {
      bool won = false;
      unsigned long long old = 1ull, w1p = 0ull;
      if (todo && !own) {
        slot &= mask;
        // most records find their problem already there: look before the (much slower) atomic -- at both words of the
        // slot at once (one round trip to the L2 instead of two dependent ones; a second word that is not there yet
        // reads as "not published", which the retry below handles anyway)
#if KR_DEDUP_PROBE16
        { // ONE 16-byte request for the slot (half the L2 requests of the kernel) with the cache policy of the two agent-scope
          // atomic loads it replaces (sc1 = agent scope: past the per-CU cache, coherent in the L2 where the CAS and the
          // publishing store of this kernel live; the compiler has no 16-byte atomic load and emits a volatile one as sc0 sc1).
          // A torn pair is harmless: every decision below is re-validated by the CAS or by the words' own consistency (a
          // second word seen before its first reads as "another histogram": next slot, its own problem at worst).
          typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
          u64x2 sv;
          asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(sv) : "v"(&out.dd_table[slot]) : "memory");
          old = sv.x, w1p = sv.y;
        }
#else
        old = __hip_atomic_load(&tab[2ull * slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w1p = __hip_atomic_load(&tab[2ull * slot + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        if (old == 0ull) {
          if (crowded) {
            own = true; // not in the table and no room for it
            old = 1ull;
          } else {
            old = atomicCAS(&tab[2ull * slot], 0ull, (unsigned long long)w0);
          }
        }
        won = old == 0ull; // claimed: this record represents the problem
      }
      // list positions for the winners of this round: ONE atomic per wave (a single word serves ~90 M atomics/s)
      const uint64_t wm = __ballot(won);
      if (wm != 0) {
        const uint32_t base = take_positions((uint32_t)__popcll(wm));
        crowded = crowded || base > crowded_at;
        if (won) {
          pos = base + (uint32_t)__popcll(wm & lt);
          out.rep_list[pos] = i;
          __hip_atomic_store(&tab[2ull * slot + 1], (unsigned long long)se | ((unsigned long long)(pos + 1u) << 32), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT); // nothing else is published through it in this kernel
          todo = false;
        }
      }
      if (todo && !own && !won) {
        if (old == (unsigned long long)w0) {
          const unsigned long long w1 = w1p;
          if ((uint32_t)(w1 >> 32) != 0u) {
            if ((uint32_t)w1 == se) { // the same problem
              pos = (uint32_t)(w1 >> 32) - 1u;
              todo = false;
            } else {
              ++slot; // same histogram, another leaf
            }
          } // else: not published yet, same slot again
        } else {
          ++slot;
        }
      }
    }
    { // not describable, or the table is crowded: its own problem
      const uint64_t om = __ballot(todo);
      if (om != 0) {
        const uint32_t base = take_positions((uint32_t)__popcll(om));
        if (todo) {
          pos = base + (uint32_t)__popcll(om & lt);
          out.rep_list[pos] = i;
        }
      }
    }
    if (i < nrec) out.rec_rep[i] = pos;
  }
  for (uint32_t q = lp_next + lane_id(); q < lp_end; q += 64) out.rep_list[q] = 0xFFFFFFFFu;
}
// The marked places of the direct part become list positions: a thread looks at 16 consecutive places, a workgroup takes its
// positions with ONE atomic (4,096 places), the place then holds the position instead of the record index.
__global__ __launch_bounds__(256) void kr_dedup_direct_kernel(BatchOut out)
{
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_base;
  if (!out.dd_nodes) return;
  const uint32_t nd = kDdOslots * kDdClasses * out.dd_nodes, lane = lane_id(), w = threadIdx.x >> 6;
  const uint32_t nblk = (nd + 4095u) / 4096u;
  for (uint32_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    const uint32_t a0 = b * 4096u + threadIdx.x * 16u;
    uint32_t v[16], cnt = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      u32x4 x = u32x4{~0u, ~0u, ~0u, ~0u};
      if (a0 + 4u * q < nd) x = *reinterpret_cast<const u32x4*>(out.dd_direct + a0 + 4u * q); // (allocated in multiples of 4 words, the tail all-ones)
      v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
    }
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) cnt += v[q] != 0xFFFFFFFFu ? 1u : 0u;
    const uint32_t inc = wave_scan_incl(cnt);
    if (lane == 63u) s_w[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
      s_base = tot ? atomicAdd(&out.counters[kCtProblems], tot) : 0u;
      if ((uint64_t)s_base + tot > out.rep_cap) { // (see take_positions; at most 4,095 holes, once per batch that fails)
        atomicOr(&out.counters[kCtErr], kErrRecCap);
        for (uint64_t q = s_base; q < out.rep_cap; ++q) out.rep_list[q] = 0xFFFFFFFFu;
        s_base = 0;
      }
    }
    __syncthreads();
    uint32_t at = s_base + inc - cnt;
    for (uint32_t q = 0; q < w; ++q) at += s_w[q];
    if (cnt) {
#pragma unroll
      for (uint32_t q = 0; q < 16; ++q)
        if (v[q] != 0xFFFFFFFFu) {
          out.rep_list[at] = v[q];
          out.dd_direct[a0 + q] = at;
          ++at;
        }
    }
    __syncthreads();
  }
}
// a record's position in the list of distinct problems: its own (kr_dedup_kernel's table) or the one its direct place was given
__device__ __forceinline__ uint32_t rep_pos(const BatchOut& out, uint32_t rep)
{
  return (KR_DD_DIRECT && rep != 0xFFFFFFFFu && (rep & kDdDirectFlag)) ? out.dd_direct[rep & ~kDdDirectFlag] : rep;
}
// ... and, after the likelihood kernels, the values of the direct part's places beside them (dd_dv): the select kernels walk chains of
// dependent look-ups (record -> place -> list position -> value), and four records in five are direct.
#ifndef KR_DD_DV
#define KR_DD_DV 1
#endif
__global__ __launch_bounds__(256) void kr_dedup_dv_kernel(BatchOut out)
{
  const uint32_t nd = kDdOslots * kDdClasses * out.dd_nodes;
  for (uint32_t a0 = (blockIdx.x * 256u + threadIdx.x) * 4u; a0 < nd; a0 += gridDim.x * 1024u) { // (allocated in multiples of 4 words, the tail all-ones)
    const u32x4 x = *reinterpret_cast<const u32x4*>(out.dd_direct + a0);
    if (x.x != 0xFFFFFFFFu) out.dd_dv[a0] = out.rep_dv[x.x];
    if (x.y != 0xFFFFFFFFu) out.dd_dv[a0 + 1] = out.rep_dv[x.y];
    if (x.z != 0xFFFFFFFFu) out.dd_dv[a0 + 2] = out.rep_dv[x.z];
    if (x.w != 0xFFFFFFFFu) out.dd_dv[a0 + 3] = out.rep_dv[x.w];
  }
}
// a record's (d, v) by its rec_rep entry: one look-up, in the list of distinct problems or in the direct part's values
__device__ __forceinline__ double2 rep_value(const BatchOut& out, uint32_t rep)
{
  double2 v = make_double2(nan(""), nan(""));
  if (rep == 0xFFFFFFFFu) return v;
  if (KR_DD_DIRECT && !KR_DD_DV && (rep & kDdDirectFlag)) rep = out.dd_direct[rep & ~kDdDirectFlag];
  // (one load with the address chosen per lane, not a branch with a load on either side)
  const double2* src = (KR_DD_DIRECT && KR_DD_DV && (rep & kDdDirectFlag)) ? out.dd_dv + (rep & ~kDdDirectFlag) : out.rep_dv + rep;
  if (rep != 0xFFFFFFFFu) v = *src;
  return v;
}
// Every minimisation starts with the same abscissas: the upper bracket end 0.5, the golden-section point below
// it, and -- two coincident points make the parabolic step degenerate (p = q = 0 exactly) -- a second
// golden-section point that depends only on WHICH of the first two values is smaller.  kr_llh_pre_kernel
// evaluates the d-part of the objective at those four points ONCE per workgroup and combines it with every
// record's histogram (one log per evaluation instead of a full evaluation): 3 of the ~11.6 evaluations of a
// record leave the divergent main loop.  The three values travel in rec_d / rec_v / rec_chisq, which the later
// kernels overwrite with their results.
__device__ __forceinline__ void brent_shared_points(double& u1, double& u2a, double& u2b)
{
  BrentState s;
  double u = 0.0;
  brent_start(s, 0.5, 1.0);
  brent_next(s, u1); // golden section from the upper end: no objective value enters
  BrentState sa = s, sb = s;
  brent_update(sa, u1, 0.0); // f(u1) <= f(0.5)
  brent_next(sa, u2a);
  brent_update(sb, u1, 2.0); // f(u1) > f(0.5)
  brent_next(sb, u2b);
  (void)u;
}
template <int NPT>
__global__ __launch_bounds__(256) void kr_llh_pre_kernel(LlhConst C, DevIndex ix, BatchOut out)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes], s_g[4][3];
  LlhTables T{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, T.bk, T.hnk);
  double u1, u2a, u2b;
  brent_shared_points(u1, u2a, u2b);
  if (threadIdx.x < 4) {
    const double d = threadIdx.x == 0 ? 0.5 : (threadIdx.x == 1 ? u1 : (threadIdx.x == 2 ? u2a : u2b));
    const LlhShared g = llh_dpart<NPT>(C, T, d);
    s_g[threadIdx.x][0] = g.logdn, s_g[threadIdx.x][1] = g.logdp, s_g[threadIdx.x][2] = g.lv_m;
  }
  __syncthreads();
  const LlhShared g0{s_g[0][0], s_g[0][1], s_g[0][2]}, g1{s_g[1][0], s_g[1][1], s_g[1][2]};
  const uint32_t nrep = min(out.counters[kCtProblems], out.rep_cap); // (beyond the slice: the batch has been flagged, take_positions)
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nrep; j += gridDim.x * blockDim.x) {
    const uint32_t i = out.rep_list[j];
    if (i == 0xFFFFFFFFu) continue; // hole at the end of a wave's chunk of list positions
    const uint32_t key = out.rec_key[i];
    LlhProblem p;
    load_record<NPT>(C, out, i, ix.libs[0].rho[key >> 1], p);
    const double f0 = llh_combine<NPT>(C, g0, p), f1 = llh_combine<NPT>(C, g1, p);
    const int w = f1 <= f0 ? 2 : 3; // the branch brent_update takes
    const LlhShared g2{s_g[w][0], s_g[w][1], s_g[w][2]};
    out.rec_d[i] = f0;
    out.rec_v[i] = f1;
    out.rec_chisq[i] = llh_combine<NPT>(C, g2, p);
  }
}

// One record per lane, refilled: a lane whose minimisation has converged stores its result and, once
// kLlhRefill lanes are idle, the idle lanes take the next records of the wave's current chunk (chunks of
// kLlhChunk records are handed out through counters[kCtLlhCursor]) together with their first two objective values.
// Every step evaluates the objective once for all busy lanes.
#ifndef KR_LLH_REFILL
#define KR_LLH_REFILL 8
#endif
#ifndef KR_LLH_WPE
#define KR_LLH_WPE 4
#endif
constexpr uint32_t kLlhChunkMax = 2048, kLlhRefill = KR_LLH_REFILL;
template <int NPT>
__device__ __forceinline__ void llh_records(const LlhConst& C, const LlhTables& T, const DevIndex& ix, const BatchOut& out)
{
  const uint32_t nrec = min(out.counters[kCtProblems], out.rep_cap); // distinct problems (rep_list)
  const uint32_t lane = lane_id();
  const uint64_t lt = (1ull << lane) - 1ull;
  // chunk size: about four chunks per wave, 64 .. kLlhChunkMax records
  const uint32_t kLlhChunk = min(kLlhChunkMax, max(64u, (nrec / (gridDim.x * (blockDim.x / kWave) * 4u)) & ~63u));
  uint32_t next = 0, end = 0; // wave-uniform cursor into the current chunk
  bool more = true;           // wave-uniform: chunks may remain
  bool busy = false;
  uint32_t rec = 0, pos = 0;
  LlhProblem p;
  BrentState s;
  for (;;) {
    double u = 0.5;
    bool has_u = false;
    if (busy) {
      has_u = brent_next(s, u);
      if (!has_u) {
        out.rep_dv[pos] = make_double2(s.x, s.fx);
        busy = false;
      }
    }
    // ---- refill
    const uint64_t idle = __ballot(!busy);
    if (idle != 0 && (more || next < end) && ((uint32_t)__popcll(idle) >= kLlhRefill || idle == __ballot(true))) {
      if (next == end) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&out.counters[kCtLlhCursor], kLlhChunk);
        base = __shfl(base, 0);
        next = min(base, nrec);
        end = min(base + kLlhChunk, nrec);
        more = base + kLlhChunk < nrec;
      }
      const uint32_t mine = next + __popcll(idle & lt);
      if (!busy && mine < end) {
        pos = mine;
        rec = out.rep_list[mine];
        if (rec != 0xFFFFFFFFu) { // else: hole at the end of a wave's chunk of list positions
          const uint32_t key = out.rec_key[rec];
          load_record<NPT>(C, out, rec, ix.libs[0].rho[key >> 1], p);
          // the first three steps of the minimisation, with the objective values of kr_llh_pre_kernel
          const double f0 = out.rec_d[rec], f1 = out.rec_v[rec], f2 = out.rec_chisq[rec];
          brent_start(s, 0.5, f0);
          double u1 = 0.0, u2 = 0.0;
          brent_next(s, u1);
          brent_update(s, u1, f1);
          brent_next(s, u2);
          brent_update(s, u2, f2);
          has_u = brent_next(s, u);
          busy = has_u;
          if (!has_u) out.rep_dv[pos] = make_double2(s.x, s.fx); // converged at once (not with these brackets, but cheap to honour)
        }
      }
      next = min(end, next + (uint32_t)__popcll(idle));
    }
    if (__ballot(busy) == 0) {
      if (!more && next == end) break;
      continue;
    }
    // ---- one objective evaluation for every busy lane
    if (has_u) brent_update(s, u, llh_eval<NPT>(C, T, p, u));
  }
}

// NPT = 5: --hdist-th default, histogram in registers; NPT = 0: any threshold
template <int NPT>
__global__ __launch_bounds__(256, KR_LLH_WPE) void kr_llh_kernel(LlhConst C, DevIndex ix, BatchOut out)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables T{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, T.bk, T.hnk);
  llh_records<NPT>(C, T, ix, out);
}

// summarize_matches' strand merge and closest (src/query.cpp:96-139) + the row selection
// of report_distances (src/query.cpp:158-196).  Records of a read are sorted by
// key = (se << 1) | strand.  Iteration order of the reference's maps is arbitrary; the
// order used here (all forward leaves by ascending se, then all reverse ones) is the
// oracle's, so `<=` ties resolve identically.
// a wave per read, one record per lane (reads have tens of records; all record arrays are read
// coalesced).
// FILT: --filter (the chi-square needs an objective evaluation per record); without it the kernel carries no
// likelihood code and runs at full occupancy.
#ifndef KR_SELECT_GL
#define KR_SELECT_GL 64
#endif
// Cross-lane moves of the select kernels.  A read's closest record is an arg-min over the group's lanes and its strand merge looks at the
// records before and after: as __shfl_xor / __shfl_up / __shfl_down that was ~35 ds_bpermute a read (24 cycles each on the LDS pipe and a
// round trip of its own each time the result is waited for: scripts/calib_issue.hip).  On the DPP network: rotations within the 16-lane
// rows for the arg-min's first four steps (the permutes remain for the steps across rows), wave shifts by one lane for the neighbours.
#ifndef KR_SELECT_DPP
#define KR_SELECT_DPP 1
#endif
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v, uint32_t fill)
{ // lanes without a source lane keep `fill`
  return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v, double fill)
{
  const uint64_t b = (uint64_t)__double_as_longlong(v), f = (uint64_t)__double_as_longlong(fill);
  const uint32_t lo = dpp_u32<CTRL>((uint32_t)b, (uint32_t)f), hi = dpp_u32<CTRL>((uint32_t)(b >> 32), (uint32_t)(f >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138; // lane l takes lane l + 1 / l - 1 (across the rows)
// the record before / after this lane's in a group of GL lanes (the group's first / last lane: unspecified, as with __shfl_up / __shfl_down
// nobody looks at it)
template <uint32_t GL> __device__ __forceinline__ uint32_t lane_before(uint32_t v) { return KR_SELECT_DPP ? dpp_u32<kDppWaveShr1>(v, v) : (uint32_t)__shfl_up((int)v, 1, GL); }
template <uint32_t GL> __device__ __forceinline__ uint32_t lane_after(uint32_t v) { return KR_SELECT_DPP ? dpp_u32<kDppWaveShl1>(v, v) : (uint32_t)__shfl_down((int)v, 1, GL); }
template <uint32_t GL> __device__ __forceinline__ double lane_before(double v) { return KR_SELECT_DPP ? dpp_f64<kDppWaveShr1>(v, v) : __shfl_up(v, 1, GL); }
template <uint32_t GL> __device__ __forceinline__ double lane_after(double v) { return KR_SELECT_DPP ? dpp_f64<kDppWaveShl1>(v, v) : __shfl_down(v, 1, GL); }
// (smallest d, among equal d the largest ord) over the group's lanes, in every lane of the group; a lane without a candidate brings
// (+inf, 0).  The order is total, so the result does not depend on how the lanes are paired.
template <uint32_t GL>
__device__ __forceinline__ void group_closest(double& bd, uint32_t& bo)
{
#define KR_CL_STEP(OD, OO)                                             \
  {                                                                    \
    const double od_ = (OD);                                           \
    const uint32_t oo_ = (OO);                                         \
    if (od_ < bd || (od_ == bd && oo_ > bo)) bd = od_, bo = oo_;       \
  }
  if (KR_SELECT_DPP) { // row_ror:1, 2, 4, 8: every lane of a 16-lane row has the row's
    KR_CL_STEP(dpp_f64<0x121>(bd, bd), dpp_u32<0x121>(bo, bo))
    KR_CL_STEP(dpp_f64<0x122>(bd, bd), dpp_u32<0x122>(bo, bo))
    KR_CL_STEP(dpp_f64<0x124>(bd, bd), dpp_u32<0x124>(bo, bo))
    KR_CL_STEP(dpp_f64<0x128>(bd, bd), dpp_u32<0x128>(bo, bo))
  } else {
#pragma unroll
    for (int sft = 8; sft >= 1; sft >>= 1) KR_CL_STEP(__shfl_xor(bd, sft, GL), __shfl_xor(bo, sft, GL))
  }
  if (GL >= 32u) KR_CL_STEP(__shfl_xor(bd, 16, GL), __shfl_xor(bo, 16, GL))
  if (GL >= 64u) KR_CL_STEP(__shfl_xor(bd, 32, GL), __shfl_xor(bo, 32, GL))
#undef KR_CL_STEP
}
// One read (record slots [o, o + n)) by a group of GL lanes, lane gl of the group: closest, strand merge, row selection.
template <int NPT, bool FILT, uint32_t GL>
__device__ __forceinline__ void select_one_read(const LlhConst& C, const LlhTables& T, const DevIndex& ix, const DevParams& P, const BatchOut& out,
                                                uint32_t r, uint32_t o, uint32_t n, uint32_t gl)
{
  const double kMax = 1.7976931348623157e308;
  uint32_t rows_here = 0; // output rows among this lane's records
  const bool fast = n <= GL; // (uniform over the read's lanes)
  // ---- closest: last record in (strand, se) order with d <= best, i.e. the smallest d and among
  //      equal d the largest (strand, index)
  double bd = __builtin_inf(), d0 = 0, v0 = 0; // (no candidate yet: +inf, which every d <= kMax beats)
  uint32_t bo = 0, key0 = 0;
  for (uint32_t i = gl; i < n; i += GL) {
    // every record takes its value from the table of distinct problems (kr_dedup_kernel): rec_d / rec_v are written here
    const uint32_t rep = out.rec_rep[o + i];
    const uint32_t key = out.rec_key[o + i];
    const double2 dv = rep_value(out, rep);
    const double d = dv.x;
    out.rec_d[o + i] = d;
    if (out.rows_indexed) out.rec_rep[o + i] = rep_pos(out, rep); // (KR_ROWS_INDEXED: the resolved list position is the row's DIST column)
    if (FILT || out.keep_v) out.rec_v[o + i] = dv.y;
    if (i == gl) d0 = d, v0 = dv.y, key0 = key;
    const uint32_t ord = ((key & 1u) << 31) | i;
    if (d <= kMax && (d < bd || (d == bd && ord > bo))) bd = d, bo = ord;
  }
  group_closest<GL>(bd, bo);
  const bool any = bd <= kMax;
  const int cl = any ? (int)(o + (bo & 0x7FFFFFFFu)) : -1;
  const double best = any ? bd : kMax;
  const bool na = (n == 0) || (P.dmax_set && best > P.dist_max);
  if (gl == 0) out.rd_na[r] = na ? 1 : 0;
  LlhProblem pc;
  double vcl = 0;
  uint32_t kcl = 0;
  if (fast) {
    kcl = (uint32_t)__shfl((int)key0, (int)(bo & (GL - 1u)), GL); // (0 when the read has no record: unused then)
    vcl = __shfl(v0, (int)(bo & (GL - 1u)), GL);
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // rec_d / rec_v of this read, written by the other lanes of the group above
    if (cl >= 0) kcl = out.rec_key[cl];
    if (FILT && cl >= 0) vcl = out.rec_v[cl];
  }
  if (FILT && cl >= 0 && !P.no_filter) load_record<NPT>(C, out, (uint32_t)cl, ix.libs[0].rho[kcl >> 1], pc);
  if (fast) {
    // ---- one record per lane, all in registers
    const uint32_t i = o + gl, key = gl < n ? key0 : 0u;
    const uint32_t key_up = lane_before<GL>(key), key_dn = lane_after<GL>(key);
    const bool has_other = gl < n && ((key & 1u) ? (gl > 0 && key_up == (key ^ 1u)) : (gl + 1 < n && key_dn == (key ^ 1u)));
    const double d_up = lane_before<GL>(d0), d_dn = lane_after<GL>(d0);
    if (gl < n) {
      bool chosen = true;
      if (has_other) { // the pair: forward strand record io, reverse strand record ir = io + 1
        const uint32_t io = (key & 1u) ? i - 1 : i;
        const double d_or = (key & 1u) ? d_up : d0, d_rc = (key & 1u) ? d0 : d_dn;
        bool take_or = d_rc > d_or; // src/query.cpp:129-133: the larger distance loses, equal distances: the fewer matches
        if (d_rc == d_or) take_or = record_matches(C, out, io + 1) < record_matches(C, out, io); // (rare: looked up only here)
        if (cl >= 0 && (kcl >> 1) == (key >> 1)) take_or = ((uint32_t)cl == io); // the closest overrides (src/query.cpp:136-138)
        chosen = (key & 1u) ? !take_or : take_or;
      }
      double chi = nan("");
      bool sel = false;
      if (chosen && !na) {
        const bool dm = !P.dmax_set || d0 < P.dist_max;
        if (!P.multi) {
          sel = (int)i == cl;
        } else if (P.no_filter) {
          sel = dm;
        } else if (FILT) {
          chi = 2 * (llh_eval<NPT>(C, T, pc, d0) - vcl); // Minfo::likelihood_ratio (src/query.cpp:420-424)
          sel = (chi < P.chisq) && dm;
        }
      }
      out.rec_sel[i] = sel ? 1 : 0;
      if (FILT) out.rec_chisq[i] = chi; // (without --filter nobody reads it: the host view is filled with NaN on the host)
      rows_here = sel ? 1u : 0u;
    }
    if (out.rows_mode) { // the read's rows (the group's lanes hold one record each)
      const uint64_t sm = __ballot(rows_here != 0u);
      const uint32_t g0 = lane_id() & ~(GL - 1u);
      if (gl == 0) out.rd_rcnt[r] = (uint32_t)__popcll(GL == 64u ? sm : ((sm >> g0) & ((1ull << (GL & 63u)) - 1ull)));
    }
    return;
  }
  for (uint32_t t = gl; t < n; t += GL) {
    const uint32_t i = o + t;
    const uint32_t key = out.rec_key[i];
    // which record represents this leaf in node_to_minfo?
    bool chosen;
    const bool has_other = (key & 1u) ? (t > 0 && out.rec_key[i - 1] == (key ^ 1u)) : (t + 1 < n && out.rec_key[i + 1] == (key ^ 1u));
    if (!has_other) {
      chosen = true;
    } else {
      const uint32_t io = (key & 1u) ? i - 1 : i, ir = (key & 1u) ? i : i + 1;
      const double d_or = out.rec_d[io], d_rc = out.rec_d[ir];
      bool take_or = d_rc > d_or; // src/query.cpp:129-133
      if (d_rc == d_or) take_or = record_matches(C, out, ir) < record_matches(C, out, io);
      // the closest overrides (src/query.cpp:136-138)
      if (cl >= 0 && (kcl >> 1) == (key >> 1)) take_or = ((uint32_t)cl == io);
      chosen = (key & 1u) ? !take_or : take_or;
    }
    const double d = out.rec_d[i];
    double chi = nan("");
    bool sel = false;
    if (chosen && !na) {
      const bool dm = !P.dmax_set || d < P.dist_max;
      if (!P.multi) {
        sel = (int)i == cl;
      } else if (P.no_filter) {
        sel = dm;
      } else if (FILT) {
        chi = 2 * (llh_eval<NPT>(C, T, pc, d) - vcl); // Minfo::likelihood_ratio (src/query.cpp:420-424)
        sel = (chi < P.chisq) && dm;
      }
    }
    out.rec_sel[i] = sel ? 1 : 0;
    if (FILT) out.rec_chisq[i] = chi;
    rows_here += sel ? 1u : 0u;
  }
  if (out.rows_mode) {
#pragma unroll
    for (int sft = GL / 2; sft >= 1; sft >>= 1) rows_here += (uint32_t)__shfl_xor((int)rows_here, sft, GL);
    if (gl == 0) out.rd_rcnt[r] = rows_here;
  }
}

template <int NPT, bool FILT>
__global__ __launch_bounds__(256) void kr_select_kernel(LlhConst C, DevIndex ix, DevParams P, BatchOut out,
                                                        uint32_t nreads)
{
  if (!FILT) P.no_filter = 1;
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables T{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, T.bk, T.hnk);
  constexpr uint32_t GL = KR_SELECT_GL, GPB = 256 / GL; // lanes per read, reads per workgroup pass
  const uint32_t gl = threadIdx.x & (GL - 1u);
  // The kernel is bound by its chain of dependent loads (read -> records -> closest -> neighbours), not by bytes: the next
  // read's range is fetched one iteration ahead, and a read of at most GL records (nearly all) keeps its records in
  // registers -- the closest's key and the other strand's record come by lane shuffle instead of a second round of loads.
  const uint32_t r_first = blockIdx.x * GPB + threadIdx.x / GL, r_step = gridDim.x * GPB;
  uint32_t o_nx = 0, n_nx = 0;
  if (r_first < nreads) o_nx = out.rd_off[r_first], n_nx = out.rd_cnt[r_first];
  for (uint32_t r = r_first; r < nreads; r += r_step) {
    const uint32_t o = o_nx, n = n_nx;
    if (r + r_step < nreads) o_nx = out.rd_off[r + r_step], n_nx = out.rd_cnt[r + r_step];
    select_one_read<NPT, FILT, GL>(C, T, ix, P, out, r, o, n, gl);
  }
}

// A read of more than 64 records by a whole wave, without --filter.  Two thirds of a batch's records belong to such reads (one read
// in eight; `scripts/records_per_read_hist.py`), and select_one_read walks them 64 records at a time with three dependent round trips
// a step (record -> list position -> value) and four more loads per record pair in its second loop: the select kernel's time was
// mostly these chains.  Here four steps' loads leave together in the first loop, two in the second, and the pair's match counts are
// looked at only where the two distances are equal (src/query.cpp:129-133).  Same results as select_one_read<NPT, false, 64>.
#ifndef KR_SELECT_BIG
#define KR_SELECT_BIG 1
#endif
__device__ __forceinline__ void select_big_read(const LlhConst& C, const DevParams& P, const BatchOut& out, uint32_t r, uint32_t o, uint32_t n, uint32_t lane)
{
  const double kMax = 1.7976931348623157e308;
  double bd = __builtin_inf();
  uint32_t bo = 0, rows = 0;
  // one pair of the strand merge + the row selection (src/query.cpp:127-138,158-196) for record t of the read
  auto choose = [&](uint32_t t, uint32_t key, uint32_t key_b, uint32_t key_n, double d_c, double d_b, double d_n, bool any, uint32_t clt, uint32_t kcl,
                    bool na) -> bool {
    const bool has_other = (key & 1u) ? (t > 0 && key_b == (key ^ 1u)) : (t + 1 < n && key_n == (key ^ 1u));
    bool chosen = true;
    if (has_other) { // the pair: forward strand record io, reverse strand record io + 1
      const uint32_t io = (key & 1u) ? t - 1 : t;
      const double d_or = (key & 1u) ? d_b : d_c, d_rc = (key & 1u) ? d_c : d_n;
      bool take_or = d_rc > d_or; // src/query.cpp:129-133
      if (d_rc == d_or) take_or = record_matches(C, out, o + io + 1) < record_matches(C, out, o + io);
      if (any && (kcl >> 1) == (key >> 1)) take_or = (clt == io); // the closest overrides (src/query.cpp:136-138)
      chosen = (key & 1u) ? !take_or : take_or;
    }
    bool sel = false;
    if (chosen && !na) sel = !P.multi ? (t == clt) : (!P.dmax_set || d_c < P.dist_max);
    return sel;
  };
  if (n <= 256u) {
    // ---- at most four records a lane: everything stays in registers, one chain of two look-ups for the whole read
    uint32_t pos[4], key[4];
    double2 dv[4];
    double d[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t i = 64u * q + lane;
      pos[q] = 0xFFFFFFFFu, key[q] = 0;
      if (i < n) pos[q] = out.rec_rep[o + i], key[q] = out.rec_key[o + i];
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) dv[q] = rep_value(out, pos[q]);
    if (out.rows_indexed) {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) pos[q] = rep_pos(out, pos[q]);
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t i = 64u * q + lane;
      d[q] = 0;
      if (i < n) {
        d[q] = dv[q].x;
        out.rec_d[o + i] = d[q];
        if (out.rows_indexed) out.rec_rep[o + i] = pos[q];
        if (out.keep_v) out.rec_v[o + i] = dv[q].y;
        const uint32_t ord = ((key[q] & 1u) << 31) | i;
        if (d[q] <= kMax && (d[q] < bd || (d[q] == bd && ord > bo))) bd = d[q], bo = ord;
      }
    }
    group_closest<64u>(bd, bo);
    const bool any = bd <= kMax;
    const uint32_t clt = any ? (bo & 0x7FFFFFFFu) : 0xFFFFFFFFu; // the closest's index within the read
    const bool na = P.dmax_set && (any ? bd : kMax) > P.dist_max;
    uint32_t kq = key[0];
    if ((clt >> 6) == 1u) kq = key[1];
    if ((clt >> 6) == 2u) kq = key[2];
    if ((clt >> 6) == 3u) kq = key[3];
    const uint32_t kcl = any ? (uint32_t)__shfl((int)kq, (int)(clt & 63u)) : 0u;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      // the records before and after: the neighbouring lanes', at the wave's ends the last lane of the step before / the first of the step after
      const uint32_t kb_e = q ? (uint32_t)__builtin_amdgcn_readlane((int)key[q ? q - 1 : 0], 63) : 0u;
      const uint32_t kn_e = q < 3 ? (uint32_t)__builtin_amdgcn_readlane((int)key[q < 3 ? q + 1 : 3], 0) : 0u;
      const uint64_t dq = (uint64_t)__double_as_longlong(d[q]);
      const uint64_t db_b = q ? (uint64_t)__double_as_longlong(d[q ? q - 1 : 0]) : 0ull, dn_b = q < 3 ? (uint64_t)__double_as_longlong(d[q < 3 ? q + 1 : 3]) : 0ull;
      const uint32_t db_lo = q ? (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)db_b, 63) : 0u, db_hi = q ? (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(db_b >> 32), 63) : 0u;
      const uint32_t dn_lo = q < 3 ? (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)dn_b, 0) : 0u, dn_hi = q < 3 ? (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(dn_b >> 32), 0) : 0u;
      const uint32_t key_b = dpp_u32<kDppWaveShr1>(key[q], kb_e), key_n = dpp_u32<kDppWaveShl1>(key[q], kn_e);
      const uint32_t b_lo = dpp_u32<kDppWaveShr1>((uint32_t)dq, db_lo), b_hi = dpp_u32<kDppWaveShr1>((uint32_t)(dq >> 32), db_hi);
      const uint32_t n_lo = dpp_u32<kDppWaveShl1>((uint32_t)dq, dn_lo), n_hi = dpp_u32<kDppWaveShl1>((uint32_t)(dq >> 32), dn_hi);
      const double d_b = __longlong_as_double((long long)(((uint64_t)b_hi << 32) | b_lo)), d_n = __longlong_as_double((long long)(((uint64_t)n_hi << 32) | n_lo));
      const uint32_t t = 64u * q + lane;
      bool sel = false;
      if (t < n) {
        sel = choose(t, key[q], key_b, key_n, d[q], d_b, d_n, any, clt, kcl, na);
        out.rec_sel[o + t] = sel ? 1 : 0;
      }
      rows += (uint32_t)__popcll(__ballot(sel));
    }
    if (lane == 0) out.rd_na[r] = na ? 1 : 0;
    if (out.rows_mode && lane == 0) out.rd_rcnt[r] = rows;
    return;
  }
  for (uint32_t i0 = 0; i0 < n; i0 += 256u) { // (wave-uniform)
    uint32_t pos[4], key[4];
    double2 dv[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t i = i0 + 64u * q + lane;
      pos[q] = 0xFFFFFFFFu, key[q] = 0;
      if (i < n) pos[q] = out.rec_rep[o + i], key[q] = out.rec_key[o + i];
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) dv[q] = rep_value(out, pos[q]);
    if (out.rows_indexed) {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) pos[q] = rep_pos(out, pos[q]);
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t i = i0 + 64u * q + lane;
      if (i < n) {
        const double d = dv[q].x;
        out.rec_d[o + i] = d;
        if (out.rows_indexed) out.rec_rep[o + i] = pos[q];
        if (out.keep_v) out.rec_v[o + i] = dv[q].y;
        const uint32_t ord = ((key[q] & 1u) << 31) | i;
        if (d <= kMax && (d < bd || (d == bd && ord > bo))) bd = d, bo = ord;
      }
    }
  }
  group_closest<64u>(bd, bo);
  const bool any = bd <= kMax;
  const uint32_t clt = any ? (bo & 0x7FFFFFFFu) : 0xFFFFFFFFu;
  const bool na = P.dmax_set && (any ? bd : kMax) > P.dist_max;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // rec_d of this read, written by the other lanes above
  const uint32_t kcl = any ? out.rec_key[o + clt] : 0u;
  for (uint32_t t0 = 0; t0 < n; t0 += 128u) {
    uint32_t kc[2], kb[2], kn[2];
    double dc[2], db[2], dn[2];
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint32_t t = t0 + 64u * q + lane;
      kc[q] = kb[q] = kn[q] = 0, dc[q] = db[q] = dn[q] = 0;
      if (t < n) {
        kc[q] = out.rec_key[o + t], dc[q] = out.rec_d[o + t];
        if (t > 0) kb[q] = out.rec_key[o + t - 1], db[q] = out.rec_d[o + t - 1];
        if (t + 1 < n) kn[q] = out.rec_key[o + t + 1], dn[q] = out.rec_d[o + t + 1];
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint32_t t = t0 + 64u * q + lane;
      bool sel = false;
      if (t < n) {
        sel = choose(t, kc[q], kb[q], kn[q], dc[q], db[q], dn[q], any, clt, kcl, na);
        out.rec_sel[o + t] = sel ? 1 : 0;
      }
      rows += (uint32_t)__popcll(__ballot(sel));
    }
  }
  if (lane == 0) out.rd_na[r] = na ? 1 : 0;
  if (out.rows_mode && lane == 0) out.rd_rcnt[r] = rows;
}

// The same selection with a LANE per read (the default path, no --filter): kr_select_kernel gives a read a whole wave, and a read
// has 4 records on average -- 94 % of every instruction's lanes idle in a step that is bound by instruction issue like the rest
// of the path.  Here every lane walks its own read's records (two short loops: closest, then strand merge + selection; the
// neighbours it needs are the records before and after in the same walk); the wave iterates as long as its longest read, so
// reads of more than kSelectLaneMax records are left out of the walk and done afterwards, one at a time, by the whole wave
// (select_one_read).  Same results bit for bit: the closest is the last record in (strand, index) order among those of
// minimal d (src/query.cpp:110,123), the strand merge and the override are src/query.cpp:127-138, the rows src/query.cpp:158-196.
#ifndef KR_SELECT_LANE_MAX
#define KR_SELECT_LANE_MAX 8 // (measured on the 10 GB index, 33 records per read on average: 0 -> 5.8 ms, 8 -> 4.8, 24 -> 5.0, 48 -> 6.1; the wave-per-read kernel 5.3)
#endif
constexpr uint32_t kSelectLaneMax = KR_SELECT_LANE_MAX;
#ifndef KR_SELECT_WPE
#define KR_SELECT_WPE 6 // resident waves per SIMD the registers are allotted for (80; the code takes 84 = five waves when left alone: 8.32 -> 8.08 ms for the
                        // stage, 13.78 -> 13.32 on the 10,000-genome index; eight waves spill: 8.70)
#endif
template <int NPT>
__global__ __launch_bounds__(256, KR_SELECT_WPE) void kr_select_lane_kernel(LlhConst C, DevIndex ix, DevParams P, BatchOut out, uint32_t nreads)
{
  P.no_filter = 1;
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables T{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, T.bk, T.hnk); // (only select_one_read<FILT> evaluates anything: kept for its signature)
  const double kMax = 1.7976931348623157e308;
  const uint32_t lane = lane_id();
  for (uint32_t r0 = blockIdx.x * 256u + (threadIdx.x & ~63u); r0 < nreads; r0 += gridDim.x * 256u) { // wave-uniform
    const uint32_t r = r0 + lane;
    const bool on = r < nreads;
    const uint32_t o = on ? out.rd_off[r] : 0u, n = on ? out.rd_cnt[r] : 0u;
    const bool big = n > kSelectLaneMax;
#ifndef KR_SELECT_SKIP
#define KR_SELECT_SKIP 0 // (timing experiments, wrong results: 1 leaves out the lanes' own walks, 2 / 4 the groups of 16 / 32 lanes, 8 the reads of 33..64 records, 16 the larger ones)
#endif
    const uint32_t nl = (big || (KR_SELECT_SKIP & 1)) ? 0u : n; // records this lane walks itself
    // ---- every record takes its value from the table of distinct problems (kr_dedup_kernel); closest = smallest d, among equal
    //      d the largest (strand, index).  Four records per step: their loads leave together, then their gathers (the walk is a
    //      chain of dependent round trips, and one record per step left a wave waiting for ~70 of them).
    double bd = kMax;
    uint32_t bo = 0, kcl = 0;
    bool any = false;
    for (uint32_t i0 = 0; __ballot(i0 < nl) != 0; i0 += 4) {
      uint32_t pos[4], key[4];
      double2 dv[4];
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        pos[q] = 0xFFFFFFFFu, key[q] = 0;
        if (i0 + q < nl) pos[q] = out.rec_rep[o + i0 + q], key[q] = out.rec_key[o + i0 + q];
      }
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) dv[q] = rep_value(out, pos[q]); // (the four look-ups leave together)
      if (out.rows_indexed) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) pos[q] = rep_pos(out, pos[q]);
      }
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
        if (i0 + q < nl) {
          const double d = dv[q].x;
          out.rec_d[o + i0 + q] = d;
          if (out.rows_indexed) out.rec_rep[o + i0 + q] = pos[q]; // (KR_ROWS_INDEXED: see select_one_read)
          if (out.keep_v) out.rec_v[o + i0 + q] = dv[q].y;
          const uint32_t ord = ((key[q] & 1u) << 31) | (i0 + q);
          if (d <= kMax && (!any || d < bd || (d == bd && ord > bo))) bd = d, bo = ord, any = true, kcl = key[q];
        }
    }
    const int cl = any ? (int)(bo & 0x7FFFFFFFu) : -1; // (index within the read)
    const bool na = (n == 0) || (P.dmax_set && bd > P.dist_max);
    if (on && !big) out.rd_na[r] = na ? 1 : 0;
    // ---- strand merge + selection: records are sorted by key = se << 1 | strand, the two strands of a leaf adjacent.  Four
    //      records per step plus the one behind them (the last record's possible partner); the one in front is carried over.
    uint32_t key_p = 0, nrow = 0;
    double d_p = 0;
    for (uint32_t t0 = 0; __ballot(t0 < nl) != 0; t0 += 4) {
      uint32_t kk[5];
      double dd[5];
#pragma unroll
      for (uint32_t q = 0; q < 5; ++q) {
        kk[q] = 0, dd[q] = 0;
        if (t0 + q < nl) kk[q] = out.rec_key[o + t0 + q], dd[q] = out.rec_d[o + t0 + q];
      }
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t t = t0 + q;
        if (t < nl) {
          const uint32_t key_c = kk[q], key_b = q ? kk[q - 1] : key_p, key_n = kk[q + 1];
          const double d_c = dd[q], d_b = q ? dd[q - 1] : d_p, d_n = dd[q + 1];
          const bool has_other = (key_c & 1u) ? (t > 0 && key_b == (key_c ^ 1u)) : (t + 1 < nl && key_n == (key_c ^ 1u));
          bool chosen = true;
          if (has_other) { // the pair: forward strand record io, reverse strand record io + 1
            const uint32_t io = (key_c & 1u) ? t - 1 : t;
            const double d_or = (key_c & 1u) ? d_b : d_c, d_rc = (key_c & 1u) ? d_c : d_n;
            bool take_or = d_rc > d_or; // src/query.cpp:129-133
            if (d_rc == d_or) take_or = record_matches(C, out, o + io + 1) < record_matches(C, out, o + io);
            if (cl >= 0 && (kcl >> 1) == (key_c >> 1)) take_or = ((uint32_t)cl == io); // the closest overrides (src/query.cpp:136-138)
            chosen = (key_c & 1u) ? !take_or : take_or;
          }
          bool sel = false;
          if (chosen && !na) sel = !P.multi ? ((int)t == cl) : (!P.dmax_set || d_c < P.dist_max);
          out.rec_sel[o + t] = sel ? 1 : 0;
          nrow += sel ? 1u : 0u;
        }
      }
      key_p = kk[3], d_p = dd[3];
    }
    if (out.rows_mode && on && !big) out.rd_rcnt[r] = nrow;
    // ---- the reads left out, by groups of lanes: four reads of at most 16 records at a time (a quarter of the wave each), two of at
    //      most 32, the whole wave for a larger one.  A read is a chain of three dependent round trips (records -> list positions ->
    //      values) and a handful of shuffles: one read at a time left the wave waiting on 33 lanes' worth of loads (round 5:
    //      KR_SELECT_GROUPS=0 compiles the one-at-a-time form)
#ifndef KR_SELECT_GROUPS
#define KR_SELECT_GROUPS 1
#endif
    uint64_t bm = __ballot(on && big);
    if (KR_SELECT_GROUPS) {
      uint64_t b16 = __ballot(on && big && n <= 16u), b32 = __ballot(on && big && n > 16u && n <= 32u);
      bm &= ~(b16 | b32);
      if (KR_SELECT_SKIP & 2) b16 = 0;
      if (KR_SELECT_SKIP & 4) b32 = 0;
      while (b16 != 0) { // lanes 16 g .. 16 g + 15 take the g-th of the next four
        int l = -1;
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g) {
          const int lg = b16 ? __ffsll((long long)b16) - 1 : -1;
          if (b16) b16 &= b16 - 1;
          if ((lane >> 4) == g) l = lg;
        }
        const int src = l < 0 ? 0 : l;
        const uint32_t ro = (uint32_t)__shfl((int)o, src), rn = (uint32_t)__shfl((int)n, src);
        if (l >= 0) select_one_read<NPT, false, 16u>(C, T, ix, P, out, r0 + (uint32_t)l, ro, rn, lane & 15u);
      }
      while (b32 != 0) {
        int l = -1;
#pragma unroll
        for (uint32_t g = 0; g < 2; ++g) {
          const int lg = b32 ? __ffsll((long long)b32) - 1 : -1;
          if (b32) b32 &= b32 - 1;
          if ((lane >> 5) == g) l = lg;
        }
        const int src = l < 0 ? 0 : l;
        const uint32_t ro = (uint32_t)__shfl((int)o, src), rn = (uint32_t)__shfl((int)n, src);
        if (l >= 0) select_one_read<NPT, false, 32u>(C, T, ix, P, out, r0 + (uint32_t)l, ro, rn, lane & 31u);
      }
    }
    while (bm != 0) {
      const int l = __ffsll((long long)bm) - 1;
      bm &= bm - 1;
      const uint32_t ro = (uint32_t)__shfl((int)o, l), rn = (uint32_t)__shfl((int)n, l);
      if ((KR_SELECT_SKIP & 8) && rn <= 64u) continue;
      if ((KR_SELECT_SKIP & 16) && rn > 64u) continue;
      if (KR_SELECT_BIG && rn > 64u)
        select_big_read(C, P, out, r0 + (uint32_t)l, ro, rn, lane);
      else
        select_one_read<NPT, false, 64u>(C, T, ix, P, out, r0 + (uint32_t)l, ro, rn, lane);
    }
  }
}

// ---------------------------------------------------------------------------
// Rows-only batches: the output rows compacted on the device.  The report needs (reference, DIST) of the selected records of every
// read (src/query.cpp:158-196) -- 12 bytes a row; the record arrays hold every (read, strand, leaf) accumulator that passed the
// hdist_filt test, with a selection byte, in slots handed out to waves in chunks (holes): 13 bytes per SLOT crossed PCIe, and the
// copy back was the longest leg of a host batch (3.9 GB per 8 M reads at 48 GB/s beside the copy in: 81 ms against 74 ms of kernels).
//   kr_rows_bsum_kernel   rows per block of kRowBlock reads (the select kernels counted every read's rows)
//   kr_rows_bscan_kernel  the blocks' first rows (one workgroup), the batch's row count
//   kr_rows_write_kernel  a block's reads: their first rows (LDS scan), then a wave per read packs the selected (key, DIST) pairs
// ---------------------------------------------------------------------------
constexpr uint32_t kRowBlock = 1024;
__global__ __launch_bounds__(256) void kr_rows_bsum_kernel(BatchOut out, uint32_t nreads)
{
  for (uint32_t b = blockIdx.x; b * kRowBlock < nreads; b += gridDim.x) {
    uint32_t c = 0;
    for (uint32_t q = threadIdx.x; q < kRowBlock; q += 256u) {
      const uint32_t r = b * kRowBlock + q;
      if (r < nreads) c += out.rd_rcnt[r];
    }
    const uint32_t tot = block_sum(c);
    if (threadIdx.x == 0) out.row_bsum[b] = tot;
  }
}
__global__ __launch_bounds__(1024) void kr_rows_bscan_kernel(BatchOut out, uint32_t nreads)
{ // one workgroup: exclusive prefix of row_bsum in place, the total into counters[kCtRows]
  const uint32_t rows = scan_block_sums(out.row_bsum, (nreads + kRowBlock - 1u) / kRowBlock);
  if (threadIdx.x == 0) out.counters[kCtRows] = rows;
}
// INDEXED (KR_ROWS_INDEXED): the row's DIST as the position of its problem in the batch's list of distinct problems
// (kr_rows_dlist_kernel makes that list dense: dist_list[pos] = rep_dv[pos].x)
__global__ __launch_bounds__(256) void kr_rows_dlist_kernel(BatchOut out)
{
  const uint32_t n = min(out.counters[kCtProblems], out.dist_cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out.dist_list[i] = out.rep_dv[i].x;
}
template <bool INDEXED>
__global__ __launch_bounds__(256) void kr_rows_write_kernel(BatchOut out, uint32_t nreads)
{
  __shared__ uint32_t s_off[kRowBlock];
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  for (uint32_t b = blockIdx.x; b * kRowBlock < nreads; b += gridDim.x) {
    // ---- first row of every read of the block: thread t owns the reads 4t .. 4t+3
    const uint32_t rb = b * kRowBlock, q0 = 4u * threadIdx.x;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      c[q] = rb + q0 + q < nreads ? out.rd_rcnt[rb + q0 + q] : 0u;
      tot += c[q];
    }
    uint32_t run = out.row_bsum[b] + block_scan_excl(tot);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      s_off[q0 + q] = run;
      if (rb + q0 + q < nreads) out.rd_roff[rb + q0 + q] = run;
      run += c[q];
    }
    __syncthreads();
    // ---- a wave per read: the selected records' (key, DIST), in record order.  Round 6: FOUR reads of the wave at a time -- a read is
    //      a chain of three dependent round trips (its range -> its records -> the stores) and one at a time left the kernel waiting
    //      for them (3.7 ms per 8 M reads); the ranges of four reads leave together, then the first 64 records of each (nearly
    //      every read has no more), then the stores
    constexpr uint32_t U = 4;
    for (uint32_t qa = w; qa < kRowBlock && rb + qa < nreads; qa += 4u * U) {
      uint32_t o[U], n[U], ky[U], xr[U];
      double xd[U];
      uint8_t sl[U];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint32_t q = qa + 4u * u;
        const bool there = q < kRowBlock && rb + q < nreads;
        o[u] = there ? out.rd_off[rb + q] : 0u, n[u] = there ? out.rd_cnt[rb + q] : 0u;
      }
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const bool on = lane < n[u];
        sl[u] = on ? out.rec_sel[o[u] + lane] : (uint8_t)0;
        ky[u] = on ? out.rec_key[o[u] + lane] : 0u;
        xr[u] = 0u, xd[u] = 0.0;
        if (INDEXED)
          xr[u] = on ? out.rec_rep[o[u] + lane] : 0u; // (the select kernels left the resolved list position there; a selected record has one)
        else
          xd[u] = on ? out.rec_d[o[u] + lane] : 0.0;
      }
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint32_t q = qa + 4u * u;
        if (n[u] == 0) continue; // (wave-uniform)
        uint32_t pos = s_off[q];
        {
          const bool sel = sl[u] != 0;
          const uint64_t sm = __ballot(sel);
          if (sel) {
            const uint32_t at = pos + (uint32_t)__popcll(sm & lt);
            out.row_key[at] = ky[u];
            if (INDEXED)
              out.row_dix[at] = xr[u];
            else
              out.row_d[at] = xd[u];
          }
          pos += (uint32_t)__popcll(sm);
        }
        for (uint32_t i0 = 64u; i0 < n[u]; i0 += 64u) { // (a read of more than 64 records)
          const uint32_t i = i0 + lane;
          const bool sel = i < n[u] && out.rec_sel[o[u] + i] != 0;
          const uint64_t sm = __ballot(sel);
          if (sel) {
            const uint32_t at = pos + (uint32_t)__popcll(sm & lt);
            out.row_key[at] = out.rec_key[o[u] + i];
            if (INDEXED)
              out.row_dix[at] = out.rec_rep[o[u] + i];
            else
              out.row_d[at] = out.rec_d[o[u] + i];
          }
          pos += (uint32_t)__popcll(sm);
        }
      }
    }
    __syncthreads();
  }
}

// One bit per row of a sparse table: the bucket is not empty (see fetch_group).
__global__ void kr_build_occ(const uint64_t* bkt, uint32_t nrows, uint32_t* occ)
{
  const uint32_t nw = (nrows + 31u) / 32u;
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += gridDim.x * blockDim.x) {
    uint32_t bits = 0;
    for (uint32_t j = 0; j < 32u; ++j) {
      const uint32_t r = w * 32u + j;
      if (r < nrows && (bkt[r] & 0xFFFFFFull) != 0) bits |= 1u << j;
    }
    occ[w] = bits;
  }
}

// Slotted copy of the head of every bucket: slot r = {len, start, enc[start .. start + W - 2)}, unused words 0xFFFFFFFF.
// One thread per slot word: reads are contiguous within a bucket, writes fully coalesced.
__global__ void kr_build_slots(const uint64_t* bkt, const uint32_t* enc, uint32_t nrows, uint32_t words, uint32_t* slots)
{
  const uint64_t n = (uint64_t)nrows * words;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t row = (uint32_t)(i / words), wd = (uint32_t)(i - (uint64_t)row * words);
    const uint64_t b = bkt[row];
    const uint64_t st = b >> 24;
    const uint32_t ln = (uint32_t)(b & 0xFFFFFFu);
    uint32_t x = 0xFFFFFFFFu;
    if (wd == 0)
      x = ln;
    else if (wd == 1)
      x = (uint32_t)st;
    else if (wd - 2u < ln)
      x = enc[st + wd - 2u];
    slots[i] = x;
  }
}

