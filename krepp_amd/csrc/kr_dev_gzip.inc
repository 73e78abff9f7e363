// kr_dev_gzip.inc -- part of kr_device.hip (device side): one SUPER-CHUNK of an ordinary gzip stream inflated by four kernels
// (kr_gzdev_read, kr_host_gzip.inc).  The stages are kr_inflate_sym.h's, the code the host runs serially (GzHostBackend):
//   kr_gz_search_kernel   a wave per sub-chunk, four a workgroup: lanes test 64 consecutive bit offsets against gz_candidate, the
//                         survivors are verified one at a time, lowest first, wave-uniformly (gz_verify_start writes only its LDS tables)
//   kr_gz_decode_kernel   a wave per sub-chunk: gz_decode_sub, every lane decoding the same symbols, 64 lanes moving a copy's elements
//   kr_gz_chain_kernel    ONE workgroup of 1,024 follows the links from sub-chunk 0: output offsets as a running sum, and the
//                         32 KB window in front of every chain chunk (32 K look-ups a step: all the serial work there is)
//   kr_gz_resolve_kernel  a workgroup per chain chunk: symbols to bytes at the chunk's offset, their CRC-32 by crc_slice
// No kernel waits for another wave's result: every dependency between sub-chunks crosses a kernel boundary.
//
// Bounds: a wave reads comp[0 .. ncomp) only (InfBits, gz_peek64: zeros behind the end), writes symbols only inside its slot
// [base(S_i), base(S_next)) with base(end) <= ratio * ncomp (gz_decode_sub's cap), and the chain and resolve kernels index by the
// lengths the decode kernel wrote (len <= cap) and by window symbols only behind gz_resolve_symbol's range check.

struct SymWave {
  uint32_t l, npend, mine;
  __device__ uint32_t lane() const { return l; }
  __device__ uint32_t nlanes() const { return 64; }
  __device__ void sync() const
  {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ void flush(uint16_t* out, uint32_t pos) // pos: behind the pending literals
  {
    if (npend == 0) return;
    if (l < npend) out[pos - npend + l] = (uint16_t)mine;
    npend = 0;
    sync();
  }
  __device__ void literal(uint16_t* out, uint32_t pos, uint32_t b)
  {
    if (l == npend) mine = b;
    if (++npend == 64) flush(out, pos + 1);
  }
};

__global__ __launch_bounds__(256) void kr_gz_search_kernel(kr::GzSuper G)
{
  __shared__ kr::InfTables tables[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * 4u + wave;
  if (i >= G.nsub) return; // (no workgroup barrier in this kernel)
  if (i == 0) {
    if (lane == 0) G.S[0] = G.pbit;
    return;
  }
  SymWave L;
  L.l = lane, L.npend = 0, L.mine = 0;
  uint32_t found = kr::kGzNone;
  const uint32_t lo = i * G.sub * 8u, hi = (i + 1 < G.nsub ? (i + 1) * G.sub : G.ncomp) * 8u;
  for (uint32_t at0 = lo; at0 < hi && found == kr::kGzNone; at0 += 64u) {
    const uint32_t at = at0 + lane;
    unsigned long long m = __ballot(at < hi && kr::gz_candidate(G.comp, G.ncomp, at));
    while (m) { // wave-uniform: the ballot is
      const uint32_t k = (uint32_t)__ffsll(m) - 1u;
      m &= m - 1ull;
      if (kr::gz_verify_start(G.comp, G.ncomp, at0 + k, tables[wave], L)) {
        found = at0 + k;
        break;
      }
    }
  }
  if (lane == 0) G.S[i] = found;
}

__global__ __launch_bounds__(256) void kr_gz_decode_kernel(kr::GzSuper G)
{
  __shared__ kr::InfTables tables[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * 4u + wave;
  if (i >= G.nsub) return;
  SymWave L;
  L.l = lane, L.npend = 0, L.mine = 0;
  kr::gz_decode_sub(G, i, tables[wave], L);
}

struct GzChainIO {
  kr::GzSuper G;
  uint8_t* win;    // [nsub + 1][kGzWin]: win[k] stands in front of chain chunk k; win[0] is the host's
  uint32_t wlen0;  // bytes of win[0] that exist (its last ones)
  uint32_t* chain; // [nsub] the chain's sub-chunks
  uint32_t* off;   // [nsub] output offset of chain chunk k
  uint32_t* wlen;  // [nsub] bytes of win[k] that exist
  uint32_t* crc;   // [nsub] per sub-chunk: CRC-32 of a chain chunk's bytes (0 elsewhere)
  uint8_t* out;    // [ratio * ncomp]
  kr::GzChainSum* sum;
};

__global__ __launch_bounds__(1024) void kr_gz_chain_kernel(GzChainIO io)
{
  __shared__ uint32_t s_bad;
  const kr::GzSuper& G = io.G;
  uint32_t c = 0, k = 0, wl = io.wlen0, end_bit = G.pbit, end_status = kr::GZ_IDLE, bad_at = kr::kGzNone;
  uint32_t off = 0;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  for (;;) { // links only lead forward (checked below): at most nsub steps.  Every thread reads the same values: uniform
    const uint32_t len = G.len[c], st = G.status[c], lk = G.link[c];
    const uint16_t* sym = G.sym + kr::gz_slot_base(G, G.S[c]);
    const uint8_t* w = io.win + (uint64_t)k * kr::kGzWin;
    uint8_t* nw = io.win + (uint64_t)(k + 1) * kr::kGzWin;
    uint32_t bad = 0;
    for (uint32_t t = threadIdx.x; t < kr::kGzWin; t += 1024u) nw[t] = kr::gz_chain_window(sym, len, w, wl, t, &bad);
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads(); // win[k + 1] is complete and visible to the workgroup
    const uint32_t is_bad = s_bad;
    __syncthreads(); // (every thread has read the flag before the next step may set it)
    if (is_bad) {    // a symbol in front of the member's first byte: the chain ends in front of this chunk
      bad_at = c, end_status = kr::GZ_BAD;
      break;
    }
    if (threadIdx.x == 0) io.chain[k] = c, io.off[k] = off, io.wlen[k] = wl;
    off += len, wl = wl + len < kr::kGzWin ? wl + len : kr::kGzWin;
    ++k;
    end_bit = G.end[c], end_status = st;
    if (st != kr::GZ_LINKED || lk <= c || lk >= G.nsub) break;
    c = lk;
  }
  if (threadIdx.x == 0) {
    io.sum->nchain = k, io.sum->end_bit = end_bit, io.sum->end_status = end_status, io.sum->bad_at = bad_at;
    io.sum->total = off;
  }
}

__global__ __launch_bounds__(256) void kr_gz_resolve_kernel(GzChainIO io)
{
  __shared__ uint32_t crc_tab[256];
  __shared__ uint32_t part4[4];
  const uint32_t k = blockIdx.x;
  if (k >= io.sum->nchain) return; // (uniform over the workgroup: the chain kernel has finished)
  crc_tab[threadIdx.x] = kr::crc_table_entry(threadIdx.x);
  const kr::GzSuper& G = io.G;
  const uint32_t c = io.chain[k], len = G.len[c], wl = io.wlen[k];
  const uint16_t* sym = G.sym + kr::gz_slot_base(G, G.S[c]);
  const uint8_t* w = io.win + (uint64_t)k * kr::kGzWin;
  uint8_t* out = io.out + io.off[k];
  uint32_t bad = 0;
  for (uint32_t i = threadIdx.x; i < len; i += 256u) out[i] = kr::gz_resolve_symbol(sym[i], w, wl, &bad);
  if (bad) atomicMin(&io.sum->bad_at, c);
  __syncthreads(); // the table, and the bytes other threads wrote
  uint32_t per, a, b;
  kr::crc_slice(len, 256u, threadIdx.x, &per, &a, &b);
  uint32_t part = kr::crc_raw(crc_tab, 0u, out + a, b - a);
  uint32_t op = kr::crc_xpow8(per);
  for (uint32_t s = 1; s < 64; s <<= 1) {
    const uint32_t other = __shfl_down(part, s);
    part = kr::crc_mulmod(op, part) ^ other; // (only lanes that are multiples of 2 s hold a run's value; lane 0 is what counts)
    op = kr::crc_mulmod(op, op);
  }
  if ((threadIdx.x & 63u) == 0) part4[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) { // op = x^(8 * 64 * per): what a wave's 64 slices do to the register in front of them
    uint32_t r = part4[0];
    for (uint32_t v = 1; v < 4; ++v) r = kr::crc_mulmod(op, r) ^ part4[v];
    io.crc[c] = ~(kr::crc_mulmod(kr::crc_xpow8(len), 0xFFFFFFFFu) ^ r);
  }
}
