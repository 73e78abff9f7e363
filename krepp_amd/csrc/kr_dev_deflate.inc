// kr_dev_deflate.inc -- part of kr_device.hip (device side): report text deflated into BGZF members where it was written
// (kr_batch_collect_text_bgzf, kr_debug_bgzf_deflate; kr_host_deflate.inc).  The kernels:
//   kr_bgzf_deflate_kernel   one wave per member of io.member_in text bytes (65,280 unless kr_stream_bgzf_member says otherwise), four
//                            waves a workgroup, the grid sized from the member count.
//                            The encoder is kr_deflate.h's deflate_member, the code the host runs serially, and gives the same bytes:
//                            a lane owns one position of every tile of 64 (lookup, verify, enter, its token's bits), the parse is the
//                            same walk in every lane; head table, match lengths and the bit window live in LDS (8.7 KB a wave: four
//                            workgroups a CU).  Member m goes to slot m (stride io.slot_stride), one lane writes its size.
//   kr_bgzf_deflate_dyn_kernel   the same launch at level 2 (kr_stream_bgzf_out_level): kr_deflate.h's deflate_member_dyn, the tokens
//                            of pass 1 in a global list (io.member_in a member), the codes built by lane 0 between the passes,
//                            a lane per token in pass 2; 10.1 KB of LDS a wave: three workgroups a CU
//   kr_huffman_lengths_kernel    (tests) the code-length builder alone, one wave
//   kr_bgzf_deflate_scan_kernel   ONE workgroup of 1024: the sizes become the members' positions (scan_block_sums, kr_dev_prefix.inc:
//                            a member is a "block"), the total behind them
//   kr_bgzf_deflate_copy_kernel   a workgroup per member: its slot's bytes to its position, in words aligned to the destination
//
// Bounds (the host sized the buffers, deflate_reserve): text[0 .. n); nmembers = ceil(n / member_in) slots of slot_stride =
// bgzf_slot_stride(member_in) bytes; off[nmembers + 1]; the output holds n + 31 * nmembers bytes; at level 2, nmembers * member_in
// tokens.  deflate_member (and _dyn) never reads outside its member's input nor writes outside [slot, slot + len + 31), whatever
// the bytes are, and len + 31 <= member_in + 31 < slot_stride <= kDefSlot.  The kernels keep scalars and statically sized LDS only
// (kDefMemberIn bounds the state whatever member_in is).
// Alignment of the input: a member starts at ANY byte (text + m * member_in with an odd member_in; a text that itself starts at an
// odd address: place's d_text + 2).  Every load of the input in deflate_member / _dyn, def_tile_parse and DefWaveT::crc goes through
// a const uint8_t* one byte at a time (def_hash assembles its word from four bytes); none is a cast to a wider type, so the
// compiler may merge them only into loads the hardware takes at any address.  The slots stay 32-byte aligned (the copy kernel
// reads them in words): slot_stride is a multiple of 32.

struct DeflateIO {
  const uint8_t* text;
  uint64_t n;
  uint32_t nmembers;
  uint8_t* slots;  // [nmembers][slot_stride]
  uint64_t* off;   // [nmembers + 1]: the members' sizes, then (scan) their positions and the total
  uint8_t* out;    // [n + 31 * nmembers]
  uint32_t member_in, slot_stride; // input bytes of a member (256 .. kDefMemberIn); bgzf_slot_stride(member_in)
};

// (a type per level: each kernel has lanes of its own, so that what the compiler makes of one does not depend on the other)
template <int LEVEL>
struct DefWaveT {
  uint32_t l, total;
  __device__ uint32_t lane() const { return l; }
  __device__ uint32_t nlanes() const { return 64; }
  __device__ void sync() const { WAVE_SYNC(); } // (what other lanes of this wave wrote is read behind this: InfWave::sync)
  __device__ void head_max(uint32_t* p, uint32_t v) const { __hip_atomic_fetch_max((lds_u32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ void or_bits(uint32_t* p, uint32_t v) const { lds_or((lds_u32*)p, v); }
  __device__ void add(uint32_t* p, uint32_t v) const { __hip_atomic_fetch_add((lds_u32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ void scan_begin() {}
  __device__ uint32_t scan_excl(uint32_t v) // every lane of the wave calls it once a tile
  {
    const uint32_t incl = wave_scan_incl(v);
    total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    return incl - v;
  }
  __device__ uint32_t scan_total() const { return total; }
  __device__ void token(uint32_t, uint32_t) const {}
  __device__ uint32_t crc(const uint32_t* tab, const uint8_t* p, uint32_t n) const // contiguous slices, the 64 registers combined by x^(8 n) mod P
  {
    uint32_t per, a, b;
    kr::crc_slice(n, 64u, l, &per, &a, &b);
    uint32_t part = kr::crc_raw(tab, 0u, p + a, b - a);
    uint32_t op = kr::crc_xpow8(per);
    for (uint32_t s = 1; s < 64; s <<= 1) {
      const uint32_t other = __shfl_down(part, s);
      part = kr::crc_mulmod(op, part) ^ other; // (only lanes that are multiples of 2 s hold a run's value; lane 0 is what counts)
      op = kr::crc_mulmod(op, op);
    }
    return ~(kr::crc_mulmod(kr::crc_xpow8(n), 0xFFFFFFFFu) ^ __shfl(part, 0));
  }
};
typedef DefWaveT<1> DefWave;

__global__ __launch_bounds__(256) void kr_bgzf_deflate_kernel(DeflateIO io)
{
  __shared__ kr::DefState state[4];
  __shared__ uint32_t crc_tab[256];
  crc_tab[threadIdx.x] = kr::crc_table_entry(threadIdx.x);
  __syncthreads(); // (the only workgroup barrier: every wave passes it before any leaves)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t m = blockIdx.x * 4u + wave;
  if (m >= io.nmembers) return;
  const uint64_t a = (uint64_t)m * io.member_in;
  const uint32_t len = (uint32_t)std::min<uint64_t>(io.n - a, io.member_in);
  DefWave L;
  L.l = lane, L.total = 0;
  const uint32_t size = kr::deflate_member(io.text + a, len, io.slots + (uint64_t)m * io.slot_stride, state[wave], crc_tab, L);
  if (lane == 0) io.off[m] = size;
}

// Level 2 (dynamic codes): the same launch; member m's tokens lie in tokens[m * member_in ..), written in pass 1 and read in
// pass 2 by the same wave (a wave's memory instructions execute in order: DefWave::sync).  10,128 bytes of LDS a wave.
__global__ __launch_bounds__(256) void kr_bgzf_deflate_dyn_kernel(DeflateIO io, uint32_t* tokens)
{
  __shared__ kr::DefDynState state[4];
  __shared__ uint32_t crc_tab[256];
  crc_tab[threadIdx.x] = kr::crc_table_entry(threadIdx.x);
  __syncthreads(); // (the only workgroup barrier: every wave passes it before any leaves)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t m = blockIdx.x * 4u + wave;
  if (m >= io.nmembers) return;
  const uint64_t a = (uint64_t)m * io.member_in;
  const uint32_t len = (uint32_t)std::min<uint64_t>(io.n - a, io.member_in);
  DefWaveT<2> L;
  L.l = lane, L.total = 0;
  const uint32_t size = kr::deflate_member_dyn(io.text + a, len, io.slots + (uint64_t)m * io.slot_stride, tokens + (uint64_t)m * io.member_in,
                                               state[wave], crc_tab, L);
  if (lane == 0) io.off[m] = size;
}

// (tests) def_build_lengths as the level-2 kernel's lane 0 runs it: one wave, the counts and the scratch in LDS
__global__ __launch_bounds__(64) void kr_huffman_lengths_kernel(const uint32_t* freq, uint32_t nsym, uint32_t maxbits, uint8_t* lens, uint32_t* limited)
{
  __shared__ kr::DefBuild build;
  __shared__ uint32_t cnt[kr::kDefLL];
  __shared__ uint8_t out[kr::kDefLL];
  if (nsym > kr::kDefLL) return; // (the host checked)
  for (uint32_t i = threadIdx.x; i < nsym; i += 64u) cnt[i] = freq[i];
  WAVE_SYNC();
  if (threadIdx.x == 0) *limited = kr::def_build_lengths(cnt, nsym, maxbits, out, build) ? 1u : 0u;
  WAVE_SYNC();
  for (uint32_t i = threadIdx.x; i < nsym; i += 64u) lens[i] = out[i];
}

__global__ __launch_bounds__(1024) void kr_bgzf_deflate_scan_kernel(uint64_t* off, uint32_t nmembers)
{
  const uint64_t total = scan_block_sums<uint64_t>(off, nmembers);
  if (threadIdx.x == 0) off[nmembers] = total;
}

__global__ __launch_bounds__(256) void kr_bgzf_deflate_copy_kernel(DeflateIO io)
{
  const uint32_t m = blockIdx.x, t = threadIdx.x;
  if (m >= io.nmembers) return;
  const uint64_t a = io.off[m];
  const uint32_t sz = (uint32_t)(io.off[m + 1] - a);
  if (sz > io.slot_stride) return; // (cannot be: a member is at most member_in + 31 bytes)
  const uint8_t* src = io.slots + (uint64_t)m * io.slot_stride; // 32-byte aligned
  uint8_t* dst = io.out + a;
  const uint32_t head = std::min<uint32_t>(sz, (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u); // bytes in front of dst's first whole word
  if (t < head) dst[t] = src[t];
  const uint32_t nwords = (sz - head) >> 2, sh = 8u * (head & 3u);
  const uint32_t* srcw = (const uint32_t*)src;
  uint32_t* dstw = (uint32_t*)(dst + head);
  for (uint32_t w = t; w < nwords; w += 256u) { // dst word w = src bytes [head + 4 w, head + 4 w + 4), all below sz
    const uint32_t lo = srcw[w]; // (head < 4)
    // the second source word starts below sz whenever sh != 0: inside the slot
    dstw[w] = sh ? (lo >> sh) | (srcw[w + 1u] << (32u - sh)) : lo;
  }
  const uint32_t done = head + 4u * nwords;
  if (t < sz - done) dst[done + t] = src[done + t];
}
