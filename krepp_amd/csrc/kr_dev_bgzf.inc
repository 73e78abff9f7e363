// kr_dev_bgzf.inc -- part of kr_device.hip (device side): the members of a block-gzipped chunk inflated into the buffer the record
// finders read (kr_batch_submit_bgzf, kr_host_bgzf.inc).  One wave per member, four waves a workgroup, the grid sized from the
// member count.  The decoder is kr_inflate.h's inflate_member, the code the host runs serially: every lane decodes the same
// symbols from the same bit buffer (wave-uniform branches, tables in LDS: 3,648 bytes a wave), all 64 lanes move the bytes --
// pending literals, match copies, stored blocks -- and each takes a slice of the CRC.  A member's window is its own output in
// global memory, written and read back by this wave alone.
//
// Bounds (the host checked the table, bgzf_table): in_off + in_size <= ncomp; isize <= 65,536; a member with window == 0 has
// 0 <= out_pos and out_pos + isize <= nbytes; a member with window 1 / 2 is inflated into that 64 KB scratch window, then the bytes
// whose chunk position lies in [0, nbytes) are copied to raw.  inflate_member never reads outside its payload nor writes outside
// [out, out + isize), whatever the bytes are.

struct BgzfSum { // written by one lane per member
  uint32_t done, first_bad; // members finished; the first member that broke a rule (0xFFFFFFFF: none)
  unsigned long long bytes; // inflated bytes of the good members
};
struct BgzfIO {
  const uint8_t* comp;
  const kr::BgzfMember* tab;
  uint32_t nmembers;
  uint8_t* raw;     // the chunk: [nbytes]
  uint64_t nbytes;
  uint8_t* scratch; // [2][65536]
  uint32_t* status; // [nmembers]: 0, or rule << 24 | output position
  BgzfSum* sum;
};

struct InfWave {
  uint32_t l, npend;
  uint8_t mine;
  __device__ uint32_t lane() const { return l; }
  __device__ uint32_t nlanes() const { return 64; }
  // what other lanes of this wave wrote (LDS tables, the window in global memory) is read behind this: a wave's memory
  // instructions execute in order, the fences keep the compiler from moving them
  __device__ void sync() const
  {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ void flush(uint8_t* out, uint32_t pos) // pos: behind the pending literals
  {
    if (npend == 0) return;
    if (l < npend) out[pos - npend + l] = mine;
    npend = 0;
    sync();
  }
  __device__ void literal(uint8_t* out, uint32_t pos, uint8_t b)
  {
    if (l == npend) mine = b;
    if (++npend == 64) flush(out, pos + 1);
  }
};

__global__ __launch_bounds__(256) void kr_bgzf_inflate_kernel(BgzfIO io)
{
  __shared__ kr::InfTables tables[4];
  __shared__ uint32_t crc_tab[256];
  crc_tab[threadIdx.x] = kr::crc_table_entry(threadIdx.x);
  __syncthreads(); // (the only workgroup barrier: every wave passes it before any leaves)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t m = blockIdx.x * 4u + wave;
  if (m >= io.nmembers) return;
  const kr::BgzfMember e = io.tab[m];
  uint8_t* const win = e.window ? io.scratch + (uint64_t)(e.window - 1u) * kr::kBgzfMaxIsize : io.raw + e.out_pos;
  InfWave L;
  L.l = lane, L.npend = 0, L.mine = 0;
  uint32_t pos = 0;
  uint32_t rule = kr::inflate_member(io.comp + e.in_off, e.in_size, win, e.isize, tables[wave], L, &pos);
  if (!rule) { // CRC-32: contiguous slices, the 64 registers combined by x^(8 n) mod P
    uint32_t per, a, b;
    kr::crc_slice(e.isize, 64u, lane, &per, &a, &b);
    uint32_t part = kr::crc_raw(crc_tab, 0u, win + a, b - a);
    uint32_t op = kr::crc_xpow8(per);
    for (uint32_t s = 1; s < 64; s <<= 1) {
      const uint32_t other = __shfl_down(part, s);
      part = kr::crc_mulmod(op, part) ^ other; // (only lanes that are multiples of 2 s hold a run's value; lane 0 is what counts)
      op = kr::crc_mulmod(op, op);
    }
    const uint32_t crc = ~(kr::crc_mulmod(kr::crc_xpow8(e.isize), 0xFFFFFFFFu) ^ __shfl(part, 0));
    if (crc != e.crc) rule = kr::INF_CRC;
  }
  if (!rule && e.window) { // the part of a boundary member that belongs to this chunk
    const int64_t lo = e.out_pos < 0 ? -e.out_pos : 0;
    const int64_t hi = std::min<int64_t>((int64_t)e.isize, (int64_t)io.nbytes - e.out_pos);
    for (int64_t i = lo + lane; i < hi; i += 64) io.raw[e.out_pos + i] = win[i];
  }
  if (lane == 0) {
    io.status[m] = rule ? (rule << 24 | pos) : 0u;
    atomicAdd(&io.sum->done, 1u);
    if (rule) atomicMin(&io.sum->first_bad, m);
    else atomicAdd(&io.sum->bytes, (unsigned long long)e.isize);
  }
}
