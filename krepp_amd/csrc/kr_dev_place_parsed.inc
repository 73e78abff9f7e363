// kr_dev_place_parsed.inc -- part of kr_device.hip (one translation unit, included in order): what hands a batch that the record
// finders queued (kr_batch_submit_fastq / kr_batch_submit_fasta with KR_TAP_ACCS) to the place kernels (kr_place_stream_parsed).
//
// The record finder leaves the caller's reads as offsets[nreads + 1] and the accepted records' names as (position, length) into the
// chunk, which stays in HBM until the stream's next submit.  The place kernels want a length per read, the text kernels
// (kr_place_text_len_kernel / kr_place_text_write_kernel, unchanged) the ids back to back with an offset per read:
//   kr_pp_len_kernel     len[r] = offsets[r + 1] - offsets[r]; a tiled batch (KR_TILE_DEVICE) keeps its tiles' offsets elsewhere
//                        (Tiles::d_voff), so these are the caller's reads whatever the batch ran as
//   kr_pp_idsum_kernel   name bytes per block of kPpBlock reads                                     (kr_dev_prefix.inc, step 1)
//   kr_pp_idscan_kernel  one workgroup: the blocks' first name bytes; the batch's total behind them  (step 2)
//   kr_pp_idoff_kernel   id_off[0 .. nreads]                                                        (step 3)
//   kr_pp_idcopy_kernel  sixteen lanes per name copy its bytes from the chunk to ids + id_off[r]
// Sums are 64-bit until they are stored: a batch whose names reach 4 GB is refused by the host before anything is copied.
constexpr uint32_t kPpBlock = 1024; // reads per workgroup of the offset passes: 256 lanes x 4

struct PlaceParsedIO {
  const uint64_t* offsets; // [nreads + 1] the stream's d_offsets
  const uint8_t* raw;      // the chunk
  const uint32_t* npos;    // [nreads] where a read's name starts in the chunk
  const uint32_t* nlen;    // [nreads] its length (0: FASTA allows an empty name)
  uint32_t nreads;
  uint32_t* len;           // [nreads] the place workspace's d_len
  uint64_t* bsum;          // [nreads / kPpBlock + 2] per block, then (in place) the blocks' first name bytes; behind them the total
  uint32_t* id_off;        // [nreads + 1]
  char* ids;
};

__global__ __launch_bounds__(256) void kr_pp_len_kernel(PlaceParsedIO f)
{
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < f.nreads; r += gridDim.x * 256u) f.len[r] = (uint32_t)(f.offsets[r + 1] - f.offsets[r]);
}

__global__ __launch_bounds__(256) void kr_pp_idsum_kernel(PlaceParsedIO f)
{
  const uint32_t n = f.nreads, nb = n / kPpBlock + 1u;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    uint64_t sn = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t r = b * kPpBlock + 4u * threadIdx.x + q;
      if (r < n) sn += f.nlen[r];
    }
    const uint64_t tn = block_sum(sn);
    if (threadIdx.x == 0) f.bsum[b] = tn;
  }
}

__global__ __launch_bounds__(1024) void kr_pp_idscan_kernel(PlaceParsedIO f)
{ // one workgroup: exclusive prefix of bsum in place
  const uint32_t nb = f.nreads / kPpBlock + 1u;
  const uint64_t total = scan_block_sums(f.bsum, nb);
  if (threadIdx.x == 0) f.bsum[nb] = total;
}

__global__ __launch_bounds__(256) void kr_pp_idoff_kernel(PlaceParsedIO f)
{
  const uint32_t n = f.nreads, nb = n / kPpBlock + 1u;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t r0 = b * kPpBlock + 4u * threadIdx.x;
    uint32_t cn[4];
    uint64_t tn = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      cn[q] = r0 + q < n ? f.nlen[r0 + q] : 0u;
      tn += cn[q];
    }
    uint64_t on = f.bsum[b] + block_scan_excl(tn);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t r = r0 + q;
      if (r > n) break;
      f.id_off[r] = (uint32_t)on; // (r == n: the total)
      on += cn[q];
    }
  }
}

// Names are 10-40 bytes as a rule, a few hundred at times, and begin anywhere in the chunk: sixteen lanes a name, a byte a lane, so
// that a wave moves four names at once and a long one costs its group length / 16 rounds, no lane a whole name.
__global__ __launch_bounds__(256) void kr_pp_idcopy_kernel(PlaceParsedIO f)
{
  const uint32_t sub = threadIdx.x & 15u, ng = gridDim.x * 16u;
  for (uint32_t r = blockIdx.x * 16u + (threadIdx.x >> 4); r < f.nreads; r += ng) {
    const uint8_t* src = f.raw + f.npos[r];
    char* dst = f.ids + f.id_off[r];
    const uint32_t l = f.nlen[r];
    for (uint32_t i = sub; i < l; i += 16u) dst[i] = (char)src[i];
  }
}
