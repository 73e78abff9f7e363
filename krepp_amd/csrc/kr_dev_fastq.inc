// kr_dev_fastq.inc -- part of kr_device.hip (one translation unit, included in order): FASTQ records found on the device in a chunk
// of raw file bytes (kr_batch_submit_fastq).
//
// The host parser (clean_record, kr_host.cpp) takes a four-line FASTQ record in one step when its sequence line is clean; here the
// same records are found in a chunk that has been copied to HBM as it lies in the file, and the batch's bases, offsets and ids are
// written where kr_batch_submit / kr_batch_submit_text would have put them.  Everything downstream runs unchanged.
//   kr_fq_nl_count_kernel  newlines per tile of kFqTile bytes (a lane loads 16 bytes at once)
//   kr_fq_nl_scan_kernel   one workgroup: the tiles' first newline numbers, the chunk's newline count
//   kr_fq_nl_write_kernel  every newline's position (the first nl_cap of them)
//   kr_fq_rec_kernel       a wave per record (lines 4r .. 4r+3: the chunk starts at a record start): is it device-clean, how long are its
//                          sequence and name; the first record that is not is found by an atomicMin on (record << 8 | status)
//   kr_fq_bsum_kernel      bases and name bytes per block of kFqRecBlock accepted records
//   kr_fq_bscan_kernel     one workgroup: the blocks' first bases / name bytes
//   kr_fq_off_kernel       offsets (uint64) and id offsets (uint32, id_sep = 0) of every record; the first record that does not fit
//                          max_bases or the id buffer ends the accepted prefix (CAPACITY)
//   kr_fq_copy_kernel      a wave per accepted record copies its sequence and name; one lane writes the summary
// The three offset kernels serve FASTA records too (kr_dev_fasta.inc): they take the record count from fq_nrec.
// Device-clean: clean_record would return Ok AND the quality line is exactly as long as the sequence line, so that the accepted
// records are a subset of the host's and give the same names and sequences.  Positions are uint32_t within the chunk (< 4 GB).
constexpr uint32_t kFqTile = 4096;     // bytes per workgroup of the newline passes: 256 lanes x 16 bytes
constexpr uint32_t kFqRecBlock = 1024; // records per workgroup of the offset passes: 256 lanes x 4

struct FqIO {
  const uint8_t* raw;
  uint64_t nbytes;
  uint32_t* tile_nl;             // [ceil(nbytes / kFqTile) + 1] newlines per tile, then (in place) the tiles' first newline numbers
  uint32_t* nl;                  // [nl_cap] newline positions
  uint32_t nl_cap;               // 4 * max_reads: the lines of every record a batch can take
  uint32_t *rec_slen, *rec_npos, *rec_nlen; // [max_reads] sequence length, name position and length of every record checked
  uint64_t *bsum_b, *bsum_n;     // [max_reads / kFqRecBlock + 2] per block, then (in place) the blocks' first bases / name bytes
  unsigned long long* ctl;       // [0] newlines in the chunk  [1] min(record << 8 | status) over rejected records  [2] records scanned
                                 // [3] (FASTA, kr_dev_fasta.inc) record starts in the chunk
  uint32_t rec_lines;            // lines of a record: 4 (FASTQ); 0: a record has any number of lines and ctl[3] counts the records
  uint8_t* bases;                // the stream's d_bases
  uint64_t* offsets;             // [max_reads + 1] the stream's d_offsets
  char* ids;                     // the name bytes back to back (nullptr: names are not copied)
  uint32_t* id_off;              // [max_reads + 1]
  uint32_t max_reads;
  uint64_t max_bases, id_cap;
  uint32_t k, tile_min_pos;
  kr_fastq_parse* sum;
};

// the newlines among raw[base .. base + 16) (base + 16 lies inside the padded buffer; bytes at or past nbytes do not count)
__device__ __forceinline__ uint32_t fq_nl_mask(const uint8_t* raw, uint64_t base, uint64_t nbytes)
{
  const uint4 v = *reinterpret_cast<const uint4*>(raw + base);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t x = w[j] ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); // 0x80 exactly in the bytes that were '\n'
    m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * j);
  }
  const uint64_t left = nbytes - base;
  if (left < 16u) m &= (1u << left) - 1u;
  return m;
}

__global__ __launch_bounds__(256) void kr_fq_nl_count_kernel(FqIO f)
{
  const uint64_t ntiles = (f.nbytes + kFqTile - 1) / kFqTile;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = t * kFqTile + 16u * threadIdx.x;
    const uint32_t c = base < f.nbytes ? (uint32_t)__popc(fq_nl_mask(f.raw, base, f.nbytes)) : 0u;
    const uint32_t tot = block_sum(c);
    if (threadIdx.x == 0) f.tile_nl[t] = tot;
  }
}

__global__ __launch_bounds__(1024) void kr_fq_nl_scan_kernel(FqIO f)
{ // one workgroup: exclusive prefix of tile_nl in place (a chunk below 4 GB has fewer than 2^32 newlines)
  const uint32_t newlines = scan_block_sums(f.tile_nl, (uint32_t)((f.nbytes + kFqTile - 1) / kFqTile));
  if (threadIdx.x == 0) f.ctl[0] = newlines;
}

__global__ __launch_bounds__(256) void kr_fq_nl_write_kernel(FqIO f)
{
  const uint64_t ntiles = (f.nbytes + kFqTile - 1) / kFqTile;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = t * kFqTile + 16u * threadIdx.x;
    uint32_t m = base < f.nbytes ? fq_nl_mask(f.raw, base, f.nbytes) : 0u;
    uint32_t idx = f.tile_nl[t] + block_scan_excl((uint32_t)__popc(m));
    for (; m; m &= m - 1u, ++idx)
      if (idx < f.nl_cap) f.nl[idx] = (uint32_t)base + (uint32_t)__ffs(m) - 1u;
  }
}

// records the newline passes give complete lines for (FASTA: the record starts counted), at most max_reads
__device__ __forceinline__ uint32_t fq_nrec(const FqIO& f)
{
  return (uint32_t)min((unsigned long long)f.max_reads, f.rec_lines ? f.ctl[0] / f.rec_lines : f.ctl[3]);
}

__device__ __forceinline__ bool fq_isspace(uint32_t c) { return c == ' ' || (c - 9u) <= 4u; } // C locale: ' ' '\t' '\n' '\v' '\f' '\r'

__global__ __launch_bounds__(256) void kr_fq_rec_kernel(FqIO f)
{
  const uint32_t nrec = fq_nrec(f), lane = lane_id();
  const uint32_t nw = gridDim.x * 4u;
  for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < nrec; r += nw) {
    const uint32_t start = r ? f.nl[4u * r - 1u] + 1u : 0u;
    const uint32_t e0 = f.nl[4u * r], e1 = f.nl[4u * r + 1u], e2 = f.nl[4u * r + 2u], e3 = f.nl[4u * r + 3u];
    const uint32_t s0 = e0 + 1u, slen = e1 - s0, q0 = e2 + 1u;
    // '@' header, '+' separator, a quality line exactly as long as the sequence line (it ends at the record's fourth newline)
    uint32_t status = (f.raw[start] == '@' && f.raw[e1 + 1u] == '+' && (uint64_t)q0 + slen == e3) ? 0u : (uint32_t)KR_FASTQ_NOT_CLEAN;
    const uint32_t nkm = slen >= f.k ? slen - f.k + 1u : 0u;
    if (!status && nkm > f.tile_min_pos) status = KR_FASTQ_LONG; // (its bytes are not looked at: the host tiles it)
    if (!status) { // sequence bytes 33..126 and none of '>' '+' '@'; quality bytes 33..127
      bool bad = false;
      for (uint32_t i = lane; i < slen; i += 64u) {
        const uint32_t c = f.raw[s0 + i], q = f.raw[q0 + i];
        bad = bad || (c - 33u > 93u) || c == '>' || c == '+' || c == '@' || (q - 33u > 94u);
      }
      if (__ballot(bad) != 0) status = KR_FASTQ_NOT_CLEAN;
    }
    if (status) {
      if (lane == 0) atomicMin(&f.ctl[1], ((unsigned long long)r << 8) | status);
      continue;
    }
    // the name: from after '@' to the first whitespace of the header line (which ends at e0, a '\n')
    uint32_t ne = e0;
    for (uint32_t p0 = start + 1u; p0 < e0; p0 += 64u) {
      const uint32_t p = p0 + lane;
      const unsigned long long hit = __ballot(p < e0 && fq_isspace(f.raw[p]));
      if (hit) {
        ne = p0 + (uint32_t)__ffsll(hit) - 1u;
        break;
      }
    }
    if (lane == 0) f.rec_slen[r] = slen, f.rec_npos[r] = start + 1u, f.rec_nlen[r] = ne - start - 1u;
  }
}

// records whose offsets are scanned: up to the first one rejected by kr_fq_rec_kernel
__device__ __forceinline__ uint32_t fq_nscan(const FqIO& f) { return (uint32_t)min((unsigned long long)fq_nrec(f), f.ctl[1] >> 8); }

__global__ __launch_bounds__(256) void kr_fq_bsum_kernel(FqIO f)
{
  const uint32_t n = fq_nscan(f), nb = n / kFqRecBlock + 1u;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    uint64_t sb = 0;
    uint32_t sn = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t r = b * kFqRecBlock + 4u * threadIdx.x + q;
      if (r < n) sb += f.rec_slen[r], sn += f.rec_nlen[r];
    }
    const uint64_t tb = block_sum(sb);
    const uint32_t tn = block_sum(sn);
    if (threadIdx.x == 0) f.bsum_b[b] = tb, f.bsum_n[b] = tn;
  }
}

__global__ __launch_bounds__(1024) void kr_fq_bscan_kernel(FqIO f)
{ // one workgroup: exclusive prefixes of bsum_b and bsum_n in place, one after the other; ctl[2] = the records they cover
  const uint32_t n = fq_nscan(f), nb = n / kFqRecBlock + 1u;
  scan_block_sums(f.bsum_b, nb);
  scan_block_sums(f.bsum_n, nb);
  if (threadIdx.x == 0) f.ctl[2] = n;
}

__global__ __launch_bounds__(256) void kr_fq_off_kernel(FqIO f)
{
  const uint32_t n = (uint32_t)f.ctl[2], nb = n / kFqRecBlock + 1u;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t r0 = b * kFqRecBlock + 4u * threadIdx.x;
    uint64_t cb[4], tb = 0;
    uint32_t cn[4], tn = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      cb[q] = r0 + q < n ? f.rec_slen[r0 + q] : 0u;
      cn[q] = r0 + q < n ? f.rec_nlen[r0 + q] : 0u;
      tb += cb[q], tn += cn[q];
    }
    uint64_t ob = f.bsum_b[b] + block_scan_excl(tb), on = f.bsum_n[b] + block_scan_excl(tn);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t r = r0 + q;
      if (r > n) break;
      f.offsets[r] = ob;
      if (f.ids) f.id_off[r] = (uint32_t)on;
      if (r == n) break;
      ob += cb[q], on += cn[q];
      if (ob > f.max_bases || on > f.id_cap) atomicMin(&f.ctl[1], ((unsigned long long)r << 8) | KR_FASTQ_CAPACITY);
    }
  }
}

__global__ __launch_bounds__(256) void kr_fq_copy_kernel(FqIO f)
{
  const unsigned long long bad = f.ctl[1];
  const uint32_t nscan = (uint32_t)f.ctl[2], nacc = (uint32_t)min((unsigned long long)nscan, bad >> 8), lane = lane_id();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    kr_fastq_parse s{};
    s.nreads = nacc;
    s.rejected = nacc;
    s.consumed = nacc ? (uint64_t)f.nl[4u * nacc - 1u] + 1u : 0u;
    s.newlines = f.ctl[0];
    s.nbases = f.offsets[nacc];
    s.id_bytes = f.ids ? f.id_off[nacc] : 0u;
    if ((bad >> 8) <= nscan) s.status = (uint32_t)(bad & 0xFFu);
    else if (s.consumed == f.nbytes) s.status = KR_FASTQ_OK;
    else if (nacc == f.max_reads) s.status = KR_FASTQ_CAPACITY;
    else s.status = KR_FASTQ_INCOMPLETE; // bytes behind the last complete record (a record cut short, or no final '\n')
    *f.sum = s;
  }
  const uint32_t nw = gridDim.x * 4u;
  for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < nacc; r += nw) {
    const uint8_t* src = f.raw + f.nl[4u * r] + 1u;
    uint8_t* dst = f.bases + f.offsets[r];
    const uint32_t slen = f.rec_slen[r];
    for (uint32_t i = lane; i < slen; i += 64u) dst[i] = src[i];
    if (f.ids) {
      const uint8_t* ns = f.raw + f.rec_npos[r];
      char* nd = f.ids + f.id_off[r];
      const uint32_t nl = f.rec_nlen[r];
      for (uint32_t i = lane; i < nl; i += 64u) nd[i] = (char)ns[i];
    }
  }
}
