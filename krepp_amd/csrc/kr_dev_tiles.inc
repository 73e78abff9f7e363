// kr_dev_tiles.inc -- part of kr_device.hip (included after kr_dev_accumulate.inc): long sequences across waves.
//
// The reference scans a sequence serially (search_mers, src/query.cpp:40-94) and so did both kernels here: a contig was one
// wave's work, segment after segment -- a 1 Mb contig took ~80 ms whatever else the chip had to do.  A host batch that holds
// sequences of more than kTileMinPos k-mer positions is therefore submitted as a batch of TILES (kr_host_stream.inc): a
// long sequence becomes ceil(positions / kSegPos) reads of kSegPos positions each (kSegPos + k - 1 bases: neighbours overlap
// by k - 1 bases, every k-mer position lies in exactly one tile), which the scan and accumulate kernels handle like any
// other one-segment read, on as many waves as there are tiles.  What makes a tile different:
//   * its keys must not be filtered by the tile's own hdist_filt (src/query.cpp:101-106,119 test the SEQUENCE's minimum):
//     kr_tile_filt_kernel moves the tile's per-strand minima aside and leaves "none" (0xFFFFFFFF) in their place, which the
//     accumulate kernel's limit 2 * hdist_filt + 1 (u32 wrap) turns into "every key passes";
//   * kr_tile_merge_kernel (a wave per long sequence) then adds the tiles' histograms per (leaf, strand) key -- positions of
//     different tiles are distinct, so Minfo::update_match's per-position minimum (src/query.hpp:153-176) is the sum of the
//     tiles' counts --, takes the minima of the moved-aside hdist_filt values and the sum of the valid k-mers, applies the
//     test and writes the sequence's records (histogram planes: the counts of a contig do not fit the packed word) in
//     ascending key order at the sequence's first tile; the tiles' own records become holes;
//   * kr_tile_gather_kernel lists the per-read results of the REAL reads (first tile of a long sequence, or the read itself)
//     for the views, the copies back and `place` -- and, for a tiled batch that leaves the device as compact rows (KR_TILE_ROWS),
//     their row ranges, which the text kernels and the copy back index by the caller's reads.
// The likelihood and selection kernels run over the tiled batch unchanged: tiles without records are reads without records.
//
// Who lays the tiled batch out: build_tiles (kr_host_stream.inc) for a host batch, while it copies the batch into page-locked
// memory; the kr_tile_lay_* kernels at the end of this file for a batch whose bases are in HBM already (KR_TILE_DEVICE).  Both
// fill the same arrays and take a sequence's shape from tile_shape below.
constexpr uint32_t kTileMinPos = 1024; // sequences of more k-mer positions are tiled

// A sequence of `len` bases as tiles: its k-mer positions, its tiles of kSegPos positions (0 for a sequence shorter than k), and
// the bases it takes in the tiled batch -- every tile but the first repeats the k - 1 bases before it
struct TileShape {
  uint64_t nkm, nt, bytes;
};
__host__ __device__ inline TileShape tile_shape(uint64_t len, uint32_t k)
{
  TileShape t;
  t.nkm = len >= k ? len - k + 1 : 0;
  t.nt = (t.nkm + kSegPos - 1) / kSegPos;
  t.bytes = t.nt ? len + (t.nt - 1) * (k - 1) : len;
  return t;
}

struct TileBatch {
  const uint8_t* v_tile;    // [nv] 1: this read of the (tiled) batch is a tile of a long sequence
  const uint32_t* longs;    // [2 * nlong] first tile, number of tiles
  const uint32_t* r_first;  // [nreal] the real read's (first) read of the tiled batch
  uint32_t* tile_filt;      // [2 * nv] hdist_filt of the tiles, moved aside
  uint32_t nv, nlong, nreal;
  // per-read results of the real reads
  uint32_t* real_off;
  uint32_t* real_cnt;
  uint32_t* real_onmers;
  uint32_t* real_filt;
  uint8_t* real_na;
  uint32_t* real_roff;      // rows-mode batches (KR_TILE_ROWS), else null: the real read's first row and its rows
  uint32_t* real_rcnt;
};

__global__ __launch_bounds__(256) void kr_tile_filt_kernel(BatchOut out, TileBatch tb)
{
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < tb.nv; v += gridDim.x * blockDim.x)
    if (tb.v_tile[v]) {
      uint2* f = reinterpret_cast<uint2*>(out.rd_filt) + v;
      reinterpret_cast<uint2*>(tb.tile_filt)[v] = *f;
      *f = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    }
}

// One wave per long sequence.  Scratch: the wave's level-2 count table of the accumulate kernel (g_counts, all-zero between
// uses) and its slot list; a key bitmap in LDS.
// EMIT_ONLY: the adding was done by kr_tile_add_kernel (sequence li in scratch region li: the grid covers every sequence)
template <bool EMIT_ONLY>
__global__ __launch_bounds__(kWave) void kr_tile_merge_kernel(DevIndex ix, DevParams P, BatchOut out, TileBatch tb)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  lds_u32* bitmap = (lds_u32*)(KR_LDS uint8_t*)s_dyn; // [bm_words]
  const uint32_t lane = lane_id(), np = P.np;
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint64_t w = blockIdx.x;
  uint32_t* g_counts = out.g_counts + w * (uint64_t)out.nslots2 * np;
  uint32_t* g_list = out.g_list + w * (uint64_t)out.g_list_words;
  uint32_t* g_bitmap = out.g_planes + w * (uint64_t)out.nslots2 * np * kPlaneWords; // (EMIT_ONLY: the key bitmap kr_tile_add_kernel made)
  for (uint32_t q = lane; q < out.bm_words; q += kWave) bitmap[q] = 0;
  WAVE_SYNC();
  uint32_t rec_next = 0, rec_end = 0, n_rec = 0, n_hole = 0; // n_hole: records of tiles that became holes (wave-uniform; summed in counters[kCtTileHoles], which kr_batch_wait subtracts before it applies max_records)
  for (uint32_t li = blockIdx.x; li < tb.nlong; li += gridDim.x) {
    const uint32_t v0 = tb.longs[2 * li], nt = tb.longs[2 * li + 1];
    // ---- the sequence's hdist_filt (minimum over its tiles, src/query.cpp:366-368) and valid k-mers (src/query.cpp:66)
    uint32_t f0 = 0xFFFFFFFFu, f1 = 0xFFFFFFFFu, onm = 0;
    // (filter slots: what the scan kernel knew of a tile was moved aside, what the accumulate kernel verified lies in rd_filt;
    //  otherwise rd_filt holds "none" for a tile)
    for (uint32_t t = lane; t < nt; t += kWave) {
      f0 = min(f0, min(tb.tile_filt[2 * (v0 + t)], out.rd_filt[2 * (v0 + t)]));
      f1 = min(f1, min(tb.tile_filt[2 * (v0 + t) + 1], out.rd_filt[2 * (v0 + t) + 1]));
      onm += out.rd_onmers[v0 + t];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      f0 = min(f0, (uint32_t)__shfl_xor(f0, d));
      f1 = min(f1, (uint32_t)__shfl_xor(f1, d));
      onm += (uint32_t)__shfl_xor(onm, d);
    }
    const uint32_t lim0 = 2u * f0 + 1u, lim1 = 2u * f1 + 1u; // u32 wrap keeps "none" = max
    if (EMIT_ONLY) { // the bitmap comes from global memory, and goes back to all-zero there
      for (uint32_t q = lane; q < out.bm_words; q += kWave) {
        const uint32_t wd = g_bitmap[q];
        bitmap[q] = wd;
        if (wd) g_bitmap[q] = 0;
      }
      WAVE_SYNC();
    }
    // ---- add the tiles' histograms per key; a tile has one record per key, so the lanes of one step touch distinct keys
    for (uint32_t t = 0; t < (EMIT_ONLY ? 0u : nt); ++t) {
      const uint32_t ro = out.rd_off[v0 + t], n = out.rd_cnt[v0 + t];
      n_hole += n;
      for (uint32_t i0 = 0; i0 < n; i0 += kWave) {
        const uint32_t i = ro + i0 + lane;
        if (i0 + lane < n) {
          const uint32_t key = out.rec_key[i];
          const uint32_t rs = ((ix.node_info[key >> 1] >> 2) << 1) | (key & 1u); // 2 * leaf rank + strand
          const uint64_t w0 = out.rec_w0[i];
          for (uint32_t x = 0; x < np; ++x) {
            const uint32_t c = w0 != 0ull ? (uint32_t)(w0 >> (8u * x)) & 255u : out.rec_hist[(uint64_t)x * out.rec_stride + i];
            if (c) {
              uint32_t* cp = &g_counts[(uint64_t)rs * np + x];
              gstore(cp, gload(cp) + c);
            }
          }
          lds_or(&bitmap[rs >> 5], 1u << (rs & 31u));
          out.rec_key[i] = 0; // the tile's record is a hole from here on
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // the next tile's lanes may touch the keys of this one
      WAVE_SYNC();
    }
    // ---- keys in ascending order (= ascending colour id, strands adjacent)
    uint32_t nkeys = 0;
    for (uint32_t w0i = 0; w0i < out.bm_words; w0i += kWave) {
      const uint32_t wi = w0i + lane;
      uint32_t word = wi < out.bm_words ? bitmap[wi] : 0u;
      const uint32_t c = __popc(word), inc = wave_scan_incl(c);
      uint32_t o = nkeys + inc - c;
      while (word) {
        const uint32_t bit = (uint32_t)__ffs((int)word) - 1u;
        gstore(&g_list[o++], wi * 32u + bit);
        word &= word - 1u;
      }
      nkeys += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    WAVE_SYNC();
    auto passes = [&](uint32_t slot2) -> bool { // hdist_min <= 2 * hdist_filt + 1 (src/query.cpp:101-106,119)
      for (uint32_t x = 0; x < np; ++x)
        if (gload(&g_counts[(uint64_t)slot2 * np + x])) return x <= ((slot2 & 1u) ? lim1 : lim0);
      return false;
    };
    uint32_t nrec = 0;
    for (uint32_t t0 = 0; t0 < nkeys; t0 += kWave) {
      const uint32_t t = t0 + lane;
      nrec += (uint32_t)__popcll(__ballot(t < nkeys && passes(gload(&g_list[t]))));
    }
    uint32_t rbase = 0;
    bool room = true;
    if (nrec) {
      if (rec_next + nrec > rec_end) {
        const uint32_t chunk = max(nrec, out.rec_chunk);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&out.counters[kCtRecSlots], chunk);
        base = __shfl(base, 0);
        if ((uint64_t)base + chunk > out.rec_cap) {
          if (lane == 0) atomicOr(&out.counters[kCtErr], kErrRecCap);
          room = false;
        } else {
          rec_next = base, rec_end = base + chunk;
        }
      }
      if (room) rbase = rec_next, rec_next += nrec, n_rec += nrec;
    }
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < nkeys; t0 += kWave) {
      const uint32_t t = t0 + lane;
      uint32_t slot2 = 0;
      bool ok = false;
      if (t < nkeys) {
        slot2 = gload(&g_list[t]);
        ok = passes(slot2);
      }
      const uint64_t okm = __ballot(ok);
      if (ok && room) {
        const uint32_t ri = rbase + run + (uint32_t)__popcll(okm & lt);
        out.rec_key[ri] = (ix.leaf_se[slot2 >> 1] << 1) | (slot2 & 1u);
        out.rec_read[ri] = v0;
        for (uint32_t x = 0; x < np; ++x) out.rec_hist[(uint64_t)x * out.rec_stride + ri] = gload(&g_counts[(uint64_t)slot2 * np + x]);
        out.rec_w0[ri] = 0ull; // (the counts of a long sequence do not fit the packed word: the planes say it all)
      }
      if (t < nkeys)
        for (uint32_t x = 0; x < np; ++x) gstore(&g_counts[(uint64_t)slot2 * np + x], 0u); // all-zero again
      run += (uint32_t)__popcll(okm);
    }
    for (uint32_t q = lane; q < out.bm_words; q += kWave) bitmap[q] = 0;
    // ---- the sequence's per-read results live at its first tile; its other tiles have none
    for (uint32_t t = lane; t < nt; t += kWave) {
      out.rd_off[v0 + t] = (t == 0 && room) ? rbase : 0u;
      out.rd_cnt[v0 + t] = (t == 0 && room) ? nrec : 0u;
    }
    if (lane == 0) {
      out.rd_onmers[v0] = onm;
      out.rd_filt[2 * v0] = f0, out.rd_filt[2 * v0 + 1] = f1;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    WAVE_SYNC();
  }
  if (n_rec && lane == 0) atomicAdd(&out.counters[kCtRecords], n_rec);
  if (n_hole && lane == 0) atomicAdd(&out.counters[kCtTileHoles], n_hole);
}

// A batch of FEW long sequences (a genome as the query): one merging wave per sequence is the long pole (1.4 ms per Mb).
// Then the adding is spread over W waves per sequence -- wave j takes the tiles j, j + W, ... and adds with atomics into the
// sequence's table (region `li` of the per-wave scratch; key bitmap in the first words of that region's plane table, which
// is all-zero between uses like the counts) -- and kr_tile_merge_kernel<EMIT_ONLY> enumerates, tests and writes as above.
__global__ __launch_bounds__(kWave) void kr_tile_add_kernel(DevIndex ix, DevParams P, BatchOut out, TileBatch tb, uint32_t W)
{
  const uint32_t lane = lane_id(), np = P.np;
  const uint32_t li = blockIdx.x / W, j = blockIdx.x % W;
  if (li >= tb.nlong) return;
  uint32_t* g_counts = out.g_counts + (uint64_t)li * out.nslots2 * np;
  uint32_t* g_bitmap = out.g_planes + (uint64_t)li * out.nslots2 * np * kPlaneWords;
  const uint32_t v0 = tb.longs[2 * li], nt = tb.longs[2 * li + 1];
  uint32_t n_hole = 0;
  for (uint32_t t = j; t < nt; t += W) {
    const uint32_t ro = out.rd_off[v0 + t], n = out.rd_cnt[v0 + t];
    n_hole += n;
    for (uint32_t i0 = 0; i0 < n; i0 += kWave) {
      const uint32_t i = ro + i0 + lane;
      if (i0 + lane < n) {
        const uint32_t key = out.rec_key[i];
        const uint32_t rs = ((ix.node_info[key >> 1] >> 2) << 1) | (key & 1u);
        const uint64_t w0 = out.rec_w0[i];
        for (uint32_t x = 0; x < np; ++x) {
          const uint32_t c = w0 != 0ull ? (uint32_t)(w0 >> (8u * x)) & 255u : out.rec_hist[(uint64_t)x * out.rec_stride + i];
          if (c) atomicAdd(&g_counts[(uint64_t)rs * np + x], c);
        }
        atomicOr(&g_bitmap[rs >> 5], 1u << (rs & 31u));
        out.rec_key[i] = 0;
      }
    }
  }
  if (n_hole && lane == 0) atomicAdd(&out.counters[kCtTileHoles], n_hole);
}

// per-read results of the real reads (after the selection kernel; in a rows-mode batch after the row kernels, whose rd_roff it
// reads, and before the text kernels, which read what it writes)
__global__ __launch_bounds__(256) void kr_tile_gather_kernel(BatchOut out, TileBatch tb)
{
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < tb.nreal; r += gridDim.x * blockDim.x) {
    const uint32_t v = tb.r_first[r];
    tb.real_off[r] = out.rd_off[v];
    tb.real_cnt[r] = out.rd_cnt[v];
    tb.real_onmers[r] = out.rd_onmers[v];
    tb.real_filt[2 * r] = out.rd_filt[2 * v], tb.real_filt[2 * r + 1] = out.rd_filt[2 * v + 1];
    tb.real_na[r] = out.rd_na[v];
    if (tb.real_roff) tb.real_roff[r] = out.rd_roff[v], tb.real_rcnt[r] = out.rd_rcnt[v]; // (uniform over the grid)
  }
}

// ---------------------------------------------------------------------------
// The tiled batch laid out on the device (KR_BASES_DEVICE | KR_TILE_DEVICE, kr_batch_submit_fastq with KR_TILE_DEVICE): what
// build_tiles does on the host, from the caller's bases and offsets in HBM.  Blocks of kTileBlock reads, thread t owning the reads
// 4t .. 4t+3 of its block, and the three steps of kr_dev_prefix.inc twice over:
//   kr_tile_lay_count_kernel   per block: the reads the long sequences' tiles would ADD to the batch (nt - 1 each)
//   kr_tile_lay_escan_kernel   one workgroup: the blocks' first values of that sum
//   kr_tile_lay_choose_kernel  read r is tiled iff it is long and the inclusive prefix of the sum over the reads 0 .. r is at most
//                              `spare` (max_reads - nreads): a PREFIX of the long sequences, decided by the one scan.  (The host
//                              takes the sequences greedily and may still tile a shorter one behind one that did not fit; the
//                              results are the same either way.)  Per block: reads, bases and long sequences of the tiled batch
//   kr_tile_lay_lscan_kernel   one workgroup: the blocks' first values of the three; the summary {nv, nlong, bases}
//   kr_tile_lay_reads_kernel   per read: r_first, its place in voff; an untiled read's v_tile and source, a long one's `longs` entry
//   kr_tile_lay_tiles_kernel   a wave per long sequence: voff, v_tile and source of its nt tiles
// The host waits for the summary, makes room for the bases, and
//   kr_tile_lay_copy_kernel    a wave per read of the tiled batch copies its bases: byte loads, so that nothing outside
//                              [bases + offsets[0], bases + offsets[nreads]) is touched -- the caller's buffer may end there
// ---------------------------------------------------------------------------
constexpr uint32_t kTileBlock = 1024; // reads per workgroup of the layout passes: 256 lanes x 4

struct TileLayIO {
  const uint8_t* bases;    // the caller's
  const uint64_t* offsets; // [nreads + 1]
  uint32_t nreads, k, tile_min_pos;
  uint64_t spare;          // reads the stream has beyond the batch's
  uint32_t nblk;           // blocks of kTileBlock reads
  uint64_t *bsum_e, *bsum_v, *bsum_b, *bsum_l; // [nblk] per block, then (in place) the blocks' first values: added reads | reads | bases | long sequences
  uint8_t* choice;         // [nreads] 1: the read is tiled
  uint32_t* lread;         // [nlong] the long sequences' reads
  uint64_t* vsrc;          // [nv] where a read of the tiled batch starts in `bases`
  uint64_t* voff;          // [nv + 1]  the arrays of TileBatch / the tiled BatchIn
  uint8_t* vtile;          // [nv]
  uint32_t* rfirst;        // [nreads]
  uint32_t* longs;         // [2 * nlong]
  uint64_t* sum;           // [3] nv, nlong, bases of the tiled batch
  uint8_t* dst;            // the tiled batch's bases (kr_tile_lay_copy_kernel)
};

// reads that tiling read r would add to the batch; 0: not a long sequence (tile_min_pos >= kSegPos: a long one has two tiles at least)
__device__ __forceinline__ uint64_t tile_lay_extra(const TileLayIO& t, uint64_t r)
{
  const TileShape sh = tile_shape(t.offsets[r + 1] - t.offsets[r], t.k);
  return sh.nkm > t.tile_min_pos ? sh.nt - 1 : 0;
}

__global__ __launch_bounds__(256) void kr_tile_lay_count_kernel(TileLayIO t)
{
  for (uint32_t b = blockIdx.x; b < t.nblk; b += gridDim.x) {
    uint64_t e = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint64_t r = (uint64_t)b * kTileBlock + 4u * threadIdx.x + q;
      if (r < t.nreads) e += tile_lay_extra(t, r);
    }
    const uint64_t tot = block_sum(e);
    if (threadIdx.x == 0) t.bsum_e[b] = tot;
  }
}

__global__ __launch_bounds__(1024) void kr_tile_lay_escan_kernel(TileLayIO t) { scan_block_sums(t.bsum_e, t.nblk); }

__global__ __launch_bounds__(256) void kr_tile_lay_choose_kernel(TileLayIO t)
{
  for (uint32_t b = blockIdx.x; b < t.nblk; b += gridDim.x) {
    const uint64_t r0 = (uint64_t)b * kTileBlock + 4u * threadIdx.x;
    uint64_t e[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      e[q] = r0 + q < t.nreads ? tile_lay_extra(t, r0 + q) : 0u;
      tot += e[q];
    }
    uint64_t run = t.bsum_e[b] + block_scan_excl(tot), sv = 0, sb = 0, sl = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint64_t r = r0 + q;
      if (r >= t.nreads) break;
      run += e[q]; // inclusive
      const bool tiled = e[q] != 0 && run <= t.spare;
      const uint64_t len = t.offsets[r + 1] - t.offsets[r];
      const TileShape sh = tile_shape(len, t.k);
      t.choice[r] = tiled ? 1 : 0;
      sv += tiled ? sh.nt : 1u, sb += tiled ? sh.bytes : len, sl += tiled ? 1u : 0u;
    }
    const uint64_t tv = block_sum(sv), tb = block_sum(sb), tl = block_sum(sl);
    if (threadIdx.x == 0) t.bsum_v[b] = tv, t.bsum_b[b] = tb, t.bsum_l[b] = tl;
  }
}

__global__ __launch_bounds__(1024) void kr_tile_lay_lscan_kernel(TileLayIO t)
{
  const uint64_t nv = scan_block_sums(t.bsum_v, t.nblk);
  const uint64_t nb = scan_block_sums(t.bsum_b, t.nblk);
  const uint64_t nl = scan_block_sums(t.bsum_l, t.nblk);
  if (threadIdx.x == 0) t.sum[0] = nv, t.sum[1] = nl, t.sum[2] = nb;
}

__global__ __launch_bounds__(256) void kr_tile_lay_reads_kernel(TileLayIO t)
{
  for (uint32_t b = blockIdx.x; b < t.nblk; b += gridDim.x) {
    const uint64_t r0 = (uint64_t)b * kTileBlock + 4u * threadIdx.x;
    uint64_t uv[4], ub[4], tv = 0, tb = 0, tl = 0;
    bool c[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      uv[q] = 0, ub[q] = 0, c[q] = false;
      if (r0 + q < t.nreads) {
        const uint64_t len = t.offsets[r0 + q + 1] - t.offsets[r0 + q];
        const TileShape sh = tile_shape(len, t.k);
        c[q] = t.choice[r0 + q] != 0;
        uv[q] = c[q] ? sh.nt : 1u, ub[q] = c[q] ? sh.bytes : len;
      }
      tv += uv[q], tb += ub[q], tl += c[q] ? 1u : 0u;
    }
    uint64_t v = t.bsum_v[b] + block_scan_excl(tv), by = t.bsum_b[b] + block_scan_excl(tb), li = t.bsum_l[b] + block_scan_excl(tl);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint64_t r = r0 + q;
      if (r >= t.nreads) break;
      t.rfirst[r] = (uint32_t)v;
      t.voff[v] = by; // (a long sequence: of its first tile; kr_tile_lay_tiles_kernel goes on from here)
      if (c[q]) {
        t.longs[2 * li] = (uint32_t)v, t.longs[2 * li + 1] = (uint32_t)uv[q], t.lread[li] = (uint32_t)r;
        ++li;
      } else {
        t.vtile[v] = 0, t.vsrc[v] = t.offsets[r];
      }
      v += uv[q], by += ub[q];
      if (r + 1 == t.nreads) t.voff[v] = by; // the end of the tiled batch
    }
  }
}

__global__ __launch_bounds__(256) void kr_tile_lay_tiles_kernel(TileLayIO t)
{
  const uint32_t nlong = (uint32_t)t.sum[1], lane = lane_id(), nw = gridDim.x * 4u;
  const uint64_t step = (uint64_t)kSegPos + t.k - 1; // bases of every tile but a sequence's last
  for (uint32_t li = blockIdx.x * 4u + (threadIdx.x >> 6); li < nlong; li += nw) {
    const uint64_t v0 = t.longs[2 * li], nt = t.longs[2 * li + 1], src = t.offsets[t.lread[li]], b0 = t.voff[v0];
    for (uint64_t ti = lane; ti < nt; ti += kWave) { // tile ti: k-mer positions [ti * kSegPos, ...), bases from the first one's start
      if (ti) t.voff[v0 + ti] = b0 + ti * step;
      t.vtile[v0 + ti] = 1, t.vsrc[v0 + ti] = src + ti * kSegPos;
    }
  }
}

__global__ __launch_bounds__(256) void kr_tile_lay_copy_kernel(TileLayIO t)
{
  const uint32_t nv = (uint32_t)t.sum[0], lane = lane_id(), nw = gridDim.x * 4u;
  for (uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6); v < nv; v += nw) {
    const uint64_t d0 = t.voff[v], n = t.voff[v + 1] - d0;
    const uint8_t* src = t.bases + t.vsrc[v];
    uint8_t* dst = t.dst + d0;
    for (uint64_t i = lane; i < n; i += kWave) dst[i] = src[i];
  }
}
