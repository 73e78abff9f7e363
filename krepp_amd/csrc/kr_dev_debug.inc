// kr_dev_debug.inc -- part of kr_device.hip (one translation unit, included in order): debug / tap kernels and the re-layout kernels of kr_index_upload.

// ---------------------------------------------------------------------------
// Debug kernels
// ---------------------------------------------------------------------------
// planes == 1: through front_end_planes; 2: through front_end_tab (byte tables in LDS: the slotted scan kernels' front end); 0: front_end
__global__ __launch_bounds__(kWave) void kr_front_end_kernel(DevIndex ix, BatchIn in, uint32_t stride, uint32_t* rix,
                                                            uint32_t* enc32, uint8_t* valid, uint8_t* pass, uint32_t planes)
{
  const uint32_t lane = lane_id();
  __shared__ __attribute__((aligned(16))) uint4 s_fetab[1024];
  fe_tab_to_lds(ix, (lds_u32x4*)s_fetab);
  __syncthreads();
  for (uint32_t r = blockIdx.x; r < in.nreads; r += gridDim.x) {
    const uint64_t off0 = in.offsets[r], len = in.offsets[r + 1] - off0;
    const uint8_t* seq = in.bases + off0;
    const uint64_t nkm = len >= ix.k ? len - ix.k + 1 : 0;
    for (uint64_t base0 = 0; base0 < nkm; base0 += kSegPos) {
      const uint32_t npos_seg = (uint32_t)min((uint64_t)kSegPos, nkm - base0);
      SegBits sb;
      load_segment(seq, len, base0, sb);
      for (int pp = 0; pp < 2; ++pp) {
        FrontEnd fe = front_end(ix, sb, pp, npos_seg);
        if (planes == 2) fe = front_end_tab_sel(ix, (const lds_u32x4*)s_fetab, sb, (uint32_t)pp, npos_seg);
        if (planes == 1) {
          const PlaneFe pf = front_end_planes(ix, sb, (uint32_t)pp, npos_seg);
          fe.rix[0] = pf.rix[0], fe.rix[1] = pf.rix[1], fe.enc32[0] = pf.enc32[0], fe.enc32[1] = pf.enc32[1];
          fe.valid = ((pf.valid >> lane) & 1ull) != 0ull;
        }
        uint64_t j = base0 + 64u * pp + lane;
        if (64u * pp + lane < npos_seg && j < stride) {
          for (int s = 0; s < 2; ++s) {
            uint64_t o = ((uint64_t)r * stride + j) * 2 + s;
            int lib;
            uint32_t row;
            rix[o] = fe.rix[s];
            enc32[o] = fe.enc32[s];
            valid[o] = fe.valid;
            pass[o] = fe.valid && locate_row<false>(ix, fe.rix[s], lib, row);
          }
        }
      }
    }
  }
}

template <int NPT>
__global__ void kr_brent_kernel(LlhConst C, uint32_t n, const uint32_t* hist, const uint32_t* onmers, const double* rho,
                                double* d_out, double* v_out)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables T{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, T.bk, T.hnk);
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  LlhProblem p;
  load_problem<NPT>(C, hist + (uint64_t)i * (C.th + 1), 1, onmers[i], rho[i], p);
  brent_min<NPT>(C, T, p, d_out[i], v_out[i]);
}

// pidx != nullptr: evaluation i uses problem pidx[i] (several evaluations of one histogram at different d)
__global__ __launch_bounds__(256) void kr_llh_batch_kernel(LlhConst C, uint32_t mode, uint64_t n, const double* hist,
                                                           const double* uc, const double* rho, const double* d_in,
                                                           double* d_out, double* v_out, const uint32_t* pidx)
{
  __shared__ double s_bk[32], s_hnk[kMaxPlanes];
  LlhTables T{(lds_f64*)s_bk, (lds_f64*)s_hnk};
  llh_tables_init(C, T.bk, T.hnk);
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    LlhProblem p;
    const uint64_t q = pidx ? pidx[i] : i;
    for (uint32_t x = 0; x <= C.th; ++x) p.mc[x] = hist[q * (C.th + 1) + x];
    p.uc = uc[q];
    p.rho = rho[q];
    if (mode == 0) {
      double d, v;
      brent_min<0>(C, T, p, d, v);
      d_out[i] = d;
      v_out[i] = v;
    } else {
      v_out[i] = llh_eval<0>(C, T, p, d_in[i]);
    }
  }
}

// kr_debug_prefix: the three steps of kr_dev_prefix.inc as the rows, text and FASTQ kernels run them, on plain numbers.  A block is
// BLOCK values, thread t owns the values 4t .. 4t+3 of its block (BLOCK = 64: the first 16 threads, as in kr_place_text_write_kernel)
template <typename T, uint32_t BLOCK>
__global__ __launch_bounds__(256) void kr_prefix_bsum_kernel(const uint32_t* v, uint32_t n, T* bsum)
{
  for (uint32_t b = blockIdx.x; b * BLOCK < n; b += gridDim.x) {
    T c = 0;
    for (uint32_t q = 4u * threadIdx.x; q < min(4u * threadIdx.x + 4u, BLOCK); ++q)
      if (b * BLOCK + q < n) c += v[b * BLOCK + q];
    const T tot = block_sum(c);
    if (threadIdx.x == 0) bsum[b] = tot;
  }
}
template <typename T>
__global__ __launch_bounds__(1024) void kr_prefix_bscan_kernel(T* bsum, uint32_t nblk, uint64_t* total)
{
  const T tot = scan_block_sums(bsum, nblk);
  if (threadIdx.x == 0) *total = tot;
}
template <typename T, uint32_t BLOCK>
__global__ __launch_bounds__(256) void kr_prefix_write_kernel(const uint32_t* v, uint32_t n, const T* bsum, uint64_t* prefix)
{
  for (uint32_t b = blockIdx.x; b * BLOCK < n; b += gridDim.x) {
    const uint32_t i0 = b * BLOCK, q0 = 4u * threadIdx.x;
    T c[4], tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      c[q] = (q0 + q < BLOCK && i0 + q0 + q < n) ? v[i0 + q0 + q] : 0u;
      tot += c[q];
    }
    T run = bsum[b] + block_scan_excl(tot);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (q0 + q < BLOCK && i0 + q0 + q < n) prefix[i0 + q0 + q] = run;
      run += c[q];
    }
  }
}

// Re-layout kernels used by kr_index_upload.  cls[se] = the tagged form of colour id se (class in the top two bits, see
// kr_dev_common.inc and colour_classes in kr_host_index.inc); ids the crecord does not define are dropped.
__global__ void kr_relayout_cmer(const uint32_t* cmer, uint64_t n, uint32_t* enc, uint32_t* se, const uint32_t* cls, uint32_t nsubsets)
{
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint2 v = reinterpret_cast<const uint2*>(cmer)[i];
    enc[i] = v.x;
    se[i] = v.y < nsubsets ? cls[v.y] : 0u;
  }
}
__global__ void kr_relayout_inc(const uint64_t* inc, uint32_t nrows, uint64_t* bkt, uint32_t* bad)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nrows; i += gridDim.x * blockDim.x) {
    uint64_t e = inc[i], s = i ? inc[i - 1] : 0; // FlatHT::bucket_start/next (src/table.hpp:121-136)
    uint64_t l = e >= s ? e - s : 0;
    if (e < s || l > 0xFFFFFFull || s >= (1ull << 40)) atomicOr(bad, 1u);
    bkt[i] = (s << 24) | (l & 0xFFFFFFull);
  }
}


// A lane's kernels index its slice of the stream's record arrays from 0; the result view indexes the whole arrays.
__global__ void kr_rebase_kernel(uint32_t* rd_off, const uint32_t* rd_cnt, uint32_t n, uint32_t base)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (rd_cnt[i]) rd_off[i] += base;
}
