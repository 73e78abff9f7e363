// kr_host_gzip.inc -- part of kr_device.hip (host side): kr_gzdev_open / _read / _point / _counters / _close, kr_debug_gzdev_inflate.
// The inflater of ordinary gzip files: GzInflater (kr_gzip_super.h) over a backend that runs the four kernels of kr_dev_gzip.inc on a
// HIP stream of its own.  Independent of kr_stream; every buffer is sized at creation.

namespace {

#define GZ_HIP(expr)                                                \
  do {                                                              \
    hipError_t e__ = (expr);                                        \
    if (e__ != hipSuccess) {                                        \
      err = std::string(#expr) + ": " + hipGetErrorString(e__);     \
      return e__ == hipErrorOutOfMemory ? KR_ERR_NOMEM : KR_ERR_NO_DEVICE; \
    }                                                               \
  } while (0)

class GzDevBackend : public kr::GzBackend {
 public:
  double us_kernel[4] = {0, 0, 0, 0}, us_copy = 0; // search, decode, chain, resolve (by events); copies (host clock around them)

  ~GzDevBackend() override
  {
    if (device_ >= 0 && hipSetDevice(device_) == hipSuccess) {
      for (hipEvent_t e : ev_)
        if (e) (void)hipEventDestroy(e);
      if (st_) (void)hipStreamDestroy(st_);
      d_comp_.reset(), d_sym_.reset(), d_out_.reset(), d_win_.reset(), d_tab_.reset(), d_sum_.reset(), h_comp_.reset(), h_tab_.reset(), h_sum_.reset(), h_win_.reset();
    }
  }
  int create(int device, const kr::GzParams& p, std::string& err)
  {
    GZ_HIP(hipSetDevice(device));
    device_ = device, prm_ = p;
    nsub_max_ = (uint32_t)((p.max_comp + p.sub - 1) / p.sub);
    const uint64_t nsym = (uint64_t)p.ratio * p.max_comp;
    if (!d_comp_.reserve(p.max_comp + 16) || !d_sym_.reserve(nsym + 1) || !d_out_.reserve(nsym) || !d_win_.reserve(((uint64_t)nsub_max_ + 1) * kr::kGzWin) ||
        !d_tab_.reserve(9ull * nsub_max_) || !d_sum_.reserve(1) || !h_comp_.reserve(p.max_comp) || !h_tab_.reserve(7ull * nsub_max_) || !h_sum_.reserve(1) ||
        !h_win_.reserve(kr::kGzWin)) {
      err = "gzip inflater: cannot allocate its buffers (about 3 * ratio_cap * max_comp_bytes device bytes)";
      (void)hipGetLastError();
      return KR_ERR_NOMEM;
    }
    GZ_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    for (hipEvent_t& e : ev_) GZ_HIP(hipEventCreate(&e));
    return KR_OK;
  }
  int run(const uint8_t* comp, uint32_t nc, uint32_t pbit, uint32_t sub, uint32_t nsub, uint32_t ratio, const uint8_t* win, uint32_t wlen,
          std::vector<kr::GzSubRow>& rows, std::vector<uint32_t>& chain, kr::GzChainSum& sum, uint8_t* win_out, std::string& err) override
  {
    if (nc > prm_.max_comp || nsub > nsub_max_ || sub != prm_.sub || ratio != prm_.ratio || nsub == 0) {
      err = "gzip inflater: a super-chunk larger than the buffers";
      return KR_ERR_ARG;
    }
    GZ_HIP(hipSetDevice(device_));
    uint32_t* t = d_tab_.get();
    const uint32_t n = nsub_max_;
    kr::GzSuper G{d_comp_.get(), nc, pbit, sub, nsub, ratio, d_sym_.get(), t, t + n, t + 2 * n, t + 3 * n, t + 4 * n};
    GzChainIO io{G, d_win_.get(), wlen, t + 6 * n, t + 7 * n, t + 8 * n, t + 5 * n, d_out_.get(), d_sum_.get()};
    const auto c0 = std::chrono::steady_clock::now();
    memcpy(h_comp_.get(), comp, nc);
    memcpy(h_win_.get(), win, kr::kGzWin);
    GZ_HIP(hipMemcpyAsync(d_comp_.get(), h_comp_.get(), nc, hipMemcpyHostToDevice, st_));
    GZ_HIP(hipMemcpyAsync(d_win_.get(), h_win_.get(), kr::kGzWin, hipMemcpyHostToDevice, st_));
    GZ_HIP(hipMemsetAsync(t + 5 * n, 0, (uint64_t)nsub * 4, st_)); // CRCs: 0 but for chain chunks
    GZ_HIP(hipStreamSynchronize(st_));
    us_copy += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c0).count();
    GZ_HIP(hipEventRecord(ev_[0], st_));
    hipLaunchKernelGGL(kr_gz_search_kernel, dim3((nsub + 3) / 4), dim3(256), 0, st_, G);
    GZ_HIP(hipEventRecord(ev_[1], st_));
    hipLaunchKernelGGL(kr_gz_decode_kernel, dim3((nsub + 3) / 4), dim3(256), 0, st_, G);
    GZ_HIP(hipEventRecord(ev_[2], st_));
    hipLaunchKernelGGL(kr_gz_chain_kernel, dim3(1), dim3(1024), 0, st_, io);
    GZ_HIP(hipEventRecord(ev_[3], st_));
    hipLaunchKernelGGL(kr_gz_resolve_kernel, dim3(nsub), dim3(256), 0, st_, io);
    GZ_HIP(hipEventRecord(ev_[4], st_));
    GZ_HIP(hipGetLastError());
    for (uint32_t a = 0; a < 7; ++a) // the six per-sub-chunk arrays and the chain
      GZ_HIP(hipMemcpyAsync(h_tab_.get() + (uint64_t)a * n, t + (uint64_t)a * n, (uint64_t)nsub * 4, hipMemcpyDeviceToHost, st_));
    GZ_HIP(hipMemcpyAsync(h_sum_.get(), d_sum_.get(), sizeof(kr::GzChainSum), hipMemcpyDeviceToHost, st_));
    GZ_HIP(hipStreamSynchronize(st_));
    for (int k = 0; k < 4; ++k) {
      float ms = 0;
      GZ_HIP(hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]));
      us_kernel[k] += 1e3 * ms;
    }
    sum = *h_sum_.get();
    if (sum.nchain > nsub) {
      err = "gzip inflater: the chain kernel returned an impossible chain";
      return KR_ERR_NO_DEVICE;
    }
    const uint32_t* h = h_tab_.get();
    rows.resize(nsub);
    for (uint32_t i = 0; i < nsub; ++i) rows[i] = kr::GzSubRow{h[i], h[n + i], h[2 * n + i], h[3 * n + i], h[4 * n + i], h[5 * n + i]};
    chain.assign(h + 6ull * n, h + 6ull * n + sum.nchain);
    const auto c1 = std::chrono::steady_clock::now();
    GZ_HIP(hipMemcpyAsync(h_win_.get(), d_win_.get() + (uint64_t)sum.nchain * kr::kGzWin, kr::kGzWin, hipMemcpyDeviceToHost, st_)); // the window behind the chain
    GZ_HIP(hipStreamSynchronize(st_));
    us_copy += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c1).count();
    memcpy(win_out, h_win_.get(), kr::kGzWin);
    out_n_ = sum.total;
    return KR_OK;
  }
  int fetch(uint8_t* dst, uint64_t off, uint64_t n, std::string& err) override
  {
    if (off + n > out_n_) {
      err = "gzip inflater: bytes asked for that were not inflated";
      return KR_ERR_ARG;
    }
    if (n == 0) return KR_OK;
    GZ_HIP(hipSetDevice(device_));
    const auto c0 = std::chrono::steady_clock::now();
    GZ_HIP(hipMemcpyAsync(dst, d_out_.get() + off, n, hipMemcpyDeviceToHost, st_)); // exactly the bytes
    GZ_HIP(hipStreamSynchronize(st_));
    us_copy += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c0).count();
    return KR_OK;
  }

 private:
  int device_ = -1;
  kr::GzParams prm_;
  uint32_t nsub_max_ = 0;
  hipStream_t st_ = nullptr;
  hipEvent_t ev_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  DevBuf<uint8_t> d_comp_, d_out_, d_win_;
  DevBuf<uint16_t> d_sym_;
  DevBuf<uint32_t> d_tab_; // S | end | status | link | len | crc | chain | off | wlen, nsub_max each
  DevBuf<kr::GzChainSum> d_sum_;
  PinBuf<uint8_t> h_comp_, h_win_;
  PinBuf<uint32_t> h_tab_;
  PinBuf<kr::GzChainSum> h_sum_;
  uint64_t out_n_ = 0;
};
#undef GZ_HIP

} // namespace

struct kr_gzdev {
  int fd = -1;
  const uint8_t* map = nullptr;
  uint64_t size = 0;
  GzDevBackend be;
  std::unique_ptr<kr::GzInflater> inf;
  ~kr_gzdev()
  {
    inf.reset();
    if (map) munmap(const_cast<uint8_t*>(map), size);
    if (fd >= 0) close(fd);
  }
};

extern "C" {

int kr_gzdev_open(const char* path, int device, uint64_t max_comp_bytes, uint32_t sub_bytes, uint32_t ratio_cap, uint32_t keep_points, kr_gzdev** out)
{
  kr::clear_error();
  if (!path || !out) return kr::fail(KR_ERR_ARG, "kr_gzdev_open: null argument");
  *out = nullptr;
  kr::GzParams prm;
  prm.sub = sub_bytes, prm.ratio = ratio_cap, prm.max_comp = max_comp_bytes;
  if (const char* why = kr::gz_params_check(prm)) return kr::fail(KR_ERR_ARG, std::string("kr_gzdev_open: ") + why);
  std::unique_ptr<kr_gzdev> g(new kr_gzdev());
  g->fd = open(path, O_RDONLY);
  struct stat sb;
  if (g->fd < 0 || fstat(g->fd, &sb) != 0) return kr::fail(KR_ERR_IO, std::string("cannot open ") + path);
  if (!S_ISREG(sb.st_mode) || sb.st_size < 18) return kr::fail(KR_ERR_ARG, std::string("kr_gzdev_open: ") + path + " is no regular gzip file");
  g->size = (uint64_t)sb.st_size;
  void* m = mmap(nullptr, g->size, PROT_READ, MAP_PRIVATE, g->fd, 0);
  if (m == MAP_FAILED) return kr::fail(KR_ERR_IO, std::string("cannot map ") + path);
  g->map = (const uint8_t*)m;
  (void)madvise(m, g->size, MADV_SEQUENTIAL);
  prm.max_comp = std::max<uint64_t>(std::min<uint64_t>(prm.max_comp, g->size), prm.sub); // (a small file needs small buffers)
  std::string err;
  if (int rc = g->be.create(device, prm, err)) return kr::fail(rc, err);
  g->inf.reset(new kr::GzInflater(&g->be, g->map, g->size, prm, path));
  g->inf->keep_points = std::max<uint32_t>(keep_points, 4);
  if (int rc = g->inf->open()) return kr::fail(rc, g->inf->msg);
  *out = g.release();
  return KR_OK;
}

void kr_gzdev_close(kr_gzdev* g) { delete g; }

int kr_gzdev_read(kr_gzdev* g, uint8_t* dst, uint64_t cap, uint64_t* n)
{
  kr::clear_error();
  if (!g || !dst || !n || cap == 0) return kr::fail(KR_ERR_ARG, "kr_gzdev_read: bad argument");
  const int rc = g->inf->read(dst, cap, n);
  return rc ? kr::fail(rc, g->inf->msg) : KR_OK;
}

int kr_gzdev_point(const kr_gzdev* g, uint64_t inflated_off, kr_gzip_point* out)
{
  kr::clear_error();
  if (!g || !out) return kr::fail(KR_ERR_ARG, "kr_gzdev_point: null argument");
  const kr::GzPoint* best = nullptr;
  for (const kr::GzPoint& p : g->inf->points)
    if (p.inflated_off <= inflated_off && (!best || p.inflated_off >= best->inflated_off)) best = &p;
  if (!best) return kr::fail(KR_ERR_ARG, "kr_gzdev_point: no restart point is kept that far back");
  out->bit = best->bit, out->inflated_off = best->inflated_off, out->member_len = best->mlen, out->member_crc = best->crc, out->window_len = best->wlen;
  memcpy(out->window, best->win, kr::kGzWin);
  return KR_OK;
}

int kr_gzdev_counters(const kr_gzdev* g, uint64_t* c)
{
  kr::clear_error();
  if (!g || !c) return kr::fail(KR_ERR_ARG, "kr_gzdev_counters: null argument");
  const kr::GzCounters& k = g->inf->ctr;
  c[0] = k.super_chunks, c[1] = k.linked, c[2] = k.without_start, c[3] = k.dropped, c[4] = k.host_ranges, c[5] = k.redone_bytes;
  for (int i = 0; i < 4; ++i) c[6 + i] = (uint64_t)g->be.us_kernel[i];
  c[10] = (uint64_t)g->be.us_copy;
  return KR_OK;
}

int kr_debug_gzdev_inflate(int device, const uint8_t* comp, uint64_t n, uint32_t sub_bytes, uint32_t ratio_cap, uint64_t max_comp_bytes, uint8_t* out, uint64_t cap,
                           uint64_t* len, uint64_t tab_cap, uint32_t* S, uint32_t* end, uint32_t* status, uint32_t* link, uint32_t* length, uint32_t* crc,
                           uint64_t* ntab, uint64_t* counters)
{
  kr::clear_error();
  if (!comp || !out || !len || !S || !end || !status || !link || !length || !crc || !ntab || !counters) return kr::fail(KR_ERR_ARG, "kr_debug_gzdev_inflate: null argument");
  kr::GzParams prm;
  prm.sub = sub_bytes, prm.ratio = ratio_cap, prm.max_comp = max_comp_bytes;
  if (const char* why = kr::gz_params_check(prm)) return kr::fail(KR_ERR_ARG, std::string("kr_debug_gzdev_inflate: ") + why);
  kr::GzParams sized = prm; // the buffers: no larger than the input needs
  sized.max_comp = std::max<uint64_t>(std::min<uint64_t>(prm.max_comp, n), prm.sub);
  GzDevBackend be;
  std::string msg;
  if (int rc = be.create(device, sized, msg)) return kr::fail(rc, msg);
  const int rc = kr::gz_debug_run(be, comp, n, prm, out, cap, len, tab_cap, S, end, status, link, length, crc, ntab, counters, msg);
  return rc ? kr::fail(rc, msg) : KR_OK;
}

} // extern "C"
