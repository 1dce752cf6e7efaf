// pmmg_xfer.hpp — host-mode transfers (included by pmmg_hip.hip only): the host thread pool, the pinned staging
// buffers, uploads and row-selecting downloads through them, the one way an entry point takes an input array
// (take_input), and the streaming fill of the seed grids and output rows.
#pragma once

#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <type_traits>

#include "pmmg_ctx.hpp"

// ---------------------------------------------------------------- host-mode transfers
//
// PMMG_HIP_HOST arrays are pageable host memory (the MMG5 arrays a shim
// hands over).  A DMA from pageable memory runs at ~35 GB/s (the runtime
// stages it through its own small pinned buffers one at a time); here the
// context owns two 32 MiB pinned buffers: host threads copy chunk j into one
// while the DMA engine moves chunk j-1 out of the other (and the reverse for
// downloads, where the host side also scatters only the rows the step wrote).

struct Pool { // fixed host threads running [begin, end) slices of one job at a time
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, done;
  std::function<void(size_t, size_t)> fn;
  size_t n = 0, parts = 0, next = 0, left = 0;
  unsigned long long gen = 0;
  bool stop = false;
  explicit Pool(int nthreads) {
    for (int t = 0; t < nthreads; t++) th.emplace_back([this] { loop(); });
  }
  ~Pool() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
  bool take(size_t &b, size_t &e) { // under mu
    if (next >= parts) return false;
    const size_t p = next++;
    b = n * p / parts;
    e = n * (p + 1) / parts;
    return true;
  }
  void loop() {
    unsigned long long seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return stop || gen != seen; });
      if (stop) return;
      seen = gen;
      size_t b, e;
      while (take(b, e)) {
        lk.unlock();
        fn(b, e);
        lk.lock();
        if (--left == 0) done.notify_all();
      }
    }
  }
  void run(size_t count, size_t nparts, std::function<void(size_t, size_t)> f) {
    if (nparts <= 1 || th.empty()) {
      f(0, count);
      return;
    }
    std::unique_lock<std::mutex> lk(mu);
    fn = std::move(f);
    n = count;
    parts = nparts;
    next = 0;
    left = nparts;
    gen++;
    cv.notify_all();
    size_t b, e;
    while (take(b, e)) {
      lk.unlock();
      fn(b, e);
      lk.lock();
      left--;
    }
    done.wait(lk, [&] { return left == 0; });
  }
};

constexpr size_t kStageBytes = 32u << 20;
constexpr size_t kStageMin = 4u << 20; // smaller copies go straight through the runtime
constexpr unsigned long long kSentinel = 0x7FF4A5A5A5A5A5A5ULL; // a signalling NaN no arithmetic produces

// device -> pinned host copies by a kernel (the GPU's PCIe writes into the
// mapped staging buffer; used for every host-mode download)
__global__ __launch_bounds__(kBlock) void k_copy16(const ntd2 *src, ntd2 *dst, long long n) {
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x)
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + j), dst + j);
}
__global__ __launch_bounds__(kBlock) void k_copy1(const char *src, char *dst, long long n) {
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x)
    dst[j] = src[j];
}

static int stage_ready(pmmg_hip_ctx *c) {
  if (c->stage[0]) return 1;
  for (int b = 0; b < 2; b++) {
    HIPCK(c, hipHostMalloc(&c->stage[b], kStageBytes, hipHostMallocDefault));
    HIPCK(c, hipHostGetDevicePointer(&c->stage_dev[b], c->stage[b], 0));
    HIPCK(c, hipEventCreateWithFlags(&c->stage_ev[b], hipEventDisableTiming));
  }
  if (!c->pool) {
    // helper threads for the staging copies: 15 (a one-GPU lease of the pool
    // gives 16 CPUs; hardware_concurrency shows the whole machine), fewer on
    // a smaller host, PMMG_HIP_HOST_THREADS to override
    const int hw = (int)std::thread::hardware_concurrency();
    c->pool = new Pool(env_int("PMMG_HIP_HOST_THREADS", hw > 16 ? 16 : (hw > 1 ? hw : 1)) - 1);
  }
  return 1;
}

static void par_copy(pmmg_hip_ctx *c, void *dst, const void *src, size_t n) {
  const size_t parts = n >= (8u << 20) ? c->pool->th.size() + 1 : 1;
  c->pool->run(n, parts, [&](size_t b, size_t e) { memcpy((char *)dst + b, (const char *)src + b, e - b); });
}

// host -> device, queued on the context stream; the host buffer may be
// reused as soon as the call returns
static int h2d(pmmg_hip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return 1;
  c->bytes_up += (int64_t)bytes;
  if (bytes < kStageMin) {
    HIPCK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return 1;
  }
  if (!stage_ready(c)) return 0;
  for (size_t off = 0; off < bytes;) {
    const int b = c->stage_i;
    c->stage_i ^= 1;
    const size_t n = bytes - off < kStageBytes ? bytes - off : kStageBytes;
    HIPCK(c, hipEventSynchronize(c->stage_ev[b])); // the buffer's previous DMA is done
    par_copy(c, c->stage[b], (const char *)src + off, n);
    HIPCK(c, hipMemcpyAsync((char *)dst + off, c->stage[b], n, hipMemcpyHostToDevice, s));
    HIPCK(c, hipEventRecord(c->stage_ev[b], s));
    off += n;
  }
  return 1;
}

// device -> host of nrows rows of `row` bytes; keep(r, bytes) selects the rows
// copied into dst (AllRows: every row, one plain copy).  Synchronous.
struct AllRows {
  bool operator()(size_t, const char *) const { return true; }
};
static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class Keep>
static int d2h_rows(pmmg_hip_ctx *c, void *dst, const void *src, size_t nrows, size_t row, const Keep &keep) {
  const size_t bytes = nrows * row;
  if (bytes == 0) return 1;
  if (!stage_ready(c)) return 0;
  double t_wait = 0.0;
  const double t_start = now_s();
  const size_t per = kStageBytes / row; // rows per chunk
  const size_t nch = (nrows + per - 1) / per;
  auto issue = [&](size_t j) -> int {
    const int b = (int)(j & 1);
    const size_t r0 = j * per, n = (nrows - r0 < per ? nrows - r0 : per) * row;
    // the GPU writes the chunk into the mapped pinned buffer: its PCIe writes
    // reach ~2x the rate of the DMA engine's device->host copies (r02m: 48-byte
    // row arrays 36 -> 20-24 ms per GB; the host-side scatter now bounds it)
    const char *from = (const char *)src + r0 * row;
    if (((uintptr_t)from & 15) == 0 && (n & 15) == 0) {
      hipLaunchKernelGGL(k_copy16, dim3(1024), dim3(kBlock), 0, c->stream, (const ntd2 *)from, (ntd2 *)c->stage_dev[b],
                         (long long)(n / 16));
    } else {
      hipLaunchKernelGGL(k_copy1, dim3(1024), dim3(kBlock), 0, c->stream, from, (char *)c->stage_dev[b], (long long)n);
    }
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(c->stage_ev[b], c->stream));
    return 1;
  };
  if (!issue(0)) return 0;
  for (size_t j = 0; j < nch; j++) {
    const int b = (int)(j & 1);
    const double t0 = now_s();
    HIPCK(c, hipEventSynchronize(c->stage_ev[b]));
    const double t1 = now_s();
    t_wait += t1 - t0;
    if (j + 1 < nch && !issue(j + 1)) return 0; // the next chunk moves while this one is scattered
    const size_t r0 = j * per, nr = nrows - r0 < per ? nrows - r0 : per;
    const char *sb = (const char *)c->stage[b];
    char *db = (char *)dst + r0 * row;
    if constexpr (std::is_same<Keep, AllRows>::value) {
      par_copy(c, db, sb, nr * row);
    } else {
      // runs of consecutive kept rows go out as one memcpy each (nearly every
      // row is kept in a transfer: one copy per slice instead of one per row)
      c->pool->run(nr, nr >= 65536 ? c->pool->th.size() + 1 : 1, [&](size_t a, size_t e) {
        size_t r = a;
        while (r < e) {
          while (r < e && !keep(r0 + r, sb + r * row)) r++;
          const size_t s0 = r;
          while (r < e && keep(r0 + r, sb + r * row)) r++;
          if (r > s0) memcpy(db + s0 * row, sb + s0 * row, (r - s0) * row);
        }
      });
    }
  }
  if (c->verbose)
    fprintf(stderr, "[parmmg_hip] d2h %zu rows x %zu B: %.2f ms DMA wait, %.2f ms in total\n", nrows, row,
            1e3 * t_wait, 1e3 * (now_s() - t_start));
  return 1;
}

static int upload(pmmg_hip_ctx *c, DevBuf &b, const void *src, size_t bytes, hipStream_t s = nullptr) {
  if (!ensure(c, b, bytes)) return 0;
  return h2d(c, b.p, src, bytes, s ? s : c->stream);
}

// The device address of an input array of `bytes`, into *dev: the caller's pointer as it is (PMMG_HIP_DEVICE), else
// the array uploaded into `own` (on s, else on the context stream) and that buffer's address.  0 when the upload
// failed (*dev is then left as it was).
template <class T>
static int take_input(pmmg_hip_ctx *c, int where, const void *src, size_t bytes, DevBuf &own, const T **dev,
                      hipStream_t s = nullptr) {
  if (where != PMMG_HIP_DEVICE && !upload(c, own, src, bytes, s)) return 0;
  *dev = static_cast<const T *>(where == PMMG_HIP_DEVICE ? src : own.p);
  return 1;
}

// 16-byte streaming stores (a from hipMalloc: 16-byte aligned); the odd last
// element by the first thread.  (r05: 8-byte stores refilled cfg4's 101 MB
// seed grid in 43 us, ~2.3 TB/s)
typedef unsigned long long ntu2 __attribute__((ext_vector_type(2)));
__global__ void k_fill64(unsigned long long *a, long long n, unsigned long long v) {
  const ntu2 vv = {v, v};
  const long long n2 = n >> 1;
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n2; j += (long long)gridDim.x * blockDim.x)
    __builtin_nontemporal_store(vv, reinterpret_cast<ntu2 *>(a) + j);
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) a[n - 1] = v;
}
// seed grids of at least this many cells are refilled at the end of the call
// that used them; smaller ones (a small group's chain of launches is its
// cost) are cleared by k_reset
constexpr long long kRefillCells = 1LL << 20;
