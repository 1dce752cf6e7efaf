// pmmg_gather.hip — rows of a device array through a 1-based map (pmmg_hip_gather_rows and
// pmmg_hip_gather_rows_i32 of include/parmmg_hip.h): one kernel over the piece a thread moves.
#include "pmmg_gather.hpp"

#include "pmmg_devutil.hpp"

namespace {

// out row r = in row src[r] - 1 in pieces of T, `per` pieces a row
template <class T>
__global__ __launch_bounds__(kPBlock) void k_gather(long long total, int per, const int *src, const T *in, T *out) {
  const long long stride = (long long)gridDim.x * kPBlock;
  for (long long i = (long long)blockIdx.x * kPBlock + threadIdx.x; i < total; i += stride) {
    const long long r = i / per;
    const int e = (int)(i - r * per);
    out[i] = in[(long long)(src[r] - 1) * per + e];
  }
}

template <class T>
void launch(hipStream_t s, int64_t n, const int *src, int64_t row_bytes, const void *in, void *out) {
  const int per = (int)(row_bytes / (int64_t)sizeof(T));
  const long long total = (long long)n * per;
  hipLaunchKernelGGL(k_gather<T>, dim3(grid_for(total)), dim3(kPBlock), 0, s, total, per, src,
                     static_cast<const T *>(in), static_cast<T *>(out));
}

} // namespace

// 16-byte pieces where the rows allow them (a multiple of 16 bytes from 16-byte aligned bases), else one element
int pmmg_gather_rows(hipStream_t s, int64_t n, const int *src, int64_t row_bytes, int elem_bytes, const void *in,
                     void *out, char *msg, size_t msglen) {
  if (n == 0) return 1;
  if (row_bytes % 16 == 0 && aligned<16>(in) && aligned<16>(out))
    launch<int4>(s, n, src, row_bytes, in, out);
  else if (elem_bytes == 8)
    launch<double>(s, n, src, row_bytes, in, out);
  else
    launch<int>(s, n, src, row_bytes, in, out);
  DEVCK(hipGetLastError());
  return 1;
}
