// pmmg_comm.hpp — the split of one group over the node's GPUs, C-level
// (included by pmmg_hip.hip only; SURVEY.md §8(e), BASELINE north_star: "Located element ids and
// interpolated values are collected with RCCL all-gather over xGMI").
//
// One process per GPU (ParMmg's MPI ranks, GPU = node-local rank,
// src/parmmg.c:121): every rank transfers its part of the new points, then
// one ncclAllGather collects {K doubles, element id, hit code} per point on
// every rank.  RCCL is loaded at the first communicator call (dlopen of
// librccl.so.1, the ROCm library or the copy a host process such as PyTorch
// has already loaded: the same soname), so libpmmg_hip.so itself needs no
// RCCL to load and a caller that never splits a group never touches it.
//
// All-gather of unequal parts: each rank packs its points' rows into records
// of R = 8 K + 8 bytes (K doubles, int32 element, int8 hit, padding) in a
// send buffer of max_r counts[r] records, one ncclAllGather of that many
// bytes per rank (ring over xGMI), then one kernel unpacks every rank's
// records into the rank-order concatenation of the caller's output arrays
// (after the loader and the kernels: ag_agree and ag_points, the host side).
#pragma once

#include <dlfcn.h>
#include <rccl/rccl.h> // types only: the functions are taken from the dlopen'ed library

#include "pmmg_ctx.hpp"

namespace pmmg {

struct Rccl {
  bool tried = false, ok = false;
  char why[256] = {0};
  decltype(&::ncclGetUniqueId) getUniqueId = nullptr;
  decltype(&::ncclCommInitRank) commInitRank = nullptr;
  decltype(&::ncclCommDestroy) commDestroy = nullptr;
  decltype(&::ncclAllGather) allGather = nullptr;
  decltype(&::ncclGetErrorString) errorString = nullptr;
};

// the process's RCCL entry points (loaded once; dlopen is thread-safe, the
// races of two contexts' first calls only repeat the same lookups)
inline Rccl &rccl() {
  static Rccl R;
  if (R.tried) return R;
  void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    snprintf(R.why, sizeof(R.why), "librccl.so.1 not found: %s", dlerror());
  } else {
    R.getUniqueId = (decltype(R.getUniqueId))dlsym(h, "ncclGetUniqueId");
    R.commInitRank = (decltype(R.commInitRank))dlsym(h, "ncclCommInitRank");
    R.commDestroy = (decltype(R.commDestroy))dlsym(h, "ncclCommDestroy");
    R.allGather = (decltype(R.allGather))dlsym(h, "ncclAllGather");
    R.errorString = (decltype(R.errorString))dlsym(h, "ncclGetErrorString");
    R.ok = R.getUniqueId && R.commInitRank && R.commDestroy && R.allGather && R.errorString;
    if (!R.ok) snprintf(R.why, sizeof(R.why), "librccl.so.1 lacks the NCCL entry points");
  }
  R.tried = true;
  return R;
}

// record layout of the all-gather: the slots' rows (nslot of size[s]
// doubles), then the element id and the hit code
struct AgSlots {
  const double *in[kMaxSlot];
  double *out[kMaxSlot];
  int size[kMaxSlot];
  int n;
  int K; // doubles per record
};

__global__ __launch_bounds__(kBlock) void k_ag_pack(AgSlots S, const int *elem, const int8_t *hit, long long n,
                                                    char *send) {
  const long long R = 8LL * S.K + 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double *row = reinterpret_cast<double *>(send + R * i);
    int o = 0;
    for (int s = 0; s < S.n; s++)
      for (int j = 0; j < S.size[s]; j++) row[o++] = S.in[s][(size_t)S.size[s] * i + j];
    int *tail = reinterpret_cast<int *>(row + S.K);
    tail[0] = elem ? elem[i] : 0;
    tail[1] = hit ? (int)hit[i] : 0;
  }
}

// rank r's records at recv + r * maxn * R -> output rows off[r] .. off[r] + cnt[r]
__global__ __launch_bounds__(kBlock) void k_ag_unpack(AgSlots S, const char *recv, long long maxn, int nranks,
                                                      const long long *off, int *elem_all, int8_t *hit_all) {
  const long long R = 8LL * S.K + 8, total = off[nranks];
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < total;
       g += (long long)gridDim.x * blockDim.x) {
    int r = 0;
    while (off[r + 1] <= g) r++; // ranks are few
    const long long i = g - off[r];
    const double *row = reinterpret_cast<const double *>(recv + R * ((long long)r * maxn + i));
    int o = 0;
    for (int s = 0; s < S.n; s++)
      for (int j = 0; j < S.size[s]; j++) S.out[s][(size_t)S.size[s] * g + j] = row[o++];
    const int *tail = reinterpret_cast<const int *>(row + S.K);
    if (elem_all) elem_all[g] = tail[0];
    if (hit_all) hit_all[g] = (int8_t)tail[1];
  }
}

} // namespace pmmg

static void comm_release(pmmg_hip_ctx *c) {
  if (c->comm && c->comm_owned && rccl().ok) (void)rccl().commDestroy(c->comm);
  c->comm = nullptr;
  c->comm_owned = false;
  c->comm_rank = c->comm_size = 0;
}

static constexpr int kAgView = 8; // int64 per rank in the all-gather's agreement (ag_agree)

// The all-gather's agreement: every rank that holds a
// communicator takes part in one small all-gather of its view of the call —
// {local arguments valid and buffers allocated, K, nslot, the slot sizes, elem
// / hit given, a hash of counts[]} — before the data collective, and every
// rank then takes the same decision: either all gather, or all return 0 (a
// rank that returned early used to leave the others inside ncclAllGather, and
// records of different sizes R = 8 K + 8 were undefined behaviour).
static int ag_agree(pmmg_hip_ctx *c, const long long *mine, std::vector<long long> &all) {
  const int N = c->comm_size;
  all.assign((size_t)kAgView * N, 0);
  if (!ensure(c, c->ag_chk, sizeof(long long) * kAgView * (N + 1))) return 0;
  long long *d = c->ag_chk.as<long long>();
  hipStream_t s = c->stream;
  HIPCK(c, hipMemcpyAsync(d, mine, sizeof(long long) * kAgView, hipMemcpyHostToDevice, s));
  const ncclResult_t e = rccl().allGather(d, d + kAgView, kAgView, ncclInt64, c->comm, s);
  if (e != ncclSuccess) {
    set_err(c, "ncclAllGather (agreement): %s", rccl().errorString(e));
    return 0;
  }
  HIPCK(c, hipMemcpyAsync(all.data(), d + kAgView, sizeof(long long) * kAgView * N, hipMemcpyDeviceToHost, s));
  HIPCK(c, hipStreamSynchronize(s));
  return 1;
}

// pmmg_hip_allgather_points on a context whose device is current
static int ag_points(pmmg_hip_ctx *c, const int64_t *counts, int nslot, const int *slot_size,
                     const double *const *rows, double *const *rows_all, const int *elem, int *elem_all,
                     const int8_t *hit, int8_t *hit_all) {
  if (!c->comm) {
    set_err(c, "allgather_points: no communicator (pmmg_hip_comm_init / pmmg_hip_comm_attach)");
    return 0;
  }
  const int N = c->comm_size;
  // local checks: a failure is recorded (ok = 0), not returned, so that this
  // rank still takes part in the agreement below
  bool ok = true;
  char why[256] = {0};
  if (!counts || nslot < 0 || nslot > kMaxSlot || (nslot > 0 && (!slot_size || !rows || !rows_all)) ||
      (!elem) != (!elem_all) || (!hit) != (!hit_all)) {
    snprintf(why, sizeof(why), "allgather_points: invalid arguments (nslot=%d)", nslot);
    ok = false;
  }
  AgSlots S{};
  long long sizes_code = 0;
  if (ok) {
    S.n = nslot;
    for (int j = 0; j < nslot && ok; j++) {
      if (slot_size[j] < 1 || slot_size[j] > 6 || !rows_all[j] || (counts[c->comm_rank] > 0 && !rows[j])) {
        snprintf(why, sizeof(why), "allgather_points: slot %d (size %d) invalid", j, slot_size[j]);
        ok = false;
        break;
      }
      S.in[j] = rows[j];
      S.out[j] = rows_all[j];
      S.size[j] = slot_size[j];
      S.K += slot_size[j];
      sizes_code = sizes_code * 8 + slot_size[j];
    }
  }
  std::vector<long long> off((size_t)N + 1, 0);
  long long maxn = 0;
  unsigned long long chash = 0x9E3779B97F4A7C15ULL;
  for (int r = 0; r < N && ok; r++) {
    if (counts[r] < 0) {
      snprintf(why, sizeof(why), "allgather_points: counts[%d] = %lld", r, (long long)counts[r]);
      ok = false;
      break;
    }
    off[r + 1] = off[r] + counts[r];
    maxn = std::max(maxn, (long long)counts[r]);
    chash = (chash ^ (unsigned long long)counts[r]) * 0x100000001B3ULL;
  }
  const long long R = 8LL * S.K + 8;
  if (ok && maxn > 0 &&
      (!ensure(c, c->ag_send, (size_t)(R * maxn)) || !ensure(c, c->ag_recv, (size_t)(R * maxn * N)) ||
       !ensure(c, c->ag_off, sizeof(long long) * off.size()))) {
    snprintf(why, sizeof(why), "allgather_points: buffers: %s", c->err);
    ok = false;
  }
  // the arguments that must be identical on every rank: nslot, slot_size[],
  // whether elem / hit are given, counts[] (hence K, R and maxn)
  const long long mine[kAgView] = {ok ? 1 : 0, S.K, nslot, sizes_code, elem ? 1 : 0, hit ? 1 : 0,
                                   (long long)(chash >> 1), maxn};
  std::vector<long long> all;
  if (!ag_agree(c, mine, all)) return 0;
  if (!ok) {
    set_err(c, "%s", why);
    return 0;
  }
  for (int r = 0; r < N; r++) {
    const long long *v = &all[(size_t)kAgView * r];
    if (!v[0]) {
      set_err(c, "allgather_points: rank %d's arguments are invalid", r);
      return 0;
    }
    for (int j = 1; j < kAgView; j++)
      if (v[j] != all[j]) {
        set_err(c, "allgather_points: rank %d disagrees with rank 0 on %s", r,
                j <= 3 ? "the slot layout" : (j <= 5 ? "elem / hit" : "counts[]"));
        return 0;
      }
  }
  const long long n = counts[c->comm_rank];
  if (maxn == 0) return 1;
  hipStream_t s = c->stream;
  HIPCK(c, hipMemcpyAsync(c->ag_off.p, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice, s));
  if (n > 0)
    hipLaunchKernelGGL(k_ag_pack, dim3(blocks_for(n, 4096)), dim3(kBlock), 0, s, S, elem, hit, n,
                       c->ag_send.as<char>());
  HIPCK(c, hipGetLastError());
  const ncclResult_t e =
      rccl().allGather(c->ag_send.p, c->ag_recv.p, (size_t)(R * maxn), ncclInt8, c->comm, s);
  if (e != ncclSuccess) {
    set_err(c, "ncclAllGather: %s", rccl().errorString(e));
    return 0;
  }
  hipLaunchKernelGGL(k_ag_unpack, dim3(blocks_for(off[N], 8192)), dim3(kBlock), 0, s, S, c->ag_recv.as<const char>(),
                     maxn, N, c->ag_off.as<const long long>(), elem_all, hit_all);
  HIPCK(c, hipGetLastError());
  HIPCK(c, hipStreamSynchronize(s));
  return 1;
}
