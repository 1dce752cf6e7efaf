/* pmmg_stage.h (the device blocks of one host-layer call) against host stubs of the six calls it makes:
 * "device" memory is malloc'ed, the copies are memcpy, the gathers index on the host.  One sequence of the
 * shape of pmmg_merge_grps, run clean and then once for every k with the k-th allocation, the k-th copy and the
 * k-th gather failing: nothing may stay live on the "device", no stub may be called after the first failure
 * (pmmg_hip_free apart), and what was handed out before it is the caller's to free (ASan's leak check sees the
 * rest).  Built by tests/test_stage_host.py with -fsanitize=address,undefined. */
#include <stdio.h>
#include <string.h>

#include "pmmg_stage.h"

enum { ALLOC, COPY, GATHER, KINDS };
static int calls[KINDS], fail_kind, fail_at; /* the fail_at-th call (1-based) of fail_kind fails */
static int failed, late, live;

/* 1 when this call of `kind` is the one to fail; counts a call that comes after the failure */
static int fails(int kind) {
  if (failed) late++;
  if (++calls[kind] == fail_at && kind == fail_kind) failed = 1;
  return failed;
}

void *pmmg_hip_malloc(pmmg_hip_ctx *ctx, int64_t bytes) {
  (void)ctx;
  if (bytes <= 0 || fails(ALLOC)) return NULL; /* (the stage never asks for 0 bytes) */
  live++;
  return malloc((size_t)bytes);
}
int pmmg_hip_free(pmmg_hip_ctx *ctx, void *p) {
  (void)ctx;
  if (p) live--;
  free(p);
  return 1;
}
int pmmg_hip_memcpy_h2d(pmmg_hip_ctx *ctx, void *dst, const void *src, int64_t bytes) {
  (void)ctx;
  if (fails(COPY)) return 0;
  memcpy(dst, src, (size_t)bytes);
  return 1;
}
int pmmg_hip_memcpy_d2h(pmmg_hip_ctx *ctx, void *dst, const void *src, int64_t bytes) {
  return pmmg_hip_memcpy_h2d(ctx, dst, src, bytes);
}
int pmmg_hip_gather_rows(pmmg_hip_ctx *ctx, int64_t n, const int *src, int size, const double *in, double *out) {
  (void)ctx;
  if (fails(GATHER)) return 0;
  for (int64_t r = 0; r < n; r++)
    memcpy(out + r * size, in + (int64_t)(src[r] - 1) * size, sizeof(double) * (size_t)size);
  return 1;
}
int pmmg_hip_gather_rows_i32(pmmg_hip_ctx *ctx, int64_t n, const int *src, int size, const int *in, int *out) {
  (void)ctx;
  if (fails(GATHER)) return 0;
  for (int64_t r = 0; r < n; r++) memcpy(out + r * size, in + (int64_t)(src[r] - 1) * size, sizeof(int) * (size_t)size);
  return 1;
}

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      printf("FAILED %s (line %d; kind %d, k %d)\n", #c, __LINE__, fail_kind, fail_at); \
      return -1;                                                                  \
    }                                                                             \
  } while (0)

enum { NP = 5, NT = 4 };

/* the sequence; 1: it went through, 0: it stopped at the injected failure, -1: a check failed */
static int run(int kind, int k) {
  static const int src_pt[NP] = {3, 1, 5, 2, 4}, src_tet[NT] = {4, 3, 2, 1}, tetv[4 * NT] = {1, 2, 3, 4};
  static const int tref[NT] = {10, 20, 30, 40};
  double xyz[3 * NP], met[6 * NP];
  for (int i = 0; i < 3 * NP; i++) xyz[i] = i;
  for (int i = 0; i < 6 * NP; i++) met[i] = 100 + i;
  memset(calls, 0, sizeof(calls));
  fail_kind = kind, fail_at = k, failed = late = 0;
  const int64_t i4 = sizeof(int), d8 = sizeof(double);

  pmmg_stage st = pmmg_stage_begin(NULL);
  const int *d_tetv = pmmg_stage_up(&st, tetv, i4 * 4 * NT);
  CHECK(pmmg_stage_up(&st, NULL, i4 * 7) == NULL && pmmg_stage_up(&st, tetv, 0) == NULL); /* no list: no failure */
  CHECK(st.ok == !failed);
  int *d_srcp = pmmg_stage_up(&st, src_pt, i4 * NP), *d_srct = pmmg_stage_up(&st, src_tet, i4 * NT);
  int *d_nval = pmmg_stage_room(&st, 0); /* no positions: 16 bytes */
  CHECK(!st.ok || (d_tetv && d_srcp && d_srct && d_nval));
  if (st.ok) memset(d_nval, 0, 16);
  const double *d_xyz = pmmg_stage_up(&st, xyz, d8 * 3 * NP);
  double *rows = pmmg_stage_room(&st, d8 * 6 * NP);
  double *o_xyz = pmmg_stage_rows(&st, NP, d_srcp, 3, d_xyz, rows);
  double *o_met = pmmg_stage_rows(&st, NP, d_srcp, 6, pmmg_stage_up(&st, met, d8 * 6 * NP), rows);
  const int *d_tref = pmmg_stage_up(&st, tref, i4 * NT);
  int *o_tref = pmmg_stage_rows_i32(&st, NT, d_srct, 1, d_tref, pmmg_stage_room(&st, i4 * NT));
  int *o_srcp = pmmg_stage_down(&st, d_srcp, i4 * NP);
  void *o_nval = pmmg_stage_down(&st, d_nval, 0), *o_fval = pmmg_stage_down(&st, NULL, 0); /* one byte each */
  pmmg_stage_end(&st);

  CHECK(live == 0 && st.n == 0 && st.blk == NULL);
  CHECK(st.ok == !failed && late == 0);
  /* the outputs are there up to the failure and NULL from it on */
  void *outs[] = {o_xyz, o_met, o_tref, o_srcp, o_nval, o_fval};
  int nout = 0;
  while (nout < 6 && outs[nout]) nout++;
  for (int i = nout; i < 6; i++) CHECK(outs[i] == NULL);
  CHECK(st.ok ? nout == 6 : nout < 6);
  if (nout > 0)
    for (int r = 0; r < NP; r++)
      for (int j = 0; j < 3; j++) CHECK(o_xyz[3 * r + j] == xyz[3 * (src_pt[r] - 1) + j]);
  if (nout > 1)
    for (int r = 0; r < NP; r++)
      for (int j = 0; j < 6; j++) CHECK(o_met[6 * r + j] == met[6 * (src_pt[r] - 1) + j]);
  if (nout > 2)
    for (int r = 0; r < NT; r++) CHECK(o_tref[r] == tref[src_tet[r] - 1]);
  if (nout > 3) CHECK(memcmp(o_srcp, src_pt, sizeof(src_pt)) == 0);
  for (int i = 0; i < nout; i++) free(outs[i]); /* the caller's */
  return st.ok;
}

int main(void) {
  if (run(-1, 0) != 1) return 1;
  int total[KINDS], runs = 1;
  memcpy(total, calls, sizeof(total));
  /* 6 uploads and 3 rooms; 6 copies up and 4 down (the downloads of 0 bytes copy nothing); 3 gathers */
  if (total[ALLOC] != 9 || total[COPY] != 10 || total[GATHER] != 3) {
    printf("FAILED the clean run made %d allocations, %d copies, %d gathers\n", total[ALLOC], total[COPY],
           total[GATHER]);
    return 1;
  }
  for (int kind = 0; kind < KINDS; kind++)
    for (int k = 1; k <= total[kind]; k++, runs++)
      if (run(kind, k) != 0) {
        printf("FAILED kind %d, k %d: the failure was not latched\n", kind, k);
        return 1;
      }
  printf("%d runs, all freed\n", runs);
  return 0;
}
