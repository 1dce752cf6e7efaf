/*
 * pmmg_stage.h — the device blocks of one host-layer call (pmmg_host.c): host
 * arrays go up, results come down into new host blocks, and one call at the
 * end frees every device block.  The first failure latches (ok = 0) and every
 * later step is a no-op that returns NULL, so a function is written as a
 * straight sequence and looks at `ok` where it must.  Only the C-ABI of
 * parmmg_hip.h is called (tests/c/test_stage.c runs it against host stubs).
 */
#ifndef PMMG_STAGE_H
#define PMMG_STAGE_H
#include <stdint.h>
#include <stdlib.h>

#include "parmmg_hip.h"

typedef struct {
  pmmg_hip_ctx *ctx;
  int ok;     /* 0 from the first failure on */
  int n, cap; /* device blocks held, and the room of blk */
  void **blk;
} pmmg_stage;

static inline pmmg_stage pmmg_stage_begin(pmmg_hip_ctx *ctx) {
  pmmg_stage s = {ctx, 1, 0, 0, NULL};
  return s;
}

/* room for n bytes on the device (16 when n is 0) */
static inline void *pmmg_stage_room(pmmg_stage *s, int64_t n) {
  if (!s->ok) return NULL;
  if (s->n == s->cap) { /* (the list grows first: a block that exists is always on it) */
    void **b = (void **)realloc(s->blk, sizeof(void *) * (size_t)(s->cap + 16));
    if (!b) {
      s->ok = 0;
      return NULL;
    }
    s->blk = b;
    s->cap += 16;
  }
  void *d = pmmg_hip_malloc(s->ctx, n > 0 ? n : 16);
  if (d)
    s->blk[s->n++] = d;
  else
    s->ok = 0;
  return d;
}

/* n bytes of src on the device; no source or no bytes: NULL, and no failure */
static inline void *pmmg_stage_up(pmmg_stage *s, const void *src, int64_t n) {
  if (!src || n <= 0) return NULL;
  void *d = pmmg_stage_room(s, n);
  if (d && !pmmg_hip_memcpy_h2d(s->ctx, d, src, n)) s->ok = 0;
  return d;
}

/* n bytes of the device block d in a new host block, the caller's to free (one byte when n is 0, so that NULL
 * means failure) */
static inline void *pmmg_stage_down(pmmg_stage *s, const void *d, int64_t n) {
  if (!s->ok) return NULL;
  void *h = malloc(n > 0 ? (size_t)n : 1);
  if (h && n > 0 && !pmmg_hip_memcpy_d2h(s->ctx, h, d, n)) {
    free(h);
    h = NULL;
  }
  if (!h) s->ok = 0;
  return h;
}

/* rows map[r] - 1, r < n, of the device array `in` (`size` doubles a row), gathered into the device block
 * `rows` (the caller's, reused from one array to the next) and brought down */
static inline double *pmmg_stage_rows(pmmg_stage *s, int64_t n, const int *map, int size, const double *in,
                                      double *rows) {
  if (s->ok && !pmmg_hip_gather_rows(s->ctx, n, map, size, in, rows)) s->ok = 0;
  return (double *)pmmg_stage_down(s, rows, (int64_t)sizeof(double) * size * n);
}

/* the same for rows of `size` ints */
static inline int *pmmg_stage_rows_i32(pmmg_stage *s, int64_t n, const int *map, int size, const int *in, int *rows) {
  if (s->ok && !pmmg_hip_gather_rows_i32(s->ctx, n, map, size, in, rows)) s->ok = 0;
  return (int *)pmmg_stage_down(s, rows, (int64_t)sizeof(int) * size * n);
}

/* every device block freed; the host blocks handed out stay the caller's */
static inline void pmmg_stage_end(pmmg_stage *s) {
  for (int i = 0; i < s->n; i++) pmmg_hip_free(s->ctx, s->blk[i]);
  free(s->blk);
  s->blk = NULL;
  s->n = s->cap = 0;
}

#endif
