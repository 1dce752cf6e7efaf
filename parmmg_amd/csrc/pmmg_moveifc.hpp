// pmmg_moveifc.hpp — internal interface of pmmg_moveifc.hip (the interface
// displacement of a partition); the C-ABI wrappers live in
// pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "parmmg_hip.h"
#include "pmmg_devbuf.hpp"
#include "pmmg_tetview.hpp"

// Device scratch of the three calls, owned by a context and kept between calls
// (grown, never shrunk).
struct MoveCache {
  DevBuf words;        // the call's flag bits and the layer's count of re-marked tetra
  DevBuf weight;       // weight[ncolor] on the device
  DevBuf D;            // D[ncolor]: the layer's events per previous colour
  DevBuf key[2];       // per point: the seed's two minima; in a layer the event and the side minimum
  DevBuf side;         // per point: 1 = side point of the layer
  DevBuf mark[2];      // the marks before and after a layer, ping-ponged
  DevBuf color[2];     // the point colours, likewise
  DevBuf front[2];     // the front flags, likewise
  DevBuf set_color, set_front; // what the set points held before a layer (restored when it is dropped)
  DevBuf map;          // remap_colors: present[ncolor] bytes, then map[ncolor]
};

// The three entry points on checked arguments (tetv rows present, ne < 2^29,
// alignments).  Synchronous.  Return 1, or 0 with msg set and nothing written.
int pmmg_ifc_seed(hipStream_t s, int np, TetView m, const int *mark, int ncolor, const int *weight, int *ptcolor,
                  unsigned char *ptfront, MoveCache *c, char *msg, size_t msglen);
int pmmg_ifc_layers(hipStream_t s, int np, TetView m, int *mark, int ncolor, const int *weight, int *nelem,
                    const int *nemin, int *ptcolor, unsigned char *ptfront, int nset, const int *set_pt,
                    const int *set_color, int nlayers, int *layers_done, int *blocked, int *moved, MoveCache *c,
                    char *msg, size_t msglen);
int pmmg_ifc_remap(hipStream_t s, TetView m, const int *mark, int ncolor, const int *order, int *part, int *ngrp,
                   MoveCache *c, char *msg, size_t msglen);
