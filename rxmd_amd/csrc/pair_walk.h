// pair_walk.h -- the walk over a resident's row of the 10 A list for kernels that only READ what k_list10 (lists.hip) left: the pair graph
// (pair_graph.hip) and the structure statistics (structure.hip).  The two routes from an entry to the partner's cell-sorted position k are those
// of k_ehb_sweep (hbonds.hip): the 4-byte entry where the build wrote the stream (nb10_valid), else the 2-byte window slot: sl10 & 0x7fff ->
// win_k of the row's group (rpos[i] / WIN_ROWS) -> first position of the slot's unit + offset in the unit.  The partner is atom j = perm[k], its
// position comes from the per-atom arrays (FORCE overwrites the w of the packed cell-sorted copy with charges).  Engine::pair_list fills the struct.
#pragma once
#include "engine.h"

namespace rxmd {

struct PairList {                                // what a kernel needs to walk a row; by value
  int N, G, S10, slots, byplace;                 // slots: decode through the window slots (no 4-byte entries in this build)
  double rcut;                                   // <= 0: every entry
  const int *n10, *nb10, *rpos, *win_k, *perm;
  const unsigned short *sl10;
  const double *x, *y, *z;
};

// cell-sorted position of entry kk of the row whose streams start at `row` (wk: the window of the row's group, slot route only); clamped into
// [0, G) as the slot route of k_ehb_sweep is, so that a damaged stream cannot send the gathers behind it out of the arrays
__device__ inline int pair_partner_pos(const PairList &L, size_t row, const int *__restrict__ wk, int kk) {
  int k;
  if (L.slots) {
    const int sl = L.sl10[row + kk] & 0x7fff;
    k = wk[min(sl / WIN_UNIT, WIN_MAXUNITS - 1)] + (sl & (WIN_UNIT - 1));
  } else
    k = static_cast<int>(static_cast<unsigned>(L.nb10[row + kk]) & NB10_IDX_MASK);
  return min(max(k, 0), L.G - 1);
}

}  // namespace rxmd
