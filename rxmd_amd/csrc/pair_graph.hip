// pair_graph.hip -- rxmd_hip_get_pairs_device: the 10 A list of the last build as coordinate (COO) arrays in DEVICE memory, in the caller's order.
// No counterpart in the reference (nbplist stays inside ENbond and qeq_initialize).  The list itself is untouched: these kernels only READ what
// k_list10 (lists.hip) left -- n10, the per-entry streams nb10 / sl10 / hess in the layout of that build (row = atom, or row = place of the atom
// in the cell-sorted row order: Engine::streams_by_place) and the windows of the groups -- and nothing here is on the path of qeq(), force() or step().
//
// One wavefront per resident row i (resident order = the caller's order behind rxmd_hip_evaluate_device), three launches:
//   k_pair_count   the row in batches of 64 entries: entry -> cell-sorted position k of the partner -> atom j = perm[k] -> vec = pos[j] - pos[i]
//                  (positions from the per-atom arrays: FORCE overwrites the w of the packed cell-sorted copy with charges) -> the test
//                  |vec| <= r_cut -> __ballot / __popcll; one 64-bit count per row, cnt[N] = 0
//   hipcub exclusive sum over N + 1 counts -> 64-bit offsets (the list of a dense 10^6-atom domain has more than 2^31 entries); off[N] = E
//   k_pair_fill    the same walk; an entry's output index = off[i] + selected entries of the batches before + its rank among the set bits of its
//                  batch's ballot below its lane: list order kept, no atomics, the selected entries of a batch are stored to consecutive addresses.
//                  It decodes and gathers again: a 64-bit mask per batch kept by the count spared the fill 6-8 % and cost a buffer (NOTES.md)
// The row walk (PairList, pair_partner_pos: the two routes from an entry to k) is pair_walk.h, shared with structure.hip.
// Algorithmic bytes per LIST entry, count: 4 (entry) or 2 (slot) streamed + 4 (perm) + 24 (position) gathered; fill: the same again, + 8 for hval,
// and per SELECTED entry 16 out (src, dst) + 24 (vec3) + 12 (shift3) + 8 (hval), + 4 or 8 gathered for a ghost's owner or a global id.
#include "pair_walk.h"
#include "scan.h"

#include <cmath>
#include <string>

namespace rxmd {

constexpr int PG_ROWS = 4;                       // rows (wavefronts) of a workgroup

__global__ void __launch_bounds__(64 * PG_ROWS) k_pair_count(PairList L, long long *__restrict__ cnt) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int i = blockIdx.x * PG_ROWS + w;
  if (i > L.N) return;
  if (i == L.N) { if (lane == 0) cnt[i] = 0; return; }       // the exclusive sum behind leaves the total in off[N]
  const int n = min(L.n10[i] & N10_COUNT, L.S10);
  long long c = n;
  if (L.rcut > 0.0) {
    const int place = (L.byplace || L.slots) ? L.rpos[i] : 0;
    const size_t row = static_cast<size_t>(L.byplace ? place : i) * L.S10;
    const int *wk = L.slots ? L.win_k + static_cast<size_t>(place / WIN_ROWS) * WIN_MAXUNITS : nullptr;
    const double xi = L.x[i], yi = L.y[i], zi = L.z[i];
    c = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int kk = c0 + lane;
      bool keep = false;
      if (kk < n) {
        const int j = L.perm[pair_partner_pos(L, row, wk, kk)];
        const double d0 = L.x[j] - xi, d1 = L.y[j] - yi, d2 = L.z[j] - zi;
        keep = sqrt(d0 * d0 + d1 * d1 + d2 * d2) <= L.rcut;
      }
      c += __popcll(__ballot(keep));
    }
  }
  if (lane == 0) cnt[i] = c;
}

__global__ void __launch_bounds__(64 * PG_ROWS) k_pair_fill(PairList L, DevBox B, int as_gid, const long long *__restrict__ off, const double *__restrict__ hess,
                                                            const long long *__restrict__ gid, const int *__restrict__ groot, const long long *__restrict__ gowner,
                                                            long long *__restrict__ src, long long *__restrict__ dst, int *__restrict__ shift3,
                                                            double *__restrict__ vec3, double *__restrict__ hval) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int i = blockIdx.x * PG_ROWS + w;
  if (i >= L.N) return;
  const int n = min(L.n10[i] & N10_COUNT, L.S10);
  const int place = (L.byplace || L.slots) ? L.rpos[i] : 0;
  const size_t row = static_cast<size_t>(L.byplace ? place : i) * L.S10;
  const int *wk = L.slots ? L.win_k + static_cast<size_t>(place / WIN_ROWS) * WIN_MAXUNITS : nullptr;
  const double xi = L.x[i], yi = L.y[i], zi = L.z[i];
  const long long si = as_gid ? gid[i] : static_cast<long long>(i);
  long long base = off[i];
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int kk = c0 + lane;
    bool keep = false;
    int j = 0;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (kk < n) {
      j = L.perm[pair_partner_pos(L, row, wk, kk)];
      d0 = L.x[j] - xi; d1 = L.y[j] - yi; d2 = L.z[j] - zi;
      keep = L.rcut <= 0.0 || sqrt(d0 * d0 + d1 * d1 + d2 * d2) <= L.rcut;      // the expression of k_pair_count: the same bits, the same selection
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const size_t e = static_cast<size_t>(base) + __popcll(m & ((1ULL << lane) - 1ULL));
      const bool ghost = j >= L.N;
      int own = j;
      if (ghost && (!as_gid || shift3)) own = min(max(ghost_owner(j, gowner, groot), 0), L.N - 1);   // (clamped: its position is read below)
      src[e] = si;
      dst[e] = as_gid ? gid[j] : static_cast<long long>(own);
      if (vec3) { vec3[3 * e] = d0; vec3[3 * e + 1] = d1; vec3[3 * e + 2] = d2; }   // the ghost IS the right periodic image: no minimum-image step
      if (shift3) {
        int s0 = 0, s1 = 0, s2 = 0;
        if (ghost) {                                                               // n = rint(H^-1 (r_ghost - r_owner)); a resident partner: the zero image
          const double g0 = L.x[j] - L.x[own], g1 = L.y[j] - L.y[own], g2 = L.z[j] - L.z[own];
          s0 = static_cast<int>(rint(B.Hi[0] * g0 + B.Hi[1] * g1 + B.Hi[2] * g2));
          s1 = static_cast<int>(rint(B.Hi[3] * g0 + B.Hi[4] * g1 + B.Hi[5] * g2));
          s2 = static_cast<int>(rint(B.Hi[6] * g0 + B.Hi[7] * g1 + B.Hi[8] * g2));
        }
        shift3[3 * e] = s0; shift3[3 * e + 1] = s1; shift3[3 * e + 2] = s2;
      }
      if (hval) hval[e] = hess[row + kk];
    }
    base += __popcll(m);
  }
}

// count + exclusive sum: pg_cnt / pg_off of the residents' rows for this cut-off -> the number selected (the one host wait of the call)
long long Engine::select_pairs(double r_cut) {
  if (force_pending) finish_force();               // (FORCE itself joins the bonded chain's stream and the halo stream in front of its end)
  if (N <= 0) return 0;
  if (!nb10_valid && !win_valid) require_nb10();   // neither route to the partners exists (build_ghosts_and_lists sweeps such a build again: not met in practice)
  if (!pg_cnt || pg_rows < rows10) { regrow_group(G_PGRAPH); pg_rows = rows10; }   // first use, or the rows have grown since
  k_pair_count<<<nblk(static_cast<long long>(N) + 1, PG_ROWS), 64 * PG_ROWS, 0, stream>>>(pair_list(r_cut), pg_cnt);
  return exclusive_sum_total(pg_cnt, pg_off, N);
}

PairList Engine::pair_list(double r_cut) const {
  PairList L;
  L.N = N; L.G = G; L.S10 = S10; L.slots = nb10_valid ? 0 : 1; L.byplace = streams_by_place ? 1 : 0;
  L.rcut = r_cut;
  L.n10 = n10; L.nb10 = nb10; L.rpos = rpos; L.win_k = win_k; L.perm = perm; L.sl10 = sl10;
  L.x = pos[0]; L.y = pos[1]; L.z = pos[2];
  return L;
}

long long Engine::pairs_device(int flags, double r_cut, long long capacity, long long *src_d, long long *dst_d, int *shift3_d, double *vec3_d, double *hval_d, hipStream_t user) {
  const bool count_only = !src_d && !dst_d;
  const bool as_gid = (flags & RXMD_PAIRS_GID) != 0;
  if (flags & ~RXMD_PAIRS_GID) throw EngineError(RXMD_E_ARG, "get_pairs_device: unknown bit in flags");
  if (!std::isfinite(r_cut)) throw EngineError(RXMD_E_ARG, "get_pairs_device: r_cut must be finite");
  if (r_cut > ff.rctap) throw EngineError(RXMD_E_ARG, "get_pairs_device: r_cut is beyond the reach of the list (" + std::to_string(ff.rctap) + " A, the taper cut-off): it does not hold those pairs");
  if (!count_only && (!src_d || !dst_d)) throw EngineError(RXMD_E_ARG, "get_pairs_device: src and dst go together (both NULL: count only)");
  if (capacity < 0) throw EngineError(RXMD_E_ARG, "get_pairs_device: negative capacity");
  if (nprocs != 1 && !as_gid) throw EngineError(RXMD_E_ARG, "get_pairs_device: local indices need a single rank (vprocs 1 1 1); ask for global ids (RXMD_PAIRS_GID)");
  if (nprocs != 1 && shift3_d) throw EngineError(RXMD_E_ARG, "get_pairs_device: shift3 needs a single rank (vprocs 1 1 1): the owner of a remote ghost is on another rank");
  if (!atoms_set || !lists_valid) throw EngineError(RXMD_E_STATE, "no 10 A list: call rxmd_hip_qeq or rxmd_hip_force first");
  const long long E = select_pairs(r_cut);           // the host wait of the call
  if (count_only || capacity < E || E == 0) return E;
  UserStream io(this, user);                         // whatever the caller's stream still does with the output arrays comes first
  k_pair_fill<<<nblk(N, PG_ROWS), 64 * PG_ROWS, 0, stream>>>(pair_list(r_cut), dev_box(box), as_gid ? 1 : 0, pg_off, hess, gid, groot, multi() ? gowner : nullptr,
                                                             src_d, dst_d, shift3_d, vec3_d, hval_d);
  io.end();
  return E;
}

}  // namespace rxmd
