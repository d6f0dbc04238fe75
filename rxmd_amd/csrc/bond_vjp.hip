// bond_vjp.hip -- rxmd_hip_bonds_vjp_device: the vector-Jacobian product of the bond-order graph (rxmd_hip_get_bonds_device, device_io.hip) with
// respect to the positions.  No counterpart in the reference; the mathematics is its force assembly (ForceBbo + ForceBondedTerms, pot.F90:113-144,
// 1325-1360 -> assemble.hip) with three changes: the per-bond coefficients dL/dBO are the caller's instead of cf1..cf3, cdbnd is zero (so the
// index-ordered ForceD term, which is no exact derivative, takes no part), and there are no neighbour forces fn*.
//
// Table entry o, owner i = bown[o], partner j = nbr[o], mirror oj = brev[o].  The caller's gradients on a selected resident entry: g0 on BO(0), gs, gp,
// gpp on BO(1..3) = sigma, pi, double-pi; every other entry, all ghost rows included, carries zero.  BO(1) = BO(0) - BO(2) - BO(3) (bo.F90:215), so
//     a1 = g0 + gs,  a2 = gp - gs,  a3 = gpp - gs ;   c_k[o] = a_k[o] + a_k[oj]
//     cc[i] = sum_{o in row i} c1 bo0 A2 + (c2 bo2 + c3 bo3) A3                                            every i < G
//     cb[o] = c1 (A0 + bo0 A1) dBOp + c2 bo2 (dln2 + A1 dBOp) + c3 bo3 (dln3 + A1 dBOp) + (cc[i] + cc[j]) dBOp
//     dL/dr_i = sum_{o in row i} cb[o] (r_i - r_j)  - gv[e(o)] + gv[e(oj)]                                 every i < G, then ghosts folded onto owners
// (vec3[e] = r_j - r_i: its gradient gv leaves the owner and reaches the partner through the partner's own entry of the bond, as fn* does in FORCE.)
//
// Five launches, in the form of assemble.hip: a lane per table entry forms the entry's terms -- per-entry arrays read coalesced, the mirror's gradient
// gathered through brev and the selection's offsets -- then a thread per atom adds its row in slot order.  No atomics: two calls on one state give the
// same bits.
//   k_bvjp_cc_terms     scatters the caller's edge-ordered gradients onto the table and symmetrises them in one pass: c1..c3 [o], and the ccbnd term
//   k_bvjp_cc_sum       cc[i]
//   k_bvjp_force_terms  cb (r_i - r_j) and the bond-vector gradient, written over c1..c3 [o] (a lane reads and writes its own entry only)
//   k_bvjp_force_sum    the per-atom gradient, ghost slots included (overwritten: nothing of an earlier call survives)
//   Engine::fold_ghost_forces on that gradient: every single-rank exchange form folds it exactly as it folds forces
//   k_bvjp_egress       -> grad_pos3[natoms][3]
// Reads what the last FORCE left (bo0, bo2, bo3, A0..A3, dBOp, dln2, dln3, the tables, positions); writes only its own scratch (engine.h: bv_*), the
// selection scratch of the graph (bg_flag / bg_off) and, through the fold on a staged single rank, the exchange's message buffers.
#include "engine.h"

#include <cmath>

namespace rxmd {

// a1..a3 of table entry o from the edge-ordered gradients (zero for an entry the selection left out and for every ghost row)
__device__ inline void bvjp_coef(int o, int nres, const int *__restrict__ flag, const int *__restrict__ off, const double *__restrict__ gbo,
                                 const double *__restrict__ gbo3, double &a1, double &a2, double &a3) {
  a1 = 0.0; a2 = 0.0; a3 = 0.0;
  if (static_cast<unsigned>(o) >= static_cast<unsigned>(nres) || !flag[o]) return;      // (unsigned: an index below zero selects nothing either)
  const size_t e = static_cast<size_t>(off[o]);
  const double g0 = gbo ? gbo[e] : 0.0;
  double gs = 0.0, gp = 0.0, gpp = 0.0;
  if (gbo3) { gs = gbo3[3 * e]; gp = gbo3[3 * e + 1]; gpp = gbo3[3 * e + 2]; }
  a1 = g0 + gs; a2 = gp - gs; a3 = gpp - gs;
}

__global__ void __launch_bounds__(256) k_bvjp_cc_terms(int nbonds, int nres, const int *__restrict__ flag, const int *__restrict__ off, const int *__restrict__ brev,
                                                        const double *__restrict__ gbo, const double *__restrict__ gbo3,
                                                        const double *__restrict__ bo0, const double *__restrict__ bo2, const double *__restrict__ bo3,
                                                        const double *__restrict__ A2, const double *__restrict__ A3,
                                                        double *__restrict__ c1o, double *__restrict__ c2o, double *__restrict__ c3o, double *__restrict__ tu) {
  const int o = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (o >= nbonds) return;
  double p1, p2, p3, m1, m2, m3;
  bvjp_coef(o, nres, flag, off, gbo, gbo3, p1, p2, p3);
  bvjp_coef(brev[o], nres, flag, off, gbo, gbo3, m1, m2, m3);
  const double c1 = p1 + m1, c2 = p2 + m2, c3 = p3 + m3;      // (a sum of two: the mirror entry forms the same bits)
  c1o[o] = c1; c2o[o] = c2; c3o[o] = c3;
  // ForceBbo: Cbond(2) = cBO(1) A2 + (cBO(2)+cBO(3)) A3   (pot.F90:1354-1357)
  tu[o] = (c1 * bo0[o]) * A2[o] + (c2 * bo2[o] + c3 * bo3[o]) * A3[o];
}
__global__ void __launch_bounds__(256) k_bvjp_cc_sum(int G, const int *__restrict__ boff, const double *__restrict__ tu, double *__restrict__ cc) {
  const int i = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (i >= G) return;
  double s = 0.0;
  for (int o = boff[i], o1 = boff[i + 1]; o < o1; ++o) s += tu[o];
  cc[i] = s;
}

// tx, ty, tz alias c1, c2, c3 (no __restrict__ on either): entry o is read, then written, by this lane alone
__global__ void __launch_bounds__(256) k_bvjp_force_terms(int nbonds, int nres, const int *__restrict__ flag, const int *__restrict__ off,
                                                           const int *__restrict__ bown, const int *__restrict__ nbr, const int *__restrict__ brev,
                                                           const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                           const double *__restrict__ bo0, const double *__restrict__ bo2, const double *__restrict__ bo3,
                                                           const double *__restrict__ dln2, const double *__restrict__ dln3, const double *__restrict__ dBOp,
                                                           const double *__restrict__ A0, const double *__restrict__ A1,
                                                           const double *__restrict__ gvec, const double *__restrict__ cc,
                                                           double *c1t, double *c2t, double *c3t) {
  const int o = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (o >= nbonds) return;
  const int i = bown[o], j = nbr[o];
  const double c1 = c1t[o], c2 = c2t[o], c3 = c3t[o];
  const double B0 = bo0[o], dB = dBOp[o], a1 = A1[o];
  const double a01 = A0[o] + B0 * a1;
  // ForceBbo Cbond(1) (pot.F90:1333-1335) + ccbnd of both ends (pot.F90:129-135); no ForceD: cdbnd = 0
  const double cb = c1 * a01 * dB + c2 * bo2[o] * (dln2[o] + a1 * dB) + c3 * bo3[o] * (dln3[o] + a1 * dB) + (cc[i] + cc[j]) * dB;
  double t0 = cb * (x[i] - x[j]), t1 = cb * (y[i] - y[j]), t2 = cb * (z[i] - z[j]);
  if (gvec) {
    if (o < nres && flag[o]) { const size_t e = static_cast<size_t>(off[o]); t0 -= gvec[3 * e]; t1 -= gvec[3 * e + 1]; t2 -= gvec[3 * e + 2]; }
    const int oj = brev[o];
    if (static_cast<unsigned>(oj) < static_cast<unsigned>(nres) && flag[oj]) { const size_t e = static_cast<size_t>(off[oj]); t0 += gvec[3 * e]; t1 += gvec[3 * e + 1]; t2 += gvec[3 * e + 2]; }
  }
  c1t[o] = t0; c2t[o] = t1; c3t[o] = t2;
}
__global__ void __launch_bounds__(256) k_bvjp_force_sum(int G, const int *__restrict__ boff, const double *__restrict__ tx, const double *__restrict__ ty,
                                                         const double *__restrict__ tz, double *__restrict__ gx, double *__restrict__ gy, double *__restrict__ gz) {
  const int i = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (i >= G) return;
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  for (int o = boff[i], o1 = boff[i + 1]; o < o1; ++o) { g0 += tx[o]; g1 += ty[o]; g2 += tz[o]; }
  gx[i] = g0; gy[i] = g1; gz[i] = g2;
}
__global__ void __launch_bounds__(256) k_bvjp_egress(int n, const double *__restrict__ gx, const double *__restrict__ gy, const double *__restrict__ gz, double *__restrict__ g3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g3[3 * static_cast<size_t>(i)] = gx[i]; g3[3 * static_cast<size_t>(i) + 1] = gy[i]; g3[3 * static_cast<size_t>(i) + 2] = gz[i];
}

void Engine::bonds_vjp_device(int flags, double bo_min, long long E, const double *grad_bo_d, const double *grad_bo3_d, const double *grad_vec3_d, double *grad_pos3_d, hipStream_t user) {
  if (flags & ~RXMD_BONDS_GID) throw EngineError(RXMD_E_ARG, "bonds_vjp_device: unknown bit in flags");
  if (!std::isfinite(bo_min)) throw EngineError(RXMD_E_ARG, "bonds_vjp_device: bo_min must be finite");
  if (E < 0) throw EngineError(RXMD_E_ARG, "bonds_vjp_device: negative E");
  if (!grad_pos3_d) throw EngineError(RXMD_E_ARG, "bonds_vjp_device: grad_pos3 must not be NULL");
  if (!grad_bo_d && !grad_bo3_d && !grad_vec3_d) throw EngineError(RXMD_E_ARG, "bonds_vjp_device: at least one of grad_bo, grad_bo3, grad_vec3 must be given");
  if (nprocs != 1) throw EngineError(RXMD_E_ARG, "bonds_vjp_device: single rank only (vprocs must be 1 1 1): the fold of the ghosts' gradients would be collective");
  if (!atoms_set || !lists_valid) throw EngineError(RXMD_E_STATE, "no bond lists: call rxmd_hip_force first");
  const long long count = select_bonds(bo_min);      // the host wait of the call; bg_flag / bg_off now belong to this state and threshold
  if (count != E) throw EngineError(RXMD_E_ARG, "bonds_vjp_device: E = " + std::to_string(E) + ", but get_bonds_device selects " + std::to_string(count) + " edges for these flags and bo_min");
  if (count > 0 && (!bv_c1 || bufs.cap[G_BVJP] < bcap || bv_nb != NB)) {   // first use, or the bond tables or the atom capacity have grown since
    regrow_group(G_BVJP, bcap);                      // (the kernels of an earlier call may still read the old blocks)
    bv_nb = NB;
  }
  UserStream io(this, user);                         // the caller's stream produced the gradients and may still hold work on grad_pos3
  if (count == 0) RX_HIP(hipMemsetAsync(grad_pos3_d, 0, sizeof(double) * 3 * static_cast<size_t>(N), stream));   // nothing selected: the gradient of nothing
  else {
    const int nres = nbonds_res;
    k_bvjp_cc_terms<<<nblk(nbonds, 256), 256, 0, stream>>>(nbonds, nres, bg_flag, bg_off, brev, grad_bo_d, grad_bo3_d, bo0, bo2, bo3, A2, A3, bv_c1, bv_c2, bv_c3, bv_t);
    k_bvjp_cc_sum<<<nblk(G, 256), 256, 0, stream>>>(G, boff, bv_t, bv_cc);
    k_bvjp_force_terms<<<nblk(nbonds, 256), 256, 0, stream>>>(nbonds, nres, bg_flag, bg_off, bown, nbr, brev, pos[0], pos[1], pos[2], bo0, bo2, bo3, dln2, dln3, dBOp, A0, A1,
                                                               grad_vec3_d, bv_cc, bv_c1, bv_c2, bv_c3);
    k_bvjp_force_sum<<<nblk(G, 256), 256, 0, stream>>>(G, boff, bv_c1, bv_c2, bv_c3, bv_g[0], bv_g[1], bv_g[2]);
    fold_ghost_forces(bv_g[0], bv_g[1], bv_g[2]);
    k_bvjp_egress<<<nblk(N, 256), 256, 0, stream>>>(N, bv_g[0], bv_g[1], bv_g[2], grad_pos3_d);
  }
  io.end();
}

}  // namespace rxmd
