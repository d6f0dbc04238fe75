// bonded.hip -- bonded energy terms of FORCE (reference src/pot.F90) as own-slot accumulation kernels, one unit per term:
//   Ebond (pot.F90:926-977) + Elnpr (pot.F90:148-316) -> k_ebond_terms, k_elnpr_atoms, k_elnpr_bonds      here, with Engine::bonded_energies()
//   E3b   (pot.F90:319-557)                           -> k_e3q (work queue, wavefront per sixteen / eight / four centre atoms), k_e3b (thread per centre atom)      angles.hip
//   E4b   (pot.F90:980-1227)                          -> k_e4b   (wavefront per eight / four / two centre atoms, ballot-compacted work queue, persistent grid;
//                                                                  every torsion evaluated once, its k-l side delivered by k_e4b_deliver)      torsions.hip
//   Ehb   (pot.F90:559-673)                           -> k_ehb_donors + k_ehb_sweep (donor list; a wavefront takes whole donors, acceptors staged in LDS)      hbonds.hip
//   constants of module.F90, block_energy_add, angle_forces                                                                                   bonded_common.h
// The reference scatters every derivative at once with atomics (ForceB/ForceBbo/ForceA3/ForceA4,
// pot.F90:1276-1521).  Here a thread owns one centre atom and accumulates ONLY into that atom's own
// stretch of the compact bond tables (bond o = boff[centre] + slot, engine.h):
//     cf1,cf2,cf3[slot]  dE/dBO of the bond in that slot, in ForceBbo's cf() form (pot.F90:1331):
//                        full BO, pi-minus-full, pipi-minus-full.  ForceB(c) == cf (c,0,0).
//     cdn[slot]          contribution to cdbnd of the NEIGHBOUR in that slot (pot.F90:304,536,539,1183)
//     fnx,fny,fnz[slot]  angle/torsion force on the neighbour in that slot
//     cds, f (self)      contribution to the centre's own cdbnd / force
// assemble.hip turns these into forces by pure gathers through the mirror-bond index brev: deterministic, no FP64 atomics
// (except the acceptor atom of a hydrogen bond, which is a 10 A partner and has no slot).
#include "bonded_common.h"

namespace rxmd {

// ------------------------------------------------------------------------------------------------
// Ebond + Elnpr in three steps over the compact bond tables (round 4; one thread per atom looping over its bonds read nine per-bond arrays with a
// stride of ~5 entries between neighbouring lanes: 0.81 ms):
//   A  one lane per bond of a resident: the bond's terms of the two over-coordination sums (pot.F90:223-224), exp_coa3 * exp_coa4 of the bond as seen
//      from i (pot.F90:484-487), and Ebond with its coefficients where gid(j) < gid(i) (pot.F90:949)
//   B  one thread per resident: the sums in slot order (the order of the loop this replaces), the lone-pair / over- / under-coordination energies
//      and the six coefficients every bond of the atom needs (pot.F90:226-281)
//   C  one lane per bond of a resident: the coefficients applied to the bond (pot.F90:282-305)
__global__ void __launch_bounds__(256) k_ebond_terms(int nb_res, DevFF ff, const int *__restrict__ bown, const int *__restrict__ nbr, const unsigned char *__restrict__ btype, const int *__restrict__ type,
                                                      const long long *__restrict__ gid, const double *__restrict__ bo0, const double *__restrict__ bo1,
                                                      const double *__restrict__ bo2, const double *__restrict__ bo3, const double *__restrict__ delta, const double *__restrict__ deltalp,
                                                      double *__restrict__ cf1, double *__restrict__ cf2, double *__restrict__ cf3, double *__restrict__ ecoa,
                                                      double *__restrict__ t1, double *__restrict__ t2, double *__restrict__ pe) {
  const int o = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  double e1 = 0.0;
  if (o < nb_res) {
    const int i = bown[o], j = nbr[o];
    const int tj = btype[o];
    const DevBondP bp = ff.bond[ff.inxn2[type[i] * ff.n1 + tj]];
    const double B0 = bo0[o], dj = delta[j];
    t1[o] = bp.povun1 * bp.Desig * B0;                                  // pot.F90:223
    t2[o] = (dj - deltalp[j]) * (bo2[o] + bo3[o]);                      // pot.F90:224
    {                                                                   // exp_coa3 * exp_coa4 of this bond as seen from i (pot.F90:484-487)
      const double bs = B0 - cutof2_esub, u = -bs + (dj + ff.atom[tj].Val);
      ecoa[o] = exp(-ff.pcoa3 * (u * u)) * exp(-ff.pcoa4 * ((bs - 1.5) * (bs - 1.5)));
    }
    double c1 = 0.0, c2 = 0.0, c3 = 0.0;
    if (gid[j] < gid[i]) {                                              // Ebond, pot.F90:949
      const double B1 = bo1[o];
      const double pw = pow(B1, bp.pbe2);
      const double ex = exp(bp.pbe1 * (1.0 - pw));
      e1 = -bp.Desig * B1 * ex - bp.Depi * bo2[o] - bp.Depipi * bo3[o];
      const double CEbo = -bp.Desig * ex * (1.0 - bp.pbe1 * bp.pbe2 * pw);
      c1 = CEbo; c2 = -bp.Depi - CEbo; c3 = -bp.Depipi - CEbo;         // coeff = (CEbo,-Depi,-Depipi)
    }
    cf1[o] = c1; cf2[o] = c2; cf3[o] = c3;                              // the first writer of these accumulators SETS them (k_bo_full clears only the ghosts' bonds): 0 + x == x, bit for bit
  }
  block_energy_add(e1, pe + 1);
}

__global__ void __launch_bounds__(256) k_elnpr_atoms(int N, DevFF ff, const int *__restrict__ boff, const int *__restrict__ type, const double *__restrict__ t1, const double *__restrict__ t2,
                                                      const double *__restrict__ delta, const double *__restrict__ deltalp, const double *__restrict__ dDlp,
                                                      double *__restrict__ ecoef, double *__restrict__ pe) {
  const int i = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  double e2 = 0.0, e3 = 0.0, e4 = 0.0;
  if (i < N) {
    const DevAtomP ai = ff.atom[type[i]];
    double sum_ovun1 = 0.0, sum_ovun2 = 0.0;
    for (int o = boff[i], o1 = boff[i + 1]; o < o1; ++o) { sum_ovun1 += t1[o]; sum_ovun2 += t2[o]; }
    const double dlp = deltalp[i], dl = delta[i], dD = dDlp[i];
    const double expvd2 = exp(-75.0 * dlp);
    const double dElp = ai.plp2 * ((1.0 + expvd2) + 75.0 * dlp * expvd2) / ((1.0 + expvd2) * (1.0 + expvd2));
    const double expovun1 = ff.povun3 * exp(ff.povun4 * sum_ovun2);
    const double dcorr = dl - dlp / (1.0 + expovun1);
    const double expovun2 = exp(ai.povun2 * dcorr);
    const double DlpV = 1.0 / (dcorr + ai.Val + 1e-8);
    const double expovun2n = 1.0 / expovun2;
    const double expovun6 = exp(ff.povun6 * dcorr);
    const double expovun8 = ff.povun7 * exp(ff.povun8 * sum_ovun2);
    const double d1 = 1.0 / (1.0 + expovun1), d2 = 1.0 / (1.0 + expovun2), d2n = 1.0 / (1.0 + expovun2n), d8 = 1.0 / (1.0 + expovun8);
    e2 = ai.plp2 * dlp / (1.0 + expvd2);
    e3 = sum_ovun1 * DlpV * dcorr * d2;
    const double PEunder = -ai.povun5 * (1.0 - expovun6) * d2n * d8;
    e4 = PEunder;
    const double CElp1 = dElp * dD;
    const double CEo1 = dcorr * DlpV * d2;
    const double CEo2 = sum_ovun1 * DlpV * d2 * (1.0 - dcorr * DlpV - ai.povun2 * dcorr * d2n);
    const double CEo3 = CEo2 * (1.0 - dD * d1);
    const double CEo4 = CEo2 * dlp * ff.povun4 * expovun1 * (d1 * d1);
    const double CEu1 = (ai.povun5 * ff.povun6 * expovun6 * d8 + PEunder * ai.povun2 * expovun2n) * d2n;
    const double CEu2 = -PEunder * ff.povun8 * expovun8 * d8;
    const double CEu3 = CEu1 * (1.0 - dD * d1);
    const double CEu4 = CEu1 * dlp * ff.povun4 * expovun1 * (d1 * d1) + CEu2;
    double *c = ecoef + 6 * static_cast<size_t>(i);
    c[0] = CElp1; c[1] = CEo3; c[2] = CEo1; c[3] = CEu3; c[4] = CEo4; c[5] = CEu4;
  }
  block_energy_add(e2, pe + 2); block_energy_add(e3, pe + 3); block_energy_add(e4, pe + 4);
}

__global__ void __launch_bounds__(256) k_elnpr_bonds(int nb_res, DevFF ff, const int *__restrict__ bown, const int *__restrict__ nbr, const unsigned char *__restrict__ btype, const int *__restrict__ type,
                                                      const double *__restrict__ bo2, const double *__restrict__ bo3, const double *__restrict__ delta, const double *__restrict__ deltalp,
                                                      const double *__restrict__ dDlp, const double *__restrict__ ecoef,
                                                      double *__restrict__ cf1, double *__restrict__ cf2, double *__restrict__ cf3, double *__restrict__ cdn) {
  const int o = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (o >= nb_res) return;
  const int i = bown[o], j = nbr[o];
  const double *c = ecoef + 6 * static_cast<size_t>(i);
  const double CElp1 = c[0], CEo3 = c[1], CEo1 = c[2], CEu3 = c[3], CEo4 = c[4], CEu4 = c[5];
  const DevBondP bp = ff.bond[ff.inxn2[type[i] * ff.n1 + btype[o]]];
  const double bpp = bo2[o] + bo3[o], dj = delta[j] - deltalp[j], oneD = 1.0 - dDlp[j];
  const double CEo5 = CEo1 * bp.povun1 * bp.Desig;
  const double CElp_b = CElp1 + CEo3 + CEo5 + CEu3;
  const double CElp_bpp = CEo4 * dj + CEu4 * dj;
  cf1[o] += CElp_b; cf2[o] += CElp_bpp; cf3[o] += CElp_bpp;           // coeff = CElp_b + (0,bpp,bpp)
  cdn[o] = CEo4 * oneD * bpp + CEu4 * oneD * bpp;                      // cdbnd(j) += CElp_d (first writer: sets)
}

void Engine::bonded_energies() {
  double *pe_d = scal + SCAL_PE;   // 14 energy accumulators live behind the CG scalars
  k_ebond_terms<<<nblk(nbonds_res, 256), 256, 0, stream>>>(nbonds_res, dff, bown, nbr, btype, type, gid, bo0, bo1, bo2, bo3, delta, deltalp, cf1, cf2, cf3, ecoa, bt1, bt2, pe_d);
  k_elnpr_atoms<<<nblk(N, 256), 256, 0, stream>>>(N, dff, boff, type, bt1, bt2, delta, deltalp, dDlp, ecoef, pe_d);
  k_elnpr_bonds<<<nblk(nbonds_res, 256), 256, 0, stream>>>(nbonds_res, dff, bown, nbr, btype, type, bo2, bo3, delta, deltalp, dDlp, ecoef, cf1, cf2, cf3, cdn);
  { Timed kt3(this, &st.ms_k_e3b); valence_angles(); }
  { Timed kt4(this, &st.ms_k_e4b); torsions(); }
  { Timed kth(this, &st.ms_k_ehb); hydrogen_bonds(); }
}

}  // namespace rxmd
