// torsions.hip -- E4b, torsion + four-body conjugation of FORCE (reference src/pot.F90:980-1227): k_e4b, the delivery of its k-l side k_e4b_deliver,
// and Engine::torsions().  The accumulators the kernels add to are described at the head of bonded.hip.
#include "bonded_common.h"

#include <algorithm>
#include <type_traits>

namespace rxmd {

constexpr int E4B_SEG = ~(31 << 5);   // k_e4b queue key without its i1 field: (atom, centre bond, l)
// occupancy knob, measured on MI355X (bonded section of the step, ms): E4b at 2/3 workgroups per CU = 21.3/20.4 (before its LDS-atomic accumulators;
// with them 3 stays best: 15.2, at 4: 18.9)
#ifndef E4B_MINB
#define E4B_MINB 3
#endif
struct BoxImg { double H[9], Hi[9], L[3]; int ortho; int probe; };   // lattice vectors for the image test of the torsion's stress correction; probe: RXMD_EXPERIMENTS builds only (RXMD_E4B_PROBE: 1 = set-up only, 2 = phase B skipped, 5 = PE(8), PE(9) count batches and entries)
// Torsion + four-body conjugation.  The reference walks centre bonds j-k with gid(j) < gid(k) and scatters to i,j,k,l.
// Here ONE WAVEFRONT owns several consecutive centre atoms; every bond slot of an atom has a lane that owns its accumulators, and
// one more lane stands for the atom itself.  Four layouts (template LSL, chosen per step from the longest bond list, see
// Engine::torsions): two atoms x 32 lanes (any list, MAXNEIGHBS = 30), four atoms x 16 lanes, and the packed forms -- eight
// (lists <= 15) or four atoms with their lanes laid end to end.  More atoms per wavefront = fewer wavefronts that set up and
// enumerate, more of their lanes busy, fuller 64-lane batches (two RDX atoms queue 52 torsions: 1.38 batches per wavefront at 58 %
// of the lanes; eight atoms: 6.3 -> 3.9 ms).  Phase A enumerates every (k1,i1,l1) combination of the atoms, applies the reference's
// cheap bond-order cut-offs (pot.F90:1023,1044,1072,1078,1081) and compacts the survivors with a ballot into an LDS queue; phase B
// evaluates 64 surviving torsions at a time with every lane busy (only ~1 in 8 combinations survives in RDX).
// ONCE = false (until round 6): a torsion is visited from both ends: a lane books the energy, the j-k bond coefficient and the cdbnd
// terms only when gid(j) < gid(k) (the reference's orientation, which the index-ordered ccbnd rule depends on), the forces on i and j and
// the i-j bond coefficient always; the k/l side is booked when atom k is the centre.  Per-bond sums are formed by each
// evaluating lane adding its results to the (atom, slot) accumulators in LDS (ds_add_f64): no global atomics, and the order of the
// additions is fixed by the queue order and the lane order inside one LDS instruction.
// ONCE = true (default since round 6): only the centre bonds with gid(j) < gid(k) are enumerated -- the reference's loop, pot.F90:1021 -- and a
// visit books all four atoms: i, j and the centre bond as before, the force on k into the slot of k (k IS a neighbour of j), and the k-l side
// (ForceB coefficient of bond k-l, force on l), which belongs to a bond slot of ANOTHER wavefront's atom, through a delivery table: the queue runs
// with i fastest, so the torsions of one (centre bond, l) are neighbouring lanes; a batch is cut where such a run ends, the run's sum is formed by
// a fixed shuffle tree, and its first lane stores it at [bond (k, l1)][slot of j in the list of k] with a flag byte.  k_e4b_deliver then adds
// the flagged columns of every bond in slot order: no atomics, the same bits run to run.  Half the enumeration, 12.9 instead of 25.8
// evaluations per atom (RDX), no stress correction (all four forces are booked in the frame of j, as in the reference).
template <int LSL, bool ONCE, int WPB>
__global__ void __launch_bounds__(64 * WPB, E4B_MINB) k_e4b(int N, DevFF ff, const int *__restrict__ boff, const int *__restrict__ nbr, const unsigned char *__restrict__ btype, const int *__restrict__ nbrcnt, const int *__restrict__ type,
                                              const long long *__restrict__ gid, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                              const double *__restrict__ bo0, const double *__restrict__ bo2, const double *__restrict__ delta,
                                              const double *__restrict__ etor, const double *__restrict__ econ,
                                              double *__restrict__ cf1, double *__restrict__ cf2, double *__restrict__ cdn,
                                              double *__restrict__ fnx, double *__restrict__ fny, double *__restrict__ fnz,
                                              double *__restrict__ cds, double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz, double *__restrict__ pe, BoxImg bx,
                                              const int *__restrict__ brev, double4 *__restrict__ tkl, unsigned char *__restrict__ tflag, int TW, int VB) {
  // per (atom g, slot): the bond as seen from the centre
  __shared__ double s_bo[WPB][64], s_et[WPB][64], s_ec[WPB][64], s_rx[WPB][64], s_ry[WPB][64], s_rz[WPB][64], s_rn[WPB][64];
  __shared__ int s_nb[WPB][64], s_meta[WPB][64];     // s_meta: type of the neighbour | its bond count << 8 | "this centre owns the bond" << 16
  __shared__ int s_bofn[WPB][64];                  // first bond (CSR offset) of the neighbour in this slot: its list is bonds s_bofn .. + count
  // per (atom g, slot) as CENTRE bond k1: factors shared by all torsions around it; a bond count of 0 marks "no torsion through this bond"
  __shared__ double s_btb2[WPB][64], s_dfn11[WPB][64];
  __shared__ int s_q[WPB][128];                    // queue of surviving combinations: g<<15 | k1<<10 | i1<<5 | l1
  __shared__ int s_ql[WPB][128]; __shared__ unsigned short s_qx[WPB][128];     // ... with atom l and the torsion row of (i, j, k, l): phase A has both at hand (round 5: phase B fetched them again, four dependent round trips in front of its arithmetic)
  // phase A walks only bonds above the cut-off: the slots of each centre atom that qualify, and per centre bond the qualifying slots
  // of k with what the filter needs of them (bond order, atom l, its type) -- staged once per centre bond by the lanes side by side
  __shared__ int s_cap[WPB][64], s_capl[WPB][64], s_ll[WPB][64], s_tl[WPB][64], s_gj[WPB][8][2];   // s_gj: bond count and type of each centre atom
  __shared__ int s_cb[WPB][64];                    // the centre bonds of the pass: atom << 8 | lane of the slot
  __shared__ int s_cd[WPB][4][9];                  // per centre bond of a round: atom, lane, first lane of the atom, type of j, k, j, number of qualifying k-slots, 1/that, combinations
  __shared__ int s_base[WPB][9];                   // LSL == 0: first lane of each atom of the pass, and the end
  __shared__ double s_bokl[WPB][64];
  // per (atom g, slot) accumulators, updated with LDS atomics by the lanes that evaluate torsions: [0] cf1 and [1..3] force of the
  // i-j bond / its neighbour, [4] cf1, [5] cf2, [6] cdbnd of the centre bond; slot 31 (never a bond) holds the centre atom's own
  // force in [1..3] and cdbnd in [6].  (An earlier version wrote 11 results per torsion to LDS and let every owner lane scan all 64
  // of them: that scan cost about as many instructions as the torsion itself.)
  __shared__ double s_acc[WPB][64][7];
  // LSL = 5 / 4: two / four atoms with a fixed range of 32 / 16 lanes each.  LSL = 0 / 1 ("packed"): eight atoms with lists <= 15 /
  // four atoms with any list, each with as many lanes as it has bonds plus one, laid end to end -- RDX atoms have 5.3 bonds on
  // average, so the set-up and the enumeration run with most lanes busy instead of a third; the few groups that need more than 64
  // lanes (one group of eight in twenty in the RDX crystal) are done in two passes of half the atoms each.
  constexpr bool PACK = (LSL <= 1);
  constexpr int PKN = (LSL == 0) ? 8 : 4, CAP = (LSL == 0) ? 15 : 31;                          // packed: atoms per wavefront, longest list
  constexpr int SL = PACK ? CAP + 1 : (1 << (LSL & 31)), NG = PACK ? PKN : (64 >> (LSL & 31));  // (widest) lane range of an atom, atoms per wavefront
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));   // wave-uniform -> scalar registers
  // "is there a torsion row for these four types" (pot.F90:1078) as a bit table in LDS when the ffield has at most 7 atom types
  // (n1^4 <= 4096 bits): the enumeration asks it for every candidate, and a look-up in global memory is a dependent round trip
  // per centre bond
  extern __shared__ unsigned char s_tor[];        // the torsion row of every type quadruple (0: none), n1^4 <= 4096 entries of a force field with at most 255 rows (dynamic: e4b_tor_bytes)
  const bool tor_lds = ff.n1 <= 8 && ff.ntoty <= 255;
  if (tor_lds) {
    const int n4 = ff.n1 * ff.n1 * ff.n1 * ff.n1;
    for (int t = threadIdx.x; t < n4; t += 64 * WPB) s_tor[t] = static_cast<unsigned char>(ff.inxn4[t]);
    __syncthreads();
  }
  double e8 = 0.0, e9 = 0.0;                      // energies: per evaluating lane, summed over the wave at the end
  // The grid may be smaller than the number of atom groups (persistent: as many workgroups as fit the device at once, each walking every
  // gridDim.x-th group): a group is a "virtual workgroup" vb of VB; the XCD-aware order is that of the full grid (gridDim.x is a multiple of 8, so a
  // workgroup stays on the eighth of the atoms its XCD owns).
  for (int vb = blockIdx.x; vb < VB; vb += gridDim.x) {
  const int jbase = (xcd_swizzle(vb, VB) * WPB + w) * NG;
  if (jbase >= N) continue;                      // whole wavefront skips together; no block-level barrier below
  int npass = 1, c_me = 0, cpre = 0;
  // (round 6) packed forms: what the slot lanes need of their centre atom -- first bond, type, position, delta, global id -- is loaded by the atom's lane
  // WITH the bond count and handed over through LDS -- rows 0..7 of the slot accumulators, which the set-up clears only after it has read them --: one round
  // trip less in front of the bond data than loading it by j_me once the lanes are laid out (the rare second pass of a group loads it that way)
  if (PACK) {                                     // lanes 0..PKN-1: lanes the atom needs, inclusive prefix
    if (lane < PKN && jbase + lane < N) {
      const int ja = jbase + lane;
      c_me = min(nbrcnt[ja], CAP) + 1;
      s_acc[w][lane][0] = x[ja]; s_acc[w][lane][1] = y[ja]; s_acc[w][lane][2] = z[ja]; s_acc[w][lane][3] = delta[ja];
      s_acc[w][lane][4] = __longlong_as_double(gid[ja]); s_acc[w][lane][5] = __hiloint2double(boff[ja], type[ja]);
    }
    cpre = c_me;
#pragma unroll
    for (int o = 1; o < PKN; o <<= 1) { const int t = __shfl_up(cpre, o, 64); if (lane >= o) cpre += t; }
    npass = (__shfl(cpre, PKN - 1, 64) <= 64) ? 1 : 2;
  }
  auto gbase = [&](int g) { return PACK ? s_base[w][g] : (g << (LSL & 31)); };       // first lane of atom g of this pass
  for (int pass = 0; pass < npass; ++pass) {
  const int g0 = PACK ? (npass == 1 ? 0 : (PKN / 2) * pass) : 0, ng = PACK ? (npass == 1 ? PKN : PKN / 2) : NG;   // atoms of this pass
  int g_me, sl_me, nj_me, j_me;
  bool has_me;
  if (PACK) {
    const int off0 = __shfl(cpre - c_me, g0, 64);
    if (lane >= g0 && lane < g0 + ng) {
      s_base[w][lane - g0] = cpre - c_me - off0;
      s_gj[w][lane - g0][0] = max(c_me - 1, 0); s_gj[w][lane - g0][1] = 1;   // (an atom behind the last one has no lane to write these)
    }
    if (lane == g0 + ng - 1) s_base[w][ng] = cpre - off0;
    wave_lds_sync();
    g_me = 0;
    for (int g = 1; g < ng; ++g) g_me += (lane >= s_base[w][g]) ? 1 : 0;
    has_me = lane < s_base[w][ng];
    sl_me = has_me ? lane - s_base[w][g_me] : 1;
    nj_me = has_me ? s_base[w][g_me + 1] - s_base[w][g_me] - 1 : 0;
    j_me = jbase + g0 + g_me;
  } else {
    g_me = lane >> (LSL & 31); sl_me = lane & (SL - 1);
    j_me = jbase + g_me;
    has_me = j_me < N;
    nj_me = has_me ? min(nbrcnt[j_me], SL - 1) : 0;
  }
  const bool self_me = has_me && (PACK ? sl_me == nj_me : sl_me == SL - 1);   // the lane that stands for the atom itself (never a bond)
  int tj_me, ob_me; double xj_me, yj_me, zj_me, dj_me; long long gj_me;
  if (PACK && pass == 0) {                        // (behind the wave_lds_sync of the lane layout above)
    const int src = g0 + g_me;
    const double ot = s_acc[w][src][5];
    tj_me = has_me ? __double2loint(ot) : 1; ob_me = has_me ? __double2hiint(ot) : 0;
    xj_me = s_acc[w][src][0]; yj_me = s_acc[w][src][1]; zj_me = s_acc[w][src][2]; dj_me = s_acc[w][src][3]; gj_me = __double_as_longlong(s_acc[w][src][4]);
  } else {
    tj_me = has_me ? type[j_me] : 1;
    xj_me = has_me ? x[j_me] : 0.0; yj_me = has_me ? y[j_me] : 0.0; zj_me = has_me ? z[j_me] : 0.0;
    ob_me = has_me ? boff[j_me] : 0;              // bonds of an atom are consecutive (CSR): the lanes of this wavefront read consecutive addresses
    dj_me = has_me ? delta[j_me] : 0.0; gj_me = has_me ? gid[j_me] : 0;
  }
  s_meta[w][lane] = 0;
  bool cap_me = false, cb_me = false;              // this slot qualifies as an i / as a centre bond of this wavefront (ONCE: only in the reference's orientation gid(j) < gid(k))
  if (sl_me < nj_me) {
    const int o = ob_me + sl_me;
    const int i = nbr[o], ti = btype[o];
    const double rx = x[i] - xj_me, ry = y[i] - yj_me, rz = z[i] - zj_me;      // r_i - r_j
    const double b = bo0[o];
    // what a centre bond needs of its far end and of the bond, requested with the rest and not behind the test of the bond order (one round trip less)
    const double d_i = delta[i], b2_o = bo2[o]; const long long g_i = gid[i]; const int bi = boff[i], nc_i = nbrcnt[i], br_o = ONCE ? brev[o] : 0;
    cap_me = b > cutof2_esub;
    s_nb[w][lane] = i;
    int meta = ti;
    s_bo[w][lane] = b; s_et[w][lane] = etor[o]; s_ec[w][lane] = econ[o];
    s_rx[w][lane] = rx; s_ry[w][lane] = ry; s_rz[w][lane] = rz; s_rn[w][lane] = sqrt(rx * rx + ry * ry + rz * rz);
    if (b > cutof2_esub) {                       // this slot as a centre bond j-k (pot.F90:1023)
      const DevAtomP aj = ff.atom[tj_me];
      const double delta_ang_jk = (dj_me + aj.Val - aj.Valangle) + (d_i + ff.atom[ti].Val - ff.atom[ti].Valangle);
      const double exp_tor3 = exp(-ff.ptor3 * delta_ang_jk), exp_tor4 = exp(ff.ptor4 * delta_ang_jk);
      const double exp_tor34_i = 1.0 / (1.0 + exp_tor3 + exp_tor4);
      const double fn11 = (2.0 + exp_tor3) * exp_tor34_i;
      s_dfn11[w][lane] = (-ff.ptor3 * exp_tor3 + (ff.ptor3 * exp_tor3 - ff.ptor4 * exp_tor4) * (2.0 + exp_tor3) * exp_tor34_i) * exp_tor34_i;
      s_btb2[w][lane] = 2.0 - b2_o - fn11;
      const bool own = gj_me < g_i;
      meta |= (min(nc_i, 255) << 8) | (own ? 1 << 16 : 0);
      s_bofn[w][lane] = bi;
      if (ONCE) { meta |= (br_o - bi) << 17; cb_me = own; }   // the slot of j in the list of k (< MAXNEIGHBS = 30): where the k-l side of this centre bond is delivered
      else cb_me = true;
    }
    s_meta[w][lane] = meta;
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) s_acc[w][lane][c] = 0.0;
  const unsigned long long capmask = __ballot(cap_me);
  {                                               // the qualifying slots of each centre atom, in slot order
    const int gb_me = gbase(g_me);
    const unsigned mine = static_cast<unsigned>(capmask >> gb_me) & ((SL == 32) ? 0xffffffffu : ((1u << (SL & 31)) - 1u));   // (bits of the next atom above sl_me do not matter)
    if (cap_me) s_cap[w][gb_me + __popc(mine & ((1u << sl_me) - 1u))] = sl_me;
    if (sl_me == 0 && (has_me || !PACK)) { s_gj[w][g_me][0] = nj_me; s_gj[w][g_me][1] = tj_me; }
  }
  wave_lds_sync();
  int qn = 0, qh = 0;                             // entries in the queue; its head (ONCE: a ring of 128, otherwise always 0)

  auto evaluate = [&](int cnt) {                  // phase B: the first cnt (<= 64) queue entries, one per lane
    if (exp_probe(bx.probe, 2)) return;
    if (exp_probe(bx.probe, 5)) { if (lane == 0) { atomicAdd(pe + 8, 1.0); atomicAdd(pe + 9, static_cast<double>(cnt)); } return; }
    const bool once_math = ONCE && !exp_probe(bx.probe, 7);   // probe 7: the one-visit enumeration with the arithmetic of a two-visit evaluation (timing only)
    double o[7] = {0, 0, 0, 0, 0, 0, 0};
    V3 fself = {0.0, 0.0, 0.0};
    V3 fkk = {0.0, 0.0, 0.0}, fll = {0.0, 0.0, 0.0};   // ONCE: forces on k and on l
    double c3kl = 0.0;                                 // ONCE: ForceB(k-l, C4body_b(3)), pot.F90:1197-1198
    double cd_self = 0.0;
    int key = -1;
    if (lane < cnt) {
      key = s_q[w][(qh + lane) & 127];
      const int g = key >> 15, k1 = (key >> 10) & 31, i1 = (key >> 5) & 31, l1 = key & 31;
      const int gb = gbase(g);
      const int sk = gb + k1, si = gb + i1;
      const int k = s_nb[w][sk], mk_ = s_meta[w][sk], tk = mk_ & 255, tj = s_gj[w][g][1];
      const double BOjk_f = s_bo[w][sk], BOij_f = s_bo[w][si];
      const double BOjk = BOjk_f - cutof2_esub, BOij = BOij_f - cutof2_esub;
      const bool own = ONCE || (mk_ >> 16) != 0;
      const int ol = s_bofn[w][sk] + l1;
      const int l = s_ql[w][(qh + lane) & 127];
      const DevTorsP tp = ff.tors[s_qx[w][(qh + lane) & 127]];
      (void)tj; (void)tk;
      const V3 rjk = {-s_rx[w][sk], -s_ry[w][sk], -s_rz[w][sk]};          // r_j - r_k
      const double njk = s_rn[w][sk];
      const V3 rij = {s_rx[w][si], s_ry[w][si], s_rz[w][si]};
      const double nij = s_rn[w][si];
      const V3 rkl = {x[k] - x[l], y[k] - y[l], z[k] - z[l]};                 // r_k - r_l
      const double nkl = sqrt(dot(rkl, rkl));
      const double inij = 1.0 / nij, injk = 1.0 / njk, inkl = 1.0 / nkl;
      double cos_ijk = -dot(rij, rjk) * (inij * injk);
      if (cos_ijk > MAXANGLE) cos_ijk = MAXANGLE;
      if (cos_ijk < MINANGLE) cos_ijk = MINANGLE;
      const double sin_ijk = sqrt((1.0 - cos_ijk) * (1.0 + cos_ijk));       // sin(acos(c))
      const double tan_ijk_i = cos_ijk / sin_ijk;                            // 1/tan(theta)
      // cross_product(rij, rjk) and (rjk, rkl), pot.F90:1524-1543
      const V3 n1v = {rij.x * inij, rij.y * inij, rij.z * inij}, n2v = {rjk.x * injk, rjk.y * injk, rjk.z * injk}, n3v = {rkl.x * inkl, rkl.y * inkl, rkl.z * inkl};
      const V3 c1v = {n1v.y * n2v.z - n1v.z * n2v.y, n1v.z * n2v.x - n1v.x * n2v.z, n1v.x * n2v.y - n1v.y * n2v.x};
      const V3 c2v = {n2v.y * n3v.z - n2v.z * n3v.y, n2v.z * n3v.x - n2v.x * n3v.z, n2v.x * n3v.y - n2v.y * n3v.x};
      double nc1 = sqrt(dot(c1v, c1v)), nc2 = sqrt(dot(c2v, c2v));
      if (nc1 < NSMALL) nc1 = NSMALL;
      if (nc2 < NSMALL) nc2 = NSMALL;
      const double BOkl = bo0[ol] - cutof2_esub; (void)BOkl;
      const double et1 = s_et[w][si], et2 = s_et[w][sk], et3 = etor[ol];
      const double fn10 = (1.0 - et1) * (1.0 - et2) * (1.0 - et3);
      const double fn12 = s_ec[w][si] * s_ec[w][sk] * econ[ol];
      const double btb2 = s_btb2[w][sk];
      const double exp_tor1 = exp(tp.ptor1 * (btb2 * btb2));
      double cos_jkl = -dot(rjk, rkl) * (injk * inkl);
      if (cos_jkl > MAXANGLE) cos_jkl = MAXANGLE;
      if (cos_jkl < MINANGLE) cos_jkl = MINANGLE;
      const double sin_jkl = sqrt((1.0 - cos_jkl) * (1.0 + cos_jkl));
      const double tan_jkl_i = cos_jkl / sin_jkl;
      double c1 = dot(c1v, c2v) / (nc1 * nc2);
      if (c1 > MAXANGLE) c1 = MAXANGLE;
      if (c1 < MINANGLE) c1 = MINANGLE;
      const double c1sq = c1 * c1;
      const double cos_2w = 2.0 * c1sq - 1.0;                               // cos(2 acos c)
      const double c2 = 1.0 - cos_2w, c3 = 1.0 + (4.0 * c1sq - 3.0) * c1;   // 1 + cos(3 acos c)
      const double vsum = tp.V1 * (1.0 + c1) + tp.V2 * exp_tor1 * c2 + tp.V3 * c3;
      const double ss = sin_ijk * sin_jkl;
      const double PEconj = tp.pcot1 * fn12 * (1.0 + (c1sq - 1.0) * ss);
      if (own) { e8 += 0.5 * fn10 * ss * vsum; e9 += PEconj; }
      const double CEt1 = 0.5 * ss * vsum;
      const double CEt2 = -tp.ptor1 * fn10 * ss * tp.V2 * exp_tor1 * btb2 * c2;
      const double CEt3 = CEt2 * s_dfn11[w][sk];
      const double CEt4 = CEt1 * ff.ptor2 * et1 * (1.0 - et2) * (1.0 - et3);
      const double CEt5 = CEt1 * ff.ptor2 * (1.0 - et1) * et2 * (1.0 - et3);
      const double cmn = -0.5 * fn10 * vsum;
      const double CEt7 = cmn * sin_jkl * tan_ijk_i, CEt8 = cmn * sin_ijk * tan_jkl_i;
      const double CEt9 = fn10 * ss * (0.5 * tp.V1 - 2.0 * tp.V2 * exp_tor1 * c1 + 1.5 * tp.V3 * (cos_2w + 2.0 * c1sq));
      const double Cconj = -2.0 * ff.pcot2 * PEconj;
      const double CEc1 = Cconj * (BOij - 1.5), CEc2 = Cconj * (BOjk - 1.5);
      if (once_math) c3kl = Cconj * (BOkl - 1.5) + CEt1 * ff.ptor2 * (1.0 - et1) * (1.0 - et2) * et3;    // CEconj(3) + CEtors(6)
      const double CEc4 = -tp.pcot1 * fn12 * (c1sq - 1.0) * tan_ijk_i * sin_jkl;
      const double CEc5 = -tp.pcot1 * fn12 * (c1sq - 1.0) * sin_ijk * tan_jkl_i;
      const double CEc6 = 2.0 * tp.pcot1 * fn12 * c1 * ss;
      o[0] = CEc1 + CEt4;                                                   // ForceB(i-j, C4body_b(1)), pot.F90:1185-1186
      if (own) { o[4] = CEc2 + CEt5; o[5] = CEt2; o[6] = CEt3; if (!once_math) cd_self += CEt3; }   // pot.F90:1178-1194 (one visit: the centre's own cdbnd is the sum of its slots' terms, formed at the end)
      // angle i-j-k (coefficient C4body_a(1)): forces on i and j
      V3 fi, fk;
      angle_forces(CEc4 + CEt7, rij, nij, rjk, njk, fi, fk);
      o[1] = fi.x; o[2] = fi.y; o[3] = fi.z;
      if (once_math) fkk = fk;                                               // (one visit: the force on j is minus the sum of the other three, formed at the end)
      else { fself.x -= fi.x + fk.x; fself.y -= fi.y + fk.y; fself.z -= fi.z + fk.z; }
      // angle j-k-l (coefficient C4body_a(2)): j is the first atom
      V3 fj2, fl2;
      angle_forces(CEc5 + CEt8, rjk, njk, rkl, nkl, fj2, fl2);
      if (once_math) { fkk.x -= fj2.x + fl2.x; fkk.y -= fj2.y + fl2.y; fkk.z -= fj2.z + fl2.z; fll = fl2; }
      else { fself.x += fj2.x; fself.y += fj2.y; fself.z += fj2.z; }
      // dihedral (ForceA4, pot.F90:1369-1459): forces on i (fij) and j (-fij + fjk)
      {
        const double coeff = CEc6 + CEt9;
        const double C00 = nij * nij, C01 = dot(rij, rjk), C02 = dot(rij, rkl), C11 = njk * njk, C12 = dot(rjk, rkl), C22 = nkl * nkl;
        const double D0 = C00 * C11 - C01 * C01, Dm1 = C11 * C22 - C12 * C12;
        const double coDD = coeff * (1.0 / sqrt(D0 * Dm1));
        const double com = C01 * C12 - C02 * C11;
        const double cD0 = com / D0, cDm = com / Dm1;
        const double Cwi1 = C11 * cD0, Cwi2 = -(C12 + C01 * cD0), Cwi3 = C11;
        const double Cwj1 = -(C12 + (C11 + C01) * cD0);
        const double Cwj2 = -(-C12 - 2 * C02 - C22 * cDm - (C00 + C01) * cD0);
        const double Cwj3 = -(C01 + C11 + C12 * cDm);
        const V3 fij = {coDD * (Cwi1 * rij.x + Cwi2 * rjk.x + Cwi3 * rkl.x), coDD * (Cwi1 * rij.y + Cwi2 * rjk.y + Cwi3 * rkl.y),
                        coDD * (Cwi1 * rij.z + Cwi2 * rjk.z + Cwi3 * rkl.z)};
        const V3 fjk = {coDD * ((Cwj1 + Cwi1) * rij.x + (Cwj2 + Cwi2) * rjk.x + (Cwj3 + Cwi3) * rkl.x),
                        coDD * ((Cwj1 + Cwi1) * rij.y + (Cwj2 + Cwi2) * rjk.y + (Cwj3 + Cwi3) * rkl.y),
                        coDD * ((Cwj1 + Cwi1) * rij.z + (Cwj2 + Cwi2) * rjk.z + (Cwj3 + Cwi3) * rkl.z)};
        o[1] += fij.x; o[2] += fij.y; o[3] += fij.z;
        if (!once_math) { fself.x += -fij.x + fjk.x; fself.y += -fij.y + fjk.y; fself.z += -fij.z + fjk.z; }
        if (once_math) {                                                     // k gets -fjk + fkl, l gets -fkl (pot.F90:1417-1452)
          const double Cwl2 = C01 + C12 * cDm, Cwl3 = -(C11 * cDm);         // Cwl1 = -C11
          const V3 fkl = {-coDD * (-C11 * rij.x + Cwl2 * rjk.x + Cwl3 * rkl.x), -coDD * (-C11 * rij.y + Cwl2 * rjk.y + Cwl3 * rkl.y),
                          -coDD * (-C11 * rij.z + Cwl2 * rjk.z + Cwl3 * rkl.z)};
          fkk.x += -fjk.x + fkl.x; fkk.y += -fjk.y + fkl.y; fkk.z += -fjk.z + fkl.z;
          fll.x -= fkl.x; fll.y -= fkl.y; fll.z -= fkl.z;
        }
      }
      // stress: this visit books f_i and f_j in the frame of centre j; f_k and f_l are booked by the visit whose centre is the
      // OWNER of k.  When k is an image beyond the periodic box that owner sits one lattice vector T away, and the virial
      // sum_a pos_a f_a (pot.F90:65-72) would hold T (f_k + f_l) = -T (f_i + f_j) too much.  The owner's visit sees j as an
      // image at -T and finds the same product, so each of the two visits takes out half (rare lanes only).
      if (!ONCE) {
        const double xk = x[k], yk = y[k], zk = z[k];
        // k is bonded to a resident: it lies inside the box or in the first image layer, so comparisons name the lattice vector
        // (floor(x / L) costs three FP64 divisions per torsion)
        double t0, t1, t2;
        if (bx.ortho) {
          t0 = xk < 0.0 ? bx.L[0] : (xk >= bx.L[0] ? -bx.L[0] : 0.0); t1 = yk < 0.0 ? bx.L[1] : (yk >= bx.L[1] ? -bx.L[1] : 0.0);
          t2 = zk < 0.0 ? bx.L[2] : (zk >= bx.L[2] ? -bx.L[2] : 0.0);
        } else {                                   // skewed box: which lattice vectors bring k home, from its normalised coordinates
          const double n0 = -floor(bx.Hi[0] * xk + bx.Hi[1] * yk + bx.Hi[2] * zk), n1 = -floor(bx.Hi[3] * xk + bx.Hi[4] * yk + bx.Hi[5] * zk),
                       n2 = -floor(bx.Hi[6] * xk + bx.Hi[7] * yk + bx.Hi[8] * zk);
          t0 = bx.H[0] * n0 + bx.H[1] * n1 + bx.H[2] * n2; t1 = bx.H[3] * n0 + bx.H[4] * n1 + bx.H[5] * n2; t2 = bx.H[6] * n0 + bx.H[7] * n1 + bx.H[8] * n2;
        }
        if (t0 != 0.0 || t1 != 0.0 || t2 != 0.0) {
          const double F0 = 0.5 * (o[1] + fself.x), F1 = 0.5 * (o[2] + fself.y), F2 = 0.5 * (o[3] + fself.z);
          static_assert(SCAL_ASTR == SCAL_PE + 16, "pe = scal + SCAL_PE: the stress accumulators astr are pe + 16 .. pe + 21");
          if (t0 != 0.0) { atomicAdd(pe + 16, t0 * F0); atomicAdd(pe + 21, t0 * F1); }     // xx, xy
          if (t1 != 0.0) { atomicAdd(pe + 17, t1 * F1); atomicAdd(pe + 19, t1 * F2); }     // yy, yz
          if (t2 != 0.0) { atomicAdd(pe + 18, t2 * F2); atomicAdd(pe + 20, t2 * F0); }     // zz, zx
        }
      }
    }
    if (ONCE && !exp_probe(bx.probe, 3) && !exp_probe(bx.probe, 7)) {
      // the k-l side: C4body_b(3) and the force on l, summed over the i of one (centre bond, l) run -- neighbouring lanes of this batch (a fixed
      // tree: the same bits run to run) -- and stored ONCE by the run's first lane where the bond k-l finds it: row = bond (k, l1), column = the
      // slot of j in the list of k.  k_e4b_deliver adds the columns of a row in slot order.
      const int seg = (key >= 0) ? (key & E4B_SEG) : (-1 - lane);
      for (int d = 1; d < 32; d <<= 1) {
        const int sd = __shfl_down(seg, d, 64);                              // (every lane takes part in the exchange: no short circuit in front of it)
        const bool same = (lane + d < 64) && sd == seg;
        if (__ballot(same) == 0ULL) break;                                  // runs are contiguous: none at this distance, none beyond
        const double u0 = __shfl_down(c3kl, d, 64), u1 = __shfl_down(fll.x, d, 64), u2 = __shfl_down(fll.y, d, 64), u3 = __shfl_down(fll.z, d, 64);
        if (same) { c3kl += u0; fll.x += u1; fll.y += u2; fll.z += u3; }
      }
      const int segup = __shfl_up(seg, 1, 64);
      if (key >= 0 && (lane == 0 || segup != seg)) {
        const int g = key >> 15, sk = gbase(g) + ((key >> 10) & 31);
        const size_t ti = static_cast<size_t>(s_bofn[w][sk] + (key & 31)) * TW + ((s_meta[w][sk] >> 17) & 31);
        if (!exp_probe(bx.probe, 6)) {   // (written once, read once by another kernel: past the L2's write-allocate)
          typedef double d4v __attribute__((ext_vector_type(4)));
          d4v tv; tv.x = c3kl; tv.y = fll.x; tv.z = fll.y; tv.w = fll.z;
          __builtin_nontemporal_store(tv, reinterpret_cast<d4v *>(tkl) + ti);
          __builtin_nontemporal_store(static_cast<unsigned char>(1), tflag + ti);
        }
        // the centre atom's own force is minus the sum of the three others of every torsion: the l part once per run, here; the i and k parts from
        // the slot accumulators at the end (four LDS atomics per lane less, the ones with the most lanes per address)
        double *as = &s_acc[w][PACK ? s_base[w][g + 1] - 1 : gbase(g) + SL - 1][0];
        atomicAdd(as + 1, -fll.x); atomicAdd(as + 2, -fll.y); atomicAdd(as + 3, -fll.z);
      }
    }
    if (exp_probe(bx.probe, 4)) { if (o[0] + o[1] + o[2] + o[3] + o[4] + o[5] + o[6] + fkk.x + fkk.y + fkk.z + fself.x + fself.y + fself.z + cd_self + c3kl + fll.x == 1.2345e300) e8 += 1.0; key = -1; }
    if (key >= 0) {
      const int g = key >> 15, k1 = (key >> 10) & 31, i1 = (key >> 5) & 31;
      const int gb = gbase(g), gself = PACK ? s_base[w][g + 1] - 1 : gb + SL - 1;
      double *ai = &s_acc[w][gb + i1][0], *ak = &s_acc[w][gb + k1][0], *as = &s_acc[w][gself][0];
      atomicAdd(ai + 0, o[0]); atomicAdd(ai + 1, o[1]); atomicAdd(ai + 2, o[2]); atomicAdd(ai + 3, o[3]);
      atomicAdd(ak + 4, o[4]); atomicAdd(ak + 5, o[5]); atomicAdd(ak + 6, o[6]);
      if (once_math) { atomicAdd(ak + 1, fkk.x); atomicAdd(ak + 2, fkk.y); atomicAdd(ak + 3, fkk.z); }     // k is the neighbour in slot k1: its force rides where f_i does
      if (!once_math) { atomicAdd(as + 1, fself.x); atomicAdd(as + 2, fself.y); atomicAdd(as + 3, fself.z); atomicAdd(as + 6, cd_self); }
    }
    wave_lds_sync();
  };

  if (exp_probe(bx.probe, 1)) break;              // timing experiment: set-up only
  // phase A: enumerate, filter, compact.  The centre bonds of the pass (every slot above the cut-off, in (atom, slot) order) are taken
  // CPB at a time: the lanes stage the qualifying slots of their k atoms (pot.F90:1072: bond order, atom l, its type -- three
  // dependent loads) side by side, KW lanes per centre bond, so that a wavefront of eight atoms with ~40 centre bonds waits for ~10
  // such rounds instead of 40 (one centre bond at a time: set-up + enumeration 2.43 ms of the 3.96 ms kernel); the enumeration of a
  // centre bond then reads LDS only.
  constexpr int KW = (LSL == 5 || LSL == 1) ? 32 : 16, CPB = 64 / KW;   // lanes per centre bond (longest list of any atom + 1), centre bonds per round
  const unsigned long long cbmask = ONCE ? __ballot(cb_me) : capmask;
  const int ncb = __popcll(cbmask);
  if (cb_me) { const int r = __popcll(cbmask & ((1ULL << lane) - 1ULL)); s_cb[w][r] = (g_me << 8) | lane; }
  wave_lds_sync();
  // The k-side list of a round -- bond order, atom l and its type of every slot of k, KW lanes per centre bond -- is requested ONE ROUND AHEAD into
  // three registers (round 6): all three loads at once, whatever the bond order turns out to be, and behind them the enumeration and evaluation of the
  // round before.  (Until then: the bond order, then -- for the slots above the cut-off -- l and its type: two dependent round trips at the head of
  // every round, ~10 rounds per wavefront.)
  double nx_bl = 0.0; int nx_l = 0, nx_tl = 0;
  auto fetch_round = [&](int r0) {
    const int cbl = lane / KW, ks = lane % KW, r = r0 + cbl;
    nx_bl = 0.0; nx_l = 0; nx_tl = 0;
    if (r < ncb) {
      const int sk = s_cb[w][r] & 255;
      const int bk = s_bofn[w][sk];                 // first bond of atom k (the far end of centre bond r): its slots are bonds bk, bk + 1, ...
      if (ks < min((s_meta[w][sk] >> 8) & 255, KW == 32 ? WSLOT : KW)) { nx_bl = bo0[bk + ks]; nx_l = nbr[bk + ks]; nx_tl = btype[bk + ks]; }
    }
  };
  fetch_round(0);
  for (int r0 = 0; r0 < ncb; r0 += CPB) {
    unsigned long long ml;
    {
      const int cbl = lane / KW, ks = lane % KW;
      const double bl = nx_bl; const int l = nx_l, tl = nx_tl;
      if (r0 + CPB < ncb) fetch_round(r0 + CPB);
      // a slot of k stays in the round's list only if it can be the k-l bond of THIS centre bond: above the cut-off, BO(j,k) BO(k,l) above it, l not j
      // (pot.F90:1072,1081 -- tests that do not depend on i: applied here, once per slot, instead of once per (i, l) combination)
      bool capl = bl > cutof2_esub;
      if (r0 + cbl < ncb) {
        const int ent = s_cb[w][r0 + cbl];
        capl = capl && (s_bo[w][ent & 255] * bl > cutof2_esub) && (l != jbase + g0 + (ent >> 8));
      }
      ml = __ballot(capl);
      if (capl) {
        const unsigned sub = static_cast<unsigned>(ml >> (cbl * KW)) & ((KW == 32) ? 0xffffffffu : 0xffffu);
        const int pos = cbl * KW + __popc(sub & ((1u << ks) - 1u));
        s_capl[w][pos] = ks; s_bokl[w][pos] = bl; s_ll[w][pos] = l; s_tl[w][pos] = tl;
      }
    }
    // what the combinations of each centre bond of the round need, written by lanes 0..CPB-1: the combinations of all of them are
    // then enumerated together, 64 at a time (a centre bond of RDX has ~25: one pass per centre bond left most lanes idle)
    if (lane < CPB) {
      int T = 0;
      if (r0 + lane < ncb) {
        const int ent = s_cb[w][r0 + lane];
        const int g = ent >> 8, sk = ent & 255, gb = gbase(g), nj = s_gj[w][g][0];
        const int gw = PACK ? nj + 1 : SL;                                  // lanes of this atom
        const int ncj = __popc(static_cast<unsigned>(capmask >> gb) & ((gw == 32) ? 0xffffffffu : ((1u << (gw & 31)) - 1u)));
        const int nck = __popc(static_cast<unsigned>(ml >> (lane * KW)) & ((KW == 32) ? 0xffffffffu : 0xffffu));
        int *d = &s_cd[w][lane][0];
        // the index that runs fastest (probe 8: one-visit enumeration in the two-visit order, batches of 64, timing only): l (two visits) / i (one visit: the torsions of one (centre bond, l) are neighbours in the queue)
        const int dv = (ONCE && !exp_probe(bx.probe, 8)) ? ncj : nck;
        d[0] = g; d[1] = sk; d[2] = gb; d[3] = s_gj[w][g][1]; d[4] = s_nb[w][sk]; d[5] = jbase + g0 + g; d[6] = dv;
        d[7] = __float_as_int(1.0f / static_cast<float>(max(dv, 1)));      // c / dv for c < 1024, dv <= 31: exact through (c + 0.5) * (1 / dv) in FP32
        T = ncj * nck;
      }
      s_cd[w][lane][8] = T;
    }
    wave_lds_sync();
    int P[CPB + 1];
    P[0] = 0;
#pragma unroll
    for (int c = 0; c < CPB; ++c) P[c + 1] = P[c] + __builtin_amdgcn_readfirstlane(s_cd[w][c][8]);
    const int total = P[CPB];
    for (int c0 = 0; c0 < total; c0 += 64) {
      const int idx = c0 + lane;
      bool go = false;
      int key = 0, ql = 0, qx = 0;
      if (idx < total) {
        int cb = 0;
#pragma unroll
        for (int c = 1; c < CPB; ++c) cb += (idx >= P[c]) ? 1 : 0;
        int pb = P[0];
#pragma unroll
        for (int c = 1; c < CPB; ++c) pb = (cb >= c) ? P[c] : pb;
        const int *d = &s_cd[w][cb][0];
        const int g = d[0], sk = d[1], gb = d[2], tjc = d[3], k = d[4], j = d[5], dv = d[6], k1 = sk - gb, c = idx - pb;
        const int cq = static_cast<int>((static_cast<float>(c) + 0.5f) * __int_as_float(d[7])), cr = c - cq * dv;
        const bool ifast = ONCE && !exp_probe(bx.probe, 8);
        const int ci = ifast ? cr : cq, cl = cb * KW + (ifast ? cq : cr);
        const int i1 = s_cap[w][gb + ci], l1 = s_capl[w][cl];
        const double BOjk_f = s_bo[w][sk], BOij_f = s_bo[w][gb + i1], BOkl_f = s_bokl[w][cl];
        const int i = s_nb[w][gb + i1], l = s_ll[w][cl];
        go = (i1 != k1) && (BOij_f * BOjk_f > cutof2_esub) && (i != k) &&
             (BOjk_f * BOkl_f > cutof2_esub) && (BOij_f * (BOjk_f * BOjk_f) * BOkl_f > MINBO0) && (l != i) && (l != j);
        if (go) {
          const int i4 = (((s_meta[w][gb + i1] & 255) * ff.n1 + tjc) * ff.n1 + (s_meta[w][sk] & 255)) * ff.n1 + s_tl[w][cl];
          qx = tor_lds ? static_cast<int>(s_tor[i4]) : ff.inxn4[i4];
          go = qx != 0;
        }
        key = (g << 15) | (k1 << 10) | (i1 << 5) | l1;
        ql = l;
      }
      const unsigned long long m = __ballot(go);
      if (go) { const int qp = (qh + qn + __popcll(m & ((1ULL << lane) - 1ULL))) & 127; s_q[w][qp] = key; s_ql[w][qp] = ql; s_qx[w][qp] = static_cast<unsigned short>(qx); }
      qn += __popcll(m);
      wave_lds_sync();
      if (ONCE) {
        // one visit: the queue is a ring, and a batch ends where a (centre bond, l) run ends -- the run's sum over i is formed inside the batch and
        // leaves the wavefront ONCE (a run has <= 31 entries: among 64 there is always a boundary; the run at the tail may still grow)
        while (qn >= 64) {
          const int a = s_q[w][(qh + lane) & 127] & E4B_SEG, b = s_q[w][(qh + lane + 1) & 127] & E4B_SEG;
          const unsigned long long bm = __ballot(lane + 1 < qn && a != b);
          const int n = (bm && !exp_probe(bx.probe, 8)) ? 64 - __clzll(bm) : 64;
          evaluate(n);
          qh = (qh + n) & 127; qn -= n;
        }
      } else if (qn >= 64) {
        evaluate(64);
        const int rest = qn - 64;
        const int v = (lane < rest) ? s_q[w][64 + lane] : 0, vl = (lane < rest) ? s_ql[w][64 + lane] : 0, vx = (lane < rest) ? s_qx[w][64 + lane] : 0;
        wave_lds_sync();
        if (lane < rest) { s_q[w][lane] = v; s_ql[w][lane] = vl; s_qx[w][lane] = static_cast<unsigned short>(vx); }
        wave_lds_sync();
        qn = rest;
      }
    }
    wave_lds_sync();                                // the next round overwrites the k-side lists
  }
  if (qn > 0) evaluate(qn);

  wave_lds_sync();
  const double a_cf = s_acc[w][lane][0], a_fx = s_acc[w][lane][1], a_fy = s_acc[w][lane][2], a_fz = s_acc[w][lane][3];
  const double a_cjk1 = s_acc[w][lane][4], a_cjk2 = s_acc[w][lane][5], a_cdk = s_acc[w][lane][6];
  if (sl_me < nj_me) {
    const int o = ob_me + sl_me;
    if (a_cf != 0.0 || a_cjk1 != 0.0) cf1[o] += a_cf + a_cjk1;
    if (a_cjk2 != 0.0) cf2[o] += a_cjk2;
    if (a_cdk != 0.0) cdn[o] += a_cdk;
    if (a_fx != 0.0 || a_fy != 0.0 || a_fz != 0.0) { fnx[o] += a_fx; fny[o] += a_fy; fnz[o] += a_fz; }
  }
  if (self_me) {
    double sx = a_fx, sy = a_fy, sz = a_fz, scd = a_cdk;
    if (ONCE) {                                     // (this lane's accumulators hold minus the forces on the l atoms)
      const int gb = gbase(g_me);
      for (int t = 0; t < nj_me; ++t) { sx -= s_acc[w][gb + t][1]; sy -= s_acc[w][gb + t][2]; sz -= s_acc[w][gb + t][3]; scd += s_acc[w][gb + t][6]; }
    }
    cds[j_me] += scd;
    fx[j_me] += sx; fy[j_me] += sy; fz[j_me] += sz;
  }
  wave_lds_sync();                                // the next pass (packed form, two passes) rebuilds the tables
  }   // pass
  }   // groups
  e8 = wave_sum64(e8); e9 = wave_sum64(e9);
  if (lane == 0) {
    if (e8 != 0.0) atomicAdd(pe + 8, e8);
    if (e9 != 0.0) atomicAdd(pe + 9, e9);
  }
}

// The k-l side of the one-visit torsions (k_e4b<*, true>): row = bond (k, l1) of the compact tables, column = slot of j in the list of k, TW columns
// per row (TW = the longest bond list of the step, a multiple of 4).  A thread per bond adds the flagged columns of its row in slot order to the
// bond's own accumulators -- cf1 (ForceB on k-l) and the force on the neighbour l -- and clears the flags it used: the flag array is all zero
// again behind this kernel.
__global__ void __launch_bounds__(256) k_e4b_deliver(int nbonds, int TW, const double4 *__restrict__ tkl, unsigned *__restrict__ tflag4,
                                                      double *__restrict__ cf1, double *__restrict__ fnx, double *__restrict__ fny, double *__restrict__ fnz) {
  const int o = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (o >= nbonds) return;
  const int nw = TW >> 2;
  unsigned *fw = tflag4 + static_cast<size_t>(o) * nw;
  const double4 *row = tkl + static_cast<size_t>(o) * TW;
  double c = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0;
  bool any = false;
  for (int wd = 0; wd < nw; ++wd) {
    unsigned m = fw[wd];
    if (m == 0u) continue;
    fw[wd] = 0u;
    any = true;
    for (int b = 0; b < 4; ++b, m >>= 8)
      if (m & 255u) { const double4 t = row[4 * wd + b]; c += t.x; f0 += t.y; f1 += t.z; f2 += t.w; }
  }
  if (any) { cf1[o] += c; fnx[o] += f0; fny[o] += f1; fnz[o] += f2; }
}

void Engine::torsions() {
  double *pe_d = scal + SCAL_PE;
  const DevBox hb = dev_box(box);
  BoxImg bx;
  for (int k = 0; k < 9; ++k) { bx.H[k] = hb.H[k]; bx.Hi[k] = hb.Hi[k]; }
  for (int a = 0; a < 3; ++a) bx.L[a] = box.lat[a];
  bx.ortho = grid.ortho;
  bx.probe = static_cast<int>(opt.e4b_probe);       // (experiments build only: 0 otherwise)
  const int maxl = longest_bond_list();
  bool once = opt.e4b_once != 0;
  const int TW = (std::max(maxl, 8) + 3) & ~3;                              // columns of the k-l delivery table: the longest bond list of the step
  if (once) {
    const size_t need = static_cast<size_t>(std::max(nbonds, 1)) * TW;
    if (need > e4b_cap) {                                                   // 33 bytes per (bond, column), touched sparsely: RDX 18^3 2.9 GB; a table that would take more than
      size_t fre = 0, tot = 0;                                              // half of what is free is not allocated -- the step falls back to the two-visit form
      RX_HIP(hipMemGetInfo(&fre, &tot));
      const size_t want_entries = need + need / 4;
      if (want_entries * 33 > (fre + e4b_cap * 33) / 2) once = false; else alloc_e4b_delivery(want_entries);
    }
  }
  if (once) {
    if (e4b_dirty) RX_HIP(hipMemsetAsync(e4b_flag, 0, e4b_cap, stream));   // (an error between the torsion kernel and the delivery of an earlier call left flags behind)
    e4b_dirty = true;
  }
  // A persistent grid (default): three workgroups per CU, each walking every gridDim.x-th group of centre atoms.  One workgroup per group -- 30,618 on
  // RDX 18^3, each needing four 168-register wavefront slots and 49 KB of LDS at once -- kept only 2.0-2.4 of the 3 wavefronts per SIMD resident (SQ
  // counters, profiles/r06_e4b_*): 3.16 -> 2.54 ms for the two-visit form, 3.54 -> 1.98 ms for the one-visit form.  RXMD_E4B_WPB=1 (workgroups of one
  // wavefront, tables released per wavefront) gains 0.05 ms without the persistent grid and loses with it (the dispatcher does not spread them evenly
  // over the SIMDs).
  const int n4 = dff.n1 * dff.n1 * dff.n1 * dff.n1;
  const size_t tor_bytes = (dff.n1 <= 8 && dff.ntoty <= 255) ? static_cast<size_t>((n4 + 15) & ~15) : 0;
  const bool wpb1 = opt.e4b_wpb == 1;
  auto launch = [&](auto inst, int per_wave) {
    constexpr int L = decltype(inst)::value;
    auto go = [&](auto kern, int wpb) {
      const int VB = nblk(N, per_wave * wpb);                              // groups of atoms = workgroups of the full grid
      const int grid = opt.e4b_persist != 0 ? std::min(VB, (num_cu * (12 / wpb) + 7) & ~7) : VB;   // persistent: 3 wavefronts per SIMD resident (LDS and registers allow no more)
      kern<<<grid, 64 * wpb, tor_bytes, stream>>>(N, dff, boff, nbr, btype, nbrcnt, type, gid, pos[0], pos[1], pos[2], bo0, bo2, delta, etor, econ, cf1, cf2, cdn, fnx, fny, fnz,
                                                  cds, frc[0], frc[1], frc[2], pe_d, bx, brev, e4b_t, e4b_flag, TW, VB);
    };
    if (once) { if (wpb1) go(k_e4b<L, true, 1>, 1); else go(k_e4b<L, true, 4>, 4); }
    else      { if (wpb1) go(k_e4b<L, false, 1>, 1); else go(k_e4b<L, false, 4>, 4); }
    RX_HIP(hipGetLastError());
  };
  // The instance, from RXMD_E4B_SLOTS (0: choose; 4 / 16 / 32 force one, tests) and the longest list: packed eight atoms per wavefront when no list of the
  // step is longer than 15, else two atoms x 32 slots (forced by 32: the general kernel).  4: packed four atoms, any list (on the SiC workload, 16+ bonds
  // per atom, it needs two passes for most groups and is slower than the default there, 3.69 against 3.47 ms).  16: four atoms x 16 slots where the
  // lists allow it (<= 15), the general kernel where they do not.
  const int want = static_cast<int>(opt.e4b_slots);
  if (want == 4) launch(std::integral_constant<int, 1>{}, 4);
  else if (maxl > 15 || want == 32) launch(std::integral_constant<int, 5>{}, 2);
  else if (want == 16) launch(std::integral_constant<int, 4>{}, 4);
  else launch(std::integral_constant<int, 0>{}, 8);
  if (once) {
    k_e4b_deliver<<<nblk(nbonds, 256), 256, 0, stream>>>(nbonds, TW, e4b_t, reinterpret_cast<unsigned *>(e4b_flag), cf1, fnx, fny, fnz);
    e4b_dirty = false;
  }
}

}  // namespace rxmd
