// angles.hip -- E3b, the valence-angle, penalty and three-body conjugation terms of FORCE (reference src/pot.F90:319-557): k_e3q (work queue, the default),
// k_e3b (thread per centre atom) and Engine::valence_angles().  The accumulators the kernels add to are described at the head of bonded.hip.
// The two kernels carry the same arithmetic of a centre atom and of one angle (pot.F90:385-541), k_e3b with the library's pow and k_e3q with
// exp(p log b): a correction to the angle term is made in both.  (Written once as two function templates it compiles to other device code in all
// seven kernels -- NOTES.md, "The bonded terms, one unit each".)
#include "bonded_common.h"

#include <algorithm>

namespace rxmd {

// occupancy knob, measured on MI355X (bonded section of the step, ms): E3b at 1/2/3/4 workgroups per CU = 22.5/20.4/22.4/22.9
// (256 VGPRs + 3 AGPRs miss the 2-wave budget by three registers without the hint; beyond 2 the spills cost more than
// the occupancy buys)
#ifndef E3B_MINB
#define E3B_MINB 2
#endif
#ifndef E3B_CAP
#define E3B_CAP 448     // bonds of a wavefront's 64 atoms whose accumulators k_e3b keeps in LDS (RDX: ~340 per wavefront; 4 x 5 x 448 x 8 B = 70 KB per workgroup)
#endif
// Work order of the thread-per-centre angle kernel: atom order.  (Round 2 first handed the centres out sorted by their number of bonds
// above the cut-off -- 3.5 -> 2.8 ms while the loops walked slots; once they walk set bits (below) a lane's trip count is its own
// pair count, and the sorted order only scatters the slot-major accesses, one 64-byte line per lane: 2.7 ms sorted, 1.8 ms in atom
// order, sorted inside tiles of 128 / 256 / 512 / 1024 atoms 1.84 / 1.97 / 2.86 / 4.19 ms.)
__global__ void __launch_bounds__(256, E3B_MINB) k_e3b(int N, DevFF ff, const int *__restrict__ boff, const int *__restrict__ nbr, const unsigned char *__restrict__ btype, const int *__restrict__ type,
                                              const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                              const double *__restrict__ bo0, const double *__restrict__ bo2, const double *__restrict__ bo3,
                                              const double *__restrict__ delta, const double *__restrict__ nlp, const double *__restrict__ dDlp,
                                              const double *__restrict__ epen, const double *__restrict__ ecoa,
                                              double *__restrict__ cf1, double *__restrict__ cf2, double *__restrict__ cf3, double *__restrict__ cdn,
                                              double *__restrict__ fnx, double *__restrict__ fny, double *__restrict__ fnz,
                                              double *__restrict__ cds, double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz, double *__restrict__ pe) {
  const int tid = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;   // an XCD's workgroups own one contiguous eighth of the atoms: the neighbours they gather stay in its L2
  // Round 4: the five accumulators of the bonds of a wavefront's 64 atoms -- one contiguous stretch of the compact tables -- live in LDS while the
  // angles are walked.  Every angle adds to the j-k bond's coefficient, cdbnd term and neighbour force: five read-modify-writes of global memory per
  // angle, each a dependent round trip inside the loop (the compiler must assume that a later iteration hits the same bond).  The stretch is loaded
  // with the values the earlier kernels left (coalesced), updated in LDS by the thread that owns the atom (no atomics: a thread touches only its own
  // bonds), and stored back at the end: the same additions in the same order, bit for bit.  Bonds beyond E3B_CAP of a wavefront (SiC: 16 bonds per
  // atom) take the global path as before.
  extern __shared__ double s_e3b[];
  const int lane_ = threadIdx.x & 63, wv_ = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  double *l_cf = s_e3b + static_cast<size_t>(wv_) * 5 * E3B_CAP, *l_cd = l_cf + E3B_CAP, *l_fx = l_cd + E3B_CAP, *l_fy = l_fx + E3B_CAP, *l_fz = l_fy + E3B_CAP;
  const int a0_ = tid - lane_;                                     // first atom of this wavefront
  const int ob_w = a0_ < N ? boff[a0_] : 0, oe_w = a0_ < N ? boff[min(a0_ + 64, N)] : 0;
  const int nst = min(oe_w - ob_w, E3B_CAP);                       // staged bonds
  for (int t = lane_; t < nst; t += 64) { l_cf[t] = cf1[ob_w + t]; l_cd[t] = cdn[ob_w + t]; l_fx[t] = fnx[ob_w + t]; l_fy[t] = fny[ob_w + t]; l_fz[t] = fnz[ob_w + t]; }
  wave_lds_sync();
  auto acc1 = [&](double *__restrict__ gl, double *ld, int o, double v) { const int r = o - ob_w; if (r < nst) ld[r] += v; else gl[o] += v; };
  // the angle row of a type triple and its seven parameters from LDS (round 5): inxn3 -> angle[] were two dependent look-ups in front of every
  // angle's arithmetic, at two wavefronts per SIMD nothing hides them.  Force fields with more than 7 atom types or 63 angle rows keep the global path.
  __shared__ int s_ix3[512];
  __shared__ double s_ang[64][7];
  const bool ang_lds = ff.n1 <= 8 && ff.nvaty <= 63;
  if (ang_lds) {
    for (int t = threadIdx.x; t < ff.n1 * ff.n1 * ff.n1; t += 256) s_ix3[t] = ff.inxn3[t];
    for (int t = threadIdx.x; t < 7 * (ff.nvaty + 1); t += 256) s_ang[t / 7][t % 7] = reinterpret_cast<const double *>(ff.angle)[t];
    __syncthreads();
  }
  double e5 = 0.0, e6 = 0.0, e7 = 0.0;
  if (tid < N) {
    const int j = tid;
    const int tj = type[j], ob = boff[j], nj = min(boff[j + 1] - ob, 32);
    const DevAtomP aj = ff.atom[tj];
    const double xj = x[j], yj = y[j], zj = z[j];
    double sum_BO8 = 0.0, sum_SBO1 = 0.0;
    unsigned capmask = 0u;
    for (int n1 = 0; n1 < nj; ++n1) {
      const int o = ob + n1;
      const double b = bo0[o], b2 = b * b, b4 = b2 * b2;
      sum_BO8 -= b4 * b4;                                                  // BO**8, pot.F90:362
      sum_SBO1 += bo2[o] + bo3[o];
      if (b - cutof2_esub > 0.0) capmask |= 1u << n1;                      // pot.F90:372-373, 385-386
    }
    const double prod_SBO = exp(sum_BO8);
    const double dlj = delta[j];
    const double delta_ang = dlj + aj.Val - aj.Valangle;
    const double nlpj = nlp[j], dDj = dDlp[j];
    // per-centre factors of the penalty and conjugation terms (global parameters, pot.F90:460-462,481-483)
    const double exp_pen3 = exp(-ff.ppen3 * dlj), exp_pen4 = exp(ff.ppen4 * dlj);
    const double trm34 = 1.0 + exp_pen3 + exp_pen4;
    const double fn9 = (2.0 + exp_pen3) / trm34;
    const double Cf9j = (-ff.ppen3 * exp_pen3 * trm34 - (2.0 + exp_pen3) * (-ff.ppen3 * exp_pen3 + ff.ppen4 * exp_pen4)) / (trm34 * trm34);
    const double delta_val = dlj + aj.Val - aj.Valval;
    const double exp_coa2 = exp(ff.pcoa2 * delta_val);
    const double exp6 = exp(ff.pval6 * delta_ang);
    // SBO, SBO2, its derivative factor and exp(-pval10 (2 - SBO2)) depend on the centre only (pot.F90:415-437): once per atom
    const double SBO = sum_SBO1 + (1.0 - prod_SBO) * (-delta_ang - ff.pval8 * nlpj);
    double SBO2 = 0.0, CSBO2 = 0.0;
    if (SBO > 0.0 && SBO <= 1.0) { SBO2 = pow(SBO, ff.pval9); CSBO2 = ff.pval9 * pow(SBO, ff.pval9 - 1.0); }
    else if (SBO > 1.0 && SBO <= 2.0) { SBO2 = 2.0 - pow(2.0 - SBO, ff.pval9); CSBO2 = ff.pval9 * pow(2.0 - SBO, ff.pval9 - 1.0); }
    else if (SBO > 2.0) SBO2 = 2.0;
    const double ex10 = exp(-ff.pval10 * (2.0 - SBO2));
    const double dSBO1 = -8.0 * prod_SBO * (delta_ang + ff.pval8 * nlpj);
    const double dSBO2 = (prod_SBO - 1.0) * (1.0 - ff.pval8 * dDj);
    // sums over all angles of the terms that ForceBbo(j,n1,...) applies to EVERY bond of j (pot.F90:526-532)
    double S_d1 = 0.0, S_v6 = 0.0, S_v5 = 0.0;
    V3 fself = {0.0, 0.0, 0.0};
    for (unsigned mi = capmask; mi & (mi - 1u);) {
      const int i1 = __ffs(mi) - 1;
      mi &= mi - 1u;
      const int oi = ob + i1;
      const double BOij_f = bo0[oi], BOij = BOij_f - cutof2_esub;
      const int i = nbr[oi], ti = btype[oi];
      const V3 rij = {x[i] - xj, y[i] - yj, z[i] - zj};
      const double nij = sqrt(dot(rij, rij));
      double ai_cf = 0.0, ai_cd = 0.0, ai_fx = 0.0, ai_fy = 0.0, ai_fz = 0.0;      // the i-j bond's own sums over k1: one write after the loop
      for (unsigned mk = mi; mk; mk &= mk - 1u) {
        const int k1 = __ffs(mk) - 1;
        const int ok = ob + k1;
        const double BOjk_f = bo0[ok], BOjk = BOjk_f - cutof2_esub;
        if (!(BOij_f * BOjk_f > cutof2_esub)) continue;
        const int k = nbr[ok], tk = btype[ok];
        const int inxn = ang_lds ? s_ix3[(ti * ff.n1 + tj) * ff.n1 + tk] : ff.inxn3[(ti * ff.n1 + tj) * ff.n1 + tk];
        if (inxn == 0) continue;
        DevAngleP ap;
        if (ang_lds) { const double *a_ = s_ang[inxn]; ap = DevAngleP{a_[0], a_[1], a_[2], a_[3], a_[4], a_[5], a_[6]}; }
        else ap = ff.angle[inxn];
        const V3 rjk = {xj - x[k], yj - y[k], zj - z[k]};
        const double njk = sqrt(dot(rjk, rjk));
        double cos_ijk = -dot(rij, rjk) / (nij * njk);
        if (cos_ijk > MAXANGLE) cos_ijk = MAXANGLE;
        if (cos_ijk < MINANGLE) cos_ijk = MINANGLE;
        const double theta_ijk = acos(cos_ijk), sin_ijk = sqrt((1.0 - cos_ijk) * (1.0 + cos_ijk));   // sin(acos(c))
        const double BOij_p4 = pow(BOij, ap.pval4), exp3ij = exp(-aj.pval3 * BOij_p4), fn7ij = 1.0 - exp3ij;
        const double BOjk_p4 = pow(BOjk, ap.pval4), exp3jk = exp(-aj.pval3 * BOjk_p4), fn7jk = 1.0 - exp3jk;
        const double exp7 = exp(-ap.pval7 * delta_ang), trm8 = 1.0 + exp6 + exp7;
        const double fn8j = aj.pval5 - (aj.pval5 - 1.0) * (2.0 + exp6) / trm8;
        const double theta0 = PI_ - ap.theta00 * (1.0 - ex10);
        const double theta_diff = theta0 - theta_ijk;
        const double exp2 = exp(-ap.pval2 * theta_diff * theta_diff);
        e5 += fn7ij * fn7jk * fn8j * (ap.pval1 - ap.pval1 * exp2);
        const double Cf7ij = aj.pval3 * ap.pval4 * (BOij_p4 / BOij) * exp3ij;                 // BO**(pval4-1) = BO**pval4 / BO
        const double Cf7jk = aj.pval3 * ap.pval4 * (BOjk_p4 / BOjk) * exp3jk;
        const double Cf8j = (1.0 - aj.pval5) / (trm8 * trm8) * (ff.pval6 * exp6 * trm8 - (2.0 + exp6) * (ff.pval6 * exp6 - ap.pval7 * exp7));
        const double Ctheta0 = ff.pval10 * ap.theta00 * ex10;
        const double CEval1 = Cf7ij * fn7jk * fn8j * ap.pval1 * (1.0 - exp2);
        const double CEval2 = fn7ij * Cf7jk * fn8j * ap.pval1 * (1.0 - exp2);
        const double CEval3 = fn7ij * fn7jk * Cf8j * ap.pval1 * (1.0 - exp2);
        const double CEval4 = 2.0 * ap.pval1 * ap.pval2 * fn7ij * fn7jk * fn8j * exp2 * theta_diff;
        const double CEval5 = CEval4 * Ctheta0 * CSBO2;
        const double CEval6 = CEval5 * dSBO1, CEval7 = CEval5 * dSBO2, CEval8 = CEval4 / sin_ijk;
        // penalty, pot.F90:460-476
        const double PEpen = ap.ppen1 * fn9 * epen[oi] * epen[ok];
        e6 += PEpen;
        const double CEpen1 = Cf9j / fn9 * PEpen, CEpen2 = -2.0 * ff.ppen2 * (BOij - 2.0) * PEpen, CEpen3 = -2.0 * ff.ppen2 * (BOjk - 2.0) * PEpen;
        // three-body conjugation, pot.F90:479-497
        const double sum_BOi = delta[i] + ff.atom[ti].Val, sum_BOk = delta[k] + ff.atom[tk].Val;
        const double ui = -BOij + sum_BOi, uk = -BOjk + sum_BOk;
        const double PEcoa = ap.pcoa1 / (1.0 + exp_coa2) * ecoa[oi] * ecoa[ok];
        e7 += PEcoa;
        const double CEcoa1 = -2.0 * ff.pcoa4 * (BOij - 1.5) * PEcoa, CEcoa2 = -2.0 * ff.pcoa4 * (BOjk - 1.5) * PEcoa;
        const double CEcoa3 = -ff.pcoa2 * exp_coa2 / (1.0 + exp_coa2) * PEcoa;
        const double CEcoa4 = -2.0 * ff.pcoa3 * ui * PEcoa, CEcoa5 = -2.0 * ff.pcoa3 * uk * PEcoa;
        // accumulate, pot.F90:509-541
        ai_cf += CEpen2 + CEcoa1 - CEcoa4 + CEval1;        // ForceB on bond i-j
        acc1(cf1, l_cf, ok, CEpen3 + CEcoa2 - CEcoa5 + CEval2);      // ForceB on bond j-k
        S_d1 += CEpen1 + CEcoa3 + CEval3 + CEval7; S_v6 += CEval6; S_v5 += CEval5;
        ai_cd += CEcoa4; acc1(cdn, l_cd, ok, CEcoa5);      // cdbnd(i), cdbnd(k)
        V3 fi, fk;
        angle_forces(CEval8, rij, nij, rjk, njk, fi, fk);
        ai_fx += fi.x; ai_fy += fi.y; ai_fz += fi.z;
        acc1(fnx, l_fx, ok, fk.x); acc1(fny, l_fy, ok, fk.y); acc1(fnz, l_fz, ok, fk.z);
        fself.x -= fi.x + fk.x; fself.y -= fi.y + fk.y; fself.z -= fi.z + fk.z;
      }
      if (ai_cf != 0.0) acc1(cf1, l_cf, oi, ai_cf);
      if (ai_cd != 0.0) acc1(cdn, l_cd, oi, ai_cd);
      if (ai_fx != 0.0 || ai_fy != 0.0 || ai_fz != 0.0) { acc1(fnx, l_fx, oi, ai_fx); acc1(fny, l_fy, oi, ai_fy); acc1(fnz, l_fz, oi, ai_fz); }
    }
    if (S_d1 != 0.0 || S_v6 != 0.0 || S_v5 != 0.0)
      for (int n1 = 0; n1 < nj; ++n1) {
        const int o = ob + n1;
        acc1(cf1, l_cf, o, S_d1 + S_v6 * ipow7(bo0[o])); cf2[o] += S_v5; cf3[o] += S_v5;
      }
    fx[j] += fself.x; fy[j] += fself.y; fz[j] += fself.z;
  }
  wave_lds_sync();
  for (int t = lane_; t < nst; t += 64) { cf1[ob_w + t] = l_cf[t]; cdn[ob_w + t] = l_cd[t]; fnx[ob_w + t] = l_fx[t]; fny[ob_w + t] = l_fy[t]; fnz[ob_w + t] = l_fz[t]; }
  block_energy_add(e5, pe + 5); block_energy_add(e6, pe + 6); block_energy_add(e7, pe + 7);
}

// Valence angles through a work queue (round 6, late).  k_e3b gives every centre atom a thread: a lane's trip count is its own number of angles (1 to ~40)
// and a wavefront runs as long as its busiest lane -- the vector unit issues for 0.62 of the kernel's 1.25 ms with mostly empty lanes.  Here a wavefront owns
// SIXTEEN consecutive centre atoms (the shape of k_e4b): lanes 0..15 set the atoms up (per-centre factors -> LDS), all 64 lanes enumerate the pairs of
// qualifying bonds (four lanes per atom), apply the reference's cut-offs (pot.F90:385-400) and compact the survivors with a ballot into an LDS ring; a full
// batch of 64 angles is then evaluated one per lane.  Every angle adds to the accumulators of its two bonds in LDS (ds_add_f64, queue order: the same bits
// run to run); the centre's own force is minus the sum of its bonds' forces, its all-bond terms are sums per atom; one coalesced pass adds everything to
// the bond tables.  Persistent grid.  Sixteen centres per wavefront with bond lists up to 12, eight up to 24, four beyond; needs the type-triple table in
// LDS (at most 7 atom types, 255 angle rows; the rows' parameters from LDS up to 63 rows, from memory beyond); otherwise k_e3b runs.
constexpr int E3Q_BC = 192;                           // bonds of a wavefront's centre atoms: NA atoms x MAXL = 192 / NA list entries -- 16 x 12 (RDX, water), 8 x 24, 4 x 48 (lists up to MAXNEIGHBS: SiC, iron sulfide)
template <int MINW, int NA>                           // wavefronts per SIMD the register budget is cut for (3: 168 registers + scratch, 2: 256); centre atoms per wavefront
__global__ void __launch_bounds__(256, MINW) k_e3q(int N, int NG, DevFF ff, const int *__restrict__ boff, const int *__restrict__ nbr, const unsigned char *__restrict__ btype, const int *__restrict__ type,
                                              const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                              const double *__restrict__ bo0, const double *__restrict__ bo2, const double *__restrict__ bo3,
                                              const double *__restrict__ delta, const double *__restrict__ nlp, const double *__restrict__ dDlp,
                                              const double *__restrict__ epen, const double *__restrict__ ecoa,
                                              double *__restrict__ cf1, double *__restrict__ cf2, double *__restrict__ cf3, double *__restrict__ cdn,
                                              double *__restrict__ fnx, double *__restrict__ fny, double *__restrict__ fnz,
                                              double *__restrict__ cds, double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz, double *__restrict__ pe, int probe) {
  constexpr int E3Q_NA = NA, E3Q_MAXL = (E3Q_BC / NA < 32) ? E3Q_BC / NA : 32, LPA = 64 / NA;     // longest bond list (MAXNEIGHBS = 30), lanes per atom of the enumeration
  __shared__ unsigned char s_ix3[512];             // angle row of a type triple (at most 63 rows)
  __shared__ double s_ang[64][7];
  // per wavefront: factors of the 16 centres, accumulators of their bonds and of the atoms, the qualifying slots, the queue
  __shared__ double s_c[4][16][12];            // x, y, z, delta_ang, exp6, ex10, CSBO2, dSBO1, dSBO2, fn9, Cf9j / fn9, exp_coa2
  __shared__ int s_ci[4][16][4];               // type, first bond, bonds, qualifying bonds
  __shared__ double s_acc[4][5][E3Q_BC];           // per bond: cf1, cdn, force on the neighbour
  __shared__ double s_at[4][16][3];            // per atom: S_d1, S_v6, S_v5 (the terms every bond of the centre receives, pot.F90:526-532)
  __shared__ unsigned char s_cap[4][256], s_own[4][E3Q_BC];        // qualifying slots: NA x (at most 32 = 256 / NA ... 16) entries, [a * CAPW + u]
  __shared__ float s_cbo[4][E3Q_BC];               // [a * MAXL + u]     // bond orders of the qualifying slots, single precision: the product test of the enumeration asks memory only at the edge
  __shared__ unsigned short s_q[4][128];
  constexpr int CAPW = (256 / NA < 32) ? 256 / NA : 32;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  for (int t = threadIdx.x; t < ff.n1 * ff.n1 * ff.n1; t += 256) s_ix3[t] = static_cast<unsigned char>(ff.inxn3[t]);
  const bool ang_lds = ff.nvaty <= 63;              // (more angle rows than the LDS table holds, up to 255: their parameters come from memory, requested with the angle's other operands)
  if (ang_lds) for (int t = threadIdx.x; t < 7 * (ff.nvaty + 1); t += 256) s_ang[t / 7][t % 7] = reinterpret_cast<const double *>(ff.angle)[t];
  __syncthreads();
  double e5 = 0.0, e6 = 0.0, e7 = 0.0;
  for (int vb = blockIdx.x; vb < NG; vb += gridDim.x) {
  const int jbase = (xcd_swizzle(vb, NG) * 4 + w) * E3Q_NA;
  if (jbase >= N) continue;                        // (whole wavefront; no block-level barrier below)
  const int na = min(E3Q_NA, N - jbase);
  const int ob_w = boff[jbase], nb_w = boff[jbase + na] - ob_w;             // the bonds of the wavefront's atoms: one contiguous stretch of the compact tables
  // the bond orders of the wavefront's bonds with coalesced loads into the (not yet used) accumulator rows 0 and 1: the centres' loops over their bonds
  // below read LDS -- as loads from memory they were up to twelve round trips one after the other in front of everything else
  for (int r = lane; r < nb_w; r += 64) { s_acc[w][0][r] = bo0[ob_w + r]; s_acc[w][1][r] = bo2[ob_w + r] + bo3[ob_w + r]; }
  for (int t = lane; t < 3 * E3Q_BC; t += 64) (&s_acc[w][2][0])[t] = 0.0;
  if (lane < E3Q_NA) { s_at[w][lane][0] = 0.0; s_at[w][lane][1] = 0.0; s_at[w][lane][2] = 0.0; s_ci[w][lane][2] = 0; s_ci[w][lane][3] = 0; }
  wave_lds_sync();
  if (lane < na) {                                 // set-up of a centre (pot.F90:352-437, 460-462, 481-483): everything that depends on the centre only
    const int j = jbase + lane;
    const int tj = type[j], ob = boff[j], nj = min(boff[j + 1] - ob, E3Q_MAXL);
    const DevAtomP aj = ff.atom[tj];
    double sum_BO8 = 0.0, sum_SBO1 = 0.0;
    int nc = 0;
    for (int n1 = 0; n1 < nj; ++n1) {
      const int r = ob + n1 - ob_w;
      const double b = s_acc[w][0][r], b2 = b * b, b4 = b2 * b2;
      sum_BO8 -= b4 * b4;                                                  // BO**8, pot.F90:362
      sum_SBO1 += s_acc[w][1][r];
      if (b - cutof2_esub > 0.0) { s_cbo[w][lane * E3Q_MAXL + nc] = static_cast<float>(b); s_cap[w][lane * CAPW + nc++] = static_cast<unsigned char>(n1); }   // pot.F90:372-373, 385-386
      s_own[w][r] = static_cast<unsigned char>(lane);
    }
    const double prod_SBO = exp(sum_BO8);
    const double dlj = delta[j];
    const double delta_ang = dlj + aj.Val - aj.Valangle;
    const double nlpj = nlp[j], dDj = dDlp[j];
    const double exp_pen3 = exp(-ff.ppen3 * dlj), exp_pen4 = exp(ff.ppen4 * dlj);
    const double trm34 = 1.0 + exp_pen3 + exp_pen4;
    const double fn9 = (2.0 + exp_pen3) / trm34;
    const double Cf9j = (-ff.ppen3 * exp_pen3 * trm34 - (2.0 + exp_pen3) * (-ff.ppen3 * exp_pen3 + ff.ppen4 * exp_pen4)) / (trm34 * trm34);
    const double delta_val = dlj + aj.Val - aj.Valval;
    const double SBO = sum_SBO1 + (1.0 - prod_SBO) * (-delta_ang - ff.pval8 * nlpj);
    double SBO2 = 0.0, CSBO2 = 0.0;
    // (b ** p and b ** (p - 1) from ONE exp(p log b), b > 0 in both branches: two calls of the library's pow are ~600 of the set-up's ~900 instructions)
    if (SBO > 0.0 && SBO <= 1.0) { const double pw = exp(ff.pval9 * log(SBO)); SBO2 = pw; CSBO2 = ff.pval9 * (pw / SBO); }
    else if (SBO > 1.0 && SBO < 2.0) { const double b_ = 2.0 - SBO, pw = exp(ff.pval9 * log(b_)); SBO2 = 2.0 - pw; CSBO2 = ff.pval9 * (pw / b_); }
    else if (SBO >= 2.0) SBO2 = 2.0;
    double *c = s_c[w][lane];
    c[0] = x[j]; c[1] = y[j]; c[2] = z[j]; c[3] = delta_ang; c[4] = exp(ff.pval6 * delta_ang); c[5] = exp(-ff.pval10 * (2.0 - SBO2)); c[6] = CSBO2;
    c[7] = -8.0 * prod_SBO * (delta_ang + ff.pval8 * nlpj); c[8] = (prod_SBO - 1.0) * (1.0 - ff.pval8 * dDj); c[9] = fn9; c[10] = Cf9j / fn9; c[11] = exp(ff.pcoa2 * delta_val);
    s_ci[w][lane][0] = tj; s_ci[w][lane][1] = ob; s_ci[w][lane][2] = nj; s_ci[w][lane][3] = nc;
  }
  wave_lds_sync();
  for (int t = lane; t < 2 * E3Q_BC; t += 64) (&s_acc[w][0][0])[t] = 0.0;         // rows 0 and 1 become accumulators
  wave_lds_sync();
  int qn = 0, qh = 0;
  auto evaluate = [&](int cnt) {                   // one angle per lane: queue entry = atom << 10 | slot i1 << 5 | slot k1 (i1 < k1)
    if (exp_probe(probe, 2)) return;
    if (exp_probe(probe, 5)) { if (lane == 0) { atomicAdd(pe + 5, 1.0); atomicAdd(pe + 6, static_cast<double>(cnt)); } return; }
    if (lane < cnt) {
      const int key = s_q[w][(qh + lane) & 127];
      const int a = key >> 10, i1 = (key >> 5) & 31, k1 = key & 31;
      const double *c = s_c[w][a];
      const int tj = s_ci[w][a][0], ob = s_ci[w][a][1];
      const int oi = ob + i1, ok = ob + k1;
      const double xj = c[0], yj = c[1], zj = c[2], delta_ang = c[3], exp6 = c[4], ex10 = c[5], CSBO2 = c[6], dSBO1 = c[7], dSBO2 = c[8], fn9 = c[9], Cf9j_fn9 = c[10], exp_coa2 = c[11];
      const DevAtomP aj = ff.atom[tj];
      const int i = nbr[oi], ti = btype[oi], k = nbr[ok], tk = btype[ok];
      const double BOij = bo0[oi] - cutof2_esub, BOjk = bo0[ok] - cutof2_esub;
      const V3 rij = {x[i] - xj, y[i] - yj, z[i] - zj};
      const double nij = sqrt(dot(rij, rij));
      const V3 rjk = {xj - x[k], yj - y[k], zj - z[k]};
      const double njk = sqrt(dot(rjk, rjk));
      const int inxn = s_ix3[(ti * ff.n1 + tj) * ff.n1 + tk];
      DevAngleP ap;
      if (ang_lds) { const double *a_ = s_ang[inxn]; ap = DevAngleP{a_[0], a_[1], a_[2], a_[3], a_[4], a_[5], a_[6]}; }
      else ap = ff.angle[inxn];
      double cos_ijk = -dot(rij, rjk) / (nij * njk);
      if (cos_ijk > MAXANGLE) cos_ijk = MAXANGLE;
      if (cos_ijk < MINANGLE) cos_ijk = MINANGLE;
      const double theta_ijk = acos(cos_ijk), sin_ijk = sqrt((1.0 - cos_ijk) * (1.0 + cos_ijk));   // sin(acos(c))
      // BO ** pval4 as exp(pval4 log BO): BO > 0 here, and the library's pow spends most of its ~300 instructions on cases that cannot occur (1e-15 relative apart)
      const double BOij_p4 = exp(ap.pval4 * log(BOij)), exp3ij = exp(-aj.pval3 * BOij_p4), fn7ij = 1.0 - exp3ij;
      const double BOjk_p4 = exp(ap.pval4 * log(BOjk)), exp3jk = exp(-aj.pval3 * BOjk_p4), fn7jk = 1.0 - exp3jk;
      const double exp7 = exp(-ap.pval7 * delta_ang), trm8 = 1.0 + exp6 + exp7;
      const double fn8j = aj.pval5 - (aj.pval5 - 1.0) * (2.0 + exp6) / trm8;
      const double theta0 = PI_ - ap.theta00 * (1.0 - ex10);
      const double theta_diff = theta0 - theta_ijk;
      const double exp2 = exp(-ap.pval2 * theta_diff * theta_diff);
      e5 += fn7ij * fn7jk * fn8j * (ap.pval1 - ap.pval1 * exp2);
      const double Cf7ij = aj.pval3 * ap.pval4 * (BOij_p4 / BOij) * exp3ij;                 // BO**(pval4-1) = BO**pval4 / BO
      const double Cf7jk = aj.pval3 * ap.pval4 * (BOjk_p4 / BOjk) * exp3jk;
      const double Cf8j = (1.0 - aj.pval5) / (trm8 * trm8) * (ff.pval6 * exp6 * trm8 - (2.0 + exp6) * (ff.pval6 * exp6 - ap.pval7 * exp7));
      const double Ctheta0 = ff.pval10 * ap.theta00 * ex10;
      const double CEval1 = Cf7ij * fn7jk * fn8j * ap.pval1 * (1.0 - exp2);
      const double CEval2 = fn7ij * Cf7jk * fn8j * ap.pval1 * (1.0 - exp2);
      const double CEval3 = fn7ij * fn7jk * Cf8j * ap.pval1 * (1.0 - exp2);
      const double CEval4 = 2.0 * ap.pval1 * ap.pval2 * fn7ij * fn7jk * fn8j * exp2 * theta_diff;
      const double CEval5 = CEval4 * Ctheta0 * CSBO2;
      const double CEval6 = CEval5 * dSBO1, CEval7 = CEval5 * dSBO2, CEval8 = CEval4 / sin_ijk;
      const double PEpen = ap.ppen1 * fn9 * epen[oi] * epen[ok];             // penalty, pot.F90:460-476
      e6 += PEpen;
      const double CEpen1 = Cf9j_fn9 * PEpen, CEpen2 = -2.0 * ff.ppen2 * (BOij - 2.0) * PEpen, CEpen3 = -2.0 * ff.ppen2 * (BOjk - 2.0) * PEpen;
      const double sum_BOi = delta[i] + ff.atom[ti].Val, sum_BOk = delta[k] + ff.atom[tk].Val;   // three-body conjugation, pot.F90:479-497
      const double ui = -BOij + sum_BOi, uk = -BOjk + sum_BOk;
      const double PEcoa = ap.pcoa1 / (1.0 + exp_coa2) * ecoa[oi] * ecoa[ok];
      e7 += PEcoa;
      const double CEcoa1 = -2.0 * ff.pcoa4 * (BOij - 1.5) * PEcoa, CEcoa2 = -2.0 * ff.pcoa4 * (BOjk - 1.5) * PEcoa;
      const double CEcoa3 = -ff.pcoa2 * exp_coa2 / (1.0 + exp_coa2) * PEcoa;
      const double CEcoa4 = -2.0 * ff.pcoa3 * ui * PEcoa, CEcoa5 = -2.0 * ff.pcoa3 * uk * PEcoa;
      V3 fi, fk;
      angle_forces(CEval8, rij, nij, rjk, njk, fi, fk);
      const int ri = oi - ob_w, rk = ok - ob_w;                             // accumulate, pot.F90:509-541
      atomicAdd(&s_acc[w][0][ri], CEpen2 + CEcoa1 - CEcoa4 + CEval1); atomicAdd(&s_acc[w][1][ri], CEcoa4);
      atomicAdd(&s_acc[w][2][ri], fi.x); atomicAdd(&s_acc[w][3][ri], fi.y); atomicAdd(&s_acc[w][4][ri], fi.z);
      atomicAdd(&s_acc[w][0][rk], CEpen3 + CEcoa2 - CEcoa5 + CEval2); atomicAdd(&s_acc[w][1][rk], CEcoa5);
      atomicAdd(&s_acc[w][2][rk], fk.x); atomicAdd(&s_acc[w][3][rk], fk.y); atomicAdd(&s_acc[w][4][rk], fk.z);
      atomicAdd(&s_at[w][a][0], CEpen1 + CEcoa3 + CEval3 + CEval7); atomicAdd(&s_at[w][a][1], CEval6); atomicAdd(&s_at[w][a][2], CEval5);
    }
    wave_lds_sync();
  };
  if (exp_probe(probe, 1)) continue;
  // enumeration: LPA = 64 / NA lanes per atom; lane s of an atom takes the first bonds u = s, s + LPA, ... of its qualifying list, each with every later one
  {
    const int a = lane / LPA, sub = lane % LPA;
    const int nc = s_ci[w][a][3], tj = s_ci[w][a][0], ob = s_ci[w][a][1];
    int u = sub, v = sub + 1;
    for (;;) {
      bool live = u < nc - 1;
      const unsigned long long any = __ballot(live);
      if (any == 0ULL) break;
      bool go = false;
      int key = 0;
      if (live) {
        const int i1 = s_cap[w][a * CAPW + u], k1 = s_cap[w][a * CAPW + v];
        const int oi = ob + i1, ok = ob + k1;
        const float pr = s_cbo[w][a * E3Q_MAXL + u] * s_cbo[w][a * E3Q_MAXL + v];                   // pot.F90:397, BO(i,j) BO(j,k) > cut-off: decided in single precision except within 1e-3 of the
        go = pr > 1.001e-4f;                                                // cut-off, where the double-precision product from memory decides (the same answers)
        if (!go && pr > 0.999e-4f) go = bo0[oi] * bo0[ok] > cutof2_esub;
        if (go) go = s_ix3[(static_cast<int>(btype[oi]) * ff.n1 + tj) * ff.n1 + static_cast<int>(btype[ok])] != 0;
        key = (a << 10) | (i1 << 5) | k1;
        if (++v >= nc) { u += LPA; v = u + 1; }
      }
      const unsigned long long m = __ballot(go);
      if (go) s_q[w][(qh + qn + __popcll(m & ((1ULL << lane) - 1ULL))) & 127] = static_cast<unsigned short>(key);
      qn += __popcll(m);
      wave_lds_sync();
      if (qn >= 64) { evaluate(64); qh = (qh + 64) & 127; qn -= 64; }
    }
    if (qn > 0) evaluate(qn);
  }
  // write-out: every bond of the wavefront's atoms, coalesced; then the centres' own forces
  for (int r = lane; r < nb_w; r += 64) {
    const int o = ob_w + r, a = s_own[w][r];
    const double S_d1 = s_at[w][a][0], S_v6 = s_at[w][a][1], S_v5 = s_at[w][a][2];
    const double c1 = s_acc[w][0][r] + (S_d1 + S_v6 * ipow7(bo0[o]));
    if (c1 != 0.0) cf1[o] += c1;
    if (S_v5 != 0.0) { cf2[o] += S_v5; cf3[o] += S_v5; }
    const double cd = s_acc[w][1][r], f0 = s_acc[w][2][r], f1 = s_acc[w][3][r], f2 = s_acc[w][4][r];
    if (cd != 0.0) cdn[o] += cd;
    if (f0 != 0.0 || f1 != 0.0 || f2 != 0.0) { fnx[o] += f0; fny[o] += f1; fnz[o] += f2; }
  }
  if (lane < na) {                                 // the centre's force: minus the sum of the forces on its neighbours (ForceA3 books -(fi + fk) on j)
    const int j = jbase + lane, r0 = s_ci[w][lane][1] - ob_w, nj = s_ci[w][lane][2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int t = 0; t < nj; ++t) { s0 += s_acc[w][2][r0 + t]; s1 += s_acc[w][3][r0 + t]; s2 += s_acc[w][4][r0 + t]; }
    if (s0 != 0.0 || s1 != 0.0 || s2 != 0.0) { fx[j] -= s0; fy[j] -= s1; fz[j] -= s2; }
  }
  wave_lds_sync();                                 // the next group rebuilds the tables
  }   // groups
  block_energy_add(e5, pe + 5); block_energy_add(e6, pe + 6); block_energy_add(e7, pe + 7);
}

void Engine::valence_angles() {
  double *pe_d = scal + SCAL_PE;
  // the work-queue form (k_e3q) when the angle tables fit LDS: sixteen centre atoms per wavefront where no bond list of the step is longer than 12,
  // eight up to 24, four beyond
  if (opt.e3b_queue != 0 && dff.n1 <= 8 && dff.nvaty <= 255) {
    const int maxl = longest_bond_list();
    auto go = [&](auto kern, int na, int minw) {
      const int NG = nblk(N, 4 * na);
      kern<<<std::min(NG, (num_cu * minw + 7) & ~7), 256, 0, stream>>>(N, NG, dff, boff, nbr, btype, type, pos[0], pos[1], pos[2], bo0, bo2, bo3, delta, nlp, dDlp, epen, ecoa, cf1, cf2, cf3, cdn, fnx, fny, fnz,
                                                                     cds, frc[0], frc[1], frc[2], pe_d, static_cast<int>(opt.e4b_probe));
    };
    const bool w3 = opt.e3b_queue == 3;
    if (maxl <= 12) { if (w3) go(k_e3q<3, 16>, 16, 3); else go(k_e3q<2, 16>, 16, 2); }
    else if (maxl <= 24) { if (w3) go(k_e3q<3, 8>, 8, 3); else go(k_e3q<2, 8>, 8, 2); }
    else { if (w3) go(k_e3q<3, 4>, 4, 3); else go(k_e3q<2, 4>, 4, 2); }
  } else
    k_e3b<<<nblk(N, 256), 256, 4 * 5 * E3B_CAP * sizeof(double), stream>>>(N, dff, boff, nbr, btype, type, pos[0], pos[1], pos[2], bo0, bo2, bo3, delta, nlp, dDlp, epen, ecoa, cf1, cf2, cf3, cdn, fnx, fny, fnz,
                                          cds, frc[0], frc[1], frc[2], pe_d);
  RX_HIP(hipGetLastError());                       // 70 KB of dynamic LDS: a refused launch must not pass for "no valence angles"
}

}  // namespace rxmd
