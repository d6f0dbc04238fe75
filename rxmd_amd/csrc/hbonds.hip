// hbonds.hip -- Ehb, the hydrogen-bond term of FORCE (reference src/pot.F90:559-673): k_ehb_donors + k_ehb_sweep, the two utility kernels around the
// sweep, and Engine::hydrogen_bonds().  The accumulators the kernels add to are described at the head of bonded.hip.
#include "bonded_common.h"

#include <algorithm>

namespace rxmd {

// Hydrogen bonds, round 5: two kernels instead of one search-and-sweep.  The counters of the one-kernel form (profiles/r05_a_sq_*): 61,240
// wavefronts that each live ~60 us, 87 % of it parked on s_waitcnt behind ~66 dependent loads (the donor search walks type[nbr[o]] and
// bo0[o] slot by slot; then position, row, hydrogen, candidates one round trip after the other), the vector unit busy 6 % of the time, and
// 22 M atomic requests at the memory side for the 51 M acceptor-force additions.
//   k_ehb_donors  one thread per resident: the slots of its bond list that hold a hydrogen (type 2, pot.F90:595) with BO > MINBO0, from the
//                 CSR tables (the partner's type rides with the bond: no gather); atoms with one are appended to a donor list (ballot + one
//                 atomic per wavefront; the order of the list is arbitrary -- every sum behind it is an atomic or owned by one wavefront).
//   k_ehb_sweep   a persistent grid; a wavefront takes whole donors: the row's acceptor candidates are compacted into LDS (<= EHB_CAP at a time),
//                 their positions gathered ONCE into LDS, then every hydrogen slot of the donor walks the staged candidates four dense batches
//                 at a time out of LDS -- no load inside the evaluation -- and the acceptor's force is summed over the hydrogen slots in
//                 registers before its three atomics.
// Measured (979,776 atoms, profiles/r05_*): without the acceptor atomics the sweep takes 0.40 ms (the one-kernel form: 0.70), with them 1.07 --
// 51 M FP64 adds at the memory side are 0.67 ms whatever the wavefronts do around them (candidates sorted by atom index so that the acceptors of
// one molecule sit in neighbouring lanes: 1.00; RDX donors have ONE hydrogen, so summing over slots saves nothing there).  The atomics are the floor.
constexpr int EHB_CAP = 256;                              // candidates staged per flush (a 447-entry RDX row has <= 255 N / O partners)
constexpr int EHB_REGIONS = 64;                           // sub-lists of the donor list, each with its own counter
__global__ void __launch_bounds__(256) k_ehb_donors(int N, unsigned donor_types, const int *__restrict__ boff, const unsigned char *__restrict__ btype, const double *__restrict__ bo0,
                                                     const int *__restrict__ type, int2 *__restrict__ don, int *__restrict__ cnt, int region_cap) {
  // the list is EHB_REGIONS lists (workgroup b appends to region b mod EHB_REGIONS, region_cap entries each): 15,000 returning atomics on ONE
  // counter were 0.15 ms of this 0.18 ms kernel
  const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, reg = blockIdx.x & (EHB_REGIONS - 1);
  unsigned hm = 0u;
  if (i < N && ((donor_types >> (type[i] & 31)) & 1u)) {
    const int ob = boff[i], n = min(boff[i + 1] - ob, 32);
    unsigned hs = 0u;                                                   // the slots that hold a hydrogen: one pass over the type bytes (independent loads) ...
    for (int s = 0; s < n; ++s) hs |= (btype[ob + s] == 2 ? 1u : 0u) << s;
    for (unsigned m_ = hs; m_; m_ &= m_ - 1u) {                         // ... then the bond order of those only (most N / O atoms have none or one)
      const int s = __ffs(m_) - 1;
      if (bo0[ob + s] > MINBO0) hm |= 1u << s;                          // pot.F90:595
    }
  }
  const unsigned long long m = __ballot(hm != 0u);
  if (m == 0ULL) return;
  const int first = __ffsll(static_cast<long long>(m)) - 1;
  int base = 0;
  if (lane == first) base = atomicAdd(cnt + reg, __popcll(m));
  base = __shfl(base, first, 64);
  if (hm != 0u) don[static_cast<size_t>(reg) * region_cap + base + __popcll(m & ((1ULL << lane) - 1ULL))] = make_int2(i, static_cast<int>(hm));
}

// SLOTS: the build left the 4-byte entries out (lists.hip: needs_nb10).  A donor row's partners then come from its 2-byte window slots, as in
// k_nonbond_win: position = first position of the slot's unit in the window of the row's group + offset in the unit, type from the cell-sorted type
// bytes.  Both streams hold a row's entries at the same indices, so the candidates -- and the acceptor atomics -- come in the same order.
template <bool SLOTS>
__global__ void __launch_bounds__(256) k_ehb_sweep(int S10, DevFF ff, const int2 *__restrict__ don, const int *__restrict__ ndon, int region_cap, const int *__restrict__ boff, const int *__restrict__ nbr,
                                                    const int *__restrict__ type, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                    const double *__restrict__ bo0, const int *__restrict__ nb10, const int *__restrict__ n10, const double4 *__restrict__ pk, const int *__restrict__ perm,
                                                    double *__restrict__ cf1, double *__restrict__ fnx, double *__restrict__ fny, double *__restrict__ fnz,
                                                    double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz, double *__restrict__ pe,
                                                    double *__restrict__ fsx, double *__restrict__ fsy, double *__restrict__ fsz,
                                                    const unsigned short *__restrict__ sl10, const int *__restrict__ rpos, const int *__restrict__ win_k, const unsigned char *__restrict__ stype, int G, int byplace
#ifdef RXMD_EHB_DEBUG
                                                    , int *dbg, int lim_n, int lim_b, int lim_nb
#endif
                                                    ) {
#ifdef RXMD_EHB_DEBUG
#define EHB_CHECK(code, v, lim, aux) if ((v) < 0 || (v) >= (lim)) { if (atomicCAS(dbg, 0, (code)) == 0) { dbg[1] = (v); dbg[2] = (aux); dbg[3] = (lim); } return; }
#define EHB_CHECKC(code, v, lim, aux) if ((v) < 0 || (v) >= (lim)) { if (atomicCAS(dbg, 0, (code)) == 0) { dbg[1] = (v); dbg[2] = (aux); dbg[3] = (lim); } continue; }
#else
#define EHB_CHECK(code, v, lim, aux)
#define EHB_CHECKC(code, v, lim, aux)
#endif
  __shared__ unsigned s_cand[4][EHB_CAP];                 // compacted list entries of the row (type bits select the parameter row)
  __shared__ double s_px[4][EHB_CAP], s_py[4][EHB_CAP], s_pz[4][EHB_CAP];
  __shared__ int s_k[4][EHB_CAP];
  __shared__ double s_hp[4][16][4];                       // (ti, H, type k) parameter rows of the current donor, by acceptor type
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  // the donor list is EHB_REGIONS sub-lists: lane r holds the inclusive prefix of their lengths; donor d lives in the first region whose prefix exceeds d
  int pre = ndon[lane & (EHB_REGIONS - 1)];
#pragma unroll
  for (int o = 1; o < EHB_REGIONS; o <<= 1) { const int t = __shfl_up(pre, o, 64); if (lane >= o) pre += t; }
  const int nw = gridDim.x * 4, nd = __shfl(pre, EHB_REGIONS - 1, 64);
  double e10 = 0.0;
  for (int d = blockIdx.x * 4 + w; d < nd; d += nw) {
    const int reg = __popcll(__ballot(pre <= d));                       // (EHB_REGIONS == 64: one lane per region)
    const int before = reg > 0 ? __shfl(pre, reg - 1, 64) : 0;
    const int2 rec = don[static_cast<size_t>(reg) * region_cap + (d - before)];
    const int i = __builtin_amdgcn_readfirstlane(rec.x);
    const unsigned hmask = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(rec.y));
    EHB_CHECK(1, i, lim_n, d)
    const int ti = type[i], ob = boff[i], n = n10[i] & N10_COUNT;
    EHB_CHECK(2, ob, lim_b - 32, i)
    EHB_CHECK(3, n, S10 + 1, i)
    const double xi = x[i], yi = y[i], zi = z[i];
    const size_t row = static_cast<size_t>(byplace ? rpos[i] : i) * S10;   // (Engine::streams_by_place)
    const int *wk = SLOTS ? win_k + static_cast<size_t>(rpos[i] / WIN_ROWS) * WIN_MAXUNITS : nullptr;   // the window of the donor's group
    const int inx_l = (lane >= 1 && lane <= ff.nso && lane < 16) ? ff.inxn3hb[(ti * ff.n1 + 2) * ff.n1 + lane] : 0;
    if (lane < 16) { const DevHbP hp = ff.hb[inx_l]; s_hp[w][lane][0] = hp.r0hb; s_hp[w][lane][1] = hp.phb1; s_hp[w][lane][2] = hp.phb2; s_hp[w][lane][3] = hp.phb3; }   // (row 0 is never used: the compaction drops its candidates)
    int jl = 0; double bl = 0.0, xjl = 0.0, yjl = 0.0, zjl = 0.0;        // lane s holds atom, bond order and position of hydrogen slot s
    if (lane < 32 && ((hmask >> lane) & 1u)) { jl = nbr[ob + lane];
#ifdef RXMD_EHB_DEBUG
      if (jl < 0 || jl >= lim_nb) { if (atomicCAS(dbg, 0, 4) == 0) { dbg[1] = jl; dbg[2] = i; dbg[3] = lane; } jl = 0; }
#endif
      bl = bo0[ob + lane]; xjl = x[jl]; yjl = y[jl]; zjl = z[jl]; }
    V3 fi_t = {0, 0, 0};
    int qn = 0;

    auto flush = [&]() {                                    // the staged candidates against every hydrogen slot of the donor
      wave_lds_sync();
      for (int q = lane; q < qn; q += 64) {
        EHB_CHECKC(5, static_cast<int>(s_cand[w][q] & NB10_IDX_MASK), lim_nb, i)
        const int ks = static_cast<int>(s_cand[w][q] & NB10_IDX_MASK);       // list entries are cell-sorted positions; the atom comes from perm
        // x, y, z ONLY: the w component of the packed copy is rewritten with the charge by k_sorted_charge on the MAIN stream while this kernel runs
        // on the bonded chain's stream (assemble.hip: bonded_chain_begin) -- a 32-byte load of the element would be an unordered read of that word
        const double2 pxy = *reinterpret_cast<const double2 *>(pk + ks);
        s_px[w][q] = pxy.x; s_py[w][q] = pxy.y; s_pz[w][q] = reinterpret_cast<const double *>(pk + ks)[2]; s_k[w][q] = perm[ks];
      }
      wave_lds_sync();
      double akx[EHB_CAP / 64], aky[EHB_CAP / 64], akz[EHB_CAP / 64];       // acceptor force of this lane's candidate of each batch, summed over the hydrogen slots
#pragma unroll
      for (int b = 0; b < EHB_CAP / 64; ++b) { akx[b] = 0.0; aky[b] = 0.0; akz[b] = 0.0; }
      for (unsigned hm = hmask; hm; hm &= hm - 1u) {
        const int s = __ffs(hm) - 1;
        const int j = __shfl(jl, s, 64);
        const double BOij = __shfl(bl, s, 64);
        const double xj = __shfl(xjl, s, 64), yj = __shfl(yjl, s, 64), zj = __shfl(zjl, s, 64);
        const V3 rij = {xi - xj, yi - yj, zi - zj};
        const double nij = sqrt(dot(rij, rij));
        double cfs = 0.0, nterm = 0.0;
        V3 fi_s = {0, 0, 0}, fj_s = {0, 0, 0};
#pragma unroll
        for (int b = 0; b < EHB_CAP / 64; ++b) {
          const int qq = 64 * b + lane;
          if (qq >= qn) continue;
          const int k = s_k[w][qq];
          if (k == j || k == i) continue;
          const double *hp = s_hp[w][(s_cand[w][qq] >> NB10_IDX_BITS) & 15u];
          const double r0hb = hp[0], phb1 = hp[1], phb2 = hp[2], phb3 = hp[3];
          const double pxk = s_px[w][qq], pyk = s_py[w][qq], pzk = s_pz[w][qq];
          const V3 rik = {xi - pxk, yi - pyk, zi - pzk};
          if (!(dot(rik, rik) < 100.0)) continue;                          // rchb2, pot.F90:610
          const V3 rjk = {xj - pxk, yj - pyk, zj - pzk};
          const double njk = sqrt(dot(rjk, rjk));
          double cos_ijk = -dot(rij, rjk) / (nij * njk);
          if (cos_ijk > MAXANGLE) cos_ijk = MAXANGLE;
          if (cos_ijk < MINANGLE) cos_ijk = MINANGLE;
          const double sh2 = 0.5 * (1.0 - cos_ijk);                        // sin^2(theta/2)
          const double sin_xhz4 = sh2 * sh2, cos_xhz1 = 1.0 - cos_ijk;
          const double exp_hb2 = exp(-phb2 * BOij);
          const double exp_hb3 = exp(-phb3 * (r0hb / njk + njk / r0hb - 2.0));
          const double PEhb = phb1 * (1.0 - exp_hb2) * exp_hb3 * sin_xhz4;
          e10 += PEhb; nterm += 1.0;
          cfs += phb1 * phb2 * exp_hb2 * exp_hb3 * sin_xhz4;               // CEhb(1) -> ForceB(i,j)
          const double CEhb2 = -0.5 * phb1 * (1.0 - exp_hb2) * exp_hb3 * cos_xhz1;
          const double CEhb3 = -PEhb * phb3 * (-r0hb / (njk * njk) + 1.0 / r0hb) * (1.0 / njk);
          V3 fi, fk;
          angle_forces(CEhb2, rij, nij, rjk, njk, fi, fk);
          const V3 ff3 = {CEhb3 * rjk.x, CEhb3 * rjk.y, CEhb3 * rjk.z};   // f(j) -= ff ; f(k) += ff
          fi_s.x += fi.x; fi_s.y += fi.y; fi_s.z += fi.z;
          fj_s.x += -(fi.x + fk.x) - ff3.x; fj_s.y += -(fi.y + fk.y) - ff3.y; fj_s.z += -(fi.z + fk.z) - ff3.z;
          akx[b] += fk.x + ff3.x; aky[b] += fk.y + ff3.y; akz[b] += fk.z + ff3.z;
        }
        cfs = wave_sum64(cfs); nterm = wave_sum64(nterm);
        fj_s.x = wave_sum64(fj_s.x); fj_s.y = wave_sum64(fj_s.y); fj_s.z = wave_sum64(fj_s.z);
        fi_t.x += fi_s.x; fi_t.y += fi_s.y; fi_t.z += fi_s.z;
        if (lane == 0 && nterm > 0.0) {                     // the donor's bonds belong to this wavefront alone
          const int o = ob + s;
          cf1[o] += cfs;
          fnx[o] += fj_s.x; fny[o] += fj_s.y; fnz[o] += fj_s.z;
        }
      }
#pragma unroll
      for (int b = 0; b < EHB_CAP / 64; ++b) {
        const int qq = 64 * b + lane;
        if (qq < qn && (akx[b] != 0.0 || aky[b] != 0.0 || akz[b] != 0.0)) {
          // the acceptor's force goes to its CELL-SORTED position: the candidates of a row are neighbours in that order, so the lanes of one atomic
          // instruction hit neighbouring addresses and share memory-side requests (by atom index they are scattered: 2.2 lanes per request)
          const int ks = static_cast<int>(s_cand[w][qq] & NB10_IDX_MASK);
          EHB_CHECKC(6, ks, lim_nb, qq)
          atomicAdd(fsx + ks, akx[b]); atomicAdd(fsy + ks, aky[b]); atomicAdd(fsz + ks, akz[b]);
        }
      }
      wave_lds_sync();
      qn = 0;
    };

    for (int c0 = 0; c0 < n; c0 += 256) {                   // four batches of entry words requested together
      unsigned ent[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = c0 + 64 * u + lane;
        if (SLOTS) {
          ent[u] = 0xffffffffu;
          if (kk < n) {
            const int sl = sl10[row + kk] & 0x7fff;
            const int pos = min(wk[sl / WIN_UNIT] + (sl & (WIN_UNIT - 1)), G - 1);
            ent[u] = static_cast<unsigned>(pos) | (static_cast<unsigned>(stype[pos]) << NB10_IDX_BITS);
          }
        } else ent[u] = kk < n ? static_cast<unsigned>(nb10[row + kk]) : 0xffffffffu;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (c0 + 64 * u >= n) break;                                        // wave-uniform
        const int inx = __shfl(inx_l, static_cast<int>((ent[u] >> NB10_IDX_BITS) & 15u), 64);   // (ti, H, type k) row, held by lane = type k
        const bool keep = ent[u] != 0xffffffffu && inx != 0;
        const unsigned long long m = __ballot(keep);
        if (keep) s_cand[w][qn + __popcll(m & ((1ULL << lane) - 1ULL))] = ent[u];
        qn += __popcll(m);
        if (qn > EHB_CAP - 64) flush();
      }
    }
    if (qn > 0) flush();
    fi_t.x = wave_sum64(fi_t.x); fi_t.y = wave_sum64(fi_t.y); fi_t.z = wave_sum64(fi_t.z);
    if (lane == 0 && (fi_t.x != 0.0 || fi_t.y != 0.0 || fi_t.z != 0.0)) { atomicAdd(fx + i, fi_t.x); atomicAdd(fy + i, fi_t.y); atomicAdd(fz + i, fi_t.z); }
    wave_lds_sync();                                        // the next donor rewrites the parameter rows
  }
  block_energy_add(e10, pe + 10);
}

__global__ void k_zero3(int n, double *__restrict__ a, double *__restrict__ b, double *__restrict__ c) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) { a[k] = 0.0; b[k] = 0.0; c[k] = 0.0; }
}
// frc[atom at sorted position k] += the acceptor forces the hydrogen-bond sweep left at position k (perm is a permutation: no two threads meet)
__global__ void k_add_sorted3(int G, const int *__restrict__ perm, const double *__restrict__ sx, const double *__restrict__ sy, const double *__restrict__ sz,
                              double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= G) return;
  const double a = sx[k], b = sy[k], c = sz[k];
  if (a != 0.0 || b != 0.0 || c != 0.0) { const int i = perm[k]; fx[i] += a; fy[i] += b; fz[i] += c; }
}

void Engine::hydrogen_bonds() {
  if (ehb_donor_types == 0u) return;              // (a force field without a hydrogen-bond row for hydrogen = type 2 has no donors: water, pot.F90:595)
  double *pe_d = scal + SCAL_PE;
  const int region_cap = (nblk(N, 256) + EHB_REGIONS - 1) / EHB_REGIONS * 256;            // every atom of the workgroups of a region a donor: cannot overflow
  if (static_cast<size_t>(region_cap) * EHB_REGIONS > ehb_don_cap) throw EngineError(RXMD_E_STATE, "hydrogen-bond donor list: capacity");
  RX_HIP(hipMemsetAsync(ehb_cnt, 0, sizeof(int) * EHB_REGIONS, stream));
  k_ehb_donors<<<nblk(N, 256), 256, 0, stream>>>(N, ehb_donor_types, boff, btype, bo0, type, ehb_don, ehb_cnt, region_cap);
  k_zero3<<<nblk(G, 256), 256, 0, stream>>>(G, fsort[0], fsort[1], fsort[2]);
  if (ehb_blocks_per_cu == 0) {                   // the persistent grid fills the device exactly: workgroups per CU from the kernel's own register / LDS footprint
    int nbk = 0;
    RX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbk, k_ehb_sweep<false>, 256, 0));
    ehb_blocks_per_cu = std::max(nbk, 1);
    RX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbk, k_ehb_sweep<true>, 256, 0));
    ehb_blocks_per_cu_sl = std::max(nbk, 1);
  }
  const bool slots = !nb10_valid;                 // (then this build has its windows: build_ghosts_and_lists sweeps a build without either again)
  const int ehb_grid = num_cu * (slots ? ehb_blocks_per_cu_sl : ehb_blocks_per_cu);
  auto sweep = [&](auto... dbg) {                 // dbg: the kernel's trailing arguments under RXMD_EHB_DEBUG, empty otherwise
    auto go = [&](auto kern) {
      kern<<<ehb_grid, 256, 0, stream>>>(S10, dff, ehb_don, ehb_cnt, region_cap, boff, nbr, type, pos[0], pos[1], pos[2], bo0, nb10, n10, sorted_xyzi, perm, cf1, fnx, fny, fnz, frc[0], frc[1], frc[2], pe_d,
                                         fsort[0], fsort[1], fsort[2], sl10, rpos, win_k, sorted_type, G, streams_by_place ? 1 : 0, dbg...);
    };
    if (slots) go(k_ehb_sweep<true>); else go(k_ehb_sweep<false>);
  };
#ifdef RXMD_EHB_DEBUG
  RX_HIP(hipMemsetAsync(ehb_cnt + EHB_REGIONS, 0, 4 * sizeof(int), stream));
  sweep(ehb_cnt + EHB_REGIONS, N, static_cast<int>(bcap), NB);
  { int hd[EHB_REGIONS + 4]; RX_HIP(hipMemcpyAsync(hd, ehb_cnt, sizeof(hd), hipMemcpyDeviceToHost, stream)); RX_HIP(hipStreamSynchronize(stream));
    for (int r = 1; r < EHB_REGIONS; ++r) hd[0] += hd[r];
    hd[4] = hd[EHB_REGIONS]; hd[5] = hd[EHB_REGIONS + 1]; hd[6] = hd[EHB_REGIONS + 2]; hd[7] = hd[EHB_REGIONS + 3];
    std::fprintf(stderr, "[ehb debug] donors %d  blocks/CU %d  first violation: code %d value %d aux %d lim %d   (N %d bcap %zu NB %d S10 %d rows10 %d)\n", hd[0], ehb_blocks_per_cu, hd[4], hd[5], hd[6], hd[7], N, bcap, NB, S10, rows10); }
#else
  sweep();
#endif
  k_add_sorted3<<<nblk(G, 256), 256, 0, stream>>>(G, perm, fsort[0], fsort[1], fsort[2], frc[0], frc[1], frc[2]);
}

}  // namespace rxmd
