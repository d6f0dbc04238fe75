// device_io.hip -- rxmd_hip_evaluate_device: QEq + FORCE on arrays that already live on the device, in the caller's order.
// No counterpart in the reference (its QEq / FORCE take host arrays of module atoms); the array-shaped entry points of capi.hip are the same call
// through host memory.  Two kernels of this file frame the existing Engine::qeq() and Engine::force():
//   k_ingest_device   one pass over the atoms: pos3[natoms][3] -> the SoA pos[a], wrapped into the box; type and gid written; velocities and the
//                     extended-Lagrangian state zeroed; the start charges; a type outside the ffield raises the device error word
//   k_egress_device   frc[a] -> f3[natoms][3], q -> q_out, and the six virial sums this FORCE call added to the stress accumulators
// Single rank only: the atoms keep the caller's order because nothing migrates between ingest and egress.
// rxmd_hip_get_bonds_device, at the end of the file, is the way OUT for the bond-order graph FORCE leaves in the compact bond tables: two more kernels
//   k_bond_select / k_bond_fill   flag per table entry, exclusive sum, coordinate arrays (src, dst, bo, the three parts of bo, the bond vector)
#include "scan.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace rxmd {

// What the ghost build and the cell binning expect of a resident is the state COPYATOMS(MODE_MOVE) leaves (exchange.hip, k_seg_count<true> with
// dr = 0): an atom moves up when s <= 0 and down when lbox < s, s = Hi r - obox as xu2xs forms it, so residents have 0 < s <= lbox -- up to the
// rounding of the trip back to real coordinates, which is why every sweep pads its bounds (lists.hip, SWEEP_PAD = 1e-6 A) and clamps its cell
// indices.  One rank: lbox = 1, obox = 0.  The wrap here is n = floor(s), r' = r - (n1 a1 + n2 a2 + n3 a3):
//   - an atom with all three s in [0, 1) has n = 0 and keeps its coordinates bit for bit (s = 0 stays: within the rounding above of the face);
//   - r' is NOT formed as H frac(s): one subtraction at the magnitude of the input, a handful of roundings;
//   - s' = Hi r' is formed again and an axis that rounding left more than WRAP_TOL outside [0, 1] (inputs thousands of boxes away) is wrapped once
//     more; WRAP_TOL (normalised) times any box edge a run can hold stays three orders below SWEEP_PAD.  A coordinate of -1e-18 gives n = -1 and
//     r' = exactly one box length, s' = 1 to an ulp: inside the tolerance, left there.
constexpr double WRAP_TOL = 1e-12;

__device__ inline void to_normalised(const DevBox &B, double r0, double r1, double r2, double (&s)[3]) {   // the expression of k_seg_count
  s[0] = B.Hi[0] * r0 + B.Hi[1] * r1 + B.Hi[2] * r2;
  s[1] = B.Hi[3] * r0 + B.Hi[4] * r1 + B.Hi[5] * r2;
  s[2] = B.Hi[6] * r0 + B.Hi[7] * r1 + B.Hi[8] * r2;
}

// q_mode: 0 keep q (the previous call's solution, same natoms), 1 q = q_in, 2 q = 0
__global__ void __launch_bounds__(256) k_ingest_device(int n, int nso, DevBox B, const double *__restrict__ pos3, const int *__restrict__ type_in,
                                                        const long long *__restrict__ gid_in, const double *__restrict__ q_in, int q_mode,
                                                        double *__restrict__ x, double *__restrict__ y, double *__restrict__ z,
                                                        double *__restrict__ vx, double *__restrict__ vy, double *__restrict__ vz,
                                                        double *__restrict__ q, double *__restrict__ qsfp, double *__restrict__ qsfv,
                                                        int *__restrict__ type, long long *__restrict__ gid, int *err,
                                                        const double *__restrict__ acc6, double *__restrict__ head6) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 6) head6[threadIdx.x] = acc6[threadIdx.x];   // the stress accumulators as this call found them
  if (i >= n) return;
  double r0 = pos3[3 * static_cast<size_t>(i)], r1 = pos3[3 * static_cast<size_t>(i) + 1], r2 = pos3[3 * static_cast<size_t>(i) + 2];
  double s[3];
  to_normalised(B, r0, r1, r2, s);
  double n0 = floor(s[0]), n1 = floor(s[1]), n2 = floor(s[2]);
  if (n0 != 0.0 || n1 != 0.0 || n2 != 0.0) {
    r0 -= n0 * B.H[0] + n1 * B.H[1] + n2 * B.H[2];
    r1 -= n0 * B.H[3] + n1 * B.H[4] + n2 * B.H[5];
    r2 -= n0 * B.H[6] + n1 * B.H[7] + n2 * B.H[8];
    to_normalised(B, r0, r1, r2, s);
    n0 = (s[0] < -WRAP_TOL || s[0] > 1.0 + WRAP_TOL) ? floor(s[0]) : 0.0;
    n1 = (s[1] < -WRAP_TOL || s[1] > 1.0 + WRAP_TOL) ? floor(s[1]) : 0.0;
    n2 = (s[2] < -WRAP_TOL || s[2] > 1.0 + WRAP_TOL) ? floor(s[2]) : 0.0;
    if (n0 != 0.0 || n1 != 0.0 || n2 != 0.0) {
      r0 -= n0 * B.H[0] + n1 * B.H[1] + n2 * B.H[2];
      r1 -= n0 * B.H[3] + n1 * B.H[4] + n2 * B.H[5];
      r2 -= n0 * B.H[6] + n1 * B.H[7] + n2 * B.H[8];
    }
  }
  x[i] = r0; y[i] = r1; z[i] = r2;
  vx[i] = 0.0; vy[i] = 0.0; vz[i] = 0.0;
  qsfp[i] = 0.0; qsfv[i] = 0.0;
  if (q_mode == 1) q[i] = q_in[i]; else if (q_mode == 2) q[i] = 0.0;
  int t = type_in[i];
  if (t < 1 || t > nso) { atomicCAS(&err[0], DERR_NONE, DERR_TYPE); t = 1; }      // as k_split_atype: the kernels behind stay inside the tables
  type[i] = t;
  gid[i] = gid_in ? gid_in[i] : static_cast<long long>(i) + 1;
}

// virial_host: pinned host memory (h_scal); the host reads it behind the stream synchronisation of finish_force
__global__ void __launch_bounds__(256) k_egress_device(int n, const double *__restrict__ fx, const double *__restrict__ fy, const double *__restrict__ fz,
                                                        const double *__restrict__ q, double *__restrict__ f3, double *__restrict__ q_out,
                                                        const double *__restrict__ acc6, const double *__restrict__ head6, double *virial_host) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 6) virial_host[threadIdx.x] = acc6[threadIdx.x] - head6[threadIdx.x];
  if (i >= n) return;
  if (f3) { f3[3 * static_cast<size_t>(i)] = fx[i]; f3[3 * static_cast<size_t>(i) + 1] = fy[i]; f3[3 * static_cast<size_t>(i) + 2] = fz[i]; }
  if (q_out) q_out[i] = q[i];
}

// The first call sizes the engine as rxmd_hip_set_atoms_rxff does: types and positions cross to the host ONCE, as rxff.bin records with the
// normalised coordinates folded into [0, 1); the ingest kernel then overwrites what the records left on the device.
void Engine::size_from_device_arrays(int natoms, const int *type_d, const double *pos3_d, hipStream_t user) {
  RX_HIP(hipStreamSynchronize(user));
  std::vector<int> ht(natoms);
  std::vector<double> hp(3 * static_cast<size_t>(natoms)), rec(10 * static_cast<size_t>(natoms), 0.0);
  RX_HIP(hipMemcpy(ht.data(), type_d, sizeof(int) * natoms, hipMemcpyDeviceToHost));
  RX_HIP(hipMemcpy(hp.data(), pos3_d, sizeof(double) * 3 * static_cast<size_t>(natoms), hipMemcpyDeviceToHost));
  for (int i = 0; i < natoms; ++i) {
    const double *r = hp.data() + 3 * static_cast<size_t>(i);
    double *o = rec.data() + 10 * static_cast<size_t>(i);
    for (int a = 0; a < 3; ++a) {
      const double s = box.Hi[a][0] * r[0] + box.Hi[a][1] * r[1] + box.Hi[a][2] * r[2];
      o[a] = std::isfinite(s) ? s - std::floor(s) : 0.0;
    }
    o[7] = static_cast<double>(ht[i]);              // (the gid comes with the ingest)
  }
  set_atoms_rxff(natoms, rec.data());               // RXMD_E_ARG for a type outside the ffield
}

void Engine::evaluate_device(int natoms, const long long *gid_d, const int *type_d, const double *pos3_d, const double *q_in_d, double *f3_d, double *q_out_d,
                             double pe_out[14], double virial_out[6], hipStream_t user) {
  if (nprocs != 1) throw EngineError(RXMD_E_ARG, "evaluate_device: single rank only (vprocs must be 1 1 1)");
  if (ff.pqeq) throw EngineError(RXMD_E_ARG, "evaluate_device: not available on an engine created with pqeq_path (the shells would have to persist between calls)");
  if (cfg.isQEq == 2) throw EngineError(RXMD_E_ARG, "evaluate_device: isQEq = 2 is not available (the extended-Lagrangian state belongs to the integrator)");
  if (natoms < 1) throw EngineError(RXMD_E_ARG, "evaluate_device: natoms must be positive");
  if (!type_d || !pos3_d) throw EngineError(RXMD_E_ARG, "evaluate_device: type and pos3 must not be NULL");
  const int warm_n = eval_natoms;
  if (!tables_ready) size_from_device_arrays(natoms, type_d, pos3_d, user);
  if (natoms > rows10 || natoms >= NB) throw EngineError(RXMD_E_NBUFFER, "evaluate_device: more atoms than the engine was sized for (" + std::to_string(std::min(rows10, NB - 1)) + ")");
  sync_stream();                                   // nothing of the previous call may still read what is overwritten
  eval_natoms = -1;                                // (until this call has gone through)
  last_atype.clear();                              // the array-shaped entry points must not take these atoms for theirs
  UserStream io(this, user);
  for (int a = 0; a < 3; ++a) RX_HIP(hipMemsetAsync(frc[a], 0, sizeof(double) * NB, stream));
  const int q_mode = q_in_d ? 1 : (warm_n == natoms ? 0 : 2);
  k_ingest_device<<<nblk(natoms, 256), 256, 0, stream>>>(natoms, ff.nso, dev_box(box), pos3_d, type_d, gid_d, q_in_d, q_mode, pos[0], pos[1], pos[2], vel[0], vel[1], vel[2],
                                                          q, qsfp, qsfv, type, gid, d_err, scal + SCAL_ASTR, scal + SCAL_EVAL_HEAD);
  N = natoms; G = natoms;
  atoms_set = true; lists_valid = false; ghosts_valid = false;
  atype_resid = 0.0;
  st.natoms = N;
  qeq();                                           // (isQEq = 0: returns at once, the charges are the caller's)
  force(true);                                     // the list build in front of either reports a type outside the ffield (RXMD_E_ARG)
  k_egress_device<<<nblk(natoms, 256), 256, 0, stream>>>(natoms, frc[0], frc[1], frc[2], q, f3_d, q_out_d, scal + SCAL_ASTR, scal + SCAL_EVAL_HEAD, h_scal + H_SCAL_EVAL_VIRIAL);
  io.end();                                        // (in front of the NaN trap: the caller's stream is joined even when it throws)
  finish_force();                                  // the host wait of the call: energies, NaN trap
  if (pe_out) for (int k = 0; k < 14; ++k) pe_out[k] = pe[k];
  if (virial_out) for (int c = 0; c < 6; ++c) virial_out[c] = h_scal[H_SCAL_EVAL_VIRIAL + c];
  eval_natoms = natoms;
}

// ---- rxmd_hip_get_bonds_device: the bond-order graph as coordinate arrays ---------------------------------------------------------------
// A lane per entry o of the residents' part of the compact tables (o < boff[N] = nbonds_res), three launches:
//   k_bond_select   flag[o] = bo0[o] >= bo_min (bo_min <= 0: every entry); flag[n] = 0 so that the exclusive sum behind it leaves the total in off[n]
//   hipcub exclusive sum flag -> off: a stable compaction in table order (resident order, then list order), no atomics
//   k_bond_fill     entry o -> output e = off[o].  bown / nbr / bo0..3 / flag / off are read coalesced and the outputs stored coalesced where the selection
//                   is dense; gid / groot / pos are gathers by atom index.  Per selected entry: 4 + 4 + 4 + 4 bytes of indices and 8 of bo0 in, 24 out
//                   (src, dst, bo); + 24 in and 24 out for bo3; + 48 gathered and 24 out for vec3; + 16 gathered for global ids or 4 for a ghost's root.
// Nothing here is on the path of qeq(), force() or step().
__global__ void __launch_bounds__(256) k_bond_select(int n, double bo_min, const double *__restrict__ bo0, int *__restrict__ flag) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o > n) return;
  flag[o] = (o < n && (bo_min <= 0.0 || bo0[o] >= bo_min)) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_bond_fill(int n, int nres, int as_gid, const int *__restrict__ flag, const int *__restrict__ off,
                                                    const int *__restrict__ bown, const int *__restrict__ nbr, const double *__restrict__ bo0,
                                                    const double *__restrict__ bo1, const double *__restrict__ bo2, const double *__restrict__ bo3,
                                                    const long long *__restrict__ gid, const int *__restrict__ groot, const long long *__restrict__ gowner,
                                                    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                    long long *__restrict__ src, long long *__restrict__ dst, double *__restrict__ bo,
                                                    double *__restrict__ parts3, double *__restrict__ vec3) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n || !flag[o]) return;
  const size_t e = static_cast<size_t>(off[o]);
  const int i = bown[o], j = nbr[o];
  if (as_gid) { src[e] = gid[i]; dst[e] = gid[j]; }
  else {
    src[e] = i;
    dst[e] = j < nres ? j : ghost_owner(j, gowner, groot);
  }
  bo[e] = bo0[o];
  if (parts3) { parts3[3 * e] = bo1[o]; parts3[3 * e + 1] = bo2[o]; parts3[3 * e + 2] = bo3[o]; }
  if (vec3) { vec3[3 * e] = x[j] - x[i]; vec3[3 * e + 1] = y[j] - y[i]; vec3[3 * e + 2] = z[j] - z[i]; }   // the ghost IS the right periodic image: no minimum-image step
}

// select + exclusive sum over the residents' entries, shared with the VJP of the graph (bond_vjp.hip): the same flags, the same offsets, the same count
long long Engine::select_bonds(double bo_min) {
  if (force_pending) finish_force();               // (FORCE itself joins the bonded chain's stream and the halo stream in front of its end)
  const int n = nbonds_res;
  if (n <= 0) return 0;
  if (!bg_flag || bufs.cap[G_BGRAPH] < bcap) regrow_group(G_BGRAPH, bcap);   // first use, or the bond tables have grown since (the fill kernel of an earlier call may still read the old blocks)
  k_bond_select<<<nblk(static_cast<long long>(n) + 1, 256), 256, 0, stream>>>(n, bo_min, bo0, bg_flag);
  return exclusive_sum_total(bg_flag, bg_off, n);
}

long long Engine::bonds_device(int flags, double bo_min, long long capacity, long long *src_d, long long *dst_d, double *bo_d, double *bo3_d, double *vec3_d, hipStream_t user) {
  const bool count_only = !src_d && !dst_d && !bo_d;
  const bool as_gid = (flags & RXMD_BONDS_GID) != 0;
  if (flags & ~RXMD_BONDS_GID) throw EngineError(RXMD_E_ARG, "get_bonds_device: unknown bit in flags");
  if (!std::isfinite(bo_min)) throw EngineError(RXMD_E_ARG, "get_bonds_device: bo_min must be finite");
  if (!count_only && (!src_d || !dst_d || !bo_d)) throw EngineError(RXMD_E_ARG, "get_bonds_device: src, dst and bo go together (all three NULL: count only)");
  if (!count_only && capacity < 0) throw EngineError(RXMD_E_ARG, "get_bonds_device: negative capacity");
  if (!as_gid && nprocs != 1) throw EngineError(RXMD_E_ARG, "get_bonds_device: local indices need a single rank (vprocs 1 1 1); ask for global ids (RXMD_BONDS_GID)");
  if (!atoms_set || !lists_valid) throw EngineError(RXMD_E_STATE, "no bond lists: call rxmd_hip_force first");
  const int n = nbonds_res;
  const long long E = select_bonds(bo_min);          // the host wait of the call
  if (count_only || capacity < E || E == 0) return E;
  UserStream io(this, user);                         // whatever the caller's stream still does with the output arrays comes first
  k_bond_fill<<<nblk(n, 256), 256, 0, stream>>>(n, N, as_gid ? 1 : 0, bg_flag, bg_off, bown, nbr, bo0, bo1, bo2, bo3, gid, groot, multi() ? gowner : nullptr,
                                                pos[0], pos[1], pos[2], src_d, dst_d, bo_d, bo3_d, vec3_d);
  io.end();
  return E;
}

}  // namespace rxmd
