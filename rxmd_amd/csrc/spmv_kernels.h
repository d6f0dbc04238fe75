// spmv_kernels.h -- the two forms of the QEq matrix pass (get_hsh / get_gradient, reference src/qeq.F90:271-363) and what they share with the
// vector kernels of the CG: k_spmv (one wavefront per row, 16-byte gather per entry) and k_spmv_win (the window pass: 16 cell-sorted rows per
// workgroup, partners staged in LDS, 16-bit slots).  Included by qeq.hip (the product) and by experiments.hip (timing probes and variants that
// launch the same kernels; compiled only by `make experiments`).
#pragma once
#include "engine.h"

#include <type_traits>

namespace rxmd {

enum { MODE_HSH = 0, MODE_GRAD = 1 };      // (the CG scalars S_* and their snapshot slots: the layout block of engine.h)
typedef double f64x2 __attribute__((ext_vector_type(2)));
#ifndef SPMV_UNR
#define SPMV_UNR 4
#endif
constexpr int UNR = SPMV_UNR;
__device__ inline double wave_sum(double v) { return wave_sum64(v); }   // DPP reduction, engine.h

template <int NC>
__device__ inline void block_store_partials(double (&acc)[NC], double *partials, int ncomp_stride) {
  // acc holds lane-0-of-wave partials; combine the block's waves in wave order, then one store per component
  __shared__ double sm[16][NC];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (lane == 0)
    for (int c = 0; c < NC; ++c) sm[w][c] = acc[c];
  __syncthreads();
  if (threadIdx.x < NC) {
    double s = 0.0;
    for (int k = 0; k < nw; ++k) s += sm[k][threadIdx.x];
    // device-scope store: written through to the coherence point, so the in-kernel tail (block_finish) needs no L2 write-back
    __hip_atomic_store(partials + static_cast<size_t>(blockIdx.x) * ncomp_stride + threadIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// PQEq (pqrow != nullptr): the second pair of sums (gs_,gt_) is over the shell-core matrix hsc instead of the ghost columns;
// gradient gets the field term fpqeq (pqeq.F90:466), Est the core/shell terms of pqeq.F90:381-411 without the resident doubling
__device__ inline double pq_est_row(const DevAtomP &ap, double Zi, const double4 &pr, double qi, double hq, double bq) {
  return ap.chi * qi + 0.5 * ap.eta * qi * qi + 0.5 * (qi + Zi) * (hq + pr.y) + pr.w - (bq + pr.z);
}
// STORE (qeq_mode 1): additionally keep the raw row sums (all columns / ghost columns) so that the next gradient and Est
// follow from  H.(q + l h) = H.q + l H.h  with N-sized vector kernels instead of a second matrix pass.
// One wavefront = one row (the launch covers the rows exactly), 16 rows per workgroup: workgroup dispatch is not free at a million
// wavefronts per pass (measured 1.25 / 1.24 / 1.15-1.19 / 1.13 / 1.08-1.11 ms at 1 / 2 / 4 / 8 / 16 wavefronts per workgroup; splitting
// a row over 2 or 4 wavefronts instead: 1.22 / 2.19 ms).  The pass is bound by
// LATENCY x occupancy, not by instruction issue: a wavefront lives for a chain of dependent memory round trips (row length ->
// the two streams -> the gathers -> the operands of the tail), so (a) the tail operands are requested first, next to the row
// length, (b) four batches of 64 entries are in flight instead of eight, which brings the kernel from 99 to <= 80 VGPRs and from
// 4 to 6 wavefronts per SIMD (measured on one box: 1.276 ms -> 1.21 with (a), 1.157 with (b), 1.06-1.12 with both), (c) PQEq is
// a template parameter so that the plain kernel does not carry its code.
// PIPE (default; RXMD_SPMV_NO_PIPE=1 switches it off): the first batch of the two streams is requested BEFORE the row length is known (it lies
// inside the row's S10-entry slot whatever the length; entries behind the row's end get weight 0 once the length has arrived), one
// dependent round trip less per wavefront.  Measured 0.98 -> 0.93 ms per pass on one box and no difference on another (0.941 / 0.949 /
// 0.938): the pass is insensitive to its latency chain.  It is insensitive to the BYTES of its streams too: a 16-bit column stream
// (stencil column + offset in the column's run, 10 instead of 12 bytes per entry) gave 0.968 vs 0.988 ms without the early request and
// 0.931 vs 0.921 ms with it; requesting every batch ahead of the previous one's gathers, a tighter row stride (448 or 512 instead of
// 640 entries) and skipping the ghost-column sums on the three rows in four that have no ghost partner (7 % SLOWER: the flag is one
// more scalar round trip in front of the loop) changed nothing or lost.  All were dropped again; see NOTES.md 3.
template <int MODE, bool STORE, bool PQ, int PIPE>
__global__ void __launch_bounds__(1024) k_spmv(int N, int S10, DevFF ff, const int *__restrict__ nb10, const double *__restrict__ hess, const int *__restrict__ n10,
                                               const double2 *__restrict__ xv, const double2 *__restrict__ hst, double2 *__restrict__ gst,
                                               const double2 *__restrict__ qst, const double *__restrict__ q, const int *__restrict__ type,
                                               const double *__restrict__ scal, double *__restrict__ partials,
                                               double2 *__restrict__ rs_all, double2 *__restrict__ rs_gh,
                                               const double *__restrict__ hsc, const double4 *__restrict__ pqrow, int swz,
                                               const int *__restrict__ rowlist, int nrows, int pbase, const double *__restrict__ stopflag,
                                               const int *__restrict__ rplace = nullptr) {           // rplace != nullptr: the streams are laid out by place (Engine::stream_rpos)
  if (stopflag && *stopflag != 0.0) return;        // run-ahead CG loop: the iteration this launch belongs to was decided not to happen (scalar_algebra stage 6)
  // rowlist != nullptr: this launch covers nrows rows named by the list (interior or boundary rows of a multi-rank domain);
  // its workgroups write their partial sums behind the pbase workgroups of the other launch
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  // the row is the same for the 64 lanes: say so (readfirstlane), and the row's base addresses, its length and the loop bounds live in
  // scalar registers -- 44 instead of 57 VGPRs and scalar address arithmetic: 1.03-1.09 -> 0.95 ms per pass on the same box
  const int widx = (swz ? xcd_swizzle(blockIdx.x, gridDim.x) : static_cast<int>(blockIdx.x)) * wpb + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int row = rowlist ? (widx < nrows ? rowlist[widx] : N) : widx;
  // the row tails of a workgroup are run by the first lanes of its wavefront 0 after the barrier the partial sums need anyway -- the
  // operands of consecutive rows (type, hst / qst, gst / q) and their results (row sums, gradient) are then a handful of coalesced requests
  // per workgroup instead of five per row (k_spmv_bisect: tail operands, row stores and partials are 6-8 % of the pass)
  __shared__ double s_row[16][4];
  const int wave_in_wg = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (row < N) {
    const size_t base = static_cast<size_t>(rplace ? rplace[row] : row) * S10;
    unsigned e[UNR];
    double h[UNR], c[UNR];
    // one batch of the row's streams (entry, hessian value, PQEq: shell-core value) for entries [kb, kb + 256) below `bound`
    auto request = [&](int kb, int bound, unsigned (&ee)[UNR], double (&hh)[UNR], double (&cc)[UNR]) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int k = kb + lane + 64 * u;
        const bool ok = k < bound;
        ee[u] = ok ? static_cast<unsigned>(__builtin_nontemporal_load(nb10 + base + k)) : 0u;   // streamed once: keep it out of
        hh[u] = ok ? __builtin_nontemporal_load(hess + base + k) : 0.0;                        // the caches that hold the vector
        if (PQ && (MODE == MODE_GRAD || STORE)) cc[u] = ok ? __builtin_nontemporal_load(hsc + base + k) : 0.0;
      }
    };
    if (PIPE) request(0, S10, e, h, c);
    const int n = n10[row] & N10_COUNT;
    double as = 0.0, at = 0.0, gs_ = 0.0, gt_ = 0.0;
    if (PIPE) {                                    // entries behind the row's end get weight 0
#pragma unroll
      for (int u = 0; u < UNR; ++u) { const bool ok = lane + 64 * u < n; e[u] = ok ? e[u] : 0u; h[u] = ok ? h[u] : 0.0; if (PQ) c[u] = ok ? c[u] : 0.0; }
    }
    for (int kb = 0; kb < n; kb += 64 * UNR) {   // wave-uniform trip count
      if (PIPE == 0 || (PIPE == 1 && kb > 0)) request(kb, n, e, h, c);
#pragma unroll
      for (int u = 0; u < UNR; ++u) {            // one 16-byte gather per entry from the cell-sorted vector copy
        const double2 v = xv[e[u] & NB10_IDX_MASK];
        as += h[u] * v.x;
        at += h[u] * v.y;
        if ((MODE == MODE_GRAD || STORE) && !PQ) { const double hg = (e[u] & NB10_GHOST) ? h[u] : 0.0; gs_ += hg * v.x; gt_ += hg * v.y; }   // select the weight, not the sums
        if ((MODE == MODE_GRAD || STORE) && PQ) { gs_ += c[u] * v.x; gt_ += c[u] * v.y; }      // PQEq: second matrix (shell-core) over the same columns
      }
    }
    as = wave_sum(as); at = wave_sum(at);
    if (MODE == MODE_GRAD || STORE) { gs_ = wave_sum(gs_); gt_ = wave_sum(gt_); }
    if (lane == 0) { s_row[wave_in_wg][0] = as; s_row[wave_in_wg][1] = at; s_row[wave_in_wg][2] = gs_; s_row[wave_in_wg][3] = gt_; }
  }
  __syncthreads();
  if (wave_in_wg != 0) return;
  {
    const int r_idx = (swz ? xcd_swizzle(blockIdx.x, gridDim.x) : static_cast<int>(blockIdx.x)) * wpb + lane;     // lane r = the row of wavefront r
    const int r = (lane < wpb) ? (rowlist ? (r_idx < nrows ? rowlist[r_idx] : N) : r_idx) : N;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (r < N) {
      const double as = s_row[lane][0], at = s_row[lane][1], gs_ = s_row[lane][2], gt_ = s_row[lane][3];
      const int t = type[r];
      const double2 pa = (MODE == MODE_HSH) ? hst[r] : qst[r];
      const DevAtomP ap = ff.atom[t];
      if (STORE) { rs_all[r] = make_double2(as, at); rs_gh[r] = make_double2(gs_, gt_); }
      if (MODE == MODE_HSH) {
        const double2 pb = gst[r];
        const double ts = ap.eta * pa.x + as, tt = ap.eta * pa.y + at;          // qeq.F90:294-302
        a0 = ts * pa.x; a1 = tt * pa.y;                                         // hshs_sum, hsht_sum (:309-310)
        a2 = pb.x * pa.x; a3 = pb.y * pa.y;                                     // g.h (:119,123)
      } else {
        const double mu = scal[S_MU];
        const double fpq = PQ ? pqrow[r].x : 0.0;
        const double g1 = -ap.chi - ap.eta * pa.x - as - fpq;                   // qeq.F90:349-350 (pqeq.F90:466)
        const double g2 = -1.0 - ap.eta * pa.y - at;
        gst[r] = make_double2(g1, g2);
        a0 = g1 * g1; a1 = g2 * g2;                                             // Gnew (:355-356)
        const double qi = q[r];
        const double hq_all = as - mu * at, hq_res = (as - gs_) - mu * (at - gt_);
        if (PQ) a2 = pq_est_row(ap, ff.Zpq[t], pqrow[r], qi, hq_all, gs_ - mu * gt_);
        else a2 = ap.chi * qi + 0.5 * ap.eta * qi * qi + 0.5 * qi * (hq_all + hq_res);  // Est (:297-306)
      }
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);           // fixed order over the workgroup's rows
    if (lane < 4) {
      const double v = lane == 0 ? a0 : (lane == 1 ? a1 : (lane == 2 ? a2 : a3));
      __hip_atomic_store(partials + (static_cast<size_t>(pbase) + blockIdx.x) * 4 + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- window pass (k_spmv_win) -------------------------------------------------------------------------------------------------------------
// The 16 rows of a group (consecutive residents in cell-sorted order, engine.h WIN_*) couple to nearly the same partners: ~1,500 cell-sorted
// positions for ~430 entries per row.  The workgroup copies the vector entries of that window into LDS with coalesced loads (8 consecutive
// positions = one 128-byte line per unit) and every row reads its partners from there: a 16-bit slot per entry (bit 15: ghost column) replaces
// the 4-byte entry and the 16-byte gather per entry through the vector memory path disappears.  Streams: value 8 + slot 2 bytes per entry, two
// entries per lane and request (16-byte / 4-byte loads), 256 entries of a row in flight.  Same sums in the same per-row roles as k_spmv; the
// order in which a row's products are added differs (lane = entry pair), i.e. the last bits of a row sum do.
// (A timing probe with synthetic slots promised 0.76 against 0.93 ms of k_spmv before anything real was built; the real pass: 0.80 against 0.89 ms
// back to back in one process, NOTES.md 3.  Variants are compared compiled side by side through VAR and debug tap 104.)
// FORM (bit set): WIN_PREFETCH = the second batch of a row is requested before the workgroup's barrier; WIN_LEAN = groups without a ghost partner skip the
// ghost-column sums; WIN_RANKROWS = experiments build only.  Plain QEq runs WIN_PREFETCH | WIN_LEAN (RXMD_SPMV_ONE_TRIP=1 and rows of 257-384 entries: NSTEP 3, WIN_LEAN), PQEq NSTEP 1 with WIN_PREFETCH
// (RXMD_PQ_PREFETCH=0: the instance <PQ, 2, WIN_PREFETCH | WIN_LEAN>, in which both bits are inert -- with PQ the prefetch form needs NSTEP 1 and the lean body is plain QEq's -- i.e. two
// batches of 128 entries in one register set, loaded and then used).  Which instance runs: Engine::win_instance (qeq.hip).
// VT (value type of the matrix stream): double, or float for the mixed-precision solver (Engine::set_qeq_precision(32), plain QEq, NSTEP 2, WIN_PREFETCH |
// WIN_LEAN only): the values were rounded once to REAL(4) by the list sweep and arrive as float pairs -- 8 bytes per lane and request, 6 instead of 10
// bytes per entry with the slot -- sit in the register sets as floats and are widened where they are used; window, slots, products, sums, tail and
// partial sums are those of the double instance.  The double instances are the same code with or without this parameter
// (profiles/qeq_f32_resource_usage_parent_vs_change.txt).
[[maybe_unused]] constexpr int WIN_RANKROWS = 1;
constexpr int WIN_PREFETCH = 2, WIN_LEAN = 4;
template <class VT> struct WinVal;
template <> struct WinVal<double> { typedef double2 pair; static __device__ inline pair make(double a, double b) { return make_double2(a, b); } };
template <> struct WinVal<float> { typedef float2 pair; static __device__ inline pair make(float a, float b) { return make_float2(a, b); } };
// BP (streams by place, engine.h: streams_by_place): the row's streams lie at its PLACE ridx = group * WIN_ROWS + wavefront, so their address needs nothing
// but the group number and the first batch is requested at the top of the wavefront -- behind the loads of the window descriptor (a wavefront's vector
// loads return in order: the descriptor must not wait for the streams) and next to the scalar loads of round trip 1, instead of behind them.  An unused
// place of a short group is read like any other (it lies inside the streams: places <= rows) and masked by its row length 0, by assignment.
template <int MODE, bool STORE, bool PQ, int NSTEP = 2, int VAR = 0, class VT = double, bool BP = false>      // VAR = FORM bits; VAR & 2: the second batch of a row is requested before the workgroup's barrier (below); VAR & 4: groups without a ghost partner skip the ghost-column sums (below); the default of plain QEq is 6.  NSTEP x 128 entries of a row in flight per register set (2; 3 = every row of at most 384 entries is one trip, the choice for water in rounds 4-5 -- 1.478 against 1.529 ms then, 1.61 against 1.58 since round 6, no longer the default; 1 for PQEq, whose third stream doubles a set); VAR: variants under measurement, compiled side by side and timed by debug tap 104
__global__ void __launch_bounds__(64 * WIN_ROWS, 8) k_spmv_win(int N, int G, int S10, DevFF ff, const unsigned short *__restrict__ sl10, const VT *__restrict__ hess, const int *__restrict__ n10,
                                                            const int *__restrict__ rows_sorted, const int *__restrict__ win_k, const int *__restrict__ win_cnt,
                                                            const double2 *__restrict__ xv, const double2 *__restrict__ hst, double2 *__restrict__ gst,
                                                            const double2 *__restrict__ qst, const double *__restrict__ q, const int *__restrict__ type,
                                                            const double *__restrict__ scal, double *__restrict__ partials,
                                                            double2 *__restrict__ rs_all, double2 *__restrict__ rs_gh,
                                                            const double *__restrict__ hsc, const double4 *__restrict__ pqrow,
                                                            const int *__restrict__ grouplist, int ngroups, int pbase, const double *__restrict__ stopflag,
                                                            const int *__restrict__ gflags = nullptr, int roword = 0) {
  // roword (round 6, run-ahead CG loop): the per-row operands and results of the tail -- type, (hs,ht), (gs,gt), row length in; the two row sums out -- are
  // indexed by the row's PLACE in rows_sorted (group * WIN_ROWS + wavefront) instead of by its atom: the 16 wavefronts of a workgroup then touch one
  // contiguous run per array instead of 16 scattered 64-byte sectors (the caller hands over the row-ordered arrays)
  if (stopflag && *stopflag != 0.0) return;
  extern __shared__ double2 s_x[];                  // the window: slot -> (xs, xt)
  __shared__ double s_row[WIN_ROWS][4];
  __shared__ int s_arrived;
  constexpr int STEPS = NSTEP;
  constexpr int NT = 64 * WIN_ROWS;
  typedef double d2v __attribute__((ext_vector_type(2)));
  typedef VT h2v __attribute__((ext_vector_type(2)));
  typedef typename WinVal<VT>::pair hpair;
  static_assert(std::is_same<VT, double>::value || (!PQ && NSTEP == 2), "the float value stream: plain QEq, two batches per register set");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int gidx = xcd_swizzle(blockIdx.x, gridDim.x);
  const int grp = grouplist ? (gidx < ngroups ? grouplist[gidx] : -1) : (gidx < ngroups ? gidx : -1);
  if (grp < 0) return;                              // (whole workgroup)
  // Round trip 1: everything that needs only the group number -- the row of this wavefront, the window's size, the first positions of the
  // window units this thread will copy (two rounds of 1,024 slots cover 256 units; the descriptor row is WIN_MAXUNITS long whatever the count).
  const int ridx = grp * WIN_ROWS + wave;
  const int *wk = win_k + static_cast<size_t>(grp) * WIN_MAXUNITS;
  const int t0 = threadIdx.x, t1 = threadIdx.x + NT;
  const int wk0 = wk[t0 / WIN_UNIT], wk1 = wk[t1 / WIN_UNIT];                      // (t1 / 8 < 256 <= WIN_MAXUNITS)
  hpair v[STEPS]; double2 c[STEPS]; unsigned ss[STEPS];
  if (BP) {
    // the row's first batch, whatever the row (and whether the place holds one): nothing of it depends on round trip 1.  UNCONDITIONAL loads (the
    // layout guarantees a stride of WIN_BP_MIN_STRIDE >= 128 x STEPS entries: all of them lie inside the place): behind a bound test the compiler
    // cannot count these loads, and the wait for the window descriptor in front of them would wait for the streams as well (s_waitcnt vmcnt(1)
    // instead of vmcnt(2 x STEPS + 1)).  The scalar loads of round trip 1 are kept BEHIND the request (below): scalar loads return in
    // any order, so the one wait for the kernel arguments of the request (stride, stream pointers) would otherwise be a wait for round trip 1.
    static_assert(128 * STEPS <= WIN_BP_MIN_STRIDE, "the first batch of a place is requested without a bound test");
    const size_t pbase_ = static_cast<size_t>(ridx) * S10;
    const h2v *ph = reinterpret_cast<const h2v *>(hess + pbase_);
    const d2v *pc = reinterpret_cast<const d2v *>(PQ ? hsc + pbase_ : nullptr);
    const unsigned *ps = reinterpret_cast<const unsigned *>(sl10 + pbase_);
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
      const int k2 = 64 * u + lane;                                // pair index
      const h2v t2 = __builtin_nontemporal_load(ph + k2); v[u] = WinVal<VT>::make(t2.x, t2.y);
      ss[u] = __builtin_nontemporal_load(ps + k2);
      if (PQ && (MODE == MODE_GRAD || STORE)) { const d2v t3 = __builtin_nontemporal_load(pc + k2); c[u] = make_double2(t3.x, t3.y); }
    }
  }
  // BP: the three scalar loads of round trip 1 -- row, window size, ghost flag of the group -- issued together BEHIND the request and waited for once
  // (left to the compiler they came out either in front of the request's own kernel-argument wait, or as three dependent round trips)
  int rt1_row = 0, rt1_cnt = 0, rt1_flag = 1;
  if constexpr (BP) {
    const int *p_row = rows_sorted + ridx, *p_cnt = win_cnt + grp, *p_flag = gflags ? gflags + grp : win_cnt + grp;
    asm volatile("s_load_dword %0, %3, 0x0\n\ts_load_dword %1, %4, 0x0\n\ts_load_dword %2, %5, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(rt1_row), "=&s"(rt1_cnt), "=&s"(rt1_flag) : "s"(p_row), "s"(p_cnt), "s"(p_flag) : "memory");
  } else { rt1_row = rows_sorted[ridx]; rt1_cnt = win_cnt[grp]; }
  const int row = min(rt1_row, N);                  // (a cell column's last group may be short: those slots hold a sentinel >= N)
  const int nslots = WIN_UNIT * rt1_cnt;
  const bool live = row < N;
#ifdef RXMD_EXPERIMENTS
  const size_t base = static_cast<size_t>(BP ? ridx : (live ? ((VAR & WIN_RANKROWS) ? ridx : row) : 0)) * S10;       // (VAR & 1, experiment: the streams' rows in cell-sorted order)
#else
  const size_t base = static_cast<size_t>(BP ? ridx : (live ? row : 0)) * S10;
#endif
  const h2v *hv2 = reinterpret_cast<const h2v *>(hess + base);
  const d2v *cv2 = reinterpret_cast<const d2v *>(PQ ? hsc + base : nullptr);
  const unsigned *sl2 = reinterpret_cast<const unsigned *>(sl10 + base);
  auto request = [&](int kb, int bound) {          // entries kb + 128 u + 2 lane and the next one
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
      const int k = kb + 128 * u + 2 * lane;
      const bool ok = k < bound;
      if (ok) { const h2v t2 = __builtin_nontemporal_load(hv2 + (k >> 1)); v[u] = WinVal<VT>::make(t2.x, t2.y); } else v[u] = WinVal<VT>::make(0.0, 0.0);
      ss[u] = ok ? __builtin_nontemporal_load(sl2 + (k >> 1)) : 0u;
      if (PQ && (MODE == MODE_GRAD || STORE)) { if (ok) { const d2v t2 = __builtin_nontemporal_load(cv2 + (k >> 1)); c[u] = make_double2(t2.x, t2.y); } else c[u] = make_double2(0.0, 0.0); }
    }
  };
  // VAR & 4: a group none of whose rows has a ghost partner (gflags[grp] == 0: three groups in four of a large domain) takes a body WITHOUT the
  // ghost-column sums -- two selects and four FMAs of the twelve vector instructions per pair of entries, and two of the four reductions.  The flag
  // rides with round trip 1 and the choice is ONE scalar branch per workgroup around two complete copies of everything below (round 6: as two loops
  // inside one body the compiler kept the first batches alive for "the other loop" and paid with folded spills under the 64-register cap -- 48 B of
  // scratch per lane, 20 after the register sets took turns, 0 now).
  const bool gh = !((VAR & WIN_LEAN) != 0 && !PQ && gflags != nullptr) || (BP ? rt1_flag : gflags[grp]) != 0;
  auto whole = [&](auto ghc) {
  constexpr bool GHC = decltype(ghc)::value;
  // Round trip 2: the window's vector entries FIRST (they return first, and the workgroup's barrier waits for them only), then the row's
  // first batch -- before the row length is known: it lies inside the row's slot whatever the length -- the length, and the operands of the
  // row's tail (the row is the same for the 64 lanes: scalar loads, no vector registers).
  double2 x0 = make_double2(0.0, 0.0), x1 = x0;
  if (t0 < nslots) x0 = xv[min(wk0 + (t0 & (WIN_UNIT - 1)), G - 1)];
  if (t1 < nslots) x1 = xv[min(wk1 + (t1 & (WIN_UNIT - 1)), G - 1)];
  if (!BP) request(0, live ? S10 : 0);             // (BP: in flight since the top of the wavefront)
  const int rowc = live ? (roword ? ridx : row) : 0;         // index of this row in the per-row arrays
  const int n = live ? (n10[rowc] & N10_COUNT) : 0;
  const int tl_t = type[rowc];
  const double2 tl_a = (MODE == MODE_HSH) ? hst[rowc] : qst[rowc];
  const double2 tl_b = (MODE == MODE_HSH) ? const_cast<const double2 *>(gst)[rowc] : make_double2(q[rowc], 0.0);
  if (threadIdx.x == 0) s_arrived = 0;
  if (t0 < nslots) s_x[t0] = x0;
  if (t1 < nslots) s_x[t1] = x1;
  for (int t = threadIdx.x + 2 * NT; t < nslots; t += NT) s_x[t] = xv[min(wk[t / WIN_UNIT] + (t & (WIN_UNIT - 1)), G - 1)];   // a window of more than 256 units
#pragma unroll
  for (int u = 0; u < STEPS; ++u) {                // entries behind the row's end: weight 0, slot 0
    const int k = 128 * u + 2 * lane;
    if (k >= n) { v[u].x = static_cast<VT>(0.0); ss[u] &= 0xffff0000u; if (PQ) c[u].x = 0.0; }
    if (k + 1 >= n) { v[u].y = static_cast<VT>(0.0); ss[u] &= 0x0000ffffu; if (PQ) c[u].y = 0.0; }
  }
  // VAR & 2 (plain QEq): the row's NEXT batch is requested before the barrier, behind the window's data (a wavefront's loads return in order:
  // the window does not wait for it) -- the round trip of the second batch runs under the barrier and the first batch's arithmetic instead of
  // after it; the batch after that is requested before the current one is used, and so on.
  // PQEq takes the prefetch form with ONE batch of 128 entries per register set (NSTEP 1): its third stream (the shell-core values) doubles the registers of a
  // set, and two sets of two batches do not fit the 64 registers of eight workgroups per CU
  constexpr bool PRE = (VAR & WIN_PREFETCH) != 0 && (!PQ || NSTEP == 1);
  hpair vn[STEPS]; double2 cn[STEPS]; unsigned sn[STEPS];
  auto request_next = [&](int kb) {
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
      const int k = kb + 128 * u + 2 * lane;
      const bool ok = k < n;
      if (ok) { const h2v t2 = __builtin_nontemporal_load(hv2 + (k >> 1)); vn[u] = WinVal<VT>::make(t2.x, t2.y); } else vn[u] = WinVal<VT>::make(0.0, 0.0);
      sn[u] = ok ? __builtin_nontemporal_load(sl2 + (k >> 1)) : 0u;
      if (PQ && (MODE == MODE_GRAD || STORE)) { if (ok) { const d2v t2 = __builtin_nontemporal_load(cv2 + (k >> 1)); cn[u] = make_double2(t2.x, t2.y); } else cn[u] = make_double2(0.0, 0.0); }
    }
  };
  if (PRE && n > 128 * STEPS) request_next(128 * STEPS);
  __syncthreads();
  double as = 0.0, at = 0.0, gs_ = 0.0, gt_ = 0.0;
    auto batch = [&](const hpair (&vv)[STEPS], const unsigned (&sv)[STEPS], const double2 (&cv)[STEPS]) {      // one batch of 128 x STEPS entries out of registers and the LDS window
#pragma unroll
      for (int u = 0; u < STEPS; ++u) {
        const double2 y0 = s_x[sv[u] & 0x7fffu], y1 = s_x[(sv[u] >> 16) & 0x7fffu];
        const double hx = vv[u].x, hy = vv[u].y;                    // (float stream: widened here, exactly)
        as += hx * y0.x; at += hx * y0.y; as += hy * y1.x; at += hy * y1.y;
        if (GHC && (MODE == MODE_GRAD || STORE) && !PQ) {
          const double g0 = (sv[u] & 0x8000u) ? hx : 0.0, g1 = (sv[u] & 0x80000000u) ? hy : 0.0;     // select the weight, not the sums
          gs_ += g0 * y0.x; gt_ += g0 * y0.y; gs_ += g1 * y1.x; gt_ += g1 * y1.y;
        }
        if ((MODE == MODE_GRAD || STORE) && PQ) { gs_ += cv[u].x * y0.x; gt_ += cv[u].x * y0.y; gs_ += cv[u].y * y1.x; gt_ += cv[u].y * y1.y; }
      }
    };
    constexpr int B = 128 * STEPS;
    if (PRE) {
      // Two register sets take turns (round 6): batch k sits in (v, ss) for even k and in (vn, sn) for odd k, and the batch after the next one is
      // requested into the set that has just been used.  Until round 6 the loop rotated `v = vn` at its head: under the 64-register cap of eight
      // workgroups per CU that copy went through 48 bytes of scratch per lane on every row longer than two batches (rows > 512 entries: any
      // condensed system at PQEq's 12.5 A cut-off, dense metals) -- and cost ten moves per row on the others.  Same products in the same order.
      for (int kb = 0;;) {                               // wave-uniform trip count
        batch(v, ss, c);
        kb += B; if (kb >= n) break;
        if (kb + B < n) request(kb + B, n);               // (an odd row end: entry n is the zero padding of the row, slot 0)
        batch(vn, sn, cn);
        kb += B; if (kb >= n) break;
        if (kb + B < n) request_next(kb + B);
      }
    } else {
      for (int kb = 0; kb < n; kb += B) {                 // wave-uniform trip count
        if (kb > 0) request(kb, n);
        batch(v, ss, c);
      }
    }

  as = wave_sum(as); at = wave_sum(at);
  if ((MODE == MODE_GRAD || STORE) && GHC) { gs_ = wave_sum(gs_); gt_ = wave_sum(gt_); }
  // The row's tail by its own wavefront (the rows of a group are scattered residents: nothing would coalesce if one wavefront ran all of them,
  // and a workgroup whose last wavefront works alone keeps 15 wavefront slots of the CU empty); a wavefront leaves when it is done.  The
  // workgroup's four partial sums: every wavefront leaves its terms in LDS, the LAST one to arrive adds them in wavefront order.
  // the lane number afresh (two mbcnt instructions): `lane` kept alive across the loop for these four uses was the one register the PQ instances spilled
  const int lane_t = static_cast<int>(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (live) {
    const DevAtomP ap = ff.atom[tl_t];
    if (MODE == MODE_HSH) {
      const double ts = ap.eta * tl_a.x + as, tt = ap.eta * tl_a.y + at;      // qeq.F90:294-302
      a0 = ts * tl_a.x; a1 = tt * tl_a.y;                                     // hshs_sum, hsht_sum (:309-310)
      a2 = tl_b.x * tl_a.x; a3 = tl_b.y * tl_a.y;                             // g.h (:119,123)
      if (STORE && lane_t == 0) { rs_all[rowc] = make_double2(as, at); rs_gh[rowc] = make_double2(gs_, gt_); }
    } else {
      const double mu = scal[S_MU];
      const double4 pr = PQ ? pqrow[row] : make_double4(0.0, 0.0, 0.0, 0.0);
      const double g1 = -ap.chi - ap.eta * tl_a.x - as - pr.x;                // qeq.F90:349-350 (pqeq.F90:466)
      const double g2 = -1.0 - ap.eta * tl_a.y - at;
      a0 = g1 * g1; a1 = g2 * g2;                                             // Gnew (:355-356)
      const double qi = tl_b.x;
      const double hq_all = as - mu * at, hq_res = (as - gs_) - mu * (at - gt_);
      if (PQ) a2 = pq_est_row(ap, ff.Zpq[tl_t], pr, qi, hq_all, gs_ - mu * gt_);
      else a2 = ap.chi * qi + 0.5 * ap.eta * qi * qi + 0.5 * qi * (hq_all + hq_res);  // Est (:297-306)
      if (lane_t == 0) { gst[rowc] = make_double2(g1, g2); if (STORE) { rs_all[rowc] = make_double2(as, at); rs_gh[rowc] = make_double2(gs_, gt_); } }
    }
  }
  int arrived = 0;
  if (lane_t == 0) {
    s_row[wave][0] = a0; s_row[wave][1] = a1; s_row[wave][2] = a2; s_row[wave][3] = a3;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    arrived = __hip_atomic_fetch_add(&s_arrived, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  arrived = __builtin_amdgcn_readfirstlane(arrived);
  if (arrived != WIN_ROWS - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane_t < 4) {
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < WIN_ROWS; ++w) sum += s_row[w][lane_t];                 // fixed order: the result does not depend on which wavefront is last
    __hip_atomic_store(partials + (static_cast<size_t>(pbase) + blockIdx.x) * 4 + lane_t, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  };
  if (gh) whole(std::true_type{}); else whole(std::false_type{});
}

// ---- host side: the ONE launch site of each pass kernel --------------------------------------------------------------------------------------
// The operands of a launch as a plain struct in the kernel's order; launch_win / launch_row expand it into the positional call (the kernels keep their
// positional signatures: the struct is not a kernel argument).  Engine::win_args / row_args (qeq.hip) fill one for the common case -- atom order, whole
// grid, no stop flag -- and a caller overrides the fields it differs in.
struct WinPassArgs {
  int N, G, S10; DevFF ff; const unsigned short *sl10; const double *hess; const float *hess32; const int *n10, *rows_sorted, *win_k, *win_cnt;   // (hess / hess32: the value stream the instance's VT names)
  const double2 *xv, *hst; double2 *gst; const double2 *qst; const double *q; const int *type; const double *scal; double *partials; double2 *rs_all, *rs_gh; const double *hsc; const double4 *pqrow;
  const int *grouplist; int ngroups, pbase; const double *stopflag; const int *gflags; int roword;
  int win_maxunits; hipStream_t stream;               // geometry: ngroups workgroups of WIN_ROWS wavefronts, the largest window of the build in LDS
  bool byplace = false;                               // layout of the streams (Engine::streams_by_place): selects the BP instance
};
template <int MODE, bool STORE, bool PQ, int NSTEP = 2, int VAR = 0, class VT = double>
inline void launch_win(const WinPassArgs &a) {
  const VT *values = [&] { if constexpr (std::is_same<VT, float>::value) return a.hess32; else return a.hess; }();
  auto go = [&](auto bp) {
    k_spmv_win<MODE, STORE, PQ, NSTEP, VAR, VT, decltype(bp)::value><<<a.ngroups, 64 * WIN_ROWS, static_cast<size_t>(a.win_maxunits) * WIN_UNIT * sizeof(double2), a.stream>>>(
        a.N, a.G, a.S10, a.ff, a.sl10, values, a.n10, a.rows_sorted, a.win_k, a.win_cnt, a.xv, a.hst, a.gst, a.qst, a.q, a.type, a.scal, a.partials, a.rs_all, a.rs_gh, a.hsc, a.pqrow,
        a.grouplist, a.ngroups, a.pbase, a.stopflag, a.gflags, a.roword);
  };
  if (a.byplace) go(std::true_type{}); else go(std::false_type{});
}
// one wavefront per row, sixteen rows per workgroup: measured faster than a persistent grid-stride launch (1.10 vs 1.28 ms
// per pass at 979,776 rows) -- many short waves overlap each other's load / gather / reduce phases (NOTES.md 3, K4/K5)
constexpr int SPMV_WPB = 16;                   // wavefronts (= rows) per workgroup of the row pass
struct RowPassArgs {
  int N, S10; DevFF ff; const int *nb10; const double *hess; const int *n10;
  const double2 *xv, *hst; double2 *gst; const double2 *qst; const double *q; const int *type; const double *scal; double *partials;
  double2 *rs_all, *rs_gh; const double *hsc; const double4 *pqrow; int swz; const int *rowlist; int nrows, pbase; const double *stopflag;
  hipStream_t stream;
  const int *rplace = nullptr;
  int nblocks() const { return nblk(rowlist ? nrows : N, SPMV_WPB); }
};
template <int MODE, bool STORE, bool PQ, int PIPE>
inline void launch_row(const RowPassArgs &a) {
  k_spmv<MODE, STORE, PQ, PIPE><<<a.nblocks(), 64 * SPMV_WPB, 0, a.stream>>>(a.N, a.S10, a.ff, a.nb10, a.hess, a.n10, a.xv, a.hst, a.gst, a.qst, a.q, a.type, a.scal, a.partials, a.rs_all, a.rs_gh, a.hsc, a.pqrow, a.swz,
                                                                            a.rowlist, a.nrows, a.pbase, a.stopflag, a.rplace);
}

// the mean time [ms] of `reps` launches behind `warm` untimed ones (events ev[2], ev[3] of the engine; returns when the last launch is through)
template <class F> inline double timed_launches_ms(Engine &e, int warm, int reps, F &&launch) {
  for (int r = 0; r < warm + reps; ++r) { if (r == warm) hipEventRecord(e.ev[2], e.stream); launch(); }
  hipEventRecord(e.ev[3], e.stream); hipEventSynchronize(e.ev[3]);
  float ms = 0; hipEventElapsedTime(&ms, e.ev[2], e.ev[3]);
  return static_cast<double>(ms) / reps;
}

}  // namespace rxmd
