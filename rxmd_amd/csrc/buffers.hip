// buffers.hip -- the one allocator of the library and the table of the engine's buffers.
//
// Every device and pinned block of the library comes from dev_alloc / pinned_alloc below and goes back through dev_free / pinned_free
// (the placement search of qeq.hip and experiments.hip draw raw blocks of their own: they tolerate a refusal on purpose).  Each buffer of
// the engine is its own hipMalloc -- no arena, no pool: the placement search depends on hess, sl10 and hsc being separately drawn blocks
// (DESIGN.md 2).
//
// Engine::declare_buffers is the ONE list of the engine's buffers: a line per buffer states its size rule, its fill, whether the
// RXMD_POISON_ALLOC refill covers it, the group it is re-allocated with and whether it is resident state.  Allocation, release, the refill and
// the state carried over a capacity change (Buffers::*) are walks over that table; they use the bytes recorded at allocation, never a formula.
#include "engine.h"

#include <algorithm>
#include <cstring>
#include <utility>

namespace rxmd {

// RXMD_POISON_ALLOC=1 (diagnostic; changes nothing that is computed): every buffer starts as 0xFF bytes -- a NaN for doubles, -1 for
// indices and counts -- instead of zeros, and the per-step scratch (ghost slots of the per-atom arrays, bonded tables, the 10 A list and its
// window form) is filled with the pattern again before every rebuild (Buffers::refill), so that a kernel which reads an element
// nobody wrote this step shows as a NaN / an index trap instead of silently using a stale or zero value.  The reference's own allocator does not
// clear (module.F90:732-744); what it clears explicitly -- ccbnd, cdbnd, f, PE per FORCE call (pot.F90:20-26), spos and qtfp/qtfv at
// allocation (init.F90:117-131) -- the kernels here clear too.  Buffers whose ZERO is part of a protocol (arrival counters, error words,
// device scalars) are declared Fill::Zero.
static const Options g_opt = Options::from_env();      // (the allocator is a set of free functions: the library-wide copy of the switches)
static const bool g_poison = g_opt.poison_alloc;
#ifdef RXMD_EXPERIMENTS
// RXMD_CONTIG_ALLOC=<bytes>: pattern-filled buffers of at most that many bytes (0: every one) come from hipExtMallocWithFlags(hipDeviceMallocContiguous) --
// the configuration that failed 15 unrelated tests in round 3 (NOTES.md 3); with RXMD_POISON_ALLOC=1 a read of stale memory shows as a NaN
static const long long g_contig = g_opt.contig_alloc;
#endif

bool poison_enabled() { return g_poison; }

void *dev_alloc(size_t bytes, Fill fill) {
  void *p = nullptr;
#ifdef RXMD_EXPERIMENTS
  if (fill == Fill::Pattern && (g_contig == 0 || (g_contig > 0 && bytes <= static_cast<size_t>(g_contig)))) RX_HIP(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocContiguous));
  else
#endif
  RX_HIP(hipMalloc(&p, bytes));
  if (fill != Fill::None && hipMemset(p, fill == Fill::Pattern && g_poison ? 0xFF : 0, bytes) != hipSuccess) {
    (void)hipFree(p);                                // (no block is lost on the error path: nobody holds the pointer yet)
    throw EngineError(RXMD_E_HIP, "hipMemset of a fresh block of " + std::to_string(bytes) + " bytes failed");
  }
  return p;
}
void dev_free(void *p) { if (p) (void)hipFree(p); }

// Pinned memory comes back from the allocator as the last owner left it, and a process may hold several engines one after another: a stale
// sequence word of an earlier engine's CG snapshot could satisfy wait_snapshot's poll, a stale word of h_pub pinned_wait's.  Every pinned block is
// zeroed where it is allocated (set-up and grow_capacity both come through here).  Which block the allocator hands out is its choice, so no
// test can pin this.
void *pinned_alloc(size_t bytes, bool coherent_mapped) {
  void *p = nullptr;
  if (coherent_mapped) RX_HIP(hipHostMalloc(&p, bytes, hipHostMallocCoherent | hipHostMallocMapped));
  else RX_HIP(hipHostMalloc(&p, bytes));
  std::memset(p, 0, bytes);
  return p;
}
void pinned_free(void *p) { if (p) (void)hipHostFree(p); }

// ---- the table ------------------------------------------------------------------------------------------------------------------------
constexpr size_t H_SEG_INTS = 32;        // totals of the 26-segment ghost build
constexpr size_t H_PUB_WORDS = 32;       // words published through pinned memory (sequence number << 32 | value, pinned_wait)

void Engine::declare_buffers() {
  Buffers &b = bufs;
  constexpr Fill P = Fill::Pattern, Z = Fill::Zero;
  constexpr Refill never = Refill::Never, whole = Refill::Whole, ghosts = Refill::Ghosts;
  constexpr unsigned pq = BUF_PQEQ, res = BUF_RESIDENT;
  // b.add(member, group, dimension, multiplier, addend, fill at allocation, refill rule, flags): count = dimension * multiplier + addend elements.
  // The order is the order of allocation.  Refill::Never on per-step scratch (gowner, dh_*, sendidx, fnb, fsort, the row-order arrays) is the
  // known gap of DESIGN.md 2: widening the refill changes behaviour.
  for (int a = 0; a < 3; ++a) {
    b.add(pos[a], G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
    b.add(vel[a], G_SETUP, Dim::NB, 1, 0, P, never, res);
    b.add(frc[a], G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
    b.add(spos[a], G_SETUP, Dim::NB, 1, 0, P, ghosts);
  }
  b.add(q, G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
  b.add(qsfp, G_SETUP, Dim::NB, 1, 0, P, never, res);
  b.add(qsfv, G_SETUP, Dim::NB, 1, 0, P, never, res);
  b.add(type, G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
  b.add(gid, G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
  for (int a = 0; a < 3; ++a) b.add(shl[a], G_SETUP, Dim::NB, 1, 0, P, ghosts, pq | res);
  b.add(sorted_shl, G_SETUP, Dim::NB, 1, 0, P, whole, pq);
  b.add(hsc, G_LIST10, Dim::List10, 1, 0, P, whole, pq);
  b.add(pqrow, G_SETUP, Dim::Rows10, 1, 0, P, whole, pq);
  b.add(qst, G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
  b.add(hst, G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
  b.add(gst, G_SETUP, Dim::NB, 1, 0, P, ghosts, res);
  b.add(hst2, G_SETUP, Dim::NB, 1, 0, P, ghosts);
  b.add(tickets, G_SETUP, Dim::Fixed, 0, 16, Z, never);
  b.add(sall, G_SETUP, Dim::Rows10, 1, 0, P, whole);
  b.add(sgh, G_SETUP, Dim::Rows10, 1, 0, P, whole);
  b.add(wall, G_SETUP, Dim::Rows10, 1, 0, P, whole);
  b.add(wgh, G_SETUP, Dim::Rows10, 1, 0, P, whole);
  b.add(gsrc, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(groot, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(gowner, G_SETUP, Dim::NB, 1, 0, P, never);
  b.add(dh_ghost, G_SETUP, Dim::NB, 1, 0, P, never);
  b.add(dh_keys, G_SETUP, Dim::NB, 1, 0, P, never);
  b.add(dh_keys2, G_SETUP, Dim::NB, 1, 0, P, never);
  b.add(dh_vals, G_SETUP, Dim::NB, 1, 0, P, never);
  b.add(dh_off, G_SETUP, Dim::Fixed, 0, 1100, P, never);
  b.add(sendidx, G_SETUP, Dim::NB, 1, 0, P, never);
  b.add(rootperm, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(invpos, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(xs, G_SETUP, Dim::NB, 1, 0, P, whole);
  for (int a = 0; a < 3; ++a) {
    b.add(fnb[a], G_SETUP, Dim::NB, 1, 0, P, never);
    b.add(fsort[a], G_SETUP, Dim::NB, 1, 0, P, never);
  }
  b.add(cellid, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(cellid_sorted, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(perm, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(perm_in, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(cellstart, G_CELLSTART, Dim::Cap, 1, 0, P, whole);
  b.add(sorted_xyzi, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(sorted_type, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(flags, G_SETUP, Dim::NB, 1, 1, P, whole);
  b.add(scanout, G_SETUP, Dim::NB, 1, 1, P, whole);
  b.add(flags2, G_SETUP, Dim::NB, 1, 1, P, whole);
  b.add(scanout2, G_SETUP, Dim::NB, 1, 1, P, whole);
  b.add(nbr_sm, G_SETUP, Dim::NB, 32, 0, P, whole);      // staging of the bonded sweep: one 128-byte line of 32 slots per atom (lists.hip, BL_STRIDE; MAXNB <= 31)
  b.add(nbrcnt, G_SETUP, Dim::NB, 1, 1, P, whole);
  b.add(boff, G_SETUP, Dim::NB, 1, 2, P, whole);
  b.add(nbr, G_BOND, Dim::Cap, 1, 0, P, whole);
  b.add(brev, G_BOND, Dim::Cap, 1, 0, P, whole);
  b.add(bown, G_BOND, Dim::Cap, 1, 0, P, whole);
  b.add(btype, G_BOND, Dim::Cap, 1, 0, P, whole);
  for (double **t : {&bo0, &bo1, &bo2, &bo3, &dln2, &dln3, &dBOp, &A0, &A1, &A2, &A3, &cf1, &cf2, &cf3, &cdn, &fnx, &fny, &fnz, &etor, &econ, &epen, &ecoa, &bt1, &bt2, &bt3})
    b.add(*t, G_BOND, Dim::Cap, 1, 0, P, whole);
  b.add(ehb_don, G_SETUP, Dim::Rows10, 1, EHB_DON_EXTRA, P, whole);
  b.add(ehb_cnt, G_SETUP, Dim::Fixed, 0, 72, Z, never);      // 64 sub-lists (hbonds.hip EHB_REGIONS) + debug words
  b.add(ecoef, G_SETUP, Dim::NB, 6, 0, P, whole);
  b.add(deltap, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(delta, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(nlp, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(dDlp, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(deltalp, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(cds, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(cd, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(cc_, G_SETUP, Dim::NB, 1, 0, P, whole);
  b.add(nb10, G_LIST10, Dim::List10, 1, 0, P, whole);
  b.add(rows_int, G_SETUP, Dim::Rows10, 1, 0, P, whole);
  b.add(rows_bnd, G_SETUP, Dim::Rows10, 1, 0, P, whole);
  b.add(hess, G_LIST10, Dim::List10, 1, 0, P, whole);
  b.add(n10, G_SETUP, Dim::Rows10, 1, 0, P, whole);
  // window groups (capacity = groups; groups never straddle a cell column of the grid: up to one short group per column, win_groups_bound) + rpos / g_rrow
  for (double2 **t : {&r_qst, &r_hst, &r_hst2, &r_gst, &r_sall, &r_sgh, &r_wall, &r_wgh}) b.add(*t, G_WIN, Dim::Cap, WIN_ROWS, 0, P, never);
  b.add(r_type, G_WIN, Dim::Cap, WIN_ROWS, 0, P, never);
  b.add(r_n10, G_WIN, Dim::Cap, WIN_ROWS, 0, P, never);
  b.add(r_xpos, G_WIN, Dim::Cap, WIN_ROWS, 0, P, never);
  b.add(rpos, G_WIN, Dim::NB, 1, 0, P, never);
  b.add(g_rrow, G_WIN, Dim::NB, 1, 0, P, never);
  b.add(rows_sorted, G_WIN, Dim::Cap, WIN_ROWS, 0, P, whole);
  b.add(rowcols, G_WIN, Dim::Cap, WIN_ROWS * 64, 0, P, whole);
  b.add(grp_base, G_WIN, Dim::Cap, 32, 0, P, whole);
  b.add(win_flag, G_WIN, Dim::Cap, 1, 1, P, whole);
  b.add(win_k, G_WIN, Dim::Cap, WIN_MAXUNITS, 0, P, whole);
  b.add(win_cnt, G_WIN, Dim::Cap, 1, 0, P, whole);
  b.add(win_gint, G_WIN, Dim::Cap, 1, 0, P, whole);
  b.add(win_gbnd, G_WIN, Dim::Cap, 1, 0, P, whole);
  b.add(sl10, G_LIST10, Dim::List10, 1, 0, P, whole);
  b.add(hess32, G_LIST10, Dim::List10, 1, 0, P, whole, BUF_QEQ_F32);      // the matrix values as REAL(4), only while set_qeq_precision(32) is in force
  b.add(partials, G_PARTIALS, Dim::Cap, 1, 1024, P, whole);   // + the 128 x 4 first-level sums of k_reduce_fused, behind the per-workgroup partials at a fixed offset
  b.add(scal, G_SETUP, Dim::Fixed, 0, SCAL_N, Z, never, res);
  b.add_pinned(h_scal, G_SETUP, H_SCAL_N, true);        // coherent: the update kernel's tail stores the CG snapshot into it and the host polls it
  b.add(tsum, G_SETUP, Dim::Fixed, 0, 128, Z, never);
  b.add_raw(reinterpret_cast<void **>(&sargs), sizeof(double), G_SETUP, Dim::Fixed, 0, 32, Z, never);   // room of 32 doubles for the ScaleArgs of assemble.hip
  b.add(d_err, G_SETUP, Dim::Fixed, 0, 16, Z, never);
  b.add_pinned(h_err, G_SETUP, H_ERR_INTS, false);
  // ---- allocated on demand ----
  b.add(cubtmp, G_CUBTMP, Dim::Cap, 1, 0, Fill::None, never);      // hipcub scratch, bytes
  b.add(ffblob, G_FFBLOB, Dim::Cap, 1, 0, Fill::None, never);      // the flattened force field, bytes (upload_ff writes all of it)
  b.add(pqblob, G_PQBLOB, Dim::Cap, 1, 0, Fill::None, never);
  b.add(e4b_t, G_E4B, Dim::Cap, 1, 0, P, never);
  b.add(e4b_flag, G_E4B, Dim::Cap, 1, 0, Z, never);
  b.add(seg_cnt, G_SEG, Dim::Cap, 27, 0, P, never);
  b.add(seg_tot, G_SEG, Dim::Fixed, 0, 32, Z, never);
  b.add(seg_code_, G_SEG, Dim::Cap, 256, 0, P, never);        // (one face code per RESIDENT: sized with the workgroup count, not with the NB of the day)
  b.add_pinned(h_seg, G_SEG_PINNED, H_SEG_INTS, false);
  b.add_pinned(h_pub, G_SEG_PINNED, H_PUB_WORDS, true);
  b.add(xbuf_send, G_XBUF, Dim::Cap, 1, 0, P, whole);         // (host-supplied exchange buffers carry no record: never refilled, never freed)
  b.add(xbuf_recv, G_XBUF, Dim::Cap, 1, 0, P, whole);
  b.add(dh_serve, G_DH_SERVE, Dim::Cap, 1, 0, P, never);
  b.add(bg_flag, G_BGRAPH, Dim::Cap, 1, 1, P, never);         // rxmd_hip_get_bonds_device (device_io.hip): selection flag and output offset per entry of the
  b.add(bg_off, G_BGRAPH, Dim::Cap, 1, 1, P, never);          // bond tables, capacity = bcap of the day of the call; an engine that never asks has neither
  // rxmd_hip_bonds_vjp_device (bond_vjp.hip): per table entry the coefficients / force terms and the ccbnd term, per atom slot ccbnd and the gradient;
  // first use allocates them, at bcap and NB of that day (Engine::bonds_vjp_device re-allocates when either has grown)
  for (double **t : {&bv_c1, &bv_c2, &bv_c3, &bv_t}) b.add(*t, G_BVJP, Dim::Cap, 1, 0, P, never);
  b.add(bv_cc, G_BVJP, Dim::NB, 1, 0, P, never);
  for (int a = 0; a < 3; ++a) b.add(bv_g[a], G_BVJP, Dim::NB, 1, 0, P, never);
  // rxmd_hip_get_pairs_device (pair_graph.hip): selected entries per resident row of the 10 A list and their exclusive sum, 64-bit (+ 1: the total);
  // first use allocates them at the rows10 of that day (Engine::select_pairs re-allocates when the rows have grown); an engine that never asks has neither
  b.add(pg_cnt, G_PGRAPH, Dim::Rows10, 1, 1, P, never);
  b.add(pg_off, G_PGRAPH, Dim::Rows10, 1, 1, P, never);
  // rxmd_hip_structure_* (structure.hip): the int64 accumulators of the structure statistics, capacity = the words structure_begin asked for; zeros
  // are the protocol; resident: they outlive a capacity change (Engine::grow_capacity allocates the group again in front of the restore).
  // LAST in the table: save_residents / restore_residents pair blocks by their order
  b.add(sg_acc, G_STRUCT, Dim::Cap, 1, 0, Z, never, res);
}

size_t Buffers::count(const Buf &b, const Engine &e) const {
  size_t d = 0;
  switch (b.dim) {
    case Dim::Fixed: break;
    case Dim::NB: d = static_cast<size_t>(e.NB); break;
    case Dim::Rows10: d = static_cast<size_t>(e.rows10); break;
    case Dim::List10: d = static_cast<size_t>(e.rows10) * e.S10; break;
    case Dim::Cap: d = cap[b.group]; break;
  }
  return std::max<size_t>(d * b.mul + b.add_, 1);
}

void Buffers::alloc_one(Buf &b, const Engine &e) {
  if ((b.flags & BUF_PQEQ) && !e.ff.pqeq) return;
  if ((b.flags & BUF_QEQ_F32) && e.qeq_bits_req != 32) return;
  const size_t bytes = count(b, e) * b.elem;
  *b.pp = b.space == Space::Device ? dev_alloc(bytes, b.fill) : pinned_alloc(bytes, b.space == Space::PinnedCoherent);
  b.bytes = bytes;
}
void Buffers::free_one(Buf &b) {
  if (!b.bytes) return;                              // (never allocated, or not ours: host-supplied exchange buffers)
  if (b.space == Space::Device) dev_free(*b.pp); else pinned_free(*b.pp);
  *b.pp = nullptr; b.bytes = 0;
}
void Buffers::alloc_setup(const Engine &e) { for (Buf &b : v) if (b.group < G_ON_DEMAND) alloc_one(b, e); }
// All or nothing: when one allocation of the group fails, the blocks this call drew are released and the group is as it was before the call
// (for a caller that keeps the old blocks alive across the call: grow_xbuf_keep_send)
void Buffers::alloc_group(const Engine &e, int g, size_t capacity) {
  const size_t old_cap = cap[g];
  std::vector<std::pair<void *, size_t>> old;
  for (const Buf &b : v) if (b.group == g) old.emplace_back(*b.pp, b.bytes);
  cap[g] = capacity;
  try {
    for (Buf &b : v) if (b.group == g) alloc_one(b, e);
  } catch (...) {
    size_t k = 0;
    for (Buf &b : v) if (b.group == g) { if (*b.pp != old[k].first) free_one(b); *b.pp = old[k].first; b.bytes = old[k].second; ++k; }
    cap[g] = old_cap;
    throw;
  }
}
void Buffers::free_group(int g) { for (Buf &b : v) if (b.group == g) free_one(b); }
void Buffers::free_all() { for (Buf &b : v) free_one(b); }

// RXMD_POISON_ALLOC: what a step rebuilds from scratch holds the pattern again before the rebuild
void Buffers::refill(const Engine &e) {
  if (!g_poison) return;
  for (const Buf &b : v) {
    if (!b.bytes || b.refill == Refill::Never) continue;
    const size_t off = b.refill == Refill::Ghosts ? static_cast<size_t>(e.N) * b.elem : 0;
    if (off < b.bytes) RX_HIP(hipMemsetAsync(static_cast<char *>(*b.pp) + off, 0xFF, b.bytes - off, e.stream));
  }
}

// the residents' state through the host: the first N elements of a per-atom array, all of a fixed block (the device scalars)
std::vector<std::vector<char>> Buffers::save_residents(const Engine &e) const {
  std::vector<std::vector<char>> h;
  for (const Buf &b : v) {
    if (!(b.flags & BUF_RESIDENT) || !b.bytes) continue;
    h.emplace_back(b.dim == Dim::NB ? static_cast<size_t>(e.N) * b.elem : b.bytes);
    if (!h.back().empty()) RX_HIP(hipMemcpy(h.back().data(), *b.pp, h.back().size(), hipMemcpyDeviceToHost));
  }
  return h;
}
void Buffers::restore_residents(const std::vector<std::vector<char>> &h) {
  size_t k = 0;
  for (const Buf &b : v) {
    if (!(b.flags & BUF_RESIDENT) || !b.bytes) continue;
    if (!h[k].empty()) RX_HIP(hipMemcpy(*b.pp, h[k].data(), h[k].size(), hipMemcpyHostToDevice));
    ++k;
  }
}

}  // namespace rxmd
