// engine.h -- device-resident state of one rank (= one MI355X) and the kernel-group entry points.
//
// Data layout in HBM (all FP64 unless noted; N = residents, G = residents + ghosts, NB = capacity):
//   per-atom SoA, index = the reference's LOCAL atom index (residents in rxff.bin / arrival order,
//   then ghosts in exchange-stage order, reference src/comm.F90:414-446,494-518).  The force
//   semantics depend on this order, so atoms are never physically re-sorted;
//   spatial sorting exists only as an index permutation for the list builds.
//   bonded tables are COMPACT (CSR): bond o = boff[i] + s is slot s of atom i, its mirror image in the partner's list is brev[o]
//   (round 4; until then slot-major [slot * NB + atom]: 30-slot strides for 5.3 bonds per atom, half-empty cache lines in every kernel)
//   the 10 A list is row-major ELL [row * S10 + k]    (coalesced for wave-per-row kernels),
//   S10 a multiple of 64 so that every row starts on a 512-byte boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rxmd_hip.h"
#include "ffparams.h"
#include "options.h"

namespace rxmd {

#define RX_HIP(call)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) throw EngineError(RXMD_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct EngineError {
  int code;
  std::string msg;
  EngineError(int c, std::string m) : code(c), msg(std::move(m)) {}
};

// ---- flattened force field in device memory -------------------------------------------------
struct DevAtomP { double Val, Valboc, mass, Vale, nlpopt, plp2, povun2, povun5, pval3, pval5, Valangle, Valval, chi, eta; };
struct DevBondP {
  double Desig, Depi, Depipi, pbe1, pbe2, povun1, ovc, v13cor;
  double pbo2, pbo4, pbo6, pboc3, pboc4, pboc5;
  double cBOp1, cBOp3, cBOp5, pbo2h, pbo4h, pbo6h, sw0, sw1, sw2, rc2;
};
struct DevAngleP { double theta00, pval1, pval2, pcoa1, pval7, ppen1, pval4; };
struct DevTorsP { double V1, V2, V3, ptor1, pcot1; };
struct DevHbP { double r0hb, phb1, phb2, phb3; };
// one r^2-table node, 64 bytes = one cache-line half: value and (next - this) for the four tabulated functions,
// so that an interpolation touches ONE node:  f(r2) = v + t * d   (reference lerp, pot.F90:729-743)
struct DevNBTab { double Evdw, dEvdw_, CEvdw, dCEvdw_, Eclmb, dEclmb_, CEclmb, dCEclmb_; };

struct DevFF {
  int nso, n1, nboty, ntoty, nvaty;
  const DevAtomP *atom; const DevBondP *bond; const DevAngleP *angle; const DevTorsP *tors; const DevHbP *hb;
  const int *inxn2, *inxn3, *inxn3hb, *inxn4;
  const unsigned *tor_bits;     // inxn4 != 0 as a bit table of 4096 bits (valid when n1 <= 8): k_e4b keeps it in LDS
  const DevNBTab *tabNB;   // [inxn * (NTABLE+2) + i]
  const double *tabQEq;    // [inxn * (NTABLE+2) + i]
  const double2 *tabQEq2;  // the same as pairs (T[i], T[i+1])
  double UDR, UDRi, rctap2, rctap_pad, cutoff_vpar30, vpar1, vpar2;   // rctap_pad: taper cutoff + the sweep padding (lists.hip)
  double plp1, povun3, povun4, povun6, povun7, povun8;
  double pval6, pval8, pval9, pval10, ppen2, ppen3, ppen4, pcoa2, pcoa3, pcoa4, ptor2, ptor3, ptor4, pcot2;
  // PQEq (pqeq != 0): per-type core charge Z and shell spring K, pair rows, and the three screened-Coulomb tables
  // (core-core, shell-core, shell-shell) as nodes (E, E_next - E, F, F_next - F), F = (1/r) dE/dr   (module.F90:537-611)
  int pqeq, npq1;
  const double *Zpq, *Kspq;
  const int *inxnpq;            // [a * npq1 + b]
  const double4 *tabPcc, *tabPsc, *tabPss;   // [row * (NTABLE+2) + i]
};

struct Box {
  double H[3][3], Hi[3][3];  // GetBoxParams / matinv, reference src/init.F90:610-633, main.F90:557-579
  double lat[6];
  double lbox[3];   // normalised local box edge = 1/vprocs          (init.F90:659)
  double obox[3];   // normalised origin of this rank                (init.F90:665)
  double volume;
};

struct Grid {       // the engine's own cell grid over [-shell, L+shell) in normalised local coords
  int n[3];         // cells per dimension
  double org[3];    // normalised origin (negative)
  double inv[3];    // cells per unit of normalised coordinate
  int ncell;
  // every cell is cut into fz slices along z and the atoms are sorted by (x, y, z-slice): a column (x, y) of the grid is one contiguous,
  // z-ordered run of the sorted arrays, so a sweep takes from each column only the slices within reach of ITS atom (lists.hip)
  int fz, nzf;      // slices per cell; n[2] * fz
  int nfine;        // n[0] * n[1] * nzf = length of cellstart - 1
  double wid[3];    // perpendicular real width of one unit of normalised coordinate (orthorhombic: the lattice constant)
  double cw[3];     // 1 / inv: cell edge in normalised units
  double iwz;       // 1 / wid[2]
  int ortho;        // 1: the three directions are orthogonal (distance^2 = sum of the three gaps^2), 0: only max(gap) is a bound
  int probe;        // timing experiments only (RXMD_LIST_PROBE): 1 = the 10 A sweep stops after its per-row set-up, 2 = it skips the emission
};

// The reference's own cell meshes (non-orthogonal boxes only).  Its linked-list cells are laid out in units of the lattice VECTORS and
// its stencils assume orthogonal axes (NEIGHBORLIST: +-1 cell, main.F90:349-351; the non-bonded mesh: cells whose offset passes an
// orthogonal distance test, init.F90:549-592), and its QEq ghost shell is rctap divided by the lattice constants (qeq.F90:32).  In a
// skewed cell these select FEWER pairs than the cutoffs do; the lists reproduce the selection so that the matrix and the forces are
// the reference's.  With 90-degree angles every pair inside a cutoff passes all three and nothing is evaluated.
struct RefMesh {
  double Hi[9], obox[3];   // xu2xs: the reference bins ALL atoms, ghosts included, by Hi.r - obox (LINKEDLIST, main.F90:298)
  double lc[3];            // bonded cell, normalised (lcsize, init.F90:661)
  double nbl[3];           // non-bonded cell, normalised (nblcsize, init.F90:605)
  double nblr[3];          // the same in length units of its lattice vector (init.F90:545)
  double qlo[3], qhi[3];   // QEq ghost shell in normalised local coordinates: (-QCopyDr, lbox + QCopyDr]  (qeq.F90:32,69; comm.F90:551-576)
};

constexpr int WAVE = 64;

// ---- the two scalar blocks, in doubles: `scal` in device memory and its pinned host mirror `h_scal`.  Every slot of either is named HERE. ----
// The CG scalars sit at the head of both (the host copies [0, S_COUNT) across as one piece); S_RAW0..7: the sums a reduction leaves for the algebra
enum { S_MU = 0, S_LMIN_S, S_LMIN_T, S_GOLD_S, S_GOLD_T, S_GNEW_S, S_GNEW_T, S_EST, S_GH_S, S_GH_T, S_HSH_S, S_HSH_T, S_SSUM, S_TSUM, S_BETA_S, S_BETA_T, S_RAW0, S_RAW1, S_RAW2, S_RAW3, S_RAW4, S_RAW5, S_RAW6, S_RAW7, S_STOP, S_STOP1, S_TOL, S_COUNT };
constexpr int SCAL_CG_N = 32, SCAL_N = 208, H_SCAL_N = 320;   // the range of the CG scalars (a QEq call clears it in front of its start vector) ; doubles of either block
constexpr int SCAL_PE = 32, SCAL_PE_N = 16, H_SCAL_PE = 32;   // the energy accumulators PE(0:13) of FORCE, and where the host reads them
constexpr int SCAL_ASTR = 48;                                 // the six stress accumulators astr: ENbond and the torsions reach them as pe + 16 (asserted next to those kernels)
constexpr int SCAL_PRINTE = 56, H_SCAL_PRINTE = 56;           // PRINTE's sums: kinetic energy, charge
constexpr int SCAL_REDUCE = 64, H_SCAL_REDUCE = 48;           // staging: of allreduce_host in device memory ; of the host all-reduce of scal[S_RAW0..] in pinned memory
constexpr int SCAL_EVAL_HEAD = 72, H_SCAL_EVAL_VIRIAL = 310;  // the device-array evaluate call (device_io.hip): astr as it found it ; its six virial sums (the egress kernel stores them there)
constexpr int H_SCAL_TOL = 60;                                // QEq_tol on its way to scal[S_TOL]
constexpr int S_SNAP = 128, S_SNAP_STRIDE = 32;               // scal[S_SNAP + 32 p ..]: snapshot of the scalars of an iteration of parity p (scalar_algebra stage 6)
constexpr int H_SCAL_SNAP = 64, H_SNAP_STRIDE = 64, H_SNAP_SEQ = 63;   // the same in pinned memory for the run-ahead CG loop, its sequence number in word 63: the update kernel's tail stores it, the host polls it
constexpr int H_SCAL_TSUM = 192, H_SCAL_TSUM_N = 6 * 16;      // per-type sums through a host transport
constexpr int SCAL_BAR_HEAD = 192, SCAL_BAR_STEP = 200, H_SCAL_BAR_OUT = 288, H_SCAL_BAR_REDUCE = 304;   // the barostat: step-head copy of astr, the step's sums ; pressure tensor and factors (p6, mu), staging of its all-reduce
struct ScalSlot { int at, n; };
constexpr bool slots_disjoint_within(const ScalSlot *s, int count, int total) {
  for (int i = 0; i < count; ++i) for (int j = 0; j <= i; ++j)
    if (s[i].at < 0 || s[i].n <= 0 || s[i].at + s[i].n > total || (j < i && s[i].at < s[j].at + s[j].n && s[j].at < s[i].at + s[i].n)) return false;
  return true;
}
constexpr ScalSlot SCAL_SLOTS[] = {{0, SCAL_CG_N}, {SCAL_PE, SCAL_PE_N}, {SCAL_ASTR, 6}, {SCAL_PRINTE, 6}, {SCAL_REDUCE, 8}, {SCAL_EVAL_HEAD, 6}, {S_SNAP, 2 * S_SNAP_STRIDE}, {SCAL_BAR_HEAD, 6}, {SCAL_BAR_STEP, 6}};
constexpr ScalSlot H_SCAL_SLOTS[] = {{0, SCAL_CG_N}, {H_SCAL_PE, SCAL_PE_N}, {H_SCAL_REDUCE, 8}, {H_SCAL_PRINTE, 2}, {H_SCAL_TOL, 1}, {H_SCAL_SNAP, 2 * H_SNAP_STRIDE}, {H_SCAL_TSUM, H_SCAL_TSUM_N}, {H_SCAL_BAR_OUT, 9}, {H_SCAL_BAR_REDUCE, 6}, {H_SCAL_EVAL_VIRIAL, 6}};
static_assert(slots_disjoint_within(SCAL_SLOTS, sizeof(SCAL_SLOTS) / sizeof(ScalSlot), SCAL_N), "two slots of the device scalar block overlap, or one leaves the block");
static_assert(slots_disjoint_within(H_SCAL_SLOTS, sizeof(H_SCAL_SLOTS) / sizeof(ScalSlot), H_SCAL_N), "two slots of the pinned scalar block overlap, or one leaves the block");
static_assert(S_COUNT <= SCAL_CG_N && S_COUNT <= S_SNAP_STRIDE && S_COUNT <= H_SNAP_SEQ, "the CG scalars fit their range and either snapshot slot");
static_assert(S_RAW0 + 8 <= S_STOP, "the eight raw sums stay inside the CG scalars");

// XCD-aware workgroup order: the dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (each with its own L2),
// so without a remap every L2 sees rows from all over the box and re-fetches the whole gather vector.  With it the
// workgroups that share an XCD own one contiguous eighth of the rows = one compact region of space (bijective for any grid).
__device__ inline int xcd_swizzle(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

inline int nblk(long long n, int b) { return n > 0 ? static_cast<int>((n + b - 1) / b) : 1; }   // workgroups of b lanes for n items; an empty rank still launches (kernels guard their range)

// The lattice for a kernel, by value: row-major, column c of H is lattice vector a_(c+1) (GetBoxParams, init.F90:610-633); Hi = H^-1
struct DevBox { double H[9], Hi[9]; };
inline DevBox dev_box(const Box &b) {
  DevBox d;
  for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) { d.H[3 * a + c] = b.H[a][c]; d.Hi[3 * a + c] = b.Hi[a][c]; }
  return d;
}

// The owner of ghost j among the residents of a single rank.  Two sources: groot[j] where the self exchange filled it (the 26-segment build and the
// local staged build, exchange.hip), or, when one rank runs through the transport (Engine::multi(): the host then passes gowner, else nullptr), the
// owner's local index that the staged exchange carries with every atom (gowner = index * 1024 + rank, k_pack_ghosts).  With several ranks the owner
// is on another rank and nothing asks for it (global ids only: the host refuses the rest).
__device__ inline int ghost_owner(int j, const long long *__restrict__ gowner, const int *__restrict__ groot) {
  return gowner ? static_cast<int>(gowner[j] >> 10) : groot[j];
}

// Sum of a double over the 64 lanes of a wavefront, the total returned to every lane.  HIP's __shfl_xor compiles to ds_bpermute (two per
// double and step: 12 dependent LDS-crossbar round trips per sum); this form stays in the vector ALU: four steps inside each row of 16
// lanes with DPP lane permutations (quad swaps, half-row mirror, row mirror), two row broadcasts (lane 15 -> next row, lane 31 -> upper
// half, written only where the row mask says), the total read from lane 63 into scalar registers.  Fixed summation order.
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_move(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  // The four full-row permutes write every lane: v_mov_dpp with NO defined `old` value (mov_dpp, not update_dpp(0, ...)) -- a defined one costs
  // a v_mov per DPP move to initialise the destination (48 of the ~300 vector instructions of a matrix-pass row).  The two masked row
  // broadcasts leave rows unwritten (rows 0 / 2, rows 0 / 1): there `old` is a defined 0, so the lanes they skip add 0.0 and every lane of the
  // wavefront holds a well-defined partial sum whatever the compiler does with the move (4 v_mov more per sum).
  if (ROW_MASK == 0xf) return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, CTRL, ROW_MASK, 0xf, false), __builtin_amdgcn_mov_dpp(lo, CTRL, ROW_MASK, 0xf, false));
  return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false), __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false));
}
__device__ inline double wave_sum64(double v) {
  v += dpp_move<0xb1, 0xf>(v);     // quad_perm:[1,0,3,2]
  v += dpp_move<0x4e, 0xf>(v);     // quad_perm:[2,3,0,1]
  v += dpp_move<0x141, 0xf>(v);    // row_half_mirror
  v += dpp_move<0x140, 0xf>(v);    // row_mirror: every lane of a row now holds the row's sum
  v += dpp_move<0x142, 0xa>(v);    // row_bcast:15 into rows 1 and 3
  v += dpp_move<0x143, 0xc>(v);    // row_bcast:31 into rows 2 and 3: lane 63 holds the total
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
// LDS hand-off between the lanes of ONE wavefront: what its lanes stored to LDS is visible to its other lanes behind this.  (The LDS queue of a wave
// is in order; the fences only stop the compiler from moving accesses across.)
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Timing probes of the experiments build (`make experiments`, -DRXMD_EXPERIMENTS) inside kernels of the step's path: "is probe n set" / "is one of
// these probe bits set" -- the literal false in the product build, so a statement guarded by one is written once and the product build's compiler
// drops it before it generates code (macros, not functions: a function's argument, the probe word, is no constant expression, and the guarded
// branch would reach the optimiser).  exp_probe is spelt !(word != n): most uses are negated, and `!exp_probe(w, n)` then reaches the compiler as the
// `w != n` it replaced -- with (word == n) the one-visit torsion kernels of the experiments build come out with other registers.
#ifdef RXMD_EXPERIMENTS
#define exp_probe(word, n) (!((word) != (n)))
#define exp_probe_mask(word, bits) (((word) & (bits)) != 0)
#else
#define exp_probe(word, n) false
#define exp_probe_mask(word, bits) false
#endif

#ifndef WIN_ROWS_DEF
#define WIN_ROWS_DEF 16
#endif
constexpr int WIN_ROWS = WIN_ROWS_DEF;   // rows of a window group = wavefronts of a workgroup of the window pass (measured: 8 -> see NOTES.md 3)
constexpr int WIN_UNIT = 8;         // cell-sorted positions per window unit (8 x 16 bytes = one 128-byte line of the sorted vector)
constexpr int WIN_BP_MIN_STRIDE = 384;   // streams by place (Engine::streams_by_place) need a row stride of at least 3 x 128 entries: the window pass then requests the first
                                        // batch of a place -- up to three register sets of 128 entries -- without a bound test (k_spmv_win, BP)
constexpr int WIN_MAXUNITS = 448;   // units a group's descriptor holds: 3,584 slots = 56 KB of LDS (two workgroups per CU)
constexpr int WIN_BMW = 2048;       // 64-bit words of the coverage map the build kernel keeps in LDS: a group's positions may span 2048 x 64 x 8 = 1 M

// ---- buffers.hip: the one allocator of the library, and the table of the engine's buffers --------------------------------------------
// Fill::Pattern: zeros, or 0xFF bytes under RXMD_POISON_ALLOC=1; Fill::Zero: the zero is part of a protocol; Fill::None: the owner writes all of it
enum class Fill : unsigned char { None, Zero, Pattern };
void *dev_alloc(size_t bytes, Fill fill);
void dev_free(void *p);
void *pinned_alloc(size_t bytes, bool coherent_mapped);   // always zeroed; coherent_mapped: a kernel stores into it and the host polls it
void pinned_free(void *p);
bool poison_enabled();
template <class T> void dev_alloc(T *&p, size_t n, Fill fill) { p = static_cast<T *>(dev_alloc(n * sizeof(T), fill)); }
template <class T> void dev_free(T *&p) { dev_free(static_cast<void *>(p)); p = nullptr; }

struct Engine;
enum class Dim : unsigned char { Fixed, NB, Rows10, List10, Cap };   // what a buffer's count scales with: nothing, NB, rows10, rows10 * S10, the capacity of its group
enum class Refill : unsigned char { Never, Whole, Ghosts };          // RXMD_POISON_ALLOC refill before a rebuild: none, the whole buffer, elements [N, NB)
enum class Space : unsigned char { Device, Pinned, PinnedCoherent };
// re-allocation groups.  Those before G_ON_DEMAND exist from set-up on (Buffers::alloc_setup); the others are allocated when first needed
enum { G_SETUP, G_BOND, G_WIN, G_CELLSTART, G_LIST10, G_PARTIALS, G_ON_DEMAND, G_CUBTMP = G_ON_DEMAND, G_FFBLOB, G_PQBLOB, G_E4B, G_SEG, G_SEG_PINNED, G_XBUF, G_DH_SERVE, G_BGRAPH, G_BVJP, G_PGRAPH, G_STRUCT, G_COUNT };
enum : unsigned { BUF_PQEQ = 1u, BUF_RESIDENT = 2u, BUF_QEQ_F32 = 4u };   // exists only with PQEq ; resident state that grow_capacity carries over ; exists only while the fp32 matrix stream is requested (set_qeq_precision)
struct Buf { void **pp; size_t elem; int group; Dim dim; size_t mul, add_; Fill fill; Refill refill; unsigned flags; Space space; size_t bytes; };   // bytes: what was allocated (0: nothing of ours)
struct Buffers {
  std::vector<Buf> v;
  size_t cap[G_COUNT] = {};        // capacity each group was last allocated at (Dim::Cap)
  template <class T> void add(T *&p, int group, Dim dim, size_t mul, size_t addend, Fill fill, Refill refill, unsigned flags = 0) {
    size_t elem = 1;               // (void *: bytes)
    if constexpr (!std::is_void_v<T>) elem = sizeof(T);
    add_raw(reinterpret_cast<void **>(&p), elem, group, dim, mul, addend, fill, refill, flags);
  }
  void add_raw(void **pp, size_t elem, int group, Dim dim, size_t mul, size_t addend, Fill fill, Refill refill, unsigned flags = 0) {
    v.push_back(Buf{pp, elem, group, dim, mul, addend, fill, refill, flags, Space::Device, 0});
  }
  template <class T> void add_pinned(T *&p, int group, size_t n, bool coherent_mapped) {
    v.push_back(Buf{reinterpret_cast<void **>(&p), sizeof(T), group, Dim::Fixed, 0, n, Fill::Zero, Refill::Never, 0u, coherent_mapped ? Space::PinnedCoherent : Space::Pinned, 0});
  }
  size_t count(const Buf &b, const Engine &e) const;
  void alloc_one(Buf &b, const Engine &e); void free_one(Buf &b);
  void alloc_setup(const Engine &e);                               // every group that exists from set-up on, at the capacities in cap[]
  void alloc_group(const Engine &e, int group, size_t capacity = 0);   // all or nothing; capacity only for groups with a Dim::Cap entry (the caller frees the group first unless it keeps the old blocks itself)
  void free_group(int group); void free_all();
  void refill(const Engine &e);
  std::vector<std::vector<char>> save_residents(const Engine &e) const;
  void restore_residents(const std::vector<std::vector<char>> &h);
};
constexpr size_t EHB_DON_EXTRA = 64 * 256 + 256;   // donor list beyond one entry per row: 64 sub-lists (hbonds.hip EHB_REGIONS) padded to 256

// engine state that a block changes and every way out of it, an exception included, puts back
template <class T> struct Restore {                   // a value: what `ref` held when the block was entered
  T &ref; const T old;
  explicit Restore(T &r) : ref(r), old(r) {}
  Restore(T &r, T inside) : ref(r), old(r) { r = inside; }
  ~Restore() { ref = old; }
};
struct StreamSwap {                                   // the engine's stream against another one; `inside` (optional) is true for as long
  hipStream_t &a, &b; bool *inside;
  StreamSwap(hipStream_t &a_, hipStream_t &b_, bool *inside_ = nullptr) : a(a_), b(b_), inside(inside_) { std::swap(a, b); if (inside) *inside = true; }
  ~StreamSwap() { if (inside) *inside = false; std::swap(a, b); }
};

struct ScaleArgs;
struct PairList;                         // what the kernels of pair_graph.hip and structure.hip need to walk a row of the 10 A list (pair_walk.h)
struct WinPassArgs; struct RowPassArgs;   // the operands of the two matrix-pass kernels (spmv_kernels.h)
struct Engine {
  const Options opt = Options::from_env();   // the environment switches of this engine (options.def), read once at create
  rxmd_config cfg{};
  std::string ffield_path, pqeq_path, err;
  ForceField ff;
  Box box{};
  int vID[3] = {0, 0, 0}, target_node[7] = {0}, nprocs = 1;
  double dt = 0, Lex_w2 = 0;
  std::vector<double> dthm, hmas;
  rxmd_comm_ops comm{};
  bool has_comm = false, tables_ready = false, atoms_set = false, lists_valid = false, ghosts_valid = false;

  // capacities
  int NB = 0, MAXNB = 30, S10 = 0, rows10 = 0;
  int max_row10 = 0, min_row10 = 0;   // longest / shortest row of the current 10 A list
  int num_cu = 256;               // compute units of the device: grid of the persistent kernels (one workgroup per CU)
  int N = 0, G = 0, copyptr[7] = {0};
  int cc[3] = {1, 1, 1};          // reference bonded cell counts, only to derive the ghost shell (init.F90:656)
  double shell[3] = {0, 0, 0};    // FORCE ghost shell in normalised units: NMINCELL*lcsize (pot.F90:28)
  Grid grid{};
  RefMesh rmesh{};

  // ---- device memory (declared once, in Engine::declare_buffers of buffers.hip) ----
  Buffers bufs;
  void declare_buffers();
  DevFF dff{};
  void *ffblob = nullptr, *pqblob = nullptr;
  double *pos[3] = {}, *vel[3] = {}, *frc[3] = {}, *spos[3] = {};  // real pos, v, f ; normalised-local pos (ghost build)
  double *q = nullptr, *qsfp = nullptr, *qsfv = nullptr;
  // PQEq: shell displacement of every atom (reference spos, module.F90:286; real units, travels with the atom), its cell-sorted
  // copy, the shell-core matrix values of the 10 A list and per-row constants (fpqeq, sum H Z, sum Hsc Z, shell-shell energy)
  double *shl[3] = {}; double4 *sorted_shl = nullptr; double *hsc = nullptr; double4 *pqrow = nullptr;
  int *type = nullptr; long long *gid = nullptr;
  double2 *qst = nullptr, *hst = nullptr, *gst = nullptr;  // (qs,qt) (hs,ht) (gs,gt) interleaved
  double2 *hst2 = nullptr;     // second (hs,ht) buffer: the fused direction kernel reads the old and writes the new one (qeq.hip)
  unsigned *tickets = nullptr; // arrival counters of the in-kernel final reductions (qeq.hip, block_finish)
  double2 *sall = nullptr, *sgh = nullptr, *wall = nullptr, *wgh = nullptr;  // qeq_mode 1: row sums H.(qs,qt), H.(hs,ht): all columns / ghost columns
  int *gsrc = nullptr, *groot = nullptr;                    // ghost -> source index on sender ; -> resident root (self exchange)
  int *rootperm = nullptr;                                  // cell-sorted position -> resident that owns the value (ghosts resolved)
  int *invpos = nullptr;                                    // atom (resident or ghost) -> its cell-sorted position: the direction kernel of the CG scatters the new vector straight into xs
  double2 *xs = nullptr;                                    // cell-sorted gather copy of a QEq vector pair (residents+ghosts)
  int *sendidx = nullptr; int sendoff[8] = {0};             // per-stage send index lists (local indices), concatenated
  // cell binning
  int *cellid = nullptr, *cellid_sorted = nullptr, *perm = nullptr, *perm_in = nullptr, *cellstart = nullptr;
  double4 *sorted_xyzi = nullptr;   // cell-sorted (x,y,z,index-as-bits) copy of real positions
  unsigned char *sorted_type = nullptr;   // cell-sorted atom types (the window form of ENbond stages them next to the positions)
  bool nb10_valid = false, nb10_sticky = false;   // this list build wrote the 4-byte entry stream / a reader once found it missing: every build writes it (lists.hip: needs_nb10)
  bool needs_nb10(bool selfcheck) const;
  bool sorted_w_charge = false;     // the w of the packed cell-sorted copy holds the charge (charge_halo) and no longer atom index | type (bin_cells), which the list sweeps read
  void sorted_positions();          // the packed cell-sorted copy of the positions, w = atom index | type
  void sorted_charge_only();
  void require_nb10();              // called in front of every reader of nb10 but the hydrogen-bond sweep: sweeps the lists again with the stream on when this build left it out
  bool list_selfcheck = false;      // this list build: some box edge is shorter than two cut-offs, an atom can meet its own image
  void *cubtmp = nullptr; size_t cubtmp_bytes = 0;
  int *flags = nullptr, *scanout = nullptr;
  // bonded tables, compact: boff[i] .. boff[i + 1] are the bonds of atom i (residents and ghosts) in list order; per bond its partner (nbr), its owner
  // (bown) and its mirror image, the same bond in the partner's list (brev = the reference's nbrindx, main.F90:383-399, as a direct index)
  int *nbr = nullptr, *nbrcnt = nullptr, *boff = nullptr, *brev = nullptr, *bown = nullptr;
  unsigned char *btype = nullptr; // per bond: type of the partner atom
  int *nbr_sm = nullptr;          // atom-major staging of the list sweep [atom * 32 + slot] (a thread appends without knowing the totals; one 128-byte line per atom)
  size_t bcap = 0; int nbonds = 0; // capacity of the per-bond arrays (grown on demand) / bonds of the current build
  void alloc_bond_tables(size_t cap); void free_bond_tables();
  double *bo0 = nullptr, *bo1 = nullptr, *bo2 = nullptr, *bo3 = nullptr, *dln2 = nullptr, *dln3 = nullptr, *dBOp = nullptr;
  double *A0 = nullptr, *A1 = nullptr, *A2 = nullptr, *A3 = nullptr;
  double *cf1 = nullptr, *cf2 = nullptr, *cf3 = nullptr, *cdn = nullptr, *fnx = nullptr, *fny = nullptr, *fnz = nullptr;
  double *etor = nullptr, *econ = nullptr, *epen = nullptr, *ecoa = nullptr;   // per-bond exponentials shared by many angles/torsions
  double *bt1 = nullptr, *bt2 = nullptr, *bt3 = nullptr;                        // per-bond scratch: terms a lane-per-bond kernel leaves for the per-atom sum behind it
  double *ecoef = nullptr;                                                      // 6 per-atom coefficients of Elnpr (bonded.hip)
  // one-visit torsions (torsions.hip, k_e4b<*, true>): the k-l side of a torsion -- ForceB coefficient of bond k-l and the force on l, summed over i -- per
  // (bond (k, l1), slot of j in the list of k), TW columns per bond, with one flag byte per entry (all zero between FORCE calls)
  double4 *e4b_t = nullptr; unsigned char *e4b_flag = nullptr; size_t e4b_cap = 0; bool e4b_dirty = false;
  void alloc_e4b_delivery(size_t entries);
  int nbonds_res = 0;                                                           // bonds of the residents = boff[N]: the first nbonds_res entries of the tables
  int2 *ehb_don = nullptr; size_t ehb_don_cap = 0; int *ehb_cnt = nullptr; unsigned ehb_donor_types = 0u; int ehb_blocks_per_cu = 0, ehb_blocks_per_cu_sl = 0; // (_sl: of the sweep over the window slots) hydrogen bonds (hbonds.hip): donor list (atom, mask of its hydrogen slots), its length, types X with a row (X, H = 2, any)
  double *deltap = nullptr, *delta = nullptr, *nlp = nullptr, *dDlp = nullptr, *deltalp = nullptr;
  double *cds = nullptr, *cd = nullptr, *cc_ = nullptr;
  // 10 A list
  int *nb10 = nullptr, *n10 = nullptr; double *hess = nullptr;
  // Mixed-precision charge solver (rxmd_hip_set_qeq_precision; plain QEq only): with 32 requested the list sweep rounds every matrix value ONCE to
  // REAL(4) and writes it to both streams -- hess (double: row pass, debug tap 7) and hess32 (float: the fp32 instance of the window pass, 6 instead
  // of 10 bytes per entry) -- and forms its row sums of the start vector from the rounded value: one operator on every path.  Products, sums,
  // vectors and scalars stay double.  qeq_bits_used: width of the value stream the last matrix pass read.
  float *hess32 = nullptr;
  int qeq_bits_req = 64, qeq_bits_used = 64;
  void set_qeq_precision(int bits);
  size_t partials_cap = 0;
  // reductions
  double *partials = nullptr;  // [nblocks_red * 16]
  double *scal = nullptr;      // device scalars (CG state)
  double *h_scal = nullptr;    // pinned host mirror
  int *d_err = nullptr, *h_err = nullptr, *h_cnt = nullptr;   // h_err: pinned, H_ERR_INTS ints: H_ERR_WORDS of the device error words, then h_cnt, the counts the host waits for (H_CNT_*)
  int longest_bond_list() const { return h_err[2]; }          // of the step's list build (read back with the error word); 0 when no list is longer than 8
  double *xbuf_send = nullptr, *xbuf_recv = nullptr; size_t xbuf_doubles = 0; bool xbuf_owned = false;   // staged-exchange message buffers
  double pe[14] = {0}, astr[6] = {0};

  hipStream_t stream = nullptr;
  // second stream for the halo exchanges that overlap with compute (multi-rank): pack / RCCL send-recv / unpack run here while
  // the main stream works on what does not need the ghosts yet; events order the two (engine.hip: on_comm_stream)
  hipStream_t comm_stream = nullptr; hipEvent_t ev_main = nullptr, ev_comm = nullptr, ev_est = nullptr, ev_pass[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // ev_est: Est of a CG iteration has reached the host
  template <class F> void on_comm_stream(F &&body) {          // body runs with `stream` == comm_stream, after everything queued on the main stream so far
    RX_HIP(hipEventRecord(ev_main, stream));
    RX_HIP(hipStreamWaitEvent(comm_stream, ev_main, 0));
    { StreamSwap on_comm(stream, comm_stream, &in_comm_region); body(); }
    RX_HIP(hipEventRecord(ev_comm, comm_stream));
  }
  bool in_comm_region = false;
  // third stream: the part of FORCE that needs no charges (bond orders, every bonded term, the assembly of the bonded forces) runs next to the
  // ghost-charge halo and the nonbonded sweep (assemble.hip: bonded_chain_begin).  RXMD_NO_BOND_OVERLAP=1: one stream, as until round 5.
  hipStream_t bond_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_bond = nullptr;
  double *fsort[3] = {nullptr, nullptr, nullptr};           // hydrogen-bond acceptor forces by CELL-SORTED position (neighbouring candidates = neighbouring addresses: the atomics coalesce); added to frc behind the sweep
  double *fnb[3] = {nullptr, nullptr, nullptr};             // ENbond's force on the residents while the bonded chain owns frc; added behind the join
  bool bond_overlap() const { return bond_stream != nullptr && !ff.pqeq; }
  void bonded_chain_begin();
  // main stream waits for what on_comm_stream queued; the wait itself is timed: that is the part of the exchange the compute did not hide
  void join_comm_stream() { Timed kt(this, &st.ms_halo_exposed, nullptr, nullptr, 2); RX_HIP(hipStreamWaitEvent(stream, ev_comm, 0)); }
  hipEvent_t ev[8] = {};
  std::vector<double> last_atype, last_pos[3];    // what the array-shaped entry points uploaded last (capi.hip)
  std::vector<double> lex_p, lex_v; bool lex_pending = false;   // qsfp/qsfv handed over by rxmd_hip_put_lex for the next array-shaped QEq/PQEq
  rxmd_stats st{};
  int nstep_qeq = 0; double last_est = 0;
  std::vector<double> est_trace;   // Est of the start vector and of every CG iteration of the last QEq call (host side, a few hundred doubles)
  double atype_resid = 0.0;        // geninit packs atype = type + gid*1e-13 + 1e-14 (geninit.F90:459), ReadXYZ without it (fileio.F90:421): what came in goes out
  long long step_count = 0;
  unsigned long long velocity_draws = 0;    // INITVELOCITY calls so far: the draw index of the counter-based generator (assemble.hip)

  // ---- host API ----
  explicit Engine(const rxmd_config &c);
  ~Engine();
  void kinetic_and_charge(double &ke, double &qsum);   // sum hmas v^2 and sum q over the residents (PRINTE, main.F90:225-230); assemble.hip
  void set_atoms_rxff(int natoms, const double *rec10);
  // the same from the reference's own arrays (atype packed as type + gid*1e-13, REAL coordinates by component): no host-side record,
  // the packed type is split on the device.  Only once the engine is sized (after a first set_atoms_rxff); velocities are zeroed.
  void set_atoms_arrays(int natoms, const double *atype, const double *x, const double *y, const double *z, const double *q, const double *lexp, const double *lexv);
  int get_atoms_rxff(double *rec10, int capacity);
  // rxmd_hip_evaluate_device (device_io.hip): caller-ordered DEVICE arrays in (wrapped into the box on the way), QEq + FORCE, forces / charges back out;
  // `user` is the caller's stream, joined to the engine's by an event on either side.  eval_natoms: atoms of the last such call whose charges are
  // still in q in the caller's order (-1: none -- another entry point has set or moved the atoms since)
  void evaluate_device(int natoms, const long long *gid_d, const int *type_d, const double *pos3_d, const double *q_in_d, double *f3_d, double *q_out_d,
                       double pe_out[14], double virial_out[6], hipStream_t user);
  void size_from_device_arrays(int natoms, const int *type_d, const double *pos3_d, hipStream_t user);
  hipEvent_t ev_io_in = nullptr, ev_io_out = nullptr;
  // The scope of that join, for every call that works on the caller's device arrays: entered, `stream` waits for what `user` has queued so far; at end()
  // -- or from the destructor on the way out of the block, an exception included -- `user` waits for what the block queued on `stream`, so that no way
  // out leaves the caller's stream unordered behind the engine's work on the caller's arrays.  The two events are created on first use.
  struct UserStream {
    Engine &e; const hipStream_t user; bool open = false;
    UserStream(Engine *eng, hipStream_t user_) : e(*eng), user(user_) {
      if (!e.ev_io_in) { RX_HIP(hipEventCreateWithFlags(&e.ev_io_in, hipEventDisableTiming)); RX_HIP(hipEventCreateWithFlags(&e.ev_io_out, hipEventDisableTiming)); }
      RX_HIP(hipEventRecord(e.ev_io_in, user));
      RX_HIP(hipStreamWaitEvent(e.stream, e.ev_io_in, 0));
      open = true;
    }
    void end() {
      if (!open) return;
      open = false;
      RX_HIP(hipEventRecord(e.ev_io_out, e.stream));
      RX_HIP(hipStreamWaitEvent(user, e.ev_io_out, 0));
    }
    ~UserStream() { try { end(); } catch (const EngineError &) {} }   // (on the way out an exception is already in flight, as in ~Timed)
    UserStream(const UserStream &) = delete;
  };
  // a scratch group on first use or when it has to grow: nothing queued may still read the old blocks
  void regrow_group(int group, size_t capacity = 0) { sync_stream(); bufs.free_group(group); bufs.alloc_group(*this, group, capacity); }
  // scan.h (the export units only): exclusive sum of cnt[0 .. n] into off[0 .. n] on `stream` -- cnt[n] = 0, so off[n] is the total --, G_CUBTMP grown
  // when n + 1 items need more than it holds, the total through the pinned slot H_CNT_EXPORT: ONE sync_stream(), the host wait of the caller
  template <class T> long long exclusive_sum_total(T *cnt, T *off, int n);
  int eval_natoms = -1;
  // rxmd_hip_get_bonds_device (device_io.hip): the residents' part of the compact bond tables as coordinate (COO) arrays in DEVICE memory, entries with
  // bo0 >= bo_min in table order -- flag per entry, exclusive sum, fill.  src = dst = bo = nullptr: count only.  Returns the number selected; nothing is
  // written when capacity is smaller.  bg_flag / bg_off: its scratch, one int per table entry + 1, allocated on first use at the capacity of the bond tables
  long long bonds_device(int flags, double bo_min, long long capacity, long long *src_d, long long *dst_d, double *bo_d, double *bo3_d, double *vec3_d, hipStream_t user);
  int *bg_flag = nullptr, *bg_off = nullptr;
  long long select_bonds(double bo_min);           // bg_flag / bg_off of the residents' entries for this threshold -> the number selected (the one host wait of either caller)
  // rxmd_hip_bonds_vjp_device (bond_vjp.hip): the vector-Jacobian product of that graph with respect to the positions.  grad_bo / grad_bo3 / grad_vec3 are
  // dL/d(bo, bo3, vec3) in the edge order of bonds_device(flags, bo_min); grad_pos3[N][3] = dL/dr of the residents, ghosts folded onto their owners.
  // The assembly of assemble.hip with the caller's coefficients in place of cf1..cf3, cd = 0 and no fn*; reads what FORCE left (bo*, A0..A3, dBOp, dln*),
  // writes its own scratch only: bv_c1..3 (per table entry: the symmetrised coefficients, then the three force-term components in place), bv_t (the
  // ccbnd term), bv_cc and bv_g (per atom, ghost slots included); allocated on first use at the capacities of the day (bv_nb: the NB they were sized for)
  void bonds_vjp_device(int flags, double bo_min, long long E, const double *grad_bo_d, const double *grad_bo3_d, const double *grad_vec3_d, double *grad_pos3_d, hipStream_t user);
  double *bv_c1 = nullptr, *bv_c2 = nullptr, *bv_c3 = nullptr, *bv_t = nullptr, *bv_cc = nullptr, *bv_g[3] = {nullptr, nullptr, nullptr}; int bv_nb = 0;
  // rxmd_hip_get_pairs_device (pair_graph.hip): the residents' rows of the 10 A list as coordinate (COO) arrays in DEVICE memory, entries with
  // |vec| <= r_cut (r_cut <= 0: all) in resident order and list order -- count per row, 64-bit exclusive sum, fill.  src = dst = nullptr: count only.
  // Returns the number selected; nothing is written when capacity is smaller.  pg_cnt / pg_off: its scratch, one 64-bit word per row + 1, allocated on
  // first use at the rows10 of the day (pg_rows) and again when the rows have grown
  long long pairs_device(int flags, double r_cut, long long capacity, long long *src_d, long long *dst_d, int *shift3_d, double *vec3_d, double *hval_d, hipStream_t user);
  long long select_pairs(double r_cut);            // pg_cnt / pg_off for this cut-off -> the number selected (the one host wait of the call)
  PairList pair_list(double r_cut) const;
  long long *pg_cnt = nullptr, *pg_off = nullptr; int pg_rows = 0;
  // rxmd_hip_structure_* (structure.hip): int64 accumulators of the structure statistics in one block sg_acc = pair counts [nso][nso][nbins_r], angle
  // counts [nshells][nso][nso][nso][nbins_angle], residents per type [nso]; allocated by structure_begin, resident state (grow_capacity carries it
  // over), freed by structure_end.  The volume sum and the frame count stay on the host: the lattice is host state
  void structure_begin(double r_max, int nbins_r, int nshells, const double *angle_cut, int nbins_angle);
  void structure_sample();                         // the state of the last list build into the accumulators, on `stream`; no host wait beyond finish_force
  void structure_get(long long *pair_counts, long long pair_capacity, long long *angle_counts, long long angle_capacity, long long *atoms_per_type, double *volume_sum, long long *frames);
  void structure_end();
  long long *sg_acc = nullptr; bool sg_on = false;
  double sg_rmax = 0, sg_cut[4] = {0, 0, 0, 0}, sg_volume = 0; int sg_nbr = 0, sg_nsh = 0, sg_nba = 0;
  size_t sg_npair = 0, sg_nangle = 0; long long sg_frames = 0;
  void build_ghosts_and_lists(bool qeq_prepass = false);   // COPYATOMS(MODE_COPY) + LINKEDLIST + NEIGHBORLIST + 10 A list/hessian, once per step
  void qeq_start_vectors();        // qs, qt, hs, ht of qeq.F90:36-63 and their cell-sorted copy (before the list sweep that uses them)
  int *rows_int = nullptr, *rows_bnd = nullptr; int n_bnd = 0; bool rows_split_pending = false;   // interior / boundary rows (multi-rank)
  bool rows_split_pending_invalid() const { return n_bnd < 0 || n_bnd > N; }
  bool sums_from_list = false;     // the list sweep left H.(qs,qt) of the CG start vector in sall / sgh
  void qeq();
  // ---- the pieces of qeq() (qeq.hip) ----
  // the instance of k_spmv_win<MODE, STORE, PQ, nstep, var, double | float> this engine runs: chosen in ONE place, for the solver and the placement search
  struct WinInstance { int nstep, var; bool f32; };
  WinInstance win_instance() const;
  WinPassArgs win_args(bool roword = false) const;   // the operands of a window pass over the whole grid, no stop flag; roword: the per-row operands by the rows' places (r_*)
  RowPassArgs row_args() const;                      // the same for the row pass k_spmv
  // one matrix pass: row sums into ra / rg (store), over all rows or the rows of rowlist (rows_int / rows_bnd: behind the pbase workgroups of the other launch)
  struct PassCall { int mode; bool store; double2 *ra = nullptr, *rg = nullptr; const int *rowlist = nullptr; int nrows = 0, pbase = 0; const double *stopflag = nullptr; bool roword = false; };
  int matrix_pass(const PassCall &c);                // returns the number of partial-sum sets (of four) the launch leaves behind partials[pbase * 4]
  void cg_reduce(int stage, int nsets, const double *stopflag = nullptr);   // the sets -> scal[S_RAW0..3], all ranks, and the scalar algebra of `stage`
  struct CgCall { int nmax, vb, vb_upd; bool onepass, runahead, est_with_update, cg_scatter; };   // what one QEq call fixes for its loops: iteration cap, grids of the vector kernels, the loop form
  double qeq_start(const CgCall &c);                 // gradient, Est and first direction of the start vector -> Est (0 when the run-ahead loop will read it later)
  int qeq_runahead(const CgCall &c, double &Est);    // the two CG loops -> iterations done
  int qeq_host_paced(const CgCall &c, double &Est);
  struct TimedSection;
  void qeq_finish(int it, double Est, TimedSection &t_qeq); // shells, iteration statistics, the call's timer, once: the placement search
  // observe_energy = false (Engine::step, every step but the last of a call): nothing reads this FORCE's energies -- ENbond skips its pair and self
  // energies, PE(11:13) stay 0 in the block that the next observed FORCE overwrites.  Forces and the virial (astr accumulates over steps) are untouched.
  void force(bool defer_host_read = false, bool observe_energy = true);   // defer: the energies stay in the pinned buffer until finish_force() (step(): no host wait between FORCE and the next step)
  void finish_force();
  bool force_pending = false;
  // run-ahead CG loop (qeq.hip): the scalars of an iteration reach the host as a snapshot the update kernel's tail writes straight into pinned host memory
  // (h_scal + H_SCAL_SNAP + H_SNAP_STRIDE * parity, sequence number in word H_SNAP_SEQ), no copy, no event: the host polls the sequence number
  unsigned long long snap_seq = 0; double snap_expect[2] = {0.0, 0.0};
  void wait_snapshot(int parity, double seq);
  // the matrix pass is timed on a SAMPLE of its launches there (opt.pass_timing_every): sum and count of the timed ones; rxmd_stats.ms_qeq_spmv = average x all launches
  unsigned long long pass_counter = 0; bool pass_timed_k[2] = {false, false}; double pass_timed_ms = 0.0; long long pass_timed_n = 0;
  void step(int nsteps);
  void migrate();                  // COPYATOMS(MODE_MOVE)
  void thermostat(int mdmode, double treq_K, double vsfact, double gke);   // velocity scaling of the MD loop head (assemble.hip)
  int minimise(double ftol, int max_loops, double *pe_final, long long *evaluations);   // mdmode 10: the reference's conjugate-gradient minimiser (minimise.hip)

  // ---- variable cell (engine.hip: set_lattice; assemble.hip: the barostat of step()) ----
  // set_lattice: the residents keep their normalised coordinates (k_affine_remap), the box-dependent half of the set-up is derived
  // again (derive_box_geometry), buffers sized by the grid follow it, and the per-atom capacity grows when the new ghost shell needs it
  void set_lattice(const double lat[6], bool check_ranks);
  void apply_lattice(const double lat[6]);     // no validation: the caller checked (set_lattice) or computed the lattice from all-reduced sums (barostat)
  void check_lattice(const double lat[6]) const;   // RXMD_E_ARG for a lattice that spans no box or a local box below the bond cutoff
  struct BoxGeom { int cc[3]; double shell[3]; Grid grid; RefMesh rmesh; };
  BoxGeom geometry_for(const Box &b) const;    // cc, shell, grid, rmesh of box b (the part of setup_after_atoms that depends on the lattice)
  void derive_box_geometry();                  // the same for `box`, into the members
  long long capacity_want(const double shell_n[3]) const;   // the NB set-up would choose for a ghost shell shell_n (rxmd_config.nbuffer = 0)
  void grow_capacity(int new_nb);              // every per-atom buffer re-allocated at new_nb; the residents' state and the device scalars kept
  void alloc_window_groups(size_t ng);   // ng window groups (win_groups_bound(rows10) + 1 of a grid) + rpos / g_rrow
  size_t cellstart_cap = 0, win_ng_cap = 0;    // what is allocated: grid.nfine + 2 ; win_groups_bound(rows10) + 1 of the grid they were sized for
  long long nsize_setup = 0;                   // the per-rank atom count set-up sized the engine for
  // Berendsen barostat (rxmd_hip_set_barostat): mode 0 off, 1 isotropic, 2 per axis; coupled behind the second half-kick of every `every`-th step
  int bar_mode = 0, bar_axes = 7, bar_every = 1;
  double bar_p0[3] = {0, 0, 0}, bar_tau = 0, bar_B = 0, bar_max = 0;
  double bar_p6[6] = {0, 0, 0, 0, 0, 0}, bar_mu[3] = {1, 1, 1}, bar_vol = 0;   // last coupling: pressure tensor [GPa], factors, the volume the forces were computed at
  long long bar_couplings = 0;
  void set_barostat(int mode, int axes, const double p0[3], double tau_fs, double bulk_GPa, int every, double max_strain);
  void barostat_couple();

  // pieces (each in its own .hip)
  void setup_after_atoms(const std::vector<long long> &natoms_per_type_global);
  void upload_ff();
  void alloc_device();
  void free_device();
  void ghost_build();
  void ghost_build_fused(); void migrate_fused(); void ensure_seg_buffers(int nblocks);   // single rank: the six-stage self exchange as 26 image segments (exchange.hip)
  // counts the host waits for, handed over through pinned host memory: word = sequence number << 32 | value; the host polls until every word carries the
  // sequence number of its request (rccl_comm.hip: pinned_wait) -- no copy, no stream synchronisation, and the kernels queued behind the producer keep running
  unsigned long long *h_pub = nullptr; unsigned pub_seq = 0u;
  void pinned_wait(int nwords, unsigned seq, const char *what);
  int *seg_cnt = nullptr, *seg_tot = nullptr, *h_seg = nullptr; unsigned char *seg_code_ = nullptr; int seg_blocks_cap = 0;
  void bin_cells();
  void build_bonded_list(bool pack_only = false);
  void build_list10();
  void build_prologue(int what);   // lists.hip: the words a list build starts from, one launch (1: bonded list, 2: 10 A list and windows)
  bool list10_retry = false;
  // Window form of the 10 A matrix (lists.hip, qeq.hip k_spmv_win): the residents in cell-sorted order in groups of WIN_ROWS rows; per group the
  // set of cell-sorted positions its rows couple to, in units of WIN_UNIT consecutive positions (win_k: first position of each unit, ascending;
  // win_cnt: units); per list entry a 16-bit slot in that window (sl10, bit 15 = ghost column).  The matrix pass stages the window's vector
  // entries in LDS with coalesced loads and reads them from there instead of gathering 16 bytes per entry.
  void build_windows();
  void tune_window_placement();   // qeq.hip: a few placements of the pass's streams in physical memory, the fastest kept (once per engine)
  bool place_tuned = false;
  int *rows_sorted = nullptr, *win_k = nullptr, *win_cnt = nullptr;
  int *win_flag = nullptr;                       // per group: 1 when one of its rows has a ghost partner (the sweep sets it; multi-rank: the boundary groups)
  int *rowcols = nullptr, *grp_base = nullptr;   // per row: first position and length of its 25 candidate runs (64 ints) ; per group: slot base of its 25 stencil columns (32 ints)
  int *win_gint = nullptr, *win_gbnd = nullptr; int win_nbnd = 0;     // multi-rank: groups without / with a row that has a ghost partner
  unsigned short *sl10 = nullptr;
  // run-ahead CG loop in ROW ORDER (qeq.hip): the CG vectors of the residents indexed by their place in rows_sorted (group * WIN_ROWS + wavefront of the window pass)
  double2 *r_qst = nullptr, *r_hst = nullptr, *r_hst2 = nullptr, *r_gst = nullptr, *r_sall = nullptr, *r_sgh = nullptr, *r_wall = nullptr, *r_wgh = nullptr;
  bool rows_live = false;       // the last QEq call ran its loop in row order: r_type, r_n10, r_hst, r_gst hold that call's rows (the placement search times the pass in the form that runs)
  int *r_type = nullptr, *r_n10 = nullptr, *r_xpos = nullptr, *rpos = nullptr, *g_rrow = nullptr;   // per row: type (0 = not a row), row length, cell-sorted position; per atom: its row; per ghost: the row of its owner
  int win_groups = 0, win_maxunits = 0;
  // upper bound of the window groups of n rows: a group holds WIN_ROWS rows of ONE cell column (x, y) of the grid, every column may end in a short group
  size_t win_groups_bound(long long n) const { return win_groups_bound_for(grid, n); }
  static size_t win_groups_bound_for(const Grid &g, long long n) { return static_cast<size_t>(n) / WIN_ROWS + static_cast<size_t>(g.n[0]) * g.n[1] + 1; }
  double qeq_iters_smooth = -1.0;               // running mean of the CG iterations per QEq call (the exit test of qeq.F90:114-115 lets single calls stop after two or three)
  bool win_valid = false, win_used = false;    // win_used: the last matrix pass was a window pass
  // Layout of the per-entry streams of the 10 A list (nb10, hess, hess32, sl10, hsc) of the current build: row r of the streams belongs to the resident at
  // PLACE r of rows_sorted (group * WIN_ROWS + wavefront of the window pass) instead of to atom r -- a window kernel then knows the address of its row's
  // streams from its group number alone and requests them before it has read rows_sorted.  Decided by the sweep itself from the words of its build
  // (k_list10: no window overflow, places <= place_cap, row stride >= WIN_BP_MIN_STRIDE) and repeated by the host from the same words; every reader that has the atom translates through
  // rpos (stream_rpos(): nullptr = atom layout).  The places of a short last group are never written: readers mask them by the row length.
  bool streams_by_place = false;
  int stream_place_cap() const;                // rows10 with RXMD_STREAMS_BY_PLACE on, 0 (atom layout) otherwise
  const int *stream_rpos() const { return streams_by_place ? rpos : nullptr; }
  void halo_refresh(double2 *v2, double *v1);       // QCOPY1/QCOPY2: ghosts <- owners (self exchange, resolved roots)
  void halo_staged(double *v, int ncomp);           // the same through the six-stage exchange (multi-rank)
  // The six exchange stages are walked in rounds (exchange.hip): a round is one stage, or the + and - stage of an axis together.  Ghost build and
  // migration pair when stage_pairs is set; vector halos and the force fold, whose receive counts are known, also need a transport that takes them.
  struct Round { int d0, n; };                      // stages d0 .. d0 + n - 1, n = 1 or 2
  bool stage_pairs = true;                          // RXMD_NO_STAGE_PAIRS=1: one round per stage as the reference does (six per walk)
  bool known_counts_pair() const { return stage_pairs && (nccl || (has_comm && comm.exchange_known)); }
  int *flags2 = nullptr, *scanout2 = nullptr;       // selection of the second stage of a round (flags / scanout: the first)
  int *sel_flags(int k) const { return k ? flags2 : flags; }
  int *sel_scan(int k) const { return k ? scanout2 : scanout; }
  int stage_sends(int d) const { return sendoff[d + 1] - sendoff[d]; }     // atoms stage d sends / ghosts it received, as the last ghost build left them
  int stage_ghosts(int d) const { return copyptr[d] - copyptr[d - 1]; }
  void select_round(Round r, int nscan, double dr, int skip_dead, int total[2]);   // flags, scans and totals of the round's stages, one host wait
  void exchange_round(Round r, bool reverse, const long long nsend[2], long long nrecv[2], bool counts_known);   // the send_recv of comm.F90:291-364 for every message of the round
  void rccl_exchange_round(int n, const int to[2], const int from[2], const long long nsend[2], long long nrecv[2], bool counts_known);
  // Direct vector halo (RXMD_HALO_DIRECT=1): every ghost value comes straight from the rank that OWNS the atom, all peers in one grouped
  // exchange, instead of the reference's x -> y -> z forwarding (comm.F90:68-86: three dependent rounds per halo).  The ghost build carries
  // (owner rank, owner's local index) along with every atom; after it each rank asks its ghosts' owners for their index lists once.
  long long *gowner = nullptr;                      // per atom: owner's local index * 1024 + owner rank
  bool halo_direct = false, dh_ready = false;
  int *dh_ghost = nullptr, *dh_serve = nullptr;     // ghost indices grouped by owner rank ; my residents grouped by the rank that asked for them
  int *dh_keys = nullptr, *dh_keys2 = nullptr, *dh_vals = nullptr, *dh_off = nullptr; int dh_serve_cap = 0;
  std::vector<long long> dh_need_off, dh_serve_off; // prefix offsets per rank (atoms)
  void direct_halo_setup();
  void halo_direct_exchange(double *v, int ncomp);
  void exchange_many(const std::vector<long long> &soff, const std::vector<long long> &roff, int ncomp);   // segment p of xbuf_send -> rank p, segment p of xbuf_recv <- rank p
  void rccl_exchange_many(const std::vector<long long> &soff, const std::vector<long long> &roff, int ncomp);
  void ensure_xbuf(size_t doubles);
  size_t migrate_xbuf_doubles(size_t from_send_count) const;
  void grow_xbuf_keep_send(size_t need, size_t keep);
  bool multi() const { return nprocs > 1 || force_staged; }
  // native RCCL transport (rccl_comm.hip); force_staged / force_remote (env RXMD_FORCE_STAGED / RXMD_FORCE_REMOTE) push a
  // single rank through the staged exchange and through RCCL self send/recv: how the multi-GPU code path runs on ONE GPU in the tests
  void *nccl = nullptr; double *cnt_dev = nullptr, *cnt_host = nullptr; bool force_staged = false, force_remote = false;
  void rccl_init(const unsigned char id128[128], int rank, int world);
  void rccl_destroy();
  void rccl_allreduce_dev(double *dev, int n);
  // every host wait of the engine.  With a RCCL communicator attached a wait can depend on a peer that died or went another way (a
  // rank-local overflow, a mismatch of the exchange pattern): the wait is then a bounded poll -- RXMD_COMM_TIMEOUT_S seconds, default
  // 300 -- that aborts the communicator and throws RXMD_E_COMM instead of hanging the job.
  void sync_stream();
  void sync_event(hipEvent_t e);
  double comm_timeout_s = 300.0;
  bool spin_wait = true;
  void allreduce_scal4(int n = 4);                 // MPI_ALLREDUCE of scal[S_RAW0..n-1] (qeq.hip)
  void allreduce_host(double *buf, int n);         // the same for a host vector (setup paths)
  // MPI_ALLREDUCE(SUM) of the n doubles at the device address dev, in place: with RCCL in stream order, otherwise through the host callback and the
  // pinned slot h_scal + h_stage (one host wait); timed into ms_allreduce, as sampled site `site` when >= 0 (engine.hip)
  void allreduce_device(double *dev, int n, int h_stage, int site = -1);
  void ghost_build_staged();                        // stage by stage: several ranks, or one rank under RXMD_NO_STAGE_PAIRS=1
  void sorted_copy(const double2 *v);               // QCOPY1/QCOPY2 fused with the cell-sorted gather copy -> xs
  void fold_ghost_forces(double *fx, double *fy, double *fz);   // CPBK of a per-atom vector given by component (FORCE: frc)
  void bond_orders();
  void bonded_energies();                           // Ebond + Elnpr, then the three below (bonded.hip)
  void valence_angles();                            // angles.hip
  void torsions();                                  // torsions.hip
  void hydrogen_bonds();                            // hbonds.hip
  void charge_halo();
  void nonbonded(bool to_fnb = false, bool energy = true);
  void pqeq_sorted_shells();      // ghost shells <- owners, cell-sorted copy (MODE_COPY payload of spos, comm.F90:129-131)
  void pqeq_update_shells();      // update_shell_positions, pqeq.F90:184-259
  bool pq_matrix_stale = false;   // PQEq: the shells have moved (end of a PQEq call) since the 10 A list formed its shell-core values and field term from them
  void nonbonded_pqeq();          // ENbond_PQEq, pot.F90:784-923
  void efield_force();            // EEfield, module.F90:359-383
  void remove_momentum();         // LinearMomentum, main.F90:766-797
  void type_sums_device();        // per-type count / KE / momentum / mass of the residents, all ranks, left in tsum (assemble.hip)
  double *tsum = nullptr; struct ScaleArgs *sargs = nullptr;   // 6 x 16 per-type sums ; the factors of a velocity-scaling action (device memory)
  void assemble_forces();
  void accumulate_stress(bool kinetic);   // astr(1:6) on the device (scal + SCAL_ASTR)
  void check_device_error(const char *where, bool fetch = true);
  void fetch_device_error();      // the error word and the counts that ride with it -> h_err (one host wait), nothing thrown
  double reduce_partials(int ncomp, int nblocks, double *out);  // host-side helper
  // Event pairs around single launches / exchanges, from a small pool; a finished pair is read back the next time the host has synchronised
  // with a stream anyway (collect_timers: only pairs whose end event has completed -- an exchange on the second stream may still be running),
  // so timing costs no host wait.  A pair adds its milliseconds to up to two rxmd_stats fields.
  struct KtPair { hipEvent_t a = nullptr, b = nullptr; double *dst = nullptr, *dst2 = nullptr; long long *cnt = nullptr; double scale = 1.0; };
  std::vector<KtPair> kt_free, kt_pending;
  KtPair kt_cur{};                                 // the pair of the open Timed (one nesting level is enough: a Timed inside an open one times nothing)
  // site >= 0: a timer that fires in EVERY CG iteration (the all-reduces, the vector halo and the join behind it on several ranks): an event pair between two
  // dependent operations costs the chain ~7 us per event (profiles/r06_ab_pass_events.txt), four pairs per iteration were ~50 us of every iteration of the
  // multi-rank loop.  Such a site is timed on every n-th call only (opt.pass_timing_every) and its milliseconds count n-fold; its calls are all counted.
  unsigned long long kt_site_calls[4] = {0, 0, 0, 0};
  int kt_every = 1, kt_phase = 0;                  // Engine::step: section / kernel timers on every kt_every-th step of a long call, milliseconds counted kt_every-fold
  // The scope of one pair: the start event where it is constructed, the end event on the stream current where it ends -- end(), or its destructor on the
  // way out of the block, by return or by exception -- so that no error path keeps a pair from the pool or leaves kt_cur set.  section: a scope that
  // CONTAINS Timed scopes (a whole QEq call, a whole FORCE, the list build); timed on every step: the iteration count differs from step to step.
  struct Timed {
    Engine &e; const bool section; KtPair p{};
    Timed(Engine *eng, double *dst, double *dst2 = nullptr, long long *cnt = nullptr, int site = -1, bool section_ = false) : e(*eng), section(section_) {
      double scale = 1.0;
      if (!section && site < 0 && e.kt_every > 1) {
        if (cnt) { *cnt += 1; cnt = nullptr; }
        if (e.kt_phase % e.kt_every != 0) return;
        scale = static_cast<double>(e.kt_every);
      }
      if (site >= 0) {
        if (cnt) { *cnt += 1; cnt = nullptr; }
        const unsigned long long every = static_cast<unsigned long long>(e.opt.pass_timing_every > 1 ? e.opt.pass_timing_every : 1);
        if ((e.kt_site_calls[site & 3]++ % every) != 0) return;
        scale = static_cast<double>(every);
      }
      if (e.kt_free.empty() || (!section && e.kt_cur.a)) { if (e.kt_free.empty()) ++e.st.timer_pairs_dropped; return; }
      p = e.kt_free.back(); e.kt_free.pop_back();
      p.dst = dst; p.dst2 = dst2; p.cnt = cnt; p.scale = scale;
      hipEventRecord(p.a, e.stream);
      if (!section) e.kt_cur = p;
    }
    void end() { if (!p.a) return; hipEventRecord(p.b, e.stream); e.kt_pending.push_back(p); p = KtPair{}; if (!section) e.kt_cur = KtPair{}; }
    ~Timed() { end(); }
    Timed(const Timed &) = delete;
  };
  struct TimedSection : Timed { TimedSection(Engine *eng, double *dst) : Timed(eng, dst, nullptr, nullptr, -1, true) {} };
  void collect_timers();          // after a stream synchronisation
  void tic(int k) { hipEventRecord(ev[k], stream); }
  double toc(int k0, int k1) { hipEventRecord(ev[k1], stream); hipEventSynchronize(ev[k1]); float ms = 0; hipEventElapsedTime(&ms, ev[k0], ev[k1]); return ms; }
};

// 10 A list entry: bits 0-25 cell-sorted position of the partner, 26-29 its atom type, 30 ghost, 31 periodic self image
constexpr int NB10_IDX_BITS = 26;
constexpr unsigned NB10_IDX_MASK = (1u << NB10_IDX_BITS) - 1u;
constexpr unsigned NB10_GHOST = 1u << 30, NB10_SELF = 1u << 31;

// n10[row] = entries of the row; bit 30: the row has a ghost partner (a boundary row of the domain).  The matrix pass needs the sums over
// ghost columns only there (74 % of the rows of a 979,776-atom domain have none) and reads the flag with the length it needs anyway.
constexpr int N10_GHOST_ROW = 1 << 30, N10_COUNT = N10_GHOST_ROW - 1;

// the pinned block h_err in ints, and the slots of its second half h_cnt = h_err + H_ERR_WORDS: the selection totals of the one or two stages of an
// exchange round (the first also takes the count of the atoms that stay, in front of the compaction of migrate(): never while a round is selected), and
// the total of an export's exclusive sum (exclusive_sum_total: an int or a long long, 8 bytes at an 8-byte boundary)
constexpr int H_ERR_WORDS = 16, H_ERR_INTS = 32;
enum { H_CNT_ROUND0 = 0, H_CNT_ROUND1 = 1, H_CNT_EXPORT = 4 };
static_assert(H_CNT_ROUND1 < H_CNT_EXPORT && H_CNT_EXPORT % 2 == 0 && H_ERR_WORDS % 2 == 0 && H_ERR_WORDS + H_CNT_EXPORT + 2 <= H_ERR_INTS, "the export total is 8 aligned bytes inside the pinned block, clear of the round counts");

// device error codes written by kernels into Engine::d_err
enum { DERR_NONE = 0, DERR_MAXNB = 1, DERR_MAXN10 = 2, DERR_GRID = 3, DERR_NBRINDX = 4, DERR_TYPE = 5 };

}  // namespace rxmd
