// engine.hip -- construction, device memory, atom I/O, cell binning, the lattice.  The exchange (COPYATOMS) is exchange.hip.
// Reference behaviour restated MI355X-first: src/main.F90:277-318 (LINKEDLIST), src/init.F90:7-288 (INITSYSTEM derived quantities).
#include "engine.h"
#include <cstdlib>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rxmd {

static const double UTIME = 1e3 / 20.455;  // reference src/module.F90:202
static const int NMINCELL = 4;             // reference src/module.F90:84

static void make_box(Box &b, const double lat[6], const int vprocs[3], const int vID[3]) {
  // GetBoxParams (reference src/init.F90:610-633)
  const double pi = std::atan(1.0) * 4.0;
  const double la = lat[0], lb = lat[1], lc = lat[2];
  const double lal = lat[3] * pi / 180.0, lbe = lat[4] * pi / 180.0, lga = lat[5] * pi / 180.0;
  const double hh1 = lc * (std::cos(lal) - std::cos(lbe) * std::cos(lga)) / std::sin(lga);
  const double hh2 = lc * std::sqrt(1.0 - std::cos(lal) * std::cos(lal) - std::cos(lbe) * std::cos(lbe) - std::cos(lga) * std::cos(lga) +
                                    2 * std::cos(lal) * std::cos(lbe) * std::cos(lga)) / std::sin(lga);
  double(*H)[3] = b.H;
  H[0][0] = la; H[1][0] = 0; H[2][0] = 0;
  H[0][1] = lb * std::cos(lga); H[1][1] = lb * std::sin(lga); H[2][1] = 0;
  H[0][2] = lc * std::cos(lbe); H[1][2] = hh1; H[2][2] = hh2;
  double(*m)[3] = b.Hi;  // matinv (src/main.F90:557-579)
  m[0][0] = H[1][1] * H[2][2] - H[1][2] * H[2][1]; m[0][1] = H[0][2] * H[2][1] - H[0][1] * H[2][2]; m[0][2] = H[0][1] * H[1][2] - H[0][2] * H[1][1];
  m[1][0] = H[1][2] * H[2][0] - H[1][0] * H[2][2]; m[1][1] = H[0][0] * H[2][2] - H[0][2] * H[2][0]; m[1][2] = H[0][2] * H[1][0] - H[0][0] * H[1][2];
  m[2][0] = H[1][0] * H[2][1] - H[1][1] * H[2][0]; m[2][1] = H[0][1] * H[2][0] - H[0][0] * H[2][1]; m[2][2] = H[0][0] * H[1][1] - H[0][1] * H[1][0];
  const double det = H[0][0] * H[1][1] * H[2][2] + H[0][1] * H[1][2] * H[2][0] + H[0][2] * H[1][0] * H[2][1] -
                     H[0][2] * H[1][1] * H[2][0] - H[0][1] * H[1][0] * H[2][2] - H[0][0] * H[1][2] * H[2][1];
  for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) m[a][c] = m[a][c] / det;
  b.volume = det;
  for (int a = 0; a < 6; ++a) b.lat[a] = lat[a];
  for (int a = 0; a < 3; ++a) { b.lbox[a] = 1.0 / vprocs[a]; b.obox[a] = b.lbox[a] * vID[a]; }
}

// a box the H matrix of GetBoxParams (init.F90:610-633) can describe: positive edges, angles inside (0,180), nonzero volume (NaN fails every test)
static bool lattice_spans_box(const double *L) {
  const double d2r = std::atan(1.0) / 45.0;
  const double ca = std::cos(L[3] * d2r), cb = std::cos(L[4] * d2r), cg = std::cos(L[5] * d2r);
  const double v2 = 1.0 - ca * ca - cb * cb - cg * cg + 2.0 * ca * cb * cg;
  bool ok = L[0] > 0.0 && L[1] > 0.0 && L[2] > 0.0 && v2 > 1e-12;
  for (int a = 3; a < 6; ++a) ok = ok && L[a] > 0.0 && L[a] < 180.0;
  return ok;
}
static bool lattice_orthorhombic(const double *L) { return std::fabs(L[3] - 90.0) < 1e-9 && std::fabs(L[4] - 90.0) < 1e-9 && std::fabs(L[5] - 90.0) < 1e-9; }   // (the test of grid.ortho)

Engine::Engine(const rxmd_config &c) : cfg(c) {
  declare_buffers();
  if (!c.ffield_path) throw EngineError(RXMD_E_ARG, "ffield_path is NULL");
  ffield_path = c.ffield_path;
  cfg.ffield_path = ffield_path.c_str();
  for (int a = 0; a < 3; ++a) if (cfg.vprocs[a] < 1) throw EngineError(RXMD_E_ARG, "vprocs must be >= 1");
  nprocs = cfg.vprocs[0] * cfg.vprocs[1] * cfg.vprocs[2];
  if (cfg.myid < 0 || cfg.myid >= nprocs) throw EngineError(RXMD_E_ARG, "myid outside the vprocs grid");
  if (!lattice_spans_box(cfg.lattice)) throw EngineError(RXMD_E_ARG, "lattice does not span a box (edges must be positive, angles inside (0,180) and not coplanar)");
  try { ff.parse(ffield_path, cfg.lg != 0); } catch (const std::exception &e) { throw EngineError(RXMD_E_FFIELD, e.what()); }
  // rank grid, reference src/init.F90:74-100
  vID[0] = cfg.myid % cfg.vprocs[0]; vID[1] = (cfg.myid / cfg.vprocs[0]) % cfg.vprocs[1]; vID[2] = cfg.myid / (cfg.vprocs[0] * cfg.vprocs[1]);
  int k = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = 1; j >= -1; j -= 2) {
      int l[3] = {vID[0], vID[1], vID[2]};
      l[i] = (vID[i] + j + cfg.vprocs[i]) % cfg.vprocs[i];
      target_node[++k] = l[0] + l[1] * cfg.vprocs[0] + l[2] * cfg.vprocs[0] * cfg.vprocs[1];
    }
  make_box(box, cfg.lattice, cfg.vprocs, vID);
  dt = cfg.dt_fs / UTIME;                         // init.F90:66
  Lex_w2 = 2.0 * cfg.Lex_k / dt / dt;             // init.F90:69
  dthm.assign(ff.nso + 1, 0.0); hmas.assign(ff.nso + 1, 0.0);
  for (int t = 1; t <= ff.nso; ++t) { dthm[t] = dt * 0.5 / ff.atom[t].mass; hmas[t] = 0.5 * ff.atom[t].mass; }  // init.F90:105-108
  if (cfg.pqeq_path && cfg.pqeq_path[0]) {          // --pqeq: chi/eta replaced, taper cutoff 12.5 A (init.F90:28-43, module.F90:282)
    pqeq_path = cfg.pqeq_path; cfg.pqeq_path = pqeq_path.c_str();
    try { ff.parse_pqeq(pqeq_path); } catch (const std::exception &e) { throw EngineError(RXMD_E_FFIELD, e.what()); }
    ff.build_taper(12.5);
  } else {
    cfg.pqeq_path = nullptr;
    ff.build_taper(10.0);                         // rctap0, module.F90:281
  }
  if (cfg.efield_dir != 0 && (!ff.pqeq || cfg.efield_dir < 1 || cfg.efield_dir > 3))
    throw EngineError(RXMD_E_ARG, "efield needs a PQEq parameter file (core charges Z) and a direction 1..3");
  stage_pairs = !opt.no_stage_pairs;
  force_staged = opt.force_staged; force_remote = opt.force_remote;
  spin_wait = opt.spin_wait != 0;
  halo_direct = opt.halo_direct;
  comm_timeout_s = opt.comm_timeout_s;
  if (opt.qeq_f32 != 0 && !ff.pqeq) qeq_bits_req = 32;      // (RXMD_QEQ_F32=1; PQEq carries a second value stream and stays at 64)
  MAXNB = cfg.maxneighbs > 0 ? cfg.maxneighbs : 30;
  if (MAXNB > 31) throw EngineError(RXMD_E_ARG, "maxneighbs must be <= 31 (the wavefront-per-centre kernels stage the bond slots of two atoms in one 64-lane wavefront; the reference uses 30)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw EngineError(RXMD_E_HIP, "no HIP device visible: this engine has no CPU path");
  RX_HIP(hipSetDevice(cfg.device));
  { hipDeviceProp_t pr; RX_HIP(hipGetDeviceProperties(&pr, cfg.device)); num_cu = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    // the angle kernel and the window kernels ask for up to 78 KB of LDS per workgroup (gfx950: 160 KB per CU, 64 KB on every earlier arch): a
    // device that cannot give it is refused here -- a launch that fails later would leave energy terms out without a word
    if (pr.sharedMemPerBlock < size_t(80) * 1024) throw EngineError(RXMD_E_HIP, "device " + std::to_string(cfg.device) + " offers " + std::to_string(pr.sharedMemPerBlock) + " bytes of LDS per workgroup; the kernels are written for gfx950 (MI355X, 160 KB per CU) and need 80 KB"); }
  RX_HIP(hipStreamCreate(&stream));
  for (int k = 0; k < 64; ++k) { KtPair p; RX_HIP(hipEventCreate(&p.a)); RX_HIP(hipEventCreate(&p.b)); kt_free.push_back(p); }
  if (opt.single_stream) comm_stream = stream;   // diagnostic: the halo work queues on the main stream (no second hardware queue)
  else {                                         // highest priority: pack / send-recv / unpack kernels of a halo go ahead of the queued compute workgroups
    int lo = 0, hi = 0;
    RX_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    RX_HIP(hipStreamCreateWithPriority(&comm_stream, hipStreamDefault, hi));
  }
  if (!opt.single_stream && !opt.no_bond_overlap && opt.bond_overlap != 0) {   // the charge-free part of FORCE next to ENbond (engine.h: bond_stream); lowest priority.  Opt-in since round 6: with the torsion kernel at 2 ms it buys nothing any more (profiles/r06_ab_bond_overlap_after_e4b.txt)
    int lo = 0, hi = 0;
    RX_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    RX_HIP(hipStreamCreateWithPriority(&bond_stream, hipStreamDefault, lo));
  }
  RX_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming)); RX_HIP(hipEventCreateWithFlags(&ev_bond, hipEventDisableTiming));
  RX_HIP(hipEventCreateWithFlags(&ev_main, hipEventDisableTiming)); RX_HIP(hipEventCreateWithFlags(&ev_comm, hipEventDisableTiming));
  RX_HIP(hipEventCreateWithFlags(&ev_est, hipEventDisableTiming));
  for (auto &pr : ev_pass) for (auto &e2 : pr) RX_HIP(hipEventCreate(&e2));
  for (auto &e : ev) RX_HIP(hipEventCreate(&e));
}

Engine::~Engine() {
  rccl_destroy();
  free_device();
  for (auto &e : ev) if (e) (void)hipEventDestroy(e);
  for (auto *v : {&kt_free, &kt_pending}) for (auto &p : *v) { if (p.a) (void)hipEventDestroy(p.a); if (p.b) (void)hipEventDestroy(p.b); }
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  if (ev_bond) (void)hipEventDestroy(ev_bond);
  if (bond_stream) (void)hipStreamDestroy(bond_stream);
  if (ev_main) (void)hipEventDestroy(ev_main);
  if (ev_comm) (void)hipEventDestroy(ev_comm);
  if (ev_est) (void)hipEventDestroy(ev_est);
  if (ev_io_in) (void)hipEventDestroy(ev_io_in);
  if (ev_io_out) (void)hipEventDestroy(ev_io_out);
  for (auto &pr : ev_pass) for (auto &e2 : pr) if (e2) (void)hipEventDestroy(e2);
  if (comm_stream && comm_stream != stream) (void)hipStreamDestroy(comm_stream);
  if (stream) (void)hipStreamDestroy(stream);
}

void Engine::allreduce_host(double *buf, int n) {
  if (nccl) {
    double *own = nullptr, *d = scal + SCAL_REDUCE;   // the usual case, a scalar or two: this slot of the device scalar block is the staging area
    if (n > 8) { dev_alloc(own, n, Fill::None); d = own; }
    RX_HIP(hipMemcpyAsync(d, buf, sizeof(double) * n, hipMemcpyHostToDevice, stream));
    rccl_allreduce_dev(d, n);
    RX_HIP(hipMemcpyAsync(buf, d, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    sync_stream();
    dev_free(own);
    return;
  }
  if (!has_comm || !comm.allreduce_sum) throw EngineError(RXMD_E_COMM, "vprocs > 1 needs a transport: call rxmd_hip_set_comm or rxmd_hip_comm_init_rccl first");
  if (comm.allreduce_sum(comm.ctx, buf, n)) throw EngineError(RXMD_E_COMM, "allreduce callback failed");
}

void Engine::allreduce_device(double *dev, int n, int h_stage, int site) {
  Timed kt(this, &st.ms_allreduce, nullptr, &st.allreduce_calls, site);
  if (nccl) { rccl_allreduce_dev(dev, n); return; }                // in stream order, no host round trip
  if (!has_comm || !comm.allreduce_sum) throw EngineError(RXMD_E_COMM, "vprocs > 1 needs a transport: call rxmd_hip_set_comm or rxmd_hip_comm_init_rccl first");
  double *h = h_scal + h_stage;                                    // a host transport (MPI callbacks): its all-reduce IS a host call
  RX_HIP(hipMemcpyAsync(h, dev, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
  sync_stream();
  if (comm.allreduce_sum(comm.ctx, h, n)) throw EngineError(RXMD_E_COMM, "allreduce callback failed");
  RX_HIP(hipMemcpyAsync(dev, h, sizeof(double) * n, hipMemcpyHostToDevice, stream));
}

void Engine::collect_timers() {
  size_t keep = 0;
  for (size_t i = 0; i < kt_pending.size(); ++i) {
    KtPair p = kt_pending[i];
    float ms = 0;
    if (hipEventQuery(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      if (p.dst) *p.dst += ms * p.scale;
      if (p.dst2) *p.dst2 += ms * p.scale;
      if (p.cnt) *p.cnt += 1;
      p.dst = p.dst2 = nullptr; p.cnt = nullptr;
      kt_free.push_back(p);
    } else kt_pending[keep++] = p;
  }
  kt_pending.resize(keep);
}

void Engine::fetch_device_error() {
  RX_HIP(hipMemcpyAsync(h_err, d_err, sizeof(int) * 16, hipMemcpyDeviceToHost, stream));
  sync_stream();
}
void Engine::check_device_error(const char *where, bool fetch) {
  if (fetch) fetch_device_error();
  const int e = h_err[0];
  if (e == DERR_NONE) return;
  RX_HIP(hipMemsetAsync(d_err, 0, sizeof(int) * 2, stream));   // [2] (longest bond list of the build) stays: a retry rebuilds the 10 A list only
  const std::string w = std::string(where) + ": ";
  if (e == DERR_MAXNB) throw EngineError(RXMD_E_MAXNEIGHBS, w + "overflow of max # in neighbor list (MAXNEIGHBS=" + std::to_string(MAXNB) + ", needed " + std::to_string(h_err[1]) + ")");
  if (e == DERR_MAXN10) throw EngineError(RXMD_E_MAXNEIGHBS10, w + "nbplist greater than MAXNEIGHBS10=" + std::to_string(S10) + " (needed " + std::to_string(h_err[1]) + ")");
  if (e == DERR_NBRINDX) throw EngineError(RXMD_E_STATE, w + "inconsistency between nbrlist and nbrindx");
  if (e == DERR_TYPE) throw EngineError(RXMD_E_ARG, w + "atom type outside the ffield");
  throw EngineError(RXMD_E_STATE, w + "device error " + std::to_string(e));
}

// ---------------------------------------------------------------------------------------------
// derived quantities that need the atoms (INITSYSTEM after ReadBIN, init.F90:141-213)
void Engine::setup_after_atoms(const std::vector<long long> &npt) {
  if (ff.pqeq)
    for (int t = ff.npq + 1; t <= ff.nso; ++t)
      if (npt[t] > 0) throw EngineError(RXMD_E_FFIELD, "PQEq: atoms of ffield type " + std::to_string(t) + " (" + ff.atom[t].name + ") have no row in the PQEq parameter file");
  ff.compute_cutoffs(npt);
  ff.build_tables();
  if (ff.pqeq) ff.build_pqeq_tables();
  derive_box_geometry();
  tables_ready = true;
}

// the half of the set-up that depends on the lattice (UpdateBoxParams, init.F90:641-667, and the engine's own grid) for box `box`: set-up and
// set_lattice (which computes it for the new box before it changes anything)
Engine::BoxGeom Engine::geometry_for(const Box &box) const {
  BoxGeom g;
  int *cc = g.cc; double *shell = g.shell; Grid &grid = g.grid; RefMesh &rmesh = g.rmesh;
  grid = this->grid;                               // (fields the lattice does not decide, such as the probe switch, stay)
  const double lreal[3] = {box.lat[0] / cfg.vprocs[0], box.lat[1] / cfg.vprocs[1], box.lat[2] / cfg.vprocs[2]};
  for (int a = 0; a < 3; ++a) {
    cc[a] = static_cast<int>(lreal[a] / ff.maxrc);            // UpdateBoxParams, init.F90:656
    if (cc[a] < 1) throw EngineError(RXMD_E_ARG, "local box smaller than the bond cutoff");
    shell[a] = NMINCELL * (box.lbox[a] / cc[a]);               // dr of the FORCE ghost copy, pot.F90:28
  }
  // the engine's own grid: one cell >= max(rctap/2, maxrc) wide, measured PERPENDICULAR to its faces (the planes of constant normalised
  // coordinate a are 1 / |row a of Hi| apart per unit; with 90-degree angles that is the lattice constant); stencil +-2 covers the taper
  // cutoff, +-1 the bonds
  const double cw = std::max(0.5 * ff.rctap, ff.maxrc) * (1.0 + 1e-9);
  grid.ortho = (std::fabs(box.lat[3] - 90.0) < 1e-9 && std::fabs(box.lat[4] - 90.0) < 1e-9 && std::fabs(box.lat[5] - 90.0) < 1e-9) ? 1 : 0;
  grid.ncell = 1;
  for (int a = 0; a < 3; ++a) {
    grid.wid[a] = grid.ortho ? box.lat[a] : 1.0 / std::sqrt(box.Hi[a][0] * box.Hi[a][0] + box.Hi[a][1] * box.Hi[a][1] + box.Hi[a][2] * box.Hi[a][2]);
    const double wn = box.lbox[a] + 2.0 * shell[a];
    const double wreal = wn * grid.wid[a];
    grid.n[a] = std::max(1, static_cast<int>(wreal / cw));
    grid.org[a] = -shell[a];
    grid.inv[a] = grid.n[a] / wn;
    grid.ncell *= grid.n[a];
    grid.cw[a] = 1.0 / grid.inv[a];
  }
  grid.iwz = 1.0 / grid.wid[2];
  // the reference's meshes (RefMesh, engine.h)
  for (int a = 0; a < 3; ++a) {
    for (int c = 0; c < 3; ++c) rmesh.Hi[3 * a + c] = box.Hi[a][c];
    rmesh.obox[a] = box.obox[a];
    rmesh.lc[a] = box.lbox[a] / cc[a];                          // lcsize, init.F90:661
    const int nbcc = std::max(1, static_cast<int>(lreal[a] / 3.0));   // nblcsize = 3 A initial estimate, init.F90:538-545
    rmesh.nblr[a] = lreal[a] / nbcc;
    rmesh.nbl[a] = rmesh.nblr[a] / box.lat[a];                  // init.F90:605
    rmesh.qlo[a] = -ff.rctap / box.lat[a];                      // QCopyDr, qeq.F90:32
    rmesh.qhi[a] = box.lbox[a] + ff.rctap / box.lat[a];
  }
  // z-slices per cell: ~1/8 of a cell (0.6 A at the 5 A cell of a 10 A cutoff); bounded so that the slice ids fit the 31-bit sort key
  grid.fz = 8;
  while (grid.fz > 1 && static_cast<long long>(grid.ncell) * grid.fz > (1LL << 28)) grid.fz >>= 1;
  grid.nzf = grid.n[2] * grid.fz;
  grid.nfine = grid.n[0] * grid.n[1] * grid.nzf;
  return g;
}
void Engine::derive_box_geometry() {
  const BoxGeom g = geometry_for(box);
  for (int a = 0; a < 3; ++a) { cc[a] = g.cc[a]; shell[a] = g.shell[a]; }
  grid = g.grid; rmesh = g.rmesh;
}

void Engine::upload_ff() {
  // one blob: atom | bond | angle | tors | hb | inxn2 | inxn3 | inxn3hb | inxn4 | tabNB | tabQEq
  const int n1 = ff.n1();
  std::vector<DevAtomP> a(ff.nso + 1);
  for (int t = 1; t <= ff.nso; ++t) {
    const auto &s = ff.atom[t];
    a[t] = {s.Val, s.Valboc, s.mass, s.Vale, s.nlpopt, s.plp2, s.povun2, s.povun5, s.pval3, s.pval5, s.Valangle, s.Valval, s.chi, s.eta};
  }
  std::vector<DevBondP> b(ff.nboty + 1);
  for (int r = 1; r <= ff.nboty; ++r) {
    const auto &s = ff.bond[r];
    b[r] = {s.Desig, s.Depi, s.Depipi, s.pbe1, s.pbe2, s.povun1, s.ovc, s.v13cor, s.pbo2, s.pbo4, s.pbo6, s.pboc3, s.pboc4, s.pboc5,
            s.cBOp1, s.cBOp3, s.cBOp5, s.pbo2h, s.pbo4h, s.pbo6h, s.sw[0], s.sw[1], s.sw[2], s.rc2};
  }
  std::vector<DevAngleP> an(ff.nvaty + 1);
  for (int r = 1; r <= ff.nvaty; ++r) { const auto &s = ff.angle[r]; an[r] = {s.theta00, s.pval1, s.pval2, s.pcoa1, s.pval7, s.ppen1, s.pval4}; }
  std::vector<DevTorsP> to(ff.ntoty + 1);
  for (int r = 1; r <= ff.ntoty; ++r) { const auto &s = ff.tors[r]; to[r] = {s.V1, s.V2, s.V3, s.ptor1, s.pcot1}; }
  std::vector<DevHbP> hb(ff.nhbty + 1);
  for (int r = 1; r <= ff.nhbty; ++r) { const auto &s = ff.hb[r]; hb[r] = {s.r0hb, s.phb1, s.phb2, s.phb3}; }
  const size_t stride = NTABLE + 2;
  std::vector<DevNBTab> nb((ff.nboty + 1) * stride);
  for (size_t i = 0; i + 1 < nb.size(); ++i)
    nb[i] = {ff.tblEvdw[i], ff.tblEvdw[i + 1] - ff.tblEvdw[i], ff.tbldEvdw[i], ff.tbldEvdw[i + 1] - ff.tbldEvdw[i],
             ff.tblEclmb[i], ff.tblEclmb[i + 1] - ff.tblEclmb[i], ff.tbldEclmb[i], ff.tbldEclmb[i + 1] - ff.tbldEclmb[i]};
  nb.back() = DevNBTab{};

  // PQEq tables as (E, dE, F, dF) nodes
  std::vector<double4> pt[3];
  std::vector<double> zk;
  if (ff.pqeq) {
    const std::vector<double> *T[3] = {&ff.tblPcc, &ff.tblPsc, &ff.tblPss};
    for (int k = 0; k < 3; ++k) {
      const size_t nn = T[k]->size() / 2;
      pt[k].assign(nn, make_double4(0, 0, 0, 0));
      for (size_t i = 0; i + 1 < nn; ++i)
        pt[k][i] = make_double4((*T[k])[2 * i], (*T[k])[2 * (i + 1)] - (*T[k])[2 * i], (*T[k])[2 * i + 1], (*T[k])[2 * (i + 1) + 1] - (*T[k])[2 * i + 1]);
    }
    zk.assign(2 * (ff.npq + 1), 0.0);
    for (int t = 1; t <= ff.npq; ++t) { zk[t] = ff.Zpq[t]; zk[ff.npq + 1 + t] = ff.Kspq[t]; }
  }
  // inxn4 followed by "is there a torsion row" as 4096 bits (ffields with at most 7 atom types)
  std::vector<int> inxn4x(ff.inxn4);
  inxn4x.resize(ff.inxn4.size() + 128, 0);
  if (n1 <= 8)
    for (size_t i = 0; i < ff.inxn4.size(); ++i)
      if (ff.inxn4[i] != 0) inxn4x[ff.inxn4.size() + (i >> 5)] |= static_cast<int>(1u << (i & 31));
  // the QEq table once more as pairs (T[i], T[i+1]): the interpolation of a list entry is ONE 16-byte load instead of two 8-byte gathers
  std::vector<double2> tq2(ff.tblQEq.size());
  for (size_t i = 0; i < tq2.size(); ++i) tq2[i] = make_double2(ff.tblQEq[i], i + 1 < tq2.size() ? ff.tblQEq[i + 1] : 0.0);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  size_t off[13], tot = 0;
  const size_t sz[12] = {a.size() * sizeof(DevAtomP), b.size() * sizeof(DevBondP), an.size() * sizeof(DevAngleP), to.size() * sizeof(DevTorsP),
                         hb.size() * sizeof(DevHbP), ff.inxn2.size() * 4, ff.inxn3.size() * 4, ff.inxn3hb.size() * 4, inxn4x.size() * 4,
                         nb.size() * sizeof(DevNBTab), ff.tblQEq.size() * 8, tq2.size() * sizeof(double2)};
  const void *src[12] = {a.data(), b.data(), an.data(), to.data(), hb.data(), ff.inxn2.data(), ff.inxn3.data(), ff.inxn3hb.data(), inxn4x.data(), nb.data(), ff.tblQEq.data(), tq2.data()};
  for (int i = 0; i < 12; ++i) { off[i] = tot; tot += al(sz[i]); }
  bufs.free_group(G_FFBLOB); bufs.alloc_group(*this, G_FFBLOB, tot);
  for (int i = 0; i < 12; ++i) RX_HIP(hipMemcpy(static_cast<char *>(ffblob) + off[i], src[i], sz[i], hipMemcpyHostToDevice));
  char *base = static_cast<char *>(ffblob);
  dff.nso = ff.nso; dff.n1 = n1; dff.nboty = ff.nboty; dff.ntoty = ff.ntoty; dff.nvaty = ff.nvaty;
  dff.atom = reinterpret_cast<DevAtomP *>(base + off[0]); dff.bond = reinterpret_cast<DevBondP *>(base + off[1]);
  dff.angle = reinterpret_cast<DevAngleP *>(base + off[2]); dff.tors = reinterpret_cast<DevTorsP *>(base + off[3]);
  dff.hb = reinterpret_cast<DevHbP *>(base + off[4]);
  dff.inxn2 = reinterpret_cast<int *>(base + off[5]); dff.inxn3 = reinterpret_cast<int *>(base + off[6]);
  dff.inxn3hb = reinterpret_cast<int *>(base + off[7]); dff.inxn4 = reinterpret_cast<int *>(base + off[8]);
  dff.tor_bits = reinterpret_cast<unsigned *>(base + off[8]) + ff.inxn4.size();
  dff.tabNB = reinterpret_cast<DevNBTab *>(base + off[9]); dff.tabQEq = reinterpret_cast<double *>(base + off[10]); dff.tabQEq2 = reinterpret_cast<double2 *>(base + off[11]);
  dff.rctap_pad = ff.rctap + 1e-6;
  dff.UDR = ff.UDR; dff.UDRi = ff.UDRi; dff.rctap2 = ff.rctap2; dff.cutoff_vpar30 = ff.cutoff_vpar30; dff.vpar1 = ff.vpar1; dff.vpar2 = ff.vpar2;
  dff.plp1 = ff.plp1; dff.povun3 = ff.povun3; dff.povun4 = ff.povun4; dff.povun6 = ff.povun6; dff.povun7 = ff.povun7; dff.povun8 = ff.povun8;
  dff.pval6 = ff.pval6; dff.pval8 = ff.pval8; dff.pval9 = ff.pval9; dff.pval10 = ff.pval10; dff.ppen2 = ff.ppen2; dff.ppen3 = ff.ppen3; dff.ppen4 = ff.ppen4;
  dff.pcoa2 = ff.pcoa2; dff.pcoa3 = ff.pcoa3; dff.pcoa4 = ff.pcoa4; dff.ptor2 = ff.ptor2; dff.ptor3 = ff.ptor3; dff.ptor4 = ff.ptor4; dff.pcot2 = ff.pcot2;
  dff.pqeq = ff.pqeq ? 1 : 0; dff.npq1 = ff.npq + 1;
  ehb_donor_types = 0u;                            // types X for which some hydrogen-bond row (X, 2, k) exists (hydrogen = type 2, pot.F90:595)
  if (ff.nso >= 2)
    for (int t = 1; t <= ff.nso && t < 32; ++t)
      for (int k = 1; k <= ff.nso; ++k)
        if (ff.inxn3hb[(t * n1 + 2) * n1 + k] != 0) ehb_donor_types |= 1u << t;
  if (ff.pqeq) {
    const size_t b0 = al(zk.size() * 8), b1 = al(ff.inxnpq.size() * 4), bt = al(pt[0].size() * sizeof(double4));
    bufs.free_group(G_PQBLOB); bufs.alloc_group(*this, G_PQBLOB, b0 + b1 + 3 * bt);
    char *pb = static_cast<char *>(pqblob);
    RX_HIP(hipMemcpy(pb, zk.data(), zk.size() * 8, hipMemcpyHostToDevice));
    RX_HIP(hipMemcpy(pb + b0, ff.inxnpq.data(), ff.inxnpq.size() * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 3; ++k) RX_HIP(hipMemcpy(pb + b0 + b1 + k * bt, pt[k].data(), pt[k].size() * sizeof(double4), hipMemcpyHostToDevice));
    dff.Zpq = reinterpret_cast<double *>(pb); dff.Kspq = dff.Zpq + (ff.npq + 1);
    dff.inxnpq = reinterpret_cast<int *>(pb + b0);
    dff.tabPcc = reinterpret_cast<double4 *>(pb + b0 + b1); dff.tabPsc = reinterpret_cast<double4 *>(pb + b0 + b1 + bt); dff.tabPss = reinterpret_cast<double4 *>(pb + b0 + b1 + 2 * bt);
  }
}

void Engine::alloc_device() {
  const size_t nb = NB;
  // the capacities of the groups that exist from set-up on; which buffers they size, and how, is the table's business (buffers.hip)
  cellstart_cap = static_cast<size_t>(grid.nfine) + 2;
  // 5.3 bonds per RDX atom, ~16 in SiC: 12 per atom slot to start with, grown when a build needs more (build_ghosts_and_lists).
  // RXMD_BOND_CAP=<bonds>: start smaller (the tests walk the growth path with it; a capacity, not a result)
  bcap = std::max<size_t>(opt.bond_cap > 0 ? static_cast<size_t>(opt.bond_cap) : nb * 12, 1024);
  win_ng_cap = win_groups_bound(rows10) + 1;
  ehb_don_cap = static_cast<size_t>(rows10) + EHB_DON_EXTRA;
  partials_cap = std::max<size_t>(size_t(1) << 16, 4 * static_cast<size_t>(rows10) + 16384);   // up to one workgroup (4 partial sums) per row
  bufs.cap[G_CELLSTART] = cellstart_cap; bufs.cap[G_BOND] = bcap; bufs.cap[G_WIN] = win_ng_cap; bufs.cap[G_PARTIALS] = partials_cap;
  bufs.alloc_setup(*this);
  h_cnt = h_err + H_ERR_WORDS;
  // hipcub scratch sized for the largest scan / sort we issue
  size_t b1 = 0, b2 = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, b1, flags, scanout, NB + 1, stream);
  hipcub::DeviceRadixSort::SortPairs(nullptr, b2, cellid, cellid_sorted, perm_in, perm, NB, 0, 32, stream);
  cubtmp_bytes = std::max(b1, b2) + 256;
  bufs.alloc_group(*this, G_CUBTMP, cubtmp_bytes);
}

void Engine::alloc_window_groups(size_t ng) { win_ng_cap = ng; bufs.alloc_group(*this, G_WIN, ng); }
void Engine::alloc_bond_tables(size_t cap) { bcap = std::max<size_t>(cap, 1024); bufs.alloc_group(*this, G_BOND, bcap); }
void Engine::alloc_e4b_delivery(size_t entries) {
  bufs.free_group(G_E4B);
  e4b_cap = (std::max<size_t>(entries, 1024) + 3) & ~static_cast<size_t>(3);
  bufs.alloc_group(*this, G_E4B, e4b_cap);
  e4b_dirty = false;
}
void Engine::free_bond_tables() { bufs.free_group(G_BOND); bcap = 0; }

void Engine::free_device() {
  bufs.free_all();
  bcap = 0; e4b_cap = 0; seg_blocks_cap = 0;
}

// ReadBIN (reference src/fileio.F90:528-552): records -> real coordinates, split atype
void Engine::set_atoms_rxff(int natoms, const double *rec) {
  if (natoms < 0 || (natoms == 0 && nprocs == 1)) throw EngineError(RXMD_E_ARG, "natoms must be positive");   // a rank of a decomposed box may own nothing
  std::vector<double> hx[3], hv[3], hq(natoms), hp(natoms), hw(natoms);
  std::vector<int> ht(natoms);
  std::vector<long long> hg(natoms);
  for (int a = 0; a < 3; ++a) { hx[a].resize(natoms); hv[a].resize(natoms); }
  std::vector<long long> npt(ff.nso + 2, 0);
  int n14 = 0;
  for (int i = 0; i < natoms; ++i) {
    const double *r = rec + 10 * static_cast<size_t>(i);
    const double s[3] = {r[0] + box.obox[0], r[1] + box.obox[1], r[2] + box.obox[2]};
    for (int a = 0; a < 3; ++a) { hx[a][i] = box.H[a][0] * s[0] + box.H[a][1] * s[1] + box.H[a][2] * s[2]; hv[a][i] = r[3 + a]; }  // xs2xu
    hq[i] = r[6];
    const int t = static_cast<int>(std::lround(r[7]));
    if (t < 1 || t > ff.nso) throw EngineError(RXMD_E_ARG, "atom type outside the ffield");
    ht[i] = t; hg[i] = std::llround((r[7] - t) * 1e13);                 // l2g, main.F90:582-593
    hp[i] = r[8]; hw[i] = r[9];
    npt[t]++;
    if (r[7] == (static_cast<double>(t) + static_cast<double>(hg[i]) * 1e-13) + 1e-14) ++n14;
  }
  atype_resid = (natoms > 0 && n14 == natoms) ? 1e-14 : 0.0;
  if (!tables_ready) {
    if (nprocs > 1) {
      std::vector<double> tmp(ff.nso + 1);
      for (int t = 0; t <= ff.nso; ++t) tmp[t] = static_cast<double>(npt[t]);
      allreduce_host(tmp.data(), ff.nso + 1);
      for (int t = 0; t <= ff.nso; ++t) npt[t] = std::llround(tmp[t]);
    }
    setup_after_atoms(npt);
    // capacities: sized from this rank's atoms, but never below the mean share (a sparse or empty domain can fill up by migration)
    long long ntot = 0;
    for (int t = 1; t <= ff.nso; ++t) ntot += npt[t];
    const long long nsize = std::max<long long>(natoms, ntot / nprocs);
    nsize_setup = nsize;
    NB = cfg.nbuffer > 0 ? cfg.nbuffer : static_cast<int>(capacity_want(shell));
    if (NB <= natoms) throw EngineError(RXMD_E_NBUFFER, "nbuffer smaller than natoms");
    const double vloc = box.volume / nprocs;
    const double est10 = nsize / vloc * (4.0 / 3.0) * 3.14159265358979 * ff.rctap * ff.rctap2;
    int s10 = cfg.maxneighbs10 > 0 ? cfg.maxneighbs10 : static_cast<int>(est10 * 1.35 + 64);
    if (opt.s10 > 0 && cfg.maxneighbs10 <= 0) s10 = static_cast<int>(opt.s10);   // (experiments build: row stride of the 10 A list)
    S10 = (s10 + 63) / 64 * 64;
    rows10 = std::min<long long>(NB, nsize + nsize / 8 + 1024);
    if (ff.nso > 15) throw EngineError(RXMD_E_ARG, "more than 15 atom types do not fit the packed 10 A list entry");
    if (NB >= (1 << NB10_IDX_BITS)) throw EngineError(RXMD_E_NBUFFER, "more than 2^26 atoms+ghosts per GPU do not fit the packed 10 A list entry");
    alloc_device();
    upload_ff();
    st.n10_stride = S10; st.nbuffer = NB;
    for (int a = 0; a < 3; ++a) { st.cells10[a] = grid.n[a]; st.cells3[a] = cc[a]; }
  }
  if (natoms > rows10) throw EngineError(RXMD_E_NBUFFER, "more atoms than the engine was sized for");
  N = natoms; G = natoms;
  for (int a = 0; a < 3; ++a) {
    RX_HIP(hipMemcpy(pos[a], hx[a].data(), sizeof(double) * natoms, hipMemcpyHostToDevice));
    RX_HIP(hipMemcpy(vel[a], hv[a].data(), sizeof(double) * natoms, hipMemcpyHostToDevice));
    RX_HIP(hipMemset(frc[a], 0, sizeof(double) * NB));
  }
  if (ff.pqeq) for (int a = 0; a < 3; ++a) RX_HIP(hipMemset(shl[a], 0, sizeof(double) * NB));      // spos(:,:)=0, init.F90:117-120
  RX_HIP(hipMemcpy(q, hq.data(), sizeof(double) * natoms, hipMemcpyHostToDevice));
  RX_HIP(hipMemcpy(qsfp, hp.data(), sizeof(double) * natoms, hipMemcpyHostToDevice));
  RX_HIP(hipMemcpy(qsfv, hw.data(), sizeof(double) * natoms, hipMemcpyHostToDevice));
  RX_HIP(hipMemcpy(type, ht.data(), sizeof(int) * natoms, hipMemcpyHostToDevice));
  RX_HIP(hipMemcpy(gid, hg.data(), sizeof(long long) * natoms, hipMemcpyHostToDevice));
  atoms_set = true; lists_valid = false; ghosts_valid = false;
  st.natoms = N; eval_natoms = -1;
}

// atype = type + l2g * 1e-13 (main.F90:582-593) -> type, global id; a type outside the ffield raises the device error word
__global__ void k_split_atype(int n, int nso, const double *__restrict__ atype, int *__restrict__ type, long long *__restrict__ gid, int *err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = atype[i];
  const int t = static_cast<int>(llround(a));
  if (t < 1 || t > nso) { atomicCAS(&err[0], DERR_NONE, DERR_TYPE); type[i] = 1; gid[i] = 0; return; }
  type[i] = t; gid[i] = llround((a - t) * 1e13);
}
void Engine::set_atoms_arrays(int natoms, const double *atype, const double *x, const double *y, const double *z, const double *qh, const double *lexp, const double *lexv) {
  if (!tables_ready) throw EngineError(RXMD_E_STATE, "set_atoms_arrays before the engine was sized");
  if (natoms < 0 || natoms > rows10 || natoms >= NB) throw EngineError(RXMD_E_NBUFFER, "more atoms than the engine was sized for");
  sync_stream();                                   // nothing of the previous call may still read what is overwritten
  const double *xyz[3] = {x, y, z};
  const size_t nbytes = sizeof(double) * static_cast<size_t>(natoms);
  if (natoms > 0) {
    RX_HIP(hipMemcpyAsync(cds, atype, nbytes, hipMemcpyHostToDevice, stream));     // cds: per-atom scratch of FORCE, free between calls
    k_split_atype<<<(natoms + 255) / 256, 256, 0, stream>>>(natoms, ff.nso, cds, type, gid, d_err);
    for (int a = 0; a < 3; ++a) {
      RX_HIP(hipMemcpyAsync(pos[a], xyz[a], nbytes, hipMemcpyHostToDevice, stream));
      RX_HIP(hipMemsetAsync(vel[a], 0, nbytes, stream));
    }
    if (qh) RX_HIP(hipMemcpyAsync(q, qh, nbytes, hipMemcpyHostToDevice, stream)); else RX_HIP(hipMemsetAsync(q, 0, nbytes, stream));
    if (lexp && lexv) { RX_HIP(hipMemcpyAsync(qsfp, lexp, nbytes, hipMemcpyHostToDevice, stream)); RX_HIP(hipMemcpyAsync(qsfv, lexv, nbytes, hipMemcpyHostToDevice, stream)); }
    else { RX_HIP(hipMemsetAsync(qsfp, 0, nbytes, stream)); RX_HIP(hipMemsetAsync(qsfv, 0, nbytes, stream)); }
  }
  for (int a = 0; a < 3; ++a) RX_HIP(hipMemsetAsync(frc[a], 0, sizeof(double) * NB, stream));
  if (ff.pqeq) for (int a = 0; a < 3; ++a) RX_HIP(hipMemsetAsync(shl[a], 0, sizeof(double) * NB, stream));
  N = natoms; G = natoms;
  atoms_set = true; lists_valid = false; ghosts_valid = false;
  atype_resid = 0.0;
  st.natoms = N; eval_natoms = -1;
  check_device_error("set_atoms_arrays");          // (synchronises: the caller's arrays are free again)
}

int Engine::get_atoms_rxff(double *rec, int capacity) {
  if (!atoms_set) throw EngineError(RXMD_E_STATE, "atoms were never set");
  if (!rec) return N;
  if (capacity < N) throw EngineError(RXMD_E_ARG, "capacity smaller than natoms");
  std::vector<double> hx[3], hv[3], hq(N), hp(N), hw(N);
  std::vector<int> ht(N);
  std::vector<long long> hg(N);
  sync_stream();
  for (int a = 0; a < 3; ++a) {
    hx[a].resize(N); hv[a].resize(N);
    RX_HIP(hipMemcpy(hx[a].data(), pos[a], sizeof(double) * N, hipMemcpyDeviceToHost));
    RX_HIP(hipMemcpy(hv[a].data(), vel[a], sizeof(double) * N, hipMemcpyDeviceToHost));
  }
  RX_HIP(hipMemcpy(hq.data(), q, sizeof(double) * N, hipMemcpyDeviceToHost));
  RX_HIP(hipMemcpy(hp.data(), qsfp, sizeof(double) * N, hipMemcpyDeviceToHost));
  RX_HIP(hipMemcpy(hw.data(), qsfv, sizeof(double) * N, hipMemcpyDeviceToHost));
  RX_HIP(hipMemcpy(ht.data(), type, sizeof(int) * N, hipMemcpyDeviceToHost));
  RX_HIP(hipMemcpy(hg.data(), gid, sizeof(long long) * N, hipMemcpyDeviceToHost));
  for (int i = 0; i < N; ++i) {
    double *r = rec + 10 * static_cast<size_t>(i);
    for (int a = 0; a < 3; ++a) r[a] = (box.Hi[a][0] * hx[0][i] + box.Hi[a][1] * hx[1][i] + box.Hi[a][2] * hx[2][i]) - box.obox[a];  // xu2xs
    for (int a = 0; a < 3; ++a) r[3 + a] = hv[a][i];
    r[6] = hq[i]; r[7] = (static_cast<double>(ht[i]) + static_cast<double>(hg[i]) * 1e-13) + atype_resid; r[8] = hp[i]; r[9] = hw[i];
  }
  return N;
}

// ---------------------------------------------------------------------------------------------
// cell binning over residents+ghosts: stable radix sort by cell id, z fastest (LINKEDLIST, main.F90:277-318)
__global__ void k_cell_ids(int G, Grid g, const double *sx, const double *sy, const double *sz, int *cellid, int *idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G) return;
  int cx = static_cast<int>(floor((sx[i] - g.org[0]) * g.inv[0]));
  int cy = static_cast<int>(floor((sy[i] - g.org[1]) * g.inv[1]));
  cx = min(max(cx, 0), g.n[0] - 1); cy = min(max(cy, 0), g.n[1] - 1);
  // z: the slice index (fz slices per cell), one monotone expression of sz -- the sweeps rely on bin(s1) <= bin(s2) for s1 <= s2
  int czf = static_cast<int>(floor((sz[i] - g.org[2]) * (g.inv[2] * g.fz)));
  czf = min(max(czf, 0), g.nzf - 1);
  cellid[i] = (cx * g.n[1] + cy) * g.nzf + czf;
  idx[i] = i;
}
// cellstart[b] = first sorted position whose slice id is >= b (lower bound; one thread per slice, so empty stretches of a sparse box
// cost nothing serial); cellstart[nfine] = G
__global__ void k_cell_starts(int G, int nfine, const int *__restrict__ cid_sorted, int *__restrict__ cellstart) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nfine) return;
  int lo = 0, hi = G;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (cid_sorted[mid] < b) lo = mid + 1; else hi = mid; }
  cellstart[b] = lo;
}
// w component of the packed copy: low 32 bits atom index, bits 32.. type (the list sweeps read both from it; k_sorted_charge later puts the charge there)
__global__ void k_sorted_pos(int G, int N, const int *perm, const int *groot, const double *x, const double *y, const double *z, const int *type, double4 *out, unsigned char *st, int *rootperm, int *invpos) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= G) return;
  const int i = perm[k];
  const double xi = x[i], yi = y[i], zi = z[i];
  const int ti = type[i];
  out[k] = make_double4(xi, yi, zi, __longlong_as_double((static_cast<long long>(ti) << 32) | static_cast<unsigned int>(i)));
  st[k] = static_cast<unsigned char>(ti);
  rootperm[k] = (i < N) ? i : groot[i];
  invpos[i] = k;
}
// xs[k] = v[owner of the atom at cell-sorted position k]: the ghost refresh (MODE_QCOPY1/2, comm.F90:187-212) and the
// spatially sorted gather copy of the vector in one pass
__global__ void k_sorted_vec(int G, const int *__restrict__ rootperm, const double2 *__restrict__ v, double2 *__restrict__ xs) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < G) xs[k] = v[rootperm[k]];
}

void Engine::bin_cells() {
  // residents need fresh normalised coordinates when ghost_build did not just compute them
  k_cell_ids<<<nblk(G, 256), 256, 0, stream>>>(G, grid, spos[0], spos[1], spos[2], cellid, perm_in);
  size_t tb = cubtmp_bytes;
  int bits = 1;
  while ((1LL << bits) < grid.nfine + 1 && bits < 31) ++bits;
  RX_HIP(hipcub::DeviceRadixSort::SortPairs(cubtmp, tb, cellid, cellid_sorted, perm_in, perm, G, 0, bits, stream));
  k_cell_starts<<<nblk(grid.nfine + 1, 256), 256, 0, stream>>>(G, grid.nfine, cellid_sorted, cellstart);
  sorted_positions();
  if (ff.pqeq) pqeq_sorted_shells();
}
void Engine::sorted_positions() {
  k_sorted_pos<<<nblk(G, 256), 256, 0, stream>>>(G, N, perm, groot, pos[0], pos[1], pos[2], type, sorted_xyzi, sorted_type, rootperm, invpos);
  sorted_w_charge = false;
}

void Engine::sorted_copy(const double2 *v) {
  if (multi()) {   // ghost slots first (six-stage exchange), then the plain permuted copy
    halo_staged(reinterpret_cast<double *>(const_cast<double2 *>(v)), 2);
    k_sorted_vec<<<nblk(G, 256), 256, 0, stream>>>(G, perm, v, xs);
    return;
  }
  k_sorted_vec<<<nblk(G, 256), 256, 0, stream>>>(G, rootperm, v, xs);
}

// the error word and the counts of a list build (d_err[0..15]) into pinned host memory, each tagged with the build's sequence number
__global__ void k_publish_words(int n, const int *__restrict__ src, unsigned long long *hpub, unsigned seq) {
  if (threadIdx.x < n) __hip_atomic_store(hpub + threadIdx.x, (static_cast<unsigned long long>(seq) << 32) | static_cast<unsigned>(src[threadIdx.x]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
void Engine::build_ghosts_and_lists(bool qeq_prepass) {
  if (!atoms_set) throw EngineError(RXMD_E_STATE, "atoms were never set");
  TimedSection t_lists(this, &st.ms_lists);           // (an event pair read at a later host wait: no wait of its own)
  bufs.refill(*this);                               // (RXMD_POISON_ALLOC only)
  { Timed kt(this, &st.ms_ghost_build); ghost_build(); }
  bin_cells();
  build_prologue(3);
  { Timed kt(this, &st.ms_k_blist); build_bonded_list(); }
  sums_from_list = qeq_prepass;
  if (qeq_prepass) qeq_start_vectors();             // the sweep below also forms H.(qs,qt) of the CG start vector
  build_list10();
  // The host wait of the build.  First of all the bond tables: a build with more bonds than they hold left them partially packed (k_bond_csr skips
  // the atoms beyond the capacity) -- they are grown and packed again from the intact staging lines BEFORE anything else can throw, so that no
  // error path leaves undersized tables and stale counts behind.
  if (h_pub && !multi()) {                           // (one rank: the words through pinned memory, no copy + stream synchronisation; h_pub exists once the fused ghost build has run)
    const unsigned seq = ++pub_seq;
    k_publish_words<<<1, 64, 0, stream>>>(16, d_err, h_pub, seq);
    pinned_wait(16, seq, "list build");
    for (int k = 0; k < 16; ++k) h_err[k] = static_cast<int>(h_pub[k] & 0xffffffffull);
  } else
    fetch_device_error();
  if (static_cast<size_t>(h_err[7]) > bcap) {
    free_bond_tables();
    alloc_bond_tables(static_cast<size_t>(h_err[7]) + static_cast<size_t>(h_err[7]) / 4 + 4096);
    build_bonded_list(true);
    fetch_device_error();          // the re-pack searched the mirror slots of the atoms the first pass had skipped: its DERR_NBRINDX must be seen THIS step, under this label
  }
  try {
    check_device_error("list build", false);             // (the words are here already)
  } catch (const EngineError &er) {
    // The row stride of the 10 A list is sized from the MEAN density; a dense region inside a sparse box (a nanoparticle in
    // vacuum) can need more.  The reference stops (fixed MAXNEIGHBS10 = 1500, qeq.F90:248-252); here the list grows once to
    // what the sweep reported -- unless the caller fixed the stride (cfg.maxneighbs10), which keeps the reference's trap.
    if (er.code != RXMD_E_MAXNEIGHBS10 || cfg.maxneighbs10 > 0) { collect_timers(); throw; }   // (the host has just waited: the pairs of a refused build go back to the pool)
    const int need = h_err[1];
    S10 = (static_cast<int>(need * 1.1) + 64 + 63) / 64 * 64;
    bufs.free_group(G_LIST10); bufs.alloc_group(*this, G_LIST10);   // (sized by rows10 * S10)
    st.n10_stride = S10;
    { Restore<bool> retry(list10_retry, true); build_list10(); }
    check_device_error("list build");
  }
  nbonds = h_err[7]; nbonds_res = h_err[9];
  win_groups = h_err[8];                               // groups of this build (build_windows; the sweep ran over the host-side bound)
  max_row10 = h_err[3]; min_row10 = std::min(h_err[4], h_err[3]);   // longest / shortest 10 A row of this build (k_list10)
  win_maxunits = h_err[5]; win_valid = win_groups > 0 && h_err[6] == 0 && win_maxunits > 0 && (!multi() || (win_nbnd >= 0 && win_nbnd <= win_groups)) && !opt.spmv_no_win;   // window form of the matrix (build_windows)
  { const int cap = stream_place_cap(); streams_by_place = cap > 0 && S10 >= WIN_BP_MIN_STRIDE && h_err[6] == 0 && static_cast<long long>(win_groups) * WIN_ROWS <= cap; }   // the sweep's own test (k_list10), on the same words
  lists_valid = true;
  if (!nb10_valid && !win_valid) require_nb10();       // the windows were lost in a build that counted on them: the row forms need the 4-byte entries (lists.hip: needs_nb10)
  collect_timers();
  pq_matrix_stale = false;
}

// Width of the matrix value stream of the QEq window pass (rxmd_hip_set_qeq_precision): 64 = the default path, 32 = values rounded once to
// REAL(4) in the list sweep and streamed as float.  Takes effect at the next QEq call: the lists are invalidated and the G_LIST10 group is
// allocated again, with or without hess32, as the stride growth of build_ghosts_and_lists does.
void Engine::set_qeq_precision(int bits) {
  if (bits != 64 && bits != 32) throw EngineError(RXMD_E_ARG, "matrix_bits must be 64 or 32");
  if (bits == 32 && ff.pqeq) throw EngineError(RXMD_E_ARG, "the fp32 matrix stream is not available with PQEq (it carries a second value stream)");
  if (bits == qeq_bits_req) return;
  qeq_bits_req = bits;
  lists_valid = false;
  if (hess) {                                        // (the group exists once the atoms are set)
    sync_stream();
    bufs.free_group(G_LIST10); bufs.alloc_group(*this, G_LIST10);
    nb10_valid = false;
  }
}

// ---------------------------------------------------------------------------------------------
// Variable cell: a new lattice for a live engine (rxmd_hip_set_lattice, and the barostat of step()).  No counterpart in the reference:
// its box is fixed after INITSYSTEM.
//
// r' = M r with M = H' H^-1 (row-major): every resident keeps its normalised coordinates; the PQEq shell displacements follow the same map
struct Mat3 { double m[9]; };
__global__ void k_affine_remap(int n, Mat3 M, double *__restrict__ x, double *__restrict__ y, double *__restrict__ z,
                               double *__restrict__ dx, double *__restrict__ dy, double *__restrict__ dz) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double r0 = x[i], r1 = y[i], r2 = z[i];
  x[i] = M.m[0] * r0 + M.m[1] * r1 + M.m[2] * r2;
  y[i] = M.m[3] * r0 + M.m[4] * r1 + M.m[5] * r2;
  z[i] = M.m[6] * r0 + M.m[7] * r1 + M.m[8] * r2;
  if (dx) {
    const double d0 = dx[i], d1 = dy[i], d2 = dz[i];
    dx[i] = M.m[0] * d0 + M.m[1] * d1 + M.m[2] * d2;
    dy[i] = M.m[3] * d0 + M.m[4] * d1 + M.m[5] * d2;
    dz[i] = M.m[6] * d0 + M.m[7] * d1 + M.m[8] * d2;
  }
}

void Engine::check_lattice(const double lat[6]) const {
  if (!lattice_spans_box(lat)) throw EngineError(RXMD_E_ARG, "lattice does not span a box (edges must be positive, angles inside (0,180) and not coplanar)");
  if (tables_ready)                                          // (before the atoms are set there is no cutoff yet: set-up checks it)
    for (int a = 0; a < 3; ++a)
      if (static_cast<int>(lat[a] / cfg.vprocs[a] / ff.maxrc) < 1) throw EngineError(RXMD_E_ARG, "local box smaller than the bond cutoff");
  if (bar_mode == 2 && !lattice_orthorhombic(lat)) throw EngineError(RXMD_E_ARG, "the per-axis barostat (mode 2) is on: the lattice must stay orthorhombic");
}

// the NB set-up chooses (set_atoms_rxff): the residents it was sized for times the volume of the box with its ghost shell, + 12 % + 4096
long long Engine::capacity_want(const double shell_n[3]) const {
  const long long nsize = std::max<long long>(nsize_setup, N);
  double fac = 1.0;
  for (int a = 0; a < 3; ++a) fac *= 1.0 + 2.0 * std::min(shell_n[a] / box.lbox[a], 1.0);
  const long long want = static_cast<long long>(nsize * fac * 1.12) + 4096;
  return std::min<long long>(want, 2000000000LL);
}

// Collective with several ranks: one all-reduce carries rank 0's six values (every other rank adds zeros, so the sum is rank 0's lattice
// bit for bit) and the count of ranks whose lattice failed its local checks; every rank compares its own lattice with rank 0's EXACTLY, and
// a second all-reduce of the mismatches makes the decision the same everywhere.  Everything is checked before any state changes.
void Engine::set_lattice(const double lat[6], bool check_ranks) {
  bool local_ok = true;
  std::string why;
  try { check_lattice(lat); } catch (const EngineError &er) { if (nprocs == 1 || !check_ranks) throw; local_ok = false; why = er.msg; }
  if (check_ranks && nprocs > 1) {
    double s[7];
    for (int a = 0; a < 6; ++a) s[a] = cfg.myid == 0 ? lat[a] : 0.0;
    s[6] = local_ok ? 0.0 : 1.0;
    allreduce_host(s, 7);
    double bad = 0.0;
    for (int a = 0; a < 6; ++a) if (!(s[a] == lat[a])) bad = 1.0;        // (exact; a NaN anywhere is a mismatch)
    allreduce_host(&bad, 1);
    if (!local_ok) throw EngineError(RXMD_E_ARG, why);
    if (s[6] != 0.0) throw EngineError(RXMD_E_ARG, "set_lattice is collective: another rank's lattice failed its checks");
    if (bad != 0.0) throw EngineError(RXMD_E_ARG, "set_lattice is collective: the ranks passed different lattices");
  }
  apply_lattice(lat);
}

// Everything the new lattice needs is computed and allocated while the engine is still at the old one (the geometry of the new box, the
// buffers sized by its grid, the capacity its ghost shell needs); only then are the residents remapped and the box replaced.
void Engine::apply_lattice(const double lat[6]) {
  if (force_pending) finish_force();               // the energies of the last FORCE reach the host before any buffer can move
  Box nbx{};
  make_box(nbx, lat, cfg.vprocs, vID);
  BoxGeom g{};
  if (tables_ready) {
    g = geometry_for(nbx);
    const long long want = cfg.nbuffer <= 0 ? capacity_want(g.shell) : NB;
    if (want >= (1LL << NB10_IDX_BITS)) throw EngineError(RXMD_E_NBUFFER, "the new lattice needs more than 2^26 atoms+ghosts per GPU (the packed 10 A list entry)");
    // a wider normalised ghost shell (compression lowered cc) needs more atom slots than set-up allocated: grown at the OLD lattice
    if (want > NB) grow_capacity(static_cast<int>(want));
    // buffers sized by the grid: cellstart (cells x z-slices) and the window groups (one short group per grid column at most)
    const size_t need_cs = static_cast<size_t>(g.grid.nfine) + 2, need_ng = win_groups_bound_for(g.grid, rows10) + 1;
    if (need_cs > cellstart_cap || need_ng > win_ng_cap) sync_stream();
    if (need_cs > cellstart_cap) { bufs.free_group(G_CELLSTART); cellstart_cap = need_cs; bufs.alloc_group(*this, G_CELLSTART, need_cs); }
    if (need_ng > win_ng_cap) { bufs.free_group(G_WIN); alloc_window_groups(need_ng); }
  }
  if (atoms_set && N > 0) {
    Mat3 M;
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) M.m[3 * a + c] = nbx.H[a][0] * box.Hi[0][c] + nbx.H[a][1] * box.Hi[1][c] + nbx.H[a][2] * box.Hi[2][c];
    k_affine_remap<<<nblk(N, 256), 256, 0, stream>>>(N, M, pos[0], pos[1], pos[2], ff.pqeq ? shl[0] : nullptr, ff.pqeq ? shl[1] : nullptr, ff.pqeq ? shl[2] : nullptr);
    RX_HIP(hipGetLastError());
  }
  box = nbx;
  for (int a = 0; a < 6; ++a) cfg.lattice[a] = lat[a];
  if (tables_ready) {
    for (int a = 0; a < 3; ++a) { cc[a] = g.cc[a]; shell[a] = g.shell[a]; }
    grid = g.grid; rmesh = g.rmesh;
    st.nbuffer = NB;
    for (int a = 0; a < 3; ++a) { st.cells10[a] = grid.n[a]; st.cells3[a] = cc[a]; }
  }
  lists_valid = false; ghosts_valid = false; win_valid = false;
  last_atype.clear(); for (auto &v : last_pos) v.clear();   // the next array-shaped QEq / FORCE call uploads again
}

// Growth: the slow exact path.  The residents' state and the device scalars go through the host, every buffer is allocated again at the new
// capacity as set-up allocates it (alloc_device zeroes the pinned blocks it allocates), and the state comes back.
void Engine::grow_capacity(int new_nb) {
  if (new_nb >= (1 << NB10_IDX_BITS)) throw EngineError(RXMD_E_NBUFFER, "more than 2^26 atoms+ghosts per GPU do not fit the packed 10 A list entry");
  RX_HIP(hipDeviceSynchronize());                  // (every stream of the engine: the bonded chain and the halo stream included)
  const auto kept = bufs.save_residents(*this);    // the first N elements of the resident arrays; the scalar block: CG state, energies, stress accumulators
  free_device();
  if (xbuf_owned) xbuf_doubles = 0;                // (host-supplied exchange buffers are the host's and stay)
  dh_serve_cap = 0; dh_ready = false; rows_live = false; win_valid = false;
  NB = new_nb;
  alloc_device();
  upload_ff();
  if (sg_on) bufs.alloc_group(*this, G_STRUCT, sg_npair + sg_nangle + static_cast<size_t>(ff.nso));   // the structure accumulators are resident state (structure.hip)
  bufs.restore_residents(kept);
  G = N;
}

void Engine::set_barostat(int mode, int axes, const double p0[3], double tau_fs, double bulk_GPa, int every, double max_strain) {
  if (mode < 0 || mode > 2) throw EngineError(RXMD_E_ARG, "barostat mode must be 0 (off), 1 (isotropic) or 2 (per axis)");
  if (mode != 0) {
    if (!p0) throw EngineError(RXMD_E_ARG, "barostat: p0_GPa is NULL");
    if (!(tau_fs > 0.0) || !(bulk_GPa > 0.0)) throw EngineError(RXMD_E_ARG, "barostat: tau_fs and bulk_modulus_GPa must be > 0");
    if (every < 1) throw EngineError(RXMD_E_ARG, "barostat: every must be >= 1");
    if (!(max_strain > 0.0 && max_strain <= 0.1)) throw EngineError(RXMD_E_ARG, "barostat: max_strain must be in (0, 0.1]");
    if (mode == 2 && (axes < 1 || axes > 7)) throw EngineError(RXMD_E_ARG, "barostat: axes is a bit mask of x (1), y (2), z (4)");
    if (mode == 2 && !lattice_orthorhombic(box.lat)) throw EngineError(RXMD_E_ARG, "the per-axis barostat (mode 2) needs an orthorhombic cell");
    const int np0 = mode == 1 ? 1 : 3;             // (isotropic: p0_GPa[0] only)
    for (int a = 0; a < np0; ++a) if (!std::isfinite(p0[a])) throw EngineError(RXMD_E_ARG, "barostat: p0_GPa must be finite");
    for (int a = 0; a < 3; ++a) bar_p0[a] = p0[a < np0 ? a : 0];
    bar_axes = mode == 2 ? axes : 7; bar_tau = tau_fs; bar_B = bulk_GPa; bar_every = every; bar_max = max_strain;
  }
  bar_mode = mode;
}

}  // namespace rxmd
