/* rxmd_hip.h -- C ABI of the MI355X-native ReaxFF force + charge-equilibration engine.
 *
 * This is the drop-in boundary for the per-step hot path of USCCACS/RXMD.  The reference has
 * no FFI layer: the path sits behind three external Fortran subroutines with implicit
 * interfaces plus module-global state:
 *
 *     subroutine QEq  (atype, pos, q)       reference src/qeq.F90:2
 *     subroutine FORCE(atype, pos, f, q)    reference src/pot.F90:2
 *     subroutine COPYATOMS(imode,dr,...)    reference src/comm.F90:2   (MODE_MOVE from main.F90:75)
 *
 * and the velocity-Verlet loop body around them (reference src/main.F90:64-98).  Every entry
 * point below names the reference interface it replaces.  All functions return 0 on success or
 * a negative RXMD_E_* code (the reference prints and calls MPI_FINALIZE/stop instead,
 * main.F90:402-407, qeq.F90:248-252, comm.F90:467-472); rxmd_hip_last_error() gives the text.
 *
 * Plain C types only (pointers and sizes); one handle per GPU / rank; the caller owns host
 * arrays, the library owns device state.  Not re-entrant per handle (as the reference).
 * The Fortran-side binding a maintainer would add is shown in INTEGRATION.md and shipped as
 * bindings/rxmd_hip_mod.F90 (iso_c_binding).
 */
#ifndef RXMD_HIP_H
#define RXMD_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rxmd_hip_engine *rxmd_handle;

#define RXMD_OK 0
#define RXMD_E_ARG (-1)         /* bad argument / missing file */
#define RXMD_E_FFIELD (-2)      /* ffield could not be parsed */
#define RXMD_E_NBUFFER (-3)     /* residents+ghosts exceed capacity      (comm.F90:467-472) */
#define RXMD_E_MAXNEIGHBS (-4)  /* bonded neighbour overflow             (main.F90:402-407) */
#define RXMD_E_MAXNEIGHBS10 (-5)/* 10 A neighbour overflow               (qeq.F90:248-252)  */
#define RXMD_E_HIP (-6)         /* HIP runtime error / no device */
#define RXMD_E_STATE (-7)       /* call order (e.g. force before atoms were set) */
#define RXMD_E_COMM (-8)        /* multi-rank exchange failed */
#define RXMD_E_NAN (-9)         /* non-finite energy (e.g. collinear torsion, pot.F90:1391-1394) */

/* Run parameters: the union of what GETPARAMS/INITSYSTEM/get_rxmd_parms hand to the path through
 * module globals (reference src/cmdline.F90:255-297, src/init.F90:28-106, src/module.F90:80-84). */
typedef struct rxmd_config {
  const char *ffield_path; /* --ffield ; parsed as src/param.F90:2-375 */
  double lattice[6];       /* lata,latb,latc,lalpha,lbeta,lgamma of the WHOLE box (rxff.bin header, fileio.F90:493-494) */
  int vprocs[3];           /* rxmd.in `processors`; 1 1 1 for a single GPU */
  int myid;                /* rank in the vprocs grid, x fastest (init.F90:75-77) */
  int isQEq;               /* 0 off, 1 CG, 2 extended Lagrangian (qeq.F90:36-63) */
  int NMAXQEq;             /* max CG iterations */
  double QEq_tol;          /* energy criterion (qeq.F90:114-115) */
  int qstep;               /* QEq every qstep MD steps (main.F90:77) */
  double dt_fs;            /* time step in fs (rxmd.in `time`) */
  double Lex_fqs, Lex_k;   /* rxmd.in `exL` (module.F90:164) */
  int nbuffer;             /* capacity residents+ghosts (NBUFFER); 0 = size from the box */
  int maxneighbs;          /* MAXNEIGHBS, 0 = 30 */
  int maxneighbs10;        /* MAXNEIGHBS10 (row stride of the 10 A list), 0 = size from density */
  int device;              /* HIP device ordinal */
  int qeq_mode;            /* 0 = reference algebra (two matrix passes per CG iteration, qeq.F90:96-166)
                              1 = one pass per iteration (gradient by recurrence); same fixed point */
  int lg;                  /* --lg (cmdline.F90:148-151): the ffield is in the low-gradient format (five-line atom blocks, C_lg column;
                              param.F90:83-86,107-109,197-200) and the vdW table carries the LG + core terms (init.F90:496-514) */
  const char *pqeq_path;   /* --pqeq / rxmd.in PQEqParm (cmdline.F90:112-128,291-293): NULL = plain QEq.  Switches the charge solver to
                              PQEq (pqeq.F90), the nonbonded term to ENbond_PQEq (pot.F90:784-923) and the taper cutoff to 12.5 A */
  int efield_dir;          /* rxmd.in `efield <dir> <strength>` / --efield (cmdline.F90:131-137,286-289): 0 = off, 1..3 = x,y,z; PQEq only */
  int reserved1;
  double efield_strength;  /* [V/A]: force -(q_i + Z_i) E Eev_kcal on every core (module.F90:359-383), -Z_i E Eev_kcal on every shell (pqeq.F90:205),
                              centre-of-mass momentum removed every step (main.F90:70-71).  NOTE the reference's EEfield addresses
                              its force array with the wrong leading extent, so for dir > 1 it pushes the x component of ghost slots;
                              the engine applies the field to atom i along dir, which equals the reference for dir = 1 */
} rxmd_config;

void rxmd_hip_default_config(rxmd_config *cfg);
int rxmd_hip_create(const rxmd_config *cfg, rxmd_handle *out);
int rxmd_hip_destroy(rxmd_handle h);
const char *rxmd_hip_last_error(rxmd_handle h);

/* ---- state in / out ------------------------------------------------------------------------- */
/* ReadBIN (src/fileio.F90:444-555): natoms records of 10 doubles exactly as DAT/rxff.bin holds them
 * for this rank: normalised LOCAL pos[3], v[3], q, atype(=type+gid*1e-13), qsfp, qsfv. */
int rxmd_hip_set_atoms_rxff(rxmd_handle h, int natoms, const double *rec10);
/* WriteBIN (src/fileio.F90:558-653): the same record layout back; returns natoms (may have changed
 * by migration).  Pass NULL to query the count. */
int rxmd_hip_get_atoms_rxff(rxmd_handle h, double *rec10, int capacity);
/* Per-atom arrays of the residents in the engine's current local order (the reference's local
 * index order, which the force semantics depend on -- SURVEY 0.9): any pointer may be NULL.
 * pos/v/f are [natoms][3] row-major REAL coordinates; gid = l2g(atype) (main.F90:582-593). */
int rxmd_hip_get_atoms(rxmd_handle h, int capacity, long long *gid, int *type, double *pos, double *v, double *f, double *q);
int rxmd_hip_set_charges(rxmd_handle h, int natoms, const double *q);
int rxmd_hip_set_velocities(rxmd_handle h, int natoms, const double *v);
/* PQEq shell displacements spos(natoms,3) of the residents, real units (module.F90:286; written by WriteXYZ, fileio.F90:332-333).
 * get returns natoms; both fail with RXMD_E_STATE when the engine was created without pqeq_path */
int rxmd_hip_get_shells(rxmd_handle h, double *spos3, int capacity);
/* Bond lists of the residents after the last rxmd_hip_force: what WriteBND reads from nbrlist / BO(0,:,:) (fileio.F90:27-148).
 * count[i] = nbrlist(i,0); partner_gid[i*maxnb + s] = l2g(atype(nbrlist(i,s+1))); bo[i*maxnb + s] = BO(0,i,s+1); maxnb >= the
 * engine's MAXNEIGHBS (30 unless rxmd_config.maxneighbs says otherwise).  Returns natoms. */
int rxmd_hip_get_bonds(rxmd_handle h, int capacity, int maxnb, int *count, long long *partner_gid, double *bo);
int rxmd_hip_set_shells(rxmd_handle h, int natoms, const double *spos3);

/* ---- the hot path, device resident ---------------------------------------------------------- */
/* QEq(atype,pos,q), src/qeq.F90:2-178.  iters = nstep_qeq, est = last GEst1. */
int rxmd_hip_qeq(rxmd_handle h, int *iters, double *est);
/* FORCE(atype,pos,f,q), src/pot.F90:2-90.  pe[0:13] as module.F90:143-146 (pe[0]=sum). */
int rxmd_hip_force(rxmd_handle h, double pe[14]);
/* nsteps passes of the MD loop body, src/main.F90:64-98 (vkick, Lex charges, drift, COPYATOMS(MOVE),
 * QEq every qstep, FORCE, vkick); mdmode 1 (NVE).  Call rxmd_hip_qeq + rxmd_hip_force once before
 * the first step, as main.F90:27-32 does. */
int rxmd_hip_step(rxmd_handle h, int nsteps);
/* mdmode 10: the reference's geometry minimiser (ConjugateGradient, src/cg.F90:26-98 -- Polak-Ribiere directions, bracketing by the
 * Armijo rule, golden-section line search, every trial point a COPYATOMS(MODE_MOVE) + QEq + FORCE) on the device-resident state:
 * positions, search direction and gradients never leave HBM.  ftol = rxmd.in `CG_tol` (energy criterion per atom), max_loops =
 * CG_MaxMinLoop (500).  Returns the number of CG loops (>= 0) or an error; *pe = final potential energy, *evaluations = QEq+FORCE
 * pairs spent.  Velocities are zero afterwards, as the reference leaves them (cg.F90:39). */
int rxmd_hip_minimise(rxmd_handle h, double ftol, int max_loops, double *pe, long long *evaluations);
/* nstep_qeq of the last QEq call (printed in the MDstep line, src/main.F90:261); negative = error */
int rxmd_hip_last_qeq_iters(rxmd_handle h);
/* The velocity scaling the reference's MD loop applies at its head when mod(nstep,sstep)==0 (src/main.F90:45-61), on the
 * device: mdmode 0 and 6 (INITVELOCITY, src/init.F90:292-360: fresh unit-variance Gaussian velocities for every atom -- a counter-based
 * generator keyed by the GLOBAL atom id, so the draw does not depend on the decomposition; RXMD_SEED in the environment changes the
 * stream -- centre-of-mass velocity removed through the all-reduce, scaled to kinetic energy 1.5 treq per atom), 4 (v *= vsfact), 5 (rescale to treq_K; gke_per_atom = kinetic energy per atom of the last PRINTE, <= 0: the
 * current one), 7 (per element, ScaleTemperature :722-763), 8 (only beyond 5 %, AdjustTemperature :684-719); 7 and 8 remove the
 * centre-of-mass momentum afterwards (LinearMomentum :766-797).  The caller keeps the sstep cadence:
 *   for (n = 0; n < nsteps; n += sstep) { rxmd_hip_thermostat(h, mdmode, treq, vsfact, -1); rxmd_hip_step(h, sstep); } */
int rxmd_hip_thermostat(rxmd_handle h, int mdmode, double treq_K, double vsfact, double gke_per_atom);
/* PRINTE reductions (src/main.F90:210-274) for this rank: ke = sum hmas*v^2, qsum, pe[14], and the stress accumulators
 * astr[6] = (xx,yy,zz,yz,zx,xy): virial sum over residents+ghosts of pos*f before the fold (pot.F90:65-72) plus m*v*v of every
 * step (main.F90:86-94), raw sums since the previous read -- passing astr != NULL resets them, as PRINTE does (main.F90:270).
 * Pressure as printed: sum(astr[0..2])/3 / MDBOX * 6.94728103 / pstep  [GPa] (main.F90:233,252). */
int rxmd_hip_get_energy(rxmd_handle h, double *ke, double *qsum, double pe[14], double astr[6]);

/* ---- variable cell: a new lattice for a live engine, Berendsen barostat --------------------- */
/* Replace the lattice of the WHOLE box (lat[6] as rxmd_config.lattice).  Every resident keeps its normalised coordinates:
 * r' = H' H^-1 r (PQEq shell displacements d' = H' H^-1 d) on the device; velocities, charges, forces, Lex state unchanged.  The
 * box-dependent set-up (ghost shell, cell grid, the reference's cell meshes) is derived again and the capacity grows when the new
 * ghost shell needs more atom slots (rxmd_config.nbuffer = 0).  Collective: every rank passes the same lattice.  RXMD_E_ARG and
 * the old lattice kept for lengths <= 0, degenerate angles, a local box below the bond cutoff, lattices that differ between ranks.
 * No counterpart in the reference (its box is fixed after INITSYSTEM). */
int rxmd_hip_set_lattice(rxmd_handle h, const double lat[6]);
int rxmd_hip_get_lattice(rxmd_handle h, double lat[6]);      /* the current lattice (after barostat steps too) */
/* mode 0 off (default), 1 isotropic (P = trace/3, P0 = p0_GPa[0], the three lattice lengths scale together, any cell),
 * 2 per axis (orthorhombic cells only: lattice length a scales with P_aa and p0_GPa[a]; only axes in the bit mask `axes` move).
 * Every `every`-th step of rxmd_hip_step, behind its second half-kick:
 *   mu_a = [1 - (every*dt/tau) (P0_a - P_a) / B]^(1/3), |mu_a - 1| clamped to max_strain, lattice lengths *= mu, angles kept.
 * P_ab [GPa] = (sum_res m v_a v_b + sum_res+ghost r_a f_b) / V * 6.94728103  -- the sums PRINTE prints (main.F90:225-252, pstep = 1),
 * of that step only, summed over all ranks; V = volume of the whole box at which the forces were computed (before the remap).
 * One host wait per coupling (the new lattice); mode 0 adds nothing to a step.  Thermostats combine as a host loop
 * (rxmd_hip_thermostat, then rxmd_hip_step(h, sstep)).  RXMD_E_ARG: tau_fs or bulk_modulus_GPa <= 0, every < 1, max_strain outside
 * (0, 0.1], mode 2 on a non-orthorhombic cell.  No counterpart in the reference. */
int rxmd_hip_set_barostat(rxmd_handle h, int mode, int axes, const double p0_GPa[3], double tau_fs, double bulk_modulus_GPa,
                          int every, double max_strain);
/* last coupling: pressure tensor (xx,yy,zz,yz,zx,xy) [GPa], mu[3], volume [A^3] the pressure was computed at, number of couplings so far */
int rxmd_hip_get_barostat(rxmd_handle h, double p6_GPa[6], double mu[3], double *volume, long long *couplings);

/* ---- mixed-precision charge solver: the QEq matrix values streamed as REAL(4) --------------- */
/* matrix_bits 64 (default): the path as it always was.  32: the list sweep rounds every value of the 10 A matrix ONCE to REAL(4) and the
 * window pass of the CG streams the values as float (6 instead of 10 bytes per entry); every product, sum, vector and scalar stays
 * double, and the row pass and the row sums of the CG start vector use the same rounded values, so every form of the pass applies one
 * operator.  The solution is the fixed point of the rounded matrix: against the full-precision one charges differ by ~5e-7 and forces by
 * ~8e-6 in the parity metric (max |dq| 2.3e-7 e, max |df| 1e-5 kcal/mol/A on RDX), energy terms by <= 2.5e-7 and the total PE by 4e-11
 * relative (QEq is variational).  May be called at any time; takes effect at the next QEq call (the lists are invalidated and the 10 A
 * streams allocated again).  The placement search of the window pass is off while 32 is requested (rxmd_stats.place_draws = 0).
 * RXMD_E_ARG: any other value, or 32 on an engine created with pqeq_path (PQEq carries a second value stream: not supported).
 * RXMD_QEQ_F32=1 in the environment: a plain-QEq engine starts with 32 requested (ignored for PQEq).
 * get: *requested_bits = what was asked for; *in_use_bits = width of the value stream the last matrix pass read -- 32 only when the
 * float instance of the window pass ran (the row pass, RXMD_SPMV_WIN=0 or a window that does not fit, reads the double stream: 64). */
int rxmd_hip_set_qeq_precision(rxmd_handle h, int matrix_bits);
int rxmd_hip_get_qeq_precision(rxmd_handle h, int *requested_bits, int *in_use_bits);

/* ---- the same path behind the reference's own argument shapes ------------------------------- */
/* Host arrays in the reference layout: atype(NBUFFER) packed type+gid*1e-13, pos/f(NBUFFER,3)
 * column-major REAL coordinates, residents 1..natoms.  These upload, run the device path and
 * download; they are what a Fortran `QEq`/`FORCE` shim calls (bindings/rxmd_hip_mod.F90). */
int rxmd_hip_QEq(rxmd_handle h, int nbuffer, int natoms, const double *atype, const double *pos, double *q);
int rxmd_hip_FORCE(rxmd_handle h, int nbuffer, int natoms, const double *atype, const double *pos, double *f, const double *q, double pe[14]);
/* the same for `subroutine PQEq(atype,pos,q)` (src/pqeq.F90:2) and FORCE with isPQEq: the shell displacements spos(NBUFFER,3)
 * of module atoms (module.F90:286) go in, PQEq returns them moved (update_shell_positions, pqeq.F90:184-259) */
int rxmd_hip_PQEq(rxmd_handle h, int nbuffer, int natoms, const double *atype, const double *pos, double *q, double *spos);
int rxmd_hip_FORCE_pqeq(rxmd_handle h, int nbuffer, int natoms, const double *atype, const double *pos, double *f, const double *q, const double *spos, double pe[14]);
/* the fictitious charges of the extended-Lagrangian method, module atoms' qsfp/qsfv (module.F90:289, integrated by the driver,
 * main.F90:67-68,98; read AND written by QEq/PQEq, qeq.F90:41-42,51-52): put_lex hands the host's arrays to the NEXT
 * rxmd_hip_QEq / rxmd_hip_PQEq call, get_lex returns what that call left (isQEq = 1: qsfp = q, qsfv = 0).  With isQEq = 2 the
 * array-shaped QEq/PQEq refuse to run (RXMD_E_ARG) unless put_lex came first: the charges would start from qsfp = 0. */
int rxmd_hip_put_lex(rxmd_handle h, int natoms, const double *qsfp, const double *qsfv);
int rxmd_hip_get_lex(rxmd_handle h, int natoms, double *qsfp, double *qsfv);

/* ---- the same path on arrays that already live on the device -------------------------------- */
/* QEq + FORCE on caller-ordered DEVICE arrays (single rank).  type[natoms] (1..nso), pos3[natoms][3] row-major REAL coordinates, anywhere in
 * space; gid[natoms] or NULL (= i + 1); q_in[natoms] or NULL; outputs f3[natoms][3], q_out[natoms] (either may be NULL); pe[14], virial6[6] on
 * the HOST.  `stream`: the hipStream_t the caller produced the inputs on and will consume the outputs on (NULL = the null stream).
 * The positions are wrapped into the box on the device, r' = r - (n1 a1 + n2 a2 + n3 a3) with n = floor(H^-1 r), triclinic cells included: an atom
 * already inside keeps its coordinates bit for bit; the caller's arrays are never written.  Charges: q_in are the starting charges of the CG (with
 * isQEq = 0 the charges used); q_in = NULL starts from the previous call's solution when natoms is unchanged, from zeros otherwise.  Velocities, the
 * extended-Lagrangian state and forces are zeroed as by rxmd_hip_QEq / rxmd_hip_FORCE.  virial6 = (xx,yy,zz,yz,zx,xy), the sum over residents and
 * ghosts of r_a f_b THIS call added to the accumulators of rxmd_hip_get_energy (same unit; the accumulators themselves are left as rxmd_hip_force
 * leaves them).  The engine works on its own stream: it waits for an event recorded on `stream` at entry and makes `stream` wait for one recorded
 * behind the output kernel; the call itself returns when pe is on the host, as every entry point does.  The first call sizes the engine as
 * rxmd_hip_set_atoms_rxff does (types and positions are staged through the host once); later calls never leave the device.  natoms may change
 * between calls within that capacity (RXMD_E_NBUFFER above it).  A type outside the ffield: RXMD_E_ARG, as from the array-shaped entry points.
 * RXMD_E_ARG also for vprocs other than 1 1 1, an engine created with pqeq_path, isQEq = 2, natoms < 1, NULL type or pos3.
 * No counterpart in the reference. */
int rxmd_hip_evaluate_device(rxmd_handle h, int natoms, const long long *gid, const int *type, const double *pos3, const double *q_in,
                             double *f3, double *q_out, double pe[14], double virial6[6], void *stream);

/* The bond-order graph of the last FORCE as coordinate (COO) arrays in DEVICE memory: the residents' bond lists -- what rxmd_hip_get_bonds copies
 * to the host as padded [natoms][32] arrays -- compacted on the device.  Every entry of a resident's list with BO(0) >= bo_min is selected
 * (bo_min <= 0: all), in resident order and list order within the atom: the row-major walk of rxmd_hip_get_bonds.  The graph is DIRECTED: a bond
 * between two residents appears once from each end.  The compaction is a scan: stable, the same order on every call.
 *   src[e]      local index of the owning resident (the order of rxmd_hip_get_atoms, and the caller's order after rxmd_hip_evaluate_device)
 *   dst[e]      local index of the resident that owns the partner (a ghost partner is resolved to its owner); single rank only
 *               with RXMD_BONDS_GID in flags both are global ids instead (any vprocs: a remote partner's id travels with its ghost)
 *   bo[e]       BO(0), the corrected total bond order: the double rxmd_hip_get_bonds returns
 *   bo3[3e..]   BO(1), BO(2), BO(3) = sigma, pi, double-pi after the corrections (bo.F90:207-215: BO(1) = BO(0) - BO(2) - BO(3)); NULL: not wanted
 *   vec3[3e..]  r_partner - r_owner with the partner's coordinates as the engine holds them: a ghost already is the right periodic image, so this is
 *               the bond vector itself in any cell, triclinic included, and it does not depend on where in space the caller's positions were; NULL: not wanted
 * All five are device pointers.  Returns E, the number of directed bonds selected, or a negative RXMD_E_* code.  src = dst = bo = NULL: count only
 * (capacity, bo3, vec3 ignored).  Otherwise src, dst and bo go together (RXMD_E_ARG when one is missing) and hold `capacity` entries (bo3, vec3:
 * 3 * capacity doubles); when capacity < E NOTHING is written and E is still returned, so the caller compares.  One host wait per call, for E.
 * The engine works on its own stream: `stream` (NULL = the null stream), on which the caller consumes the arrays, is made to wait for an event
 * recorded behind the fill kernel, and the fill kernel waits for what `stream` held at entry.
 * RXMD_E_STATE: no FORCE yet, or set_atoms / set_lattice / set_charges since the last one (the rule of rxmd_hip_get_bonds).  After rxmd_hip_step the
 * tables and positions are those of the last step's FORCE.  Engines created with pqeq_path are fine.  RXMD_E_ARG (checked first): unknown bits in
 * flags, capacity < 0, a non-finite bo_min, local indices (no RXMD_BONDS_GID) on an engine with vprocs other than 1 1 1.
 * The arrays are plain numbers; their derivative with respect to the positions is rxmd_hip_bonds_vjp_device below.  No counterpart in the
 * reference (WriteBND walks nbrlist on the host). */
#define RXMD_BONDS_GID 1   /* src/dst are global ids instead of local resident indices */
long long rxmd_hip_get_bonds_device(rxmd_handle h, int flags, double bo_min, long long capacity, long long *src, long long *dst, double *bo,
                                    double *bo3, double *vec3, void *stream);

/* The vector-Jacobian product of that graph with respect to the positions, on the device.
 * grad_pos3[natoms][3] = dL/dr for L = any function of the arrays the rxmd_hip_get_bonds_device call with the same (flags, bo_min) returns on the same
 * FORCE state; grad_bo[E] = dL/dbo, grad_bo3[3E] = dL/dbo3 or NULL, grad_vec3[3E] = dL/dvec3 or NULL: device pointers in that call's edge order.
 * At least one of the three is given.  E must be the number of edges that call selects (the selection is made again: same flags, same stable scan,
 * same order); otherwise RXMD_E_ARG and nothing is written.  The threshold is a selection, it is not differentiated; RXMD_BONDS_GID in flags only
 * names which selection was made.  grad_pos3 is OVERWRITTEN, in resident order (the order of rxmd_hip_get_atoms, and the caller's order after
 * rxmd_hip_evaluate_device); what lands on a ghost is folded onto its owner: a bond through a periodic image sends its share to the resident.
 * The derivative of a corrected bond order reaches through the neighbour shells of both atoms; it is the force assembly of FORCE (ForceBbo +
 * ForceBondedTerms) with the caller's coefficients in place of dE/dBO and without the index-ordered ForceD term, which is no exact derivative.  It
 * reads what the last FORCE left and changes nothing any other entry point returns: forces, energies, stress accumulators and timers stay as they
 * were.  No atomics: two calls on one state return the same bits.  Bond orders do not depend on the charges.
 * Stream protocol of rxmd_hip_get_bonds_device: the engine's stream waits for what `stream` held at entry, `stream` waits for an event behind the
 * last kernel; one host wait (for the count).
 * RXMD_E_STATE as for rxmd_hip_get_bonds_device: no FORCE yet, or set_atoms / set_lattice / set_charges since.  Fine after rxmd_hip_step and on engines
 * created with pqeq_path.  RXMD_E_ARG (checked first): unknown bits in flags, a non-finite bo_min, E < 0, grad_pos3 NULL, all three gradients NULL,
 * vprocs other than 1 1 1 (the fold of the ghosts' gradients would be collective).  No counterpart in the reference. */
int rxmd_hip_bonds_vjp_device(rxmd_handle h, int flags, double bo_min, long long E, const double *grad_bo, const double *grad_bo3,
                              const double *grad_vec3, double *grad_pos3, void *stream);

/* The 10 A pair graph -- the radius graph the engine builds on every step -- as coordinate (COO) arrays in DEVICE memory: the residents' rows of
 * the 10 A list (nbplist; what ENbond and the QEq matrix walk), compacted on the device.  Every entry of a resident's row with |vec| <= r_cut is
 * selected, |vec| being the norm of the vec3 this call returns (double, from the positions the engine holds, the partner as the list holds it).
 * r_cut <= 0 selects EVERY entry of the list: the reference's own membership (dr^2 of the pair inside the taper cut-off, main.F90:458; in a skewed
 * cell also its non-bonded mesh test), per-row counts equal to nbplist(0,:).  r_cut above the list's reach -- the taper cut-off: 10 A, 12.5 A on an
 * engine created with pqeq_path -- is RXMD_E_ARG: the list does not hold those pairs.  Order: resident order (the order of rxmd_hip_get_atoms, and
 * the caller's order after rxmd_hip_evaluate_device), within a resident the list's own entry order.  The compaction is a scan: stable, no atomics,
 * two calls on one state return the same bits.  The graph is DIRECTED (a pair of residents appears once from each end) and a MULTIGRAPH: in a box
 * with an edge shorter than twice r_cut the same dst appears once per periodic image within reach, each with its own shift.  src == dst with a
 * non-zero shift (an atom and its own image) is legal output: it occurs once r_cut reaches a box edge.  The engine accepts any local box above the
 * bond cut-off and its ghost shell holds ONE image per direction, as the reference's does: the list is the complete radius graph for r_cut up to
 * the shortest perpendicular width of the box; a pair that needs an image two boxes away (r_cut above that width) is not in the list.
 *   src[e], dst[e]  local indices of the owning resident and of the resident that owns the partner (a ghost partner is resolved to its owner as in
 *                   rxmd_hip_get_bonds_device); single rank only.  With RXMD_PAIRS_GID in flags both are global ids instead (any vprocs)
 *   shift3[3e..]    the integers n with vec = r[dst] - r[src] + n1 a1 + n2 a2 + n3 a3 for the engine-held (wrapped) resident positions:
 *                   rint(H^-1 (r_ghost - r_owner)), zero for a resident partner; single rank only; NULL: not wanted
 *   vec3[3e..]      r_partner - r_owner with the partner's coordinates as the engine holds them: the ghost is the right periodic image, so there is
 *                   no minimum-image step, in any cell, and it does not depend on where in space the caller's positions were; NULL: not wanted
 *   hval[e]         the off-diagonal QEq matrix value of that entry as the last list build stored it (qeq_initialize's hessian; PQEq: the
 *                   core-core value): src, dst, hval are the QEq operator as a sparse COO matrix, its diagonal being the ffield's eta (not an edge).
 *                   With the fp32 matrix stream in use (rxmd_hip_set_qeq_precision(32)): the rounded value, widened.  The list sweep forms the
 *                   values whatever isQEq is (k_list10 does not look at it), so hval needs no restriction; NULL: not wanted
 * All five are device pointers.  Returns E, the number of directed pairs selected (64-bit: a dense domain holds more than 2^31), or a negative
 * RXMD_E_* code.  src = dst = NULL: count only (capacity and the other arrays ignored).  Otherwise src and dst go together (RXMD_E_ARG when one is
 * missing) and hold `capacity` entries (shift3: 3 * capacity ints, vec3: 3 * capacity doubles); when capacity < E NOTHING is written and E is still
 * returned, so the caller compares.  One host wait per call, for E.  Stream protocol of rxmd_hip_get_bonds_device: the engine's stream waits for
 * what `stream` (NULL = the null stream) held at entry, `stream` waits for an event recorded behind the fill kernel.
 * RXMD_E_STATE: there is no valid 10 A list -- no rxmd_hip_qeq / rxmd_hip_force (or evaluate / step) yet, or set_atoms / set_lattice /
 * set_qeq_precision since.  RXMD_E_ARG (checked first): unknown bits in flags, a negative capacity, a non-finite r_cut, r_cut beyond the reach,
 * local indices (no RXMD_PAIRS_GID) or shift3 on an engine with vprocs other than 1 1 1.  Global ids with vec3 / hval work on any rank grid and on
 * engines created with pqeq_path.  The call reads the list and changes nothing any other entry point returns; an engine that never asks allocates
 * and launches nothing for it.  No counterpart in the reference. */
#define RXMD_PAIRS_GID 1   /* src/dst are global ids instead of local resident indices */
long long rxmd_hip_get_pairs_device(rxmd_handle h, int flags, double r_cut, long long capacity, long long *src, long long *dst, int *shift3,
                                    double *vec3, double *hval, void *stream);

/* Structure statistics of a live engine, accumulated on the DEVICE from the 10 A list: partial pair counts (-> g_ab(r), n_ab(r), S_ab(q)) and
 * bond-angle counts -- what the reference's offline util/stat computes from XYZ frames with a CPU voxel list.  The usual loop is
 *   structure_begin; for (...) { rxmd_hip_step(h, every); rxmd_hip_structure_sample(h); }  structure_get; structure_end
 * and rxmd_amd/structure.py holds the reference's normalisation of the counts.
 * begin   allocates zeroed int64 accumulators on the device; calling it again replaces them (counts, volume sum and frames start from zero).
 *         RXMD_E_ARG unless 0 < r_max <= the reach of the list (the taper cut-off: 10 A, 12.5 A on an engine created with pqeq_path; the rule of
 *         rxmd_hip_get_pairs_device), 1 <= nbins_r <= 4096, 0 <= nshells <= 4, and for nshells > 0: angle_cut[nshells] strictly ascending with
 *         0 < angle_cut[l] <= r_max, 1 <= nbins_angle <= 360 (nshells = 0: angle_cut and nbins_angle are ignored).  The reference's settings fit:
 *         0.01 A bins (r_max 10, nbins_r 1000), three shells at 2, 4, 6 A, 180 angle bins.
 * sample  adds the engine's current state; works on the engine's stream, no host wait beyond the end of a pending FORCE.  RXMD_E_STATE: no begin,
 *         or no valid 10 A list (no rxmd_hip_qeq / rxmd_hip_force / evaluate / step yet, or set_atoms / set_lattice / set_charges /
 *         set_qeq_precision since: the rule of rxmd_hip_get_pairs_device).  After rxmd_hip_step the state is that of the last step's FORCE.
 *   pair_counts[(a nso + b) nbins_r + k] += 1 for every entry of a resident's row with r < r_max: a = the resident's type - 1, b = the partner's
 *         type - 1, nso = the ffield's number of types, k = (int)(r nbins_r / r_max), r = |r_partner - r_resident| with the partner as the list
 *         holds it (ghosts and images included).  DIRECTED and one per image, exactly the edges of rxmd_hip_get_pairs_device.
 *   angle_counts[l][tj][ti][tk][m] += 1 and angle_counts[l][tk][ti][tj][m] += 1 (row-major, extents nshells, nso, nso, nso, nbins_angle) for every
 *         resident i and every unordered pair of distinct entries j, k of its row with both r < angle_cut[l]: theta = acos(clamp(u_j . u_k, -1, 1))
 *         180 / pi, m = min((int)(theta nbins_angle / 180), nbins_angle - 1).  This is TWICE the reference's table ba (util/stat/main.f90 books 0.5
 *         each way): the counters stay integers.  The min is a designed deviation: the reference's int(theta) + 1 leaves its table at exactly 180.
 *   atoms_per_type[a] += the residents of type a + 1; volume_sum += the TRUE volume of the whole box (the reference multiplies the three lengths:
 *         right for orthorhombic cells only); frames += 1.
 *         Integer atomics only: two samples of one state add identical counts, whatever the layout of the list.  Counts are PER RANK (the
 *         convention of rxmd_hip_get_energy): a rank books its residents' rows, ghost partners as partners; the sum over the ranks is the whole
 *         box, no collective is added (volume_sum and frames are the same on every rank: do not sum those).  Engines created with pqeq_path and
 *         any vprocs work.  Completeness is that of the pair graph: the list is the full radius graph up to the shortest perpendicular width of the
 *         box; a pair that needs an image two boxes away is not in it.
 * get     copies the accumulators to the host; any pointer may be NULL; pair_counts holds nso nso nbins_r words, angle_counts nshells nso^3
 *         nbins_angle, atoms_per_type nso; a capacity (in words) below the array size is RXMD_E_ARG and NOTHING is written.  It does not reset.
 *         RXMD_E_STATE without a begin.
 * end     frees the accumulators (no begin: nothing to do).
 * set_atoms, set_lattice and set_qeq_precision between samples are fine: the accumulators persist, the next sample needs a fresh list as usual.
 * An engine that never calls begin allocates and launches nothing for this.  No counterpart in the reference's engine. */
int rxmd_hip_structure_begin(rxmd_handle h, double r_max, int nbins_r, int nshells, const double *angle_cut, int nbins_angle);
int rxmd_hip_structure_sample(rxmd_handle h);
int rxmd_hip_structure_get(rxmd_handle h, long long *pair_counts, long long pair_capacity, long long *angle_counts, long long angle_capacity,
                           long long *atoms_per_type, double *volume_sum, long long *frames);
int rxmd_hip_structure_end(rxmd_handle h);

/* ---- introspection for tests, roofline accounting and the timers table (main.F90:135-182) ---- */
typedef struct rxmd_stats {
  int natoms, nghost_qeq, nghost_force; /* copyptr(6)-NATOMS after the QEq / FORCE ghost builds */
  long long nnz10;                      /* entries of the 10 A list (sum nbplist(0,:)) */
  long long nbonds;                     /* sum nbrlist(:,0) over residents+ghosts */
  int max_n10, max_nb;                  /* maxas(:,3), maxas(:,2) */
  int qeq_iters_last; long long qeq_iters_total; long long qeq_calls;
  double ms_qeq, ms_qeq_list, ms_qeq_spmv, ms_force, ms_lists, ms_bo, ms_nonbond, ms_bonded, ms_step_total;
  long long spmv_launches;              /* number of matrix passes timed in ms_qeq_spmv */
  int n10_stride, nbuffer, cells10[3], cells3[3];
  int n_boundary_rows;                  /* rows of the 10 A matrix with a ghost partner (vprocs > 1: the launch that waits for the vector halo) */
  int spmv_noop_launches;               /* run-ahead CG loop: matrix-pass launches that returned at once (the iteration queued ahead of the exit decision; one per QEq
                                         * call that ends by the exit test).  NOT in spmv_launches / ms_qeq_spmv; a kernel trace counts them as k_spmv calls */
  int reserved[6];
  /* the exchanges of a vprocs > 1 run (comm.F90:2-100), event-timed on the stream they run on, summed since rxmd_hip_reset_timers:
   * ghost build (MODE_COPY incl. its size messages), migration (MODE_MOVE), vector / charge halos (MODE_QCOPY1/2: pack, send-recv,
   * unpack), the part of them the main stream had to WAIT for (exposed: from the join with the halo stream to the halo's end; the
   * whole halo when overlap is off), scalar all-reduces (qeq.F90:107,129,144,357), reverse force fold (MODE_CPBK) */
  double ms_ghost_build, ms_migrate, ms_halo, ms_halo_exposed, ms_allreduce, ms_fold;
  long long halo_calls, allreduce_calls;
  /* single kernels, HIP events on the engine's stream around each launch, summed like the timers above (bench.py: roofline.kernels):
   * the 10 A sweep, ENbond (PQEq: ENbond_PQEq), E3b, E4b, Ehb, BOPRIM + BOFULL, the assembly gathers of ForceBondedTerms */
  double ms_k_list10, ms_k_nonbond, ms_k_e3b, ms_k_e4b, ms_k_ehb, ms_k_bondorder, ms_k_assemble;
  /* window form of the 10 A matrix (groups of 16 cell-sorted rows whose partners the matrix pass holds in LDS): its build per list build,
   * the number of groups, the largest window in units of 8 cell-sorted positions, 1 when the matrix pass uses it (0: the row pass) */
  double ms_k_winbuild;
  int win_groups, win_max_units, win_in_use;
  int streams_by_place;                 /* layout of the per-entry streams of the 10 A list in the last build: 1 = a row lies at its place in the cell-sorted row order of the
                                         * window groups (RXMD_STREAMS_BY_PLACE, default, when the build has windows and its places fit), 0 = at its atom index */
  /* the window pass timed on the first placement of its streams in memory and on the one that was kept (0: no search ran; see
   * Engine::tune_window_placement, RXMD_PLACE_TRIES) */
  double place_ms_first, place_ms_kept;
  /* (round 5, append-only) the placement search itself: placements timed including the first, its wall time, the bytes of device memory it
   * held at its peak beyond the engine's own streams (0 draws: it did not run -- RXMD_PLACE_TRIES=1, a small system, a nearly full device,
   * or the first placement was already within 3 % of the best this process has seen for the same matrix shape) */
  double place_total_ms, place_bytes_held;
  int place_draws;
  /* the instance of the matrix pass the engine dispatched last: k_spmv_win<MODE, STORE, PQ, spmv_nstep, spmv_var> (qeq.hip); 0, 0 = the row pass k_spmv */
  int spmv_nstep, spmv_var, reserved3;
  double ms_k_blist;                    /* the bonded list: sweep + prefix sum + packing into the compact tables (k_bonded_list, k_bond_csr) */
  /* (append-only) the charge-free part of FORCE (bond orders, bonded terms, assembly: ms_bo, ms_bonded, ms_k_e3b ... are its stream times) runs on a
   * stream of its own next to the QEq iterations and ENbond: what of it the main stream had to WAIT for in front of the stress sums, and 1 when it ran so */
  double ms_bond_exposed;
  int bond_overlap;
  long long spmv_launches_timed;        /* (round 6) matrix passes that carried the HIP event pair (RXMD_PASS_TIMING_EVERY, default every 8th in the run-ahead CG loop, every launch elsewhere);
                                         * ms_qeq_spmv = their average duration x spmv_launches */
  int timer_pairs_dropped;              /* event pairs the ms_* timers could not get since rxmd_hip_reset_timers (the pool of 64 ran dry: long rxmd_hip_step calls without a list build or
                                         * a CG loop to collect them): when > 0 the ms_* breakdown under-counts */
} rxmd_stats;
int rxmd_hip_get_stats(rxmd_handle h, rxmd_stats *out);
int rxmd_hip_reset_timers(rxmd_handle h);
/* switch rxmd_config.qeq_mode (0|1) between calls; both modes share every buffer */
int rxmd_hip_set_qeq_mode(rxmd_handle h, int mode);

/* host-side derived tables for unit tests (CUTOFFLENGTH/POTENTIALTABLE, src/init.F90:363-522):
 * which: 0 Evdw 1 dEvdw 2 Eclmb 3 dEclmb 4 Eclmb_QEq  -> out[nboty][5000]; returns nboty */
int rxmd_hip_get_table(rxmd_handle h, int which, double *out, int capacity);
int rxmd_hip_get_cutoffs(rxmd_handle h, double *rc, int capacity, double *maxrc);
/* debugging taps on device state after rxmd_hip_force (residents+ghosts, engine order):
 * what: 0 delta  1 deltap  2 bonded neighbour count  3 real pos (x3)  4 gid  5 type  6 n10 count (residents)
 *       7 hessian row sums (residents)  8 cdbnd gathered per atom  9 charges incl. ghosts
 *       10 ccbnd as ForceBondedTerms consumes it (pot.F90:129-135)  11 window form of the 10 A matrix: entries per resident whose 16-bit slot
 *       leads back to the entry's own position and ghost flag (== what 6 returns; -1 without windows)  100 read-bandwidth probe
 *       102 stripped-down forms of the row pass, 104 the real window pass / row pass back to back: {ms, ms} (experiments, after rxmd_hip_qeq) */
int rxmd_hip_debug_get(rxmd_handle h, int what, double *out, int capacity);

/* ---- multi-rank surface (COPYATOMS, src/comm.F90) ------------------------------------------- */
/* The engine performs the reference's six-direction staged exchange.  With vprocs = 1 1 1 every
 * partner is the rank itself and the exchange is a device-side copy.  For vprocs > 1 the host
 * supplies the transport: `exchange` must deliver `nsend` doubles from device pointer `send` to
 * rank `to` and receive up to `cap` doubles from rank `from` into device pointer `recv`, return the
 * number received; `allreduce_sum` sums n host doubles in place over all ranks.  (RCCL via
 * torch.distributed in bench.py; MPI_Send/Recv + MPI_Allreduce in a Fortran driver.) */
typedef struct rxmd_comm_ops {
  void *ctx;
  long long (*exchange)(void *ctx, int to, const double *send, long long nsend, int from, double *recv, long long cap);
  int (*allreduce_sum)(void *ctx, double *buf, int n);
  /* optional (may be NULL): the same as `exchange` when the receiver already knows it will get exactly `nrecv` doubles
   * (vector halos and force returns re-use the index lists of the ghost build), so no size message is needed.  `send` and
   * `recv` may point INSIDE the exchange buffers: the two stages of an axis are packed back to back and handed over as two
   * consecutive calls (RXMD_NO_STAGE_PAIRS=1 restores one message per buffer) */
  long long (*exchange_known)(void *ctx, int to, const double *send, long long nsend, int from, double *recv, long long nrecv);
} rxmd_comm_ops;
int rxmd_hip_set_comm(rxmd_handle h, const rxmd_comm_ops *ops);
/* Native transport: RCCL send/recv + all-reduce on the engine's own stream (rccl_comm.hip), one communicator per engine.
 * Rank 0 obtains a 128-byte id with rxmd_hip_rccl_unique_id, the host distributes it (MPI_Bcast, torch.distributed, a file)
 * and every rank calls rxmd_hip_comm_init_rccl(h, id, myid, nprocs); a collective call.  Takes precedence over rxmd_comm_ops. */
int rxmd_hip_rccl_unique_id(unsigned char out128[128]);
int rxmd_hip_comm_init_rccl(rxmd_handle h, const unsigned char id128[128], int rank, int world);
/* What a host transport without GPU-aware messaging needs (the MPI callbacks of bindings/rxmd_hip_mod.F90 stage every message
 * through host memory): synchronous copies between the device pointers handed to `exchange` and host buffers, and the number
 * of HIP devices this process sees (a Fortran driver picks `device = myid mod count`). */
int rxmd_hip_copy_to_host(const double *dev, double *host, long long ndoubles);
int rxmd_hip_copy_to_device(double *dev, const double *host, long long ndoubles);
int rxmd_hip_device_count(void);
/* Optional: let the host own the two message buffers (device memory, `ndoubles` each) that `exchange` is called
 * with -- e.g. torch tensors, so that torch.distributed can send them without wrapping foreign pointers. */
int rxmd_hip_set_exchange_buffers(rxmd_handle h, double *send, double *recv, long long ndoubles);
/* Transport self-test with HOST buffers (no GPU needed): every rank sends a pattern round the ring of `nprocs` ranks in
 * both directions with different lengths and all-reduces a vector; returns 0 if the callbacks honour the contract. */
int rxmd_host_comm_selftest(const rxmd_comm_ops *ops, int myid, int nprocs);

/* ---- host front-end helpers (no GPU needed) ------------------------------------------------- */
/* geninit (reference init/geninit.F90:399-575): replicate a fractional-coordinate unit cell mc times,
 * split into vprocs domains, and return this rank's rxff.bin records.  `elem` holds natoms0
 * 2-character element names ("C\0","H\0"...) 4 bytes apart.  Returns the number of atoms of rank
 * `myid` (call with rec10 == NULL to size); lattice_out gets the super-cell lattice. */
long long rxmd_host_geninit(const char *ffield_path, int natoms0, const char *elem4, const double *frac,
                            const double lattice[6], const int mc[3], const int vprocs[3], int myid,
                            double *rec10, long long capacity, double lattice_out[6]);
/* rxff.bin header + this rank's records (ReadBIN); returns natoms of `myid` or <0 */
long long rxmd_host_read_rxff(const char *path, int myid, double lattice_out[6], int vprocs_out[3], double *rec10, long long capacity);
/* ffield parser + derived tables on the host (GETPARAMS src/param.F90:2-375, CUTOFFLENGTH/POTENTIALTABLE
 * src/init.F90:363-522) without touching a GPU.  natoms_per_type[1..nso] selects the types present (index 0 unused).
 * which: 0 Evdw 1 dEvdw 2 Eclmb 3 dEclmb 4 Eclmb_QEq -> out[nboty][5000]; 5 -> out = rc[nboty] then maxrc;
 * 6 -> out = {nso,nboty,nvaty,ntoty,nhbty, chi[1..nso], eta[1..nso], mass[1..nso]}.  Returns nboty or <0. */
int rxmd_host_ffield_table(const char *ffield_path, const long long *natoms_per_type, int which, double *out, long long capacity);
/* geninit's `-lg` / rxmd's `--lg` for the host helpers above (geninit, ffield_table): nonzero = they read ffields in the
 * low-gradient format (init/geninit.F90:233,347).  Process-wide like the reference's module variable; returns the previous value.
 * The engine itself takes the switch per handle (rxmd_config.lg). */
int rxmd_host_ffield_lg(int on);
/* The environment switches of the library (rxmd_amd/csrc/options.def: one table, read once per engine at rxmd_hip_create) as the markdown rows
 * README.md shows: "| `ENV` | default | meaning |" per line, experiments-only switches marked (exp).  Returns the length of the text; copies at
 * most capacity - 1 characters and a terminating 0 into buf (buf may be NULL to size). */
int rxmd_host_describe_options(char *buf, int capacity);
/* library build info: returns 1 if the HIP code object for gfx950 is linked in */
int rxmd_hip_has_device_code(void);

#ifdef __cplusplus
}
#endif
#endif
