"""Host-side mirror of the reference's operator surface for the hot path.

The reference exposes the path as Fortran subroutines `QEq(atype,pos,q)` (src/qeq.F90:2),
`FORCE(atype,pos,f,q)` (src/pot.F90:2) and the MD loop body (src/main.F90:64-98) working on
module-global arrays.  `RxmdEngine` keeps those names and argument meanings on top of the C ABI
(include/rxmd_hip.h); device state lives in the library, numpy arrays are views for the caller.
Errors that make the reference print + MPI_FINALIZE + stop raise RxmdError with the same text.
"""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import RxmdConfig, RxmdStats

PE_NAMES = ["Esystem", "Ebond", "Elp", "Eover", "Eunder", "Eval", "Epen", "Ecoa", "Etors", "Econj", "Ehbond", "Evdwaals", "Ecoulomb", "Echarge"]
BONDS_GID = 1      # RXMD_BONDS_GID of include/rxmd_hip.h
PAIRS_GID = 1      # RXMD_PAIRS_GID


class RxmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rxmd_hip error %d: %s" % (code, msg))
        self.code = code


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _addr(a):      # a device address or a stream handle given as an integer (0: NULL) -> a void * argument
    return C.c_void_p(int(a) or None)


class RxmdEngine:
    """One engine = one rank of the vprocs grid = one MI355X."""

    def __init__(self, ffield, lattice, vprocs=(1, 1, 1), myid=0, isQEq=1, NMAXQEq=500, QEq_tol=1e-7, qstep=1, dt_fs=0.25,
                 nbuffer=0, maxneighbs=0, maxneighbs10=0, device=0, qeq_mode=0, Lex_fqs=1.0, Lex_k=2.0, pqeq=None, efield=None, lg=False):
        self.L = _lib.load()
        cfg = RxmdConfig()
        self.L.rxmd_hip_default_config(C.byref(cfg))
        self._ff = str(ffield).encode()
        cfg.ffield_path = self._ff
        for i in range(6):
            cfg.lattice[i] = float(lattice[i])
        for i in range(3):
            cfg.vprocs[i] = int(vprocs[i])
        cfg.myid = myid; cfg.isQEq = isQEq; cfg.NMAXQEq = NMAXQEq; cfg.QEq_tol = QEq_tol; cfg.qstep = qstep; cfg.dt_fs = dt_fs
        cfg.nbuffer = nbuffer; cfg.maxneighbs = maxneighbs; cfg.maxneighbs10 = maxneighbs10; cfg.device = device; cfg.qeq_mode = qeq_mode
        cfg.Lex_fqs = Lex_fqs; cfg.Lex_k = Lex_k
        self._pq = str(pqeq).encode() if pqeq else None       # --pqeq <file> (cmdline.F90:112-128): PQEq instead of QEq
        cfg.pqeq_path = self._pq
        cfg.lg = 1 if lg else 0                                # --lg: LG ffield format + low-gradient dispersion tables
        if efield:                                             # (dir 1..3, strength V/A): rxmd.in `efield`
            cfg.efield_dir = int(efield[0]); cfg.efield_strength = float(efield[1])
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.L.rxmd_hip_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RxmdError(rc, (self.L.rxmd_hip_last_error(None) or b"").decode())
        self.h = h

    @property
    def lattice(self):
        """the current lattice of the whole box: follows set_lattice and the barostat (what write_xyz / write_pdb / write_rxff write)"""
        return self.get_lattice()

    def get_lattice(self):
        out = np.zeros(6)
        self._chk(self.L.rxmd_hip_get_lattice(self.h, _ptr(out)))
        return [float(x) for x in out]

    def set_lattice(self, lat):
        """new lattice of the whole box (collective); the residents keep their normalised coordinates"""
        lat = np.ascontiguousarray(lat, np.float64).reshape(6)
        self._chk(self.L.rxmd_hip_set_lattice(self.h, _ptr(lat)))

    def set_barostat(self, mode, p0=0.0, tau_fs=100.0, bulk_modulus=15.0, every=1, max_strain=0.01, axes=7):
        """Berendsen barostat inside step(): mode 0 off, 1 isotropic (p0 [GPa] a number), 2 per axis (p0 a number or three, axes a bit mask x=1 y=2 z=4)"""
        p = np.broadcast_to(np.asarray(p0, np.float64), (3,)).copy()
        self._chk(self.L.rxmd_hip_set_barostat(self.h, int(mode), int(axes), _ptr(p), float(tau_fs), float(bulk_modulus), int(every), float(max_strain)))

    def barostat_state(self):
        """last coupling: pressure tensor p6 (xx,yy,zz,yz,zx,xy) [GPa], mu[3], the volume it was computed at [A^3], couplings so far"""
        p6 = np.zeros(6); mu = np.zeros(3); vol = C.c_double(0); n = C.c_longlong(0)
        self._chk(self.L.rxmd_hip_get_barostat(self.h, _ptr(p6), _ptr(mu), C.byref(vol), C.byref(n)))
        return dict(p6=p6, mu=mu, volume=vol.value, couplings=n.value)

    def set_qeq_precision(self, bits):
        """width of the QEq matrix value stream: 64 (default) or 32 = values rounded once to REAL(4) and streamed as float by the window pass, all
        arithmetic in double (plain QEq only; RxmdError RXMD_E_ARG otherwise).  Takes effect at the next QEq call."""
        self._chk(self.L.rxmd_hip_set_qeq_precision(self.h, int(bits)))

    def qeq_precision(self):
        """(requested, in_use): in_use is the width of the value stream the last matrix pass read, 32 only when the float window instance ran"""
        req = C.c_int(0); use = C.c_int(0)
        self._chk(self.L.rxmd_hip_get_qeq_precision(self.h, C.byref(req), C.byref(use)))
        return req.value, use.value

    def close(self):
        if getattr(self, "h", None):
            self.L.rxmd_hip_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise RxmdError(rc, self.L.rxmd_hip_last_error(self.h).decode())
        return rc

    # ---- state ----
    def set_atoms_rxff(self, rec10):
        rec10 = np.ascontiguousarray(rec10, np.float64).reshape(-1, 10)
        self._chk(self.L.rxmd_hip_set_atoms_rxff(self.h, len(rec10), _ptr(rec10)))

    def get_atoms_rxff(self):
        n = self._chk(self.L.rxmd_hip_get_atoms_rxff(self.h, None, 0))
        out = np.zeros((n, 10))
        self._chk(self.L.rxmd_hip_get_atoms_rxff(self.h, _ptr(out), n))
        return out

    @property
    def natoms(self):
        return self._chk(self.L.rxmd_hip_get_atoms_rxff(self.h, None, 0))

    def atoms(self):
        n = self.natoms
        gid = np.zeros(n, np.int64); typ = np.zeros(n, np.int32)
        pos = np.zeros((n, 3)); v = np.zeros((n, 3)); f = np.zeros((n, 3)); q = np.zeros(n)
        self._chk(self.L.rxmd_hip_get_atoms(self.h, n, _ptr(gid), _ptr(typ), _ptr(pos), _ptr(v), _ptr(f), _ptr(q)))
        return dict(gid=gid, type=typ, pos=pos, v=v, f=f, q=q)

    def set_charges(self, q):
        q = np.ascontiguousarray(q, np.float64); self._chk(self.L.rxmd_hip_set_charges(self.h, len(q), _ptr(q)))

    def set_velocities(self, v):
        v = np.ascontiguousarray(v, np.float64).reshape(-1, 3); self._chk(self.L.rxmd_hip_set_velocities(self.h, len(v), _ptr(v)))

    def thermostat(self, mdmode, treq=300.0, vsfact=1.0, gke=-1.0):
        """velocity scaling of the MD loop head, main.F90:45-61 (mdmode 4, 5, 7, 8); call every sstep steps"""
        self._chk(self.L.rxmd_hip_thermostat(self.h, int(mdmode), float(treq), float(vsfact), float(gke)))

    def write_xyz(self, path, natoms_total=None):
        """trajectory frame in the reference's WriteXYZ layout (fileio.F90:241-355); with several ranks every rank writes its part
        (natoms_total = global count on rank 0, -1 on the others) and the parts are concatenated in rank order"""
        from . import system
        a = self.atoms()
        txt = system.format_xyz(self.lattice, system.ffield_type_names(self._ff.decode()), a["gid"], a["type"], a["pos"], a["q"],
                                self.shells() if self._pq else None, natoms_total)
        with open(path, "w") as f:
            f.write(txt)

    def bonds(self):
        """bond lists of the residents after the last FORCE (nbrlist / BO(0,:,:), what WriteBND reads): (count[n], partner_gid[n,maxnb], bo[n,maxnb])"""
        n = self.natoms; mx = 32
        cnt = np.zeros(n, np.int32); pg = np.zeros((n, mx), np.int64); bo = np.zeros((n, mx))
        self._chk(self.L.rxmd_hip_get_bonds(self.h, n, mx, _ptr(cnt), _ptr(pg), _ptr(bo)))
        return cnt, pg, bo

    def write_bnd(self, path):
        """bond file of the current frame in the reference's WriteBND layout (fileio.F90:27-148); with several ranks the parts are concatenated in rank order"""
        from . import system
        a = self.atoms(); cnt, pg, bo = self.bonds()
        with open(path, "w") as f:
            f.write(system.format_bnd(a["gid"], a["type"], a["pos"], cnt, pg, bo))

    def write_pdb(self, path, astr=None):
        """pdb frame in the reference's WritePDB layout (fileio.F90:151-238); astr: the stress accumulators whose mean diagonal goes to the last
        column (default: the engine's own since the last energy read)"""
        from . import system
        a = self.atoms()
        if astr is None:
            astr = self.energy()["astr"]
        with open(path, "w") as f:
            f.write(system.format_pdb(system.ffield_type_names(self._ff.decode()), a["gid"], a["type"], a["pos"], a["q"], astr))

    def write_rxff(self, path, current_step=0):
        """checkpoint in the reference's WriteBIN layout (fileio.F90:558-653), single rank"""
        from . import system
        system.write_rxff(path, self.lattice, (1, 1, 1), [self.get_atoms_rxff()], current_step)

    # ---- native multi-GPU transport (include/rxmd_hip.h: rxmd_hip_comm_init_rccl) ----
    def rccl_unique_id(self):
        buf = C.create_string_buffer(128); self._chk(self.L.rxmd_hip_rccl_unique_id(buf)); return buf.raw

    def init_rccl(self, unique_id, rank, world):
        """collective: every rank of the vprocs grid calls it with the id rank 0 generated"""
        self._chk(self.L.rxmd_hip_comm_init_rccl(self.h, C.c_char_p(bytes(unique_id)), int(rank), int(world)))

    def shells(self):
        """PQEq shell displacements spos(natoms,3)"""
        n = self.natoms
        out = np.zeros((n, 3)); rc = self.L.rxmd_hip_get_shells(self.h, _ptr(out), n)
        if rc < 0:
            self._chk(rc)
        return out[:rc]

    def set_shells(self, s):
        s = np.ascontiguousarray(s, np.float64).reshape(-1, 3); self._chk(self.L.rxmd_hip_set_shells(self.h, len(s), _ptr(s)))

    # ---- the hot path (device resident) ----
    def QEq(self):
        """QEq(atype,pos,q), reference src/qeq.F90:2 -> (nstep_qeq, Est)"""
        it = C.c_int(0); est = C.c_double(0.0)
        self._chk(self.L.rxmd_hip_qeq(self.h, C.byref(it), C.byref(est)))
        return it.value, est.value

    def FORCE(self):
        """FORCE(atype,pos,f,q), reference src/pot.F90:2 -> PE(0:13)"""
        pe = np.zeros(14)
        self._chk(self.L.rxmd_hip_force(self.h, _ptr(pe)))
        return pe

    def step(self, nsteps=1):
        """nsteps passes of the MD loop body, reference src/main.F90:64-98"""
        self._chk(self.L.rxmd_hip_step(self.h, int(nsteps)))

    def minimise(self, ftol=1e-4, max_loops=500):
        """mdmode 10, the reference's ConjugateGradient (src/cg.F90:26-98) on the device-resident state -> (CG loops, final PE, QEq+FORCE evaluations)"""
        pe = C.c_double(0); ev = C.c_longlong(0)
        loops = self._chk(self.L.rxmd_hip_minimise(self.h, float(ftol), int(max_loops), C.byref(pe), C.byref(ev)))
        return loops, pe.value, ev.value

    def energy(self):
        ke = C.c_double(0); qs = C.c_double(0); pe = np.zeros(14); astr = np.zeros(6)
        self._chk(self.L.rxmd_hip_get_energy(self.h, C.byref(ke), C.byref(qs), _ptr(pe), _ptr(astr)))
        return dict(KE=ke.value, qsum=qs.value, PE=pe, astr=astr)

    # ---- the reference's own array shapes ----
    def QEq_arrays(self, atype, pos, q, natoms):
        """atype(NBUFFER), pos(NBUFFER,3) column-major (Fortran order), q(NBUFFER) updated in place"""
        nbuf = len(atype)
        posf = np.asfortranarray(pos, np.float64); atype = np.ascontiguousarray(atype, np.float64)
        assert q.flags["C_CONTIGUOUS"] and q.dtype == np.float64
        self._chk(self.L.rxmd_hip_QEq(self.h, nbuf, natoms, _ptr(atype), posf.ctypes.data_as(C.c_void_p), _ptr(q)))
        return q

    def FORCE_arrays(self, atype, pos, q, natoms):
        nbuf = len(atype)
        posf = np.asfortranarray(pos, np.float64); atype = np.ascontiguousarray(atype, np.float64); q = np.ascontiguousarray(q, np.float64)
        f = np.zeros((nbuf, 3), order="F"); pe = np.zeros(14)
        self._chk(self.L.rxmd_hip_FORCE(self.h, nbuf, natoms, _ptr(atype), posf.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), _ptr(q), _ptr(pe)))
        return f, pe

    # ---- the same path on arrays that already live on the device ----
    def evaluate_device(self, natoms, type_ptr, pos_ptr, f_ptr, q_out_ptr, gid_ptr=0, q_in_ptr=0, stream=0):
        """QEq + FORCE on caller-ordered device arrays given as integer addresses (include/rxmd_hip.h: rxmd_hip_evaluate_device): int32 type[natoms],
        float64 pos[natoms][3] anywhere in space, outputs float64 f[natoms][3] and q_out[natoms] (0: not wanted), optional int64 gid[natoms] and
        start charges q_in[natoms]; stream: the hipStream_t handle the arrays are produced and consumed on -> (PE(0:13), virial[6]) on the host"""
        pe = np.zeros(14); vir = np.zeros(6)
        self._chk(self.L.rxmd_hip_evaluate_device(self.h, int(natoms), *map(_addr, (gid_ptr, type_ptr, pos_ptr, q_in_ptr, f_ptr, q_out_ptr)), _ptr(pe), _ptr(vir), _addr(stream)))
        return pe, vir

    def bonds_device(self, capacity, src_ptr, dst_ptr, bo_ptr, bo3_ptr=0, vec_ptr=0, bo_min=0.0, as_gid=False, stream=0):
        """the bond-order graph of the last FORCE as coordinate arrays in device memory, given as integer addresses (include/rxmd_hip.h:
        rxmd_hip_get_bonds_device): int64 src[capacity], dst[capacity], float64 bo[capacity], optional float64 bo3[capacity][3] (sigma, pi,
        double-pi) and vec[capacity][3] (r_dst - r_src, the right periodic image).  Every list entry with bo >= bo_min, in the row-major order of
        bonds(); directed.  src / dst are local indices (the order of atoms()), global ids with as_gid.  src_ptr = dst_ptr = bo_ptr = 0: count only.
        -> E, the number of directed bonds selected; nothing is written when capacity < E"""
        return self._chk(self.L.rxmd_hip_get_bonds_device(self.h, BONDS_GID if as_gid else 0, float(bo_min), int(capacity), *map(_addr, (src_ptr, dst_ptr, bo_ptr, bo3_ptr, vec_ptr)), _addr(stream)))

    def bonds_vjp_device(self, E, grad_pos_ptr, grad_bo_ptr=0, grad_bo3_ptr=0, grad_vec_ptr=0, bo_min=0.0, as_gid=False, stream=0):
        """the vector-Jacobian product of that graph with respect to the positions (include/rxmd_hip.h: rxmd_hip_bonds_vjp_device), device arrays given
        as integer addresses: float64 grad_bo[E], grad_bo3[E][3], grad_vec[E][3] (0: not given; at least one is) are dL/d(bo, bo3, vec) in the edge
        order of bonds_device(bo_min=bo_min, as_gid=as_gid) on the same FORCE state, E the count that call returns (RxmdError -1 otherwise, nothing
        written); float64 grad_pos[natoms][3] receives dL/dpos in the order of atoms() (overwritten)"""
        self._chk(self.L.rxmd_hip_bonds_vjp_device(self.h, BONDS_GID if as_gid else 0, float(bo_min), int(E), *map(_addr, (grad_bo_ptr, grad_bo3_ptr, grad_vec_ptr, grad_pos_ptr)), _addr(stream)))

    def pairs_device(self, capacity, src_ptr, dst_ptr, shift_ptr=0, vec_ptr=0, h_ptr=0, r_cut=0.0, as_gid=False, stream=0):
        """the 10 A pair graph of the last list build as coordinate arrays in device memory, given as integer addresses (include/rxmd_hip.h:
        rxmd_hip_get_pairs_device): int64 src[capacity], dst[capacity], optional int32 shift[capacity][3] (periodic image of dst), float64
        vec[capacity][3] (r_dst - r_src through that image) and float64 h[capacity] (the QEq matrix value of the entry).  Every list entry with
        |vec| <= r_cut (r_cut <= 0: the whole list; above the taper cut-off: RxmdError -1), in the order of atoms() and list order within an atom;
        directed, one edge per image.  src / dst are local indices, global ids with as_gid.  src_ptr = dst_ptr = 0: count only.
        -> E, the number of directed pairs selected; nothing is written when capacity < E"""
        return self._chk(self.L.rxmd_hip_get_pairs_device(self.h, PAIRS_GID if as_gid else 0, float(r_cut), int(capacity), *map(_addr, (src_ptr, dst_ptr, shift_ptr, vec_ptr, h_ptr)), _addr(stream)))

    # ---- structure statistics accumulated on the device (include/rxmd_hip.h: rxmd_hip_structure_*; normalisation: rxmd_amd/structure.py) ----
    def _nso(self):
        """the ffield's number of atom types: the extent of the count arrays"""
        if getattr(self, "_nso_cached", None) is None:
            out = np.zeros(4096)
            was = self.L.rxmd_host_ffield_lg(int(self.cfg.lg))
            try:
                rc = self.L.rxmd_host_ffield_table(self._ff, None, 6, _ptr(out), len(out))
            finally:
                self.L.rxmd_host_ffield_lg(was)
            if rc < 0:
                raise RxmdError(rc, "cannot parse %s" % self._ff.decode())
            self._nso_cached = int(out[0])
        return self._nso_cached

    def structure_begin(self, r_max, nbins_r, angle_cuts=(), nbins_angle=180):
        """zeroed accumulators on the device: pair counts in nbins_r bins up to r_max (<= the reach of the 10 A list), bond-angle counts in
        nbins_angle bins up to 180 degrees for every shell of angle_cuts (ascending, at most four, each <= r_max; empty: no angles).
        Calling it again starts from zero."""
        cuts = np.ascontiguousarray(angle_cuts, np.float64).reshape(-1)
        self._chk(self.L.rxmd_hip_structure_begin(self.h, float(r_max), int(nbins_r), len(cuts), _ptr(cuts) if len(cuts) else None, int(nbins_angle)))
        self._structure = (float(r_max), int(nbins_r), [float(c) for c in cuts], int(nbins_angle) if len(cuts) else 0)

    def structure_sample(self):
        """add the state of the last QEq / FORCE / step to the accumulators (RxmdError -7 without structure_begin or without a valid 10 A list)"""
        self._chk(self.L.rxmd_hip_structure_sample(self.h))

    def structure_counts(self):
        """-> dict: pair_counts int64 [nso, nso, nbins_r] (resident type, partner type, r bin; directed), angle_counts int64 [nshells, nso, nso, nso,
        nbins_angle] (shell, end type, centre type, end type, angle bin; twice the reference's table), atoms_per_type int64 [nso], volume_sum
        [A^3], frames -- the sums over every sample so far, of THIS rank (structure.merge sums ranks) -- and the binning (r_max, angle_cuts).
        Does not reset."""
        if getattr(self, "_structure", None) is None:
            raise RxmdError(-7, "structure_counts: call structure_begin first")
        r_max, nbr, cuts, nba = self._structure
        nso = self._nso()
        pair = np.zeros((nso, nso, nbr), np.int64); ang = np.zeros((len(cuts), nso, nso, nso, nba), np.int64); npt = np.zeros(nso, np.int64)
        vol = C.c_double(0); fr = C.c_longlong(0)
        self._chk(self.L.rxmd_hip_structure_get(self.h, _ptr(pair), pair.size, _ptr(ang) if ang.size else None, ang.size, _ptr(npt), C.byref(vol), C.byref(fr)))
        return dict(pair_counts=pair, angle_counts=ang, atoms_per_type=npt, volume_sum=vol.value, frames=fr.value, r_max=r_max, angle_cuts=list(cuts))

    def structure_end(self):
        """free the accumulators"""
        self._chk(self.L.rxmd_hip_structure_end(self.h))
        self._structure = None

    # ---- introspection ----
    def stats(self):
        s = RxmdStats(); self._chk(self.L.rxmd_hip_get_stats(self.h, C.byref(s))); return s.asdict()

    def reset_timers(self):
        self._chk(self.L.rxmd_hip_reset_timers(self.h))

    def set_qeq_mode(self, mode):
        self._chk(self.L.rxmd_hip_set_qeq_mode(self.h, int(mode)))

    def table(self, which):
        rc = C.c_double(0)
        nboty = self._chk(self.L.rxmd_hip_get_cutoffs(self.h, None, 0, C.byref(rc)))
        out = np.zeros((nboty, 5000))
        self._chk(self.L.rxmd_hip_get_table(self.h, which, _ptr(out), out.size))
        return out

    def cutoffs(self):
        mx = C.c_double(0)
        n = self._chk(self.L.rxmd_hip_get_cutoffs(self.h, None, 0, C.byref(mx)))
        rc = np.zeros(n)
        self._chk(self.L.rxmd_hip_get_cutoffs(self.h, _ptr(rc), n, C.byref(mx)))
        return rc, mx.value

    def debug(self, what, width=1, cap=None):
        cap = cap or (self.stats()["nbuffer"] * width)
        out = np.zeros(cap)
        n = self._chk(self.L.rxmd_hip_debug_get(self.h, what, _ptr(out), cap))
        out = out[:n * width]
        return out.reshape(n, width) if width > 1 else out
