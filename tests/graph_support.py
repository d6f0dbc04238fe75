"""Support module (pytest does not collect it): what the tests of the device graphs, of the VJP and of the structure statistics, the ranks they spawn
and the CPU test of the structure reference share -- engines of the named systems, the brute-force radius graph, the count-then-fill calls into
sentinel-filled tensors, the table look-up that an exported matrix entry is held to, and the oracle reference of the torch front end.  The bounds are
derived in the docstring of tests/test_gpu_pair_graph.py."""
import math

import numpy as np
import torch

import oracle_api as oa
import offlattice_systems as ol
from npt_reference import hmat
from parity import _engine, _oracle, rec10

DEV = "cuda:0"
SENT_I, SENT_F = -777, -777.25                    # what the output buffers hold before a call
KW5 = dict(QEq_tol=1e-300, NMAXQEq=5)             # five fixed CG iterations, as test_gpu_offlattice runs its boxes (the list needs no charges)
TIGHT = dict(QEq_tol=1e-12, NMAXQEq=2000)
CUTS = (3.0, 6.5, 9.5)
EDGES = {                                          # directed edges at 3.0 / 6.5 / 9.5 A, from the brute force on the CPU
    "rdx168": (1722, 19676, 61488),
    "mos2_tri324": (3888, 64152, 190512),
    "rdx-shaken": (13946, 157114, 493878),
    "rdx-denser": (37132, 375960, 1176296),
    "rdx-dilute": (3058, 39404, 117128),
    "rdx168-z9.42": (1998, 22400, 70374),         # rdx168 with its z edge shortened to 0.88 x 10.71 = 9.42 A: at 9.5 A an atom meets its own image
}


def _make(case, **kw):
    """a fresh engine of a named system with its atoms set"""
    if case in ol.SYSTEMS:
        import rxmd_amd
        ff, lat2, ranks, v = ol.build(case)
        kw = dict(KW5, **kw)
        e = rxmd_amd.RxmdEngine(ff, lat2, **kw)
        e.set_atoms_rxff(rec10(ranks[0]))
        return e
    if case == "rdx168-z9.42":
        # the engine accepts any local box above the bond cut-off (Engine::check_lattice); its ghost shell holds ONE image per direction, so the list
        # is the complete radius graph for r_cut up to the shortest edge, and beyond it as long as no pair needs an image two boxes away -- which
        # the brute force (it walks |n| <= 2 here) confirms for this configuration at 9.5 A
        import rxmd_amd
        from rxmd_amd import system
        ff, names, frac, lat = oa.make_system("rdx168")
        lat3, rec = system.geninit(ff, names, frac, [lat[0], lat[1], 0.88 * lat[2]] + list(lat[3:6]))
        e = rxmd_amd.RxmdEngine(ff, lat3, **dict(KW5, **kw))
        e.set_atoms_rxff(rec)
        return e
    mc = {"mos2_tri324": (3, 3, 2), "ice644": (6, 4, 4)}.get(case, (1, 1, 1))
    return _engine(case, mc, **kw)


def rebuild(e):
    """a second list build at the same positions: the first build of an engine always writes the 4-byte entries (it has no earlier windows to count
    on, lists.hip: needs_nb10); from the second on the default leaves them out and the partners come from the window slots.  FORCE behind QEq
    does not build again; set_charges invalidates the lists and keeps the windows' standing."""
    e.set_charges(e.atoms()["q"]); e.QEq(); e.FORCE()
    return bool(e.debug(15, cap=2)[0])             # did this build write the entries?


def brute_force(pos, lat, r_max):
    """every (src, dst, n1, n2, n3) with |pos[dst] + n H - pos[src]| <= r_max, i != j or n != 0 -> (keys [M, 5] int64, vec [M, 3], dist [M]), sorted by key"""
    H = hmat(lat)
    Hi = np.linalg.inv(H)
    reach = [int(math.ceil(r_max * np.linalg.norm(Hi[a]))) for a in range(3)]
    n = len(pos)
    keys, vecs = [], []
    for n1 in range(-reach[0], reach[0] + 1):
        for n2 in range(-reach[1], reach[1] + 1):
            for n3 in range(-reach[2], reach[2] + 1):
                t = H @ np.array([n1, n2, n3], dtype=np.float64)
                d = (pos[None, :, :] + t[None, None, :]) - pos[:, None, :]           # [src, dst, 3]
                r2 = (d * d).sum(axis=2)
                ok = r2 <= r_max * r_max * (1.0 + 1e-9)
                if n1 == 0 and n2 == 0 and n3 == 0:
                    ok[np.arange(n), np.arange(n)] = False
                s, t_ = np.nonzero(ok)
                keys.append(np.stack([s, t_, np.full_like(s, n1), np.full_like(s, n2), np.full_like(s, n3)], axis=1))
                vecs.append(d[s, t_])
    keys = np.concatenate(keys).astype(np.int64); vecs = np.concatenate(vecs)
    o = np.lexsort(keys.T[::-1])
    keys, vecs = keys[o], vecs[o]
    return keys, vecs, np.linalg.norm(vecs, axis=1)


def _select(bf, r_cut):
    keys, vecs, dist = bf
    gap = np.abs(dist - r_cut).min()
    assert gap > 1e-8, "a brute-force distance lies %.2e A from r_cut %.1f: rounding could move an edge" % (gap, r_cut)
    keep = dist <= r_cut
    return keys[keep], vecs[keep], gap


def device_coo(e, r_cut, as_gid=False, capacity=None, want=(True, True, True)):
    """count, then fill sentinel-filled tensors of `capacity` (default: exactly E) -> (E, src, dst, shift [., 3], vec [., 3], hval) as numpy"""
    E = e.pairs_device(0, 0, 0, r_cut=r_cut, as_gid=as_gid)
    cap = E if capacity is None else capacity
    src = torch.full((cap,), SENT_I, dtype=torch.int64, device=DEV); dst = torch.full_like(src, SENT_I)
    shift = torch.full((cap, 3), SENT_I, dtype=torch.int32, device=DEV)
    vec = torch.full((cap, 3), SENT_F, dtype=torch.float64, device=DEV)
    hv = torch.full((cap,), SENT_F, dtype=torch.float64, device=DEV)
    got = e.pairs_device(cap, src.data_ptr(), dst.data_ptr(), shift_ptr=shift.data_ptr() if want[0] else 0, vec_ptr=vec.data_ptr() if want[1] else 0,
                         h_ptr=hv.data_ptr() if want[2] else 0, r_cut=r_cut, as_gid=as_gid, stream=torch.cuda.current_stream().cuda_stream)
    assert got == E, (got, E)
    return E, src.cpu().numpy(), dst.cpu().numpy(), shift.cpu().numpy(), vec.cpu().numpy(), hv.cpu().numpy()


# ---- hval entry by entry ------------------------------------------------------------------------------------------------------------------------
EPS = np.finfo(np.float64).eps
RCTAP = 10.0                                       # the taper cut-off of plain QEq (init.F90:28-34)


def qeq_table(o, ff):
    """what an entry of the QEq matrix is looked up in: the oracle's TBL_Eclmb_QEq (Oracle.table(4): row inxn - 1, column i - 1 of the node i = 1..NTABLE)
    and the row of a pair of types, inxn2, read from the bond section of the ffield as rxmd_oracle.c:186-206 reads it (bond `ih` of the file serves
    the two types its line starts with).  The oracle hands out the table only; UDR, UDRi and rctap2 are formed as it forms them (rxmd_oracle.c:316,1894)."""
    T = o.table(4)
    lines = open(ff).read().split("\n")
    npar = int(lines[1].split()[0])
    nso = int(lines[2 + npar].split()[0])
    at = 2 + npar + 4 + 4 * nso                    # the line with the number of bonds; one more header line, then two lines per bond
    nboty = int(lines[at].split()[0])
    assert nboty == T.shape[0]
    inxn2 = np.zeros((nso + 1, nso + 1), dtype=np.int64)
    for ih in range(1, nboty + 1):
        ta, tb = int(lines[at + 2 * ih][0:3]), int(lines[at + 2 * ih][3:6])
        inxn2[ta, tb] = inxn2[tb, ta] = ih
    rctap2 = RCTAP * RCTAP
    UDR = rctap2 / T.shape[1]
    return dict(T=T, inxn2=inxn2, UDR=UDR, UDRi=1.0 / UDR, rctap2=rctap2)


FORMS = ((False, False), (True, False), (False, True), (True, True))


def _two_product(a, b):
    """a b = p + e exactly, p the rounded product (Dekker; Veltkamp's split at 2^27 + 1)"""
    split = lambda x: (lambda c: (c - (c - x), x - (c - (c - x))))(134217729.0 * x)
    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def hval_of_r2(tab, r2f, inxn, form=(False, False)):
    """qeq_initialize's entry for REAL(4) squared distances r2f (qeq.F90:191,222-240 as rxmd_oracle.c:659-669 restates it), in numpy doubles:
    a = r2 - itb UDR, t = a UDRi, h = (1 - t) T[itb] + t T[itb + 1].  form = (f1, f2): which of the two products a compiler has contracted into the
    subtraction behind it (an FMA: one rounding instead of two) -- f1: r2 - itb UDR, f2: 1 - a UDRi.  The contracted results are formed here from
    Dekker's exact product: r2 - (rounded product) is exact (the two lie within a factor of two), 1 - (rounded product) is followed by its exact
    rounding error (TwoSum), so one rounding remains in either."""
    r2 = r2f.astype(np.float64)
    itb = (r2 * tab["UDRi"]).astype(np.int64)
    p, pe = _two_product(itb.astype(np.float64), np.float64(tab["UDR"]))
    a = ((r2 - p) - pe) if form[0] else (r2 - p)
    t, te = _two_product(a, np.float64(tab["UDRi"]))
    one_t = 1.0 - t
    if form[1]:
        bb = one_t - 1.0
        one_t = one_t + (((1.0 - (one_t - bb)) + (-t - bb)) - te)
    inside = (r2 < tab["rctap2"]) & (inxn != 0)
    assert (itb[inside] >= 1).all() and (itb[inside] < tab["T"].shape[1]).all()
    row, col = np.where(inside, inxn - 1, 0), np.where(inside, itb, 1)
    h = one_t * tab["T"][row, col - 1] + t * tab["T"][row, col]
    return np.where(inside, h, 0.0)


def check_hval_entries(vec, hv, ti, tj, tab, label, f32=False, form=None):
    """every exported value against the table look-up at float32(|vec|^2), |vec|^2 formed from the exported vec3.
    Bound 8 eps |h|: the kernel and this reference both interpolate as (1 - t) T[itb] + t T[itb + 1] (lists.hip, k_list10), three rounded operations on
    either side, and the two terms have one sign.  With the fp32 stream the reference is float64(float32(h)), exact.
    That count of roundings holds only when both sides round the SAME intermediate results, and in two places of this expression it matters far above
    the bound whether a product is rounded before the subtraction behind it: itb UDR ~ r2 carries eps r2 / 2, which UDRi turns into up to 2,500 eps in t
    and the slope of the table into tens of eps |h| (11 measured against the uncontracted form at 9.46 A); and towards the end of the taper, where
    T[itb + 1] -> 0 and t -> 1, the rounding of t is eps / 2 against 1 - t (9 eps |h| measured at r^2 = 99.9997).  hipcc contracts such products into
    FMAs; a compiler may also leave them.  So the reference is evaluated in the four forms of the same expression (hval_of_r2: each of the two
    products contracted or not), and ONE form must hold every entry of a system to 8 eps |h|: with form=None the form with the fewest misses, then
    the smallest largest error, is taken, printed and returned; a caller with several calls on one system (one per rank: one kernel build) hands
    the form of the first call to the others.  (Contracting the last line as well moves h by less than 2 eps.)
    The kernel may contract d0^2 + d1^2 + d2^2 into FMAs too: an entry whose double |vec|^2 lies within 4 ulp of the midpoint between two floats may
    match the look-up at either of them; at most 2 entries per SYSTEM may (expected ~1e-3 of one): asserted here per call, and by a caller with
    several calls on the sum of the returned counts.
    -> (largest error in units of eps |h|, entries that used the escape, the form)"""
    r2d = (vec * vec).sum(axis=1)
    r2f = r2d.astype(np.float32)
    inxn = tab["inxn2"][ti, tj]
    held = np.ones(len(hv), dtype=bool)

    def ref_at(r2f_, inxn_, form):
        h = hval_of_r2(tab, r2f_, inxn_, form)
        return h.astype(np.float32).astype(np.float64) if f32 else h

    def misses(form):
        ref = ref_at(r2f, inxn, form)
        err = np.abs(hv - ref)
        return ref, err, held & (err > (0.0 if f32 else 8 * EPS * np.abs(ref)))

    def rank(f):                                   # fewest entries beyond the bound, then the smallest largest error
        ref_, err_, bad_ = misses(f)
        nz_ = held & (ref_ != 0.0)
        return int(bad_.sum()), float((err_[nz_] / np.abs(ref_[nz_])).max()) if nz_.any() else 0.0

    if form is None:
        form = min(FORMS, key=rank)
    ref, err, bad = misses(form)
    escapes = 0
    for k in np.nonzero(bad)[0]:
        ok = False
        for nb in (np.nextafter(r2f[k], np.float32(-np.inf)), np.nextafter(r2f[k], np.float32(np.inf))):
            mid = 0.5 * (float(r2f[k]) + float(nb))
            if abs(r2d[k] - mid) <= 4 * np.spacing(r2d[k]):
                alt = ref_at(np.array([nb], dtype=np.float32), inxn[k:k + 1], form)[0]
                if abs(hv[k] - alt) <= (0.0 if f32 else 8 * EPS * abs(alt)):
                    ok = True; err[k] = abs(hv[k] - alt); ref[k] = alt
        assert ok, "%s: entry %d, |vec|^2 %.17g: hval %.17g, the table gives %.17g (form %s, %d entries beyond the bound)" % (label, k, r2d[k], hv[k], ref[k], form, int(bad.sum()))
        escapes += 1
    nz = held & (ref != 0.0)
    worst = (err[nz] / np.abs(ref[nz])).max() / EPS if nz.any() else 0.0
    print("%s: %d entries held, %d of them zero, max |hval - table| %.2f eps |h|%s, products contracted (r2 - itb UDR, 1 - a UDRi): %s, "
          "entries matched at the neighbouring float %d" % (label, int(held.sum()), int((held & (ref == 0.0)).sum()), worst, " (fp32 stream: exact)" if f32 else "", form, escapes))
    assert (err[held & (ref == 0.0)] == 0.0).all()
    assert escapes <= 2
    return worst, escapes, form


# ---- the bond-order graph -----------------------------------------------------------------------------------------------------------------------
def _offlattice_engine(name, **kw):
    import rxmd_amd
    ff, lat2, ranks, v = ol.build(name)
    e = rxmd_amd.RxmdEngine(ff, lat2, **kw)
    e.set_atoms_rxff(rec10(ranks[0]))
    return e


def _host_coo(e, bo_min=None):
    """the host path flattened row-major: (atoms, src gid, dst gid, bo)"""
    a = e.atoms()
    cnt, pg, bo = e.bonds()
    mask = np.arange(pg.shape[1])[None, :] < cnt[:, None]
    src, dst, b = np.repeat(a["gid"], cnt), pg[mask], bo[mask]
    if bo_min is not None:
        keep = b >= bo_min
        src, dst, b = src[keep], dst[keep], b[keep]
    return a, src, dst, b


def _device_coo(e, bo_min=0.0, as_gid=False, capacity=None):
    """count, then fill sentinel-filled torch tensors of `capacity` (default: exactly E) -> (E, src, dst, bo, parts [.,3], vec [.,3]) as numpy"""
    E = e.bonds_device(0, 0, 0, 0, bo_min=bo_min, as_gid=as_gid)
    cap = E if capacity is None else capacity
    src = torch.full((cap,), SENT_I, dtype=torch.int64, device=DEV); dst = torch.full_like(src, SENT_I)
    bo = torch.full((cap,), SENT_F, dtype=torch.float64, device=DEV)
    parts = torch.full((cap, 3), SENT_F, dtype=torch.float64, device=DEV); vec = torch.full_like(parts, SENT_F)
    got = e.bonds_device(cap, src.data_ptr(), dst.data_ptr(), bo.data_ptr(), bo3_ptr=parts.data_ptr(), vec_ptr=vec.data_ptr(), bo_min=bo_min, as_gid=as_gid,
                         stream=torch.cuda.current_stream().cuda_stream)
    assert got == E, (got, E)
    return E, src.cpu().numpy(), dst.cpu().numpy(), bo.cpu().numpy(), parts.cpu().numpy(), vec.cpu().numpy()


# ---- the oracle behind the torch front end (tests/test_gpu_device_eval.py) ------------------------------------------------------------------------
_REF = {}


def _lattice(case, mc):
    lat = oa.make_system(case)[3]
    return [lat[0] * mc[0], lat[1] * mc[1], lat[2] * mc[2]] + list(lat[3:6])


def _ref(case, mc):
    """the oracle at tight tolerance, once per system: positions, types, gids, charges, forces, energies, virial (arrays are read-only)"""
    if case not in _REF:
        o = _oracle(case, mc, **TIGHT); o.qeq(); o.force()
        r = dict(pos=o.pos().copy(), type=o.types().copy(), gid=o.gids().copy(), q=o.charges().copy(), f=o.forces().copy(), pe=o.energy().copy(),
                 astr=o.astr(reset=True).copy(), lat=_lattice(case, mc), ff=oa.make_system(case)[0])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[case] = r
    return _REF[case]


def _model(r, **kw):
    from rxmd_amd.torch_front import ReaxFF
    return ReaxFF(r["ff"], r["lat"], r["type"], gid=r["gid"], **kw)


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)
