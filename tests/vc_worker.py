"""rank functions of the two-rank barostat tests (tests/test_gpu_variable_cell.py, tests/test_gpu_variable_cell_oracle.py), started by ranks.run_ranks"""
import numpy as np

import ranks


def barostat_run(vp, rank, steps, attach=None):
    """rdx222 at 300 K, isotropic barostat coupling on every step: the lattice after each step and the rank-local energies at the end;
    then a set_lattice where rank 1 passes another lattice than rank 0"""
    import oracle_api as oa
    import rxmd_amd
    from rxmd_amd import system
    ff, names, frac, lat = oa.make_system("rdx222")
    lat_s, rec = system.geninit(ff, names, frac, lat, mc=(2, 2, 2), vprocs=vp, myid=rank)
    e = rxmd_amd.RxmdEngine(ff, lat_s, vprocs=vp, myid=rank, QEq_tol=1e-12, NMAXQEq=2000, device=0)
    if attach:
        attach(e)
    e.set_atoms_rxff(rec)
    e.thermostat(0, 300.0)
    a0 = e.atoms()                                       # the velocities this rank drew: the test hands them to the oracle
    e.QEq(); pe0 = e.FORCE()
    astr0 = e.energy()["astr"]                           # this rank's virial of the first FORCE (residents + ghosts before the fold)
    e.set_barostat(1, p0=0.0, tau_fs=25.0, bulk_modulus=15.0, every=1, max_strain=0.01)
    lattices, p6s = [], []
    for _ in range(steps):
        e.step(1)
        lattices.append(e.lattice); p6s.append(e.barostat_state()["p6"])
    e.QEq(); pe = e.FORCE()
    out = dict(lattices=lattices, pe=list(pe), pe0=list(pe0), astr0=list(astr0), p6=[list(x) for x in p6s], couplings=e.barostat_state()["couplings"],
               gid0=a0["gid"].tolist(), v0=a0["v"].tolist())
    if vp != (1, 1, 1):
        L = list(e.lattice)
        if rank == 1:
            L[0] *= 1.001
        try:
            e.set_lattice(L); out["mismatch_rc"] = 0
        except rxmd_amd.RxmdError as ex:
            out["mismatch_rc"] = ex.code
        out["lattice_after_mismatch"] = e.lattice
    e.close()
    return out


@ranks.entry
def barostat_rank(rank, world, steps):
    return barostat_run((2, 1, 1), rank, steps, attach=ranks.staged_transport().attach)


@ranks.entry
def npt_rank(rank, world, job):
    """one rank of a two-rank barostat run against the two-rank oracle (tests/test_gpu_variable_cell_oracle.py): rdx222 with the seeded
    velocities of the test, set to job["lattice"], job["nsteps"] steps under job["bar"] in one step() call or one call per step"""
    import oracle_api as oa
    import rxmd_amd
    from rxmd_amd import system
    from rxmd_amd.comm import TorchTransport

    class Counting(TorchTransport):                  # the largest message either way, in doubles
        biggest = 0

        def _exchange(self, ctx, to, send_ptr, nsend, frm, recv_ptr, cap):
            n = super()._exchange(ctx, to, send_ptr, nsend, frm, recv_ptr, cap)
            self.biggest = max(self.biggest, int(nsend), int(n)); return n

        def _exchange_known(self, ctx, to, send_ptr, nsend, frm, recv_ptr, nrecv):
            n = super()._exchange_known(ctx, to, send_ptr, nsend, frm, recv_ptr, nrecv)
            self.biggest = max(self.biggest, int(nsend), int(n)); return n

    cap = 1 << 20
    tr = ranks.staged_transport(cap, cls=Counting)
    vp = tuple(job["vp"])
    ff, names, frac, lat = oa.make_system("rdx222")
    lat_s, rec = system.geninit(ff, names, frac, lat, mc=(2, 2, 2), vprocs=vp, myid=rank)
    e = rxmd_amd.RxmdEngine(ff, lat_s, vprocs=vp, myid=rank, QEq_tol=1e-12, NMAXQEq=2000, device=0)
    tr.attach(e)
    e.set_atoms_rxff(rec)
    v = np.random.default_rng(job["seed"]).normal(0.0, job["sigma"], (1344, 3))     # the test's draw, in gid order
    e.set_velocities(v[e.atoms()["gid"] - 1])
    if list(job["lattice"]) != e.lattice:
        e.set_lattice(job["lattice"])
    e.QEq(); e.FORCE()
    b = job["bar"]
    e.set_barostat(b["mode"], p0=b["p0"], tau_fs=b["tau_fs"], bulk_modulus=b["bulk"], every=b.get("every", 1), max_strain=b.get("max_strain", 0.01), axes=b.get("axes", 7))
    st0 = e.stats()
    tr.biggest = 0
    lattices, p6s, mus = [], [], []
    for n in ([job["nsteps"]] if job["one_call"] else [1] * job["nsteps"]):
        e.step(n)
        s = e.barostat_state()
        lattices.append(e.lattice); p6s.append(list(s["p6"])); mus.append(list(s["mu"]))
    st1 = e.stats(); en = e.energy(); a = e.atoms()
    res = dict(rank=rank, lattices=lattices, p6=p6s, mu=mus, couplings=e.barostat_state()["couplings"], pe=list(en["PE"]), ke=float(en["KE"]),
               atoms={k: x.tolist() for k, x in a.items()}, cells3=[list(st0["cells3"]), list(st1["cells3"])],
               nbuffer=[int(st0["nbuffer"]), int(st1["nbuffer"])], xbuf_doubles=cap, max_message=int(tr.biggest),
               transport_error=repr(tr.error) if tr.error else None)
    e.close()
    return res
