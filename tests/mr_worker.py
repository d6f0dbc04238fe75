"""rank functions of the multi-process tests (started by ranks.run_ranks)"""
import os
import numpy as np

import ranks
from parity import slab_system, mode_velocities, rec10, _perturbed_rdx, KW


@ranks.entry
def transport_selftest(rank, world):
    from rxmd_amd.comm import TorchTransport
    t = TorchTransport(mode="host")
    rc = t.selftest()
    return (rc, t.n_exchange, t.n_allreduce, repr(t.error))


@ranks.entry
def engine_rank(rank, world, case, vp, steps):
    """one rank of a vprocs run; all ranks share GPU 0, messages are staged through the host over gloo"""
    import oracle_api as oa
    import rxmd_amd
    from rxmd_amd import system
    g = np.load(os.path.join(oa.GOLD, case + ".npz"))
    mc = tuple(int(x) for x in g["mc"])
    ff, names, frac, lat = oa.make_system(case)
    lat_s, rec = system.geninit(ff, names, frac, lat, mc=mc, vprocs=vp, myid=rank)
    e = rxmd_amd.RxmdEngine(ff, lat_s, vprocs=vp, myid=rank, QEq_tol=1e-12, NMAXQEq=2000, device=0)
    tr = ranks.staged_transport()
    if os.environ.get("MR_WORKER_NO_EXCHANGE_KNOWN") == "1":      # a host transport that has only `exchange` (the field is optional in rxmd_comm_ops)
        from rxmd_amd.comm import EXCHANGE_FN
        tr.ops.exchange_known = EXCHANGE_FN()
    tr.attach(e)
    e.set_atoms_rxff(rec)
    it, est = e.QEq()
    pe = e.FORCE()
    if steps:
        e.step(steps)
    a = e.atoms()
    st = e.stats()
    res = dict(gid=a["gid"], q=a["q"], f=a["f"], pos=a["pos"], iters=st["qeq_iters_last"], pe=pe, nex=tr.n_exchange, nar=tr.n_allreduce, err=repr(tr.error))
    e.close()
    return res


@ranks.entry
def engine_rank_empty(rank, world, steps, qeq_mode):
    """2x1x1 with an EMPTY second rank: it still takes part in every exchange round and all-reduce"""
    import rxmd_amd
    from rxmd_amd import system
    ff, names, frac, lat = slab_system()
    vp = (2, 1, 1)
    lat_s, rec = system.geninit(ff, names, frac, lat, vprocs=vp, myid=rank)
    e = rxmd_amd.RxmdEngine(ff, lat_s, vprocs=vp, myid=rank, QEq_tol=1e-12, NMAXQEq=2000, device=0, qeq_mode=qeq_mode, nbuffer=20000)
    tr = ranks.staged_transport()
    tr.attach(e)
    e.set_atoms_rxff(rec)
    n0 = len(rec)
    e.QEq(); pe = e.FORCE()
    if steps:
        e.step(steps)
    a = e.atoms()
    res = dict(n0=n0, gid=a["gid"], q=a["q"], f=a["f"], pos=a["pos"], pe=pe, err=repr(tr.error))
    e.close()
    return res


@ranks.entry
def engine_rank_rccl(rank, world, case, vp, steps, qeq_mode):
    """one rank of a vprocs run on ITS OWN GPU (device = rank) with the engine's native RCCL transport; gloo only carries the 128-byte id"""
    import torch
    import torch.distributed as dist
    import oracle_api as oa
    import rxmd_amd
    from rxmd_amd import system
    g = np.load(os.path.join(oa.GOLD, case + ".npz"))
    mc = tuple(int(x) for x in g["mc"])
    ff, names, frac, lat = oa.make_system(case)
    lat_s, rec = system.geninit(ff, names, frac, lat, mc=mc, vprocs=vp, myid=rank)
    e = rxmd_amd.RxmdEngine(ff, lat_s, vprocs=vp, myid=rank, QEq_tol=1e-12, NMAXQEq=2000, device=rank, qeq_mode=qeq_mode)
    idt = torch.zeros(128, dtype=torch.uint8)
    if rank == 0:
        idt.copy_(torch.frombuffer(bytearray(e.rccl_unique_id()), dtype=torch.uint8))
    dist.broadcast(idt, 0)
    e.init_rccl(bytes(idt.numpy().tobytes()), rank, world)
    e.set_atoms_rxff(rec)
    it, est = e.QEq()
    pe = e.FORCE()
    if steps:
        e.step(steps)
    a = e.atoms()
    st = e.stats()
    res = dict(gid=a["gid"], q=a["q"], f=a["f"], pos=a["pos"], iters=st["qeq_iters_last"], pe=pe, nghost=st["nghost_force"])
    e.close()
    return res


@ranks.entry
def engine_rank_perturbed(rank, world, vp, steps, qeq_mode):
    """one rank of the 36,288-atom perturbed RDX system of tests/test_gpu_scale.py; all ranks share GPU 0, messages staged over gloo"""
    import rxmd_amd
    ff, lat2, recs, vs = _perturbed_rdx(vp)
    e = rxmd_amd.RxmdEngine(ff, lat2, vprocs=vp, myid=rank, device=0, qeq_mode=qeq_mode, **KW)
    tr = ranks.staged_transport(1 << 22)
    tr.attach(e)
    e.set_atoms_rxff(rec10(recs[rank], vs[rank]))
    e.QEq(); e.FORCE()
    if steps:
        e.step(steps)
    a = e.atoms(); st = e.stats()
    res = dict(gid=a["gid"], q=a["q"], f=a["f"], pos=a["pos"], natoms=st["natoms"], n_boundary_rows=st["n_boundary_rows"], err=repr(tr.error))
    e.close()
    return res


@ranks.entry
def engine_rank_mode(rank, world, spec):
    """one rank of a vprocs run in any MODE of the driver (round 6: PQEq, isQEq 2, the velocity-scaling modes, the electric field) -- all
    ranks share GPU 0, messages host-staged over gloo.  spec: dict(case, mc, vp, steps, pqeq, isQEq, efield, qeq_mode, thermo=(mode, kw, every),
    restart=<golden with restart_rxff>, v=(seed, sigma, natoms of the whole system), kw=engine keywords)"""
    import oracle_api as oa
    import rxmd_amd
    from rxmd_amd import system
    vp = tuple(spec["vp"])
    kw = dict(spec["kw"]) if "kw" in spec else dict(QEq_tol=1e-12, NMAXQEq=2000)
    if spec.get("restart"):
        g = np.load(os.path.join(oa.GOLD, spec["restart"] + ".npz"))
        ff = oa.make_system(spec["case"])[0]
        lat_s, vp_file, _, recs = oa.parse_rxff(g["restart_rxff"])
        assert tuple(vp_file) == vp
        rec = recs[rank]
    else:
        ff, names, frac, lat = oa.make_system(spec["case"])
        lat_s, rec = system.geninit(ff, names, frac, lat, mc=tuple(spec["mc"]), vprocs=vp, myid=rank)
        if spec.get("v"):
            ty = np.rint(rec[:, 7]).astype(np.int64); gid = np.rint((rec[:, 7] - ty) * 1e13).astype(np.int64)
            rec[:, 3:6] = mode_velocities(gid, *spec["v"])
    e = rxmd_amd.RxmdEngine(ff, lat_s, vprocs=vp, myid=rank, device=0, qeq_mode=spec.get("qeq_mode", 1), isQEq=spec.get("isQEq", 1),
                            pqeq=oa.PQEQ_SICNP if spec.get("pqeq") else None, efield=spec.get("efield"), **kw)
    tr = ranks.staged_transport(1 << 21)
    tr.attach(e)
    e.set_atoms_rxff(rec)
    e.QEq(); pe = e.FORCE()
    a0 = e.atoms(); sh0 = e.shells() if spec.get("pqeq") else None          # the state after the pre-loop QEq + FORCE (main.F90:27-32)
    th = spec.get("thermo")
    for n in range(spec.get("steps", 0)):
        if th and n % th[2] == 0:
            e.thermostat(th[0], **th[1])
        e.step(1)
    a = e.atoms(); st = e.stats()
    res = dict(gid0=a0["gid"], q0=a0["q"], f0=a0["f"], pos0=a0["pos"], shells0=sh0,
               gid=a["gid"], q=a["q"], f=a["f"], pos=a["pos"], v=a["v"], pe=pe, shells=e.shells() if spec.get("pqeq") else None,
               iters=st["qeq_iters_last"], nghost=st["nghost_force"], nex=tr.n_exchange, nar=tr.n_allreduce, err=repr(tr.error))
    e.close()
    return res
