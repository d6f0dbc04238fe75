"""worker of the two-rank barostat test (tests/test_gpu_variable_cell.py), spawned by torch.multiprocessing"""
import os, sys, traceback
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))


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
    e.QEq(); pe0 = e.FORCE()
    astr0 = e.energy()["astr"]                           # this rank's virial of the first FORCE (residents + ghosts before the fold)
    e.set_barostat(1, p0=0.0, tau_fs=25.0, bulk_modulus=15.0, every=1, max_strain=0.01)
    lattices, p6s = [], []
    for _ in range(steps):
        e.step(1)
        lattices.append(e.lattice); p6s.append(e.barostat_state()["p6"])
    e.QEq(); pe = e.FORCE()
    out = dict(lattices=lattices, pe=list(pe), pe0=list(pe0), astr0=list(astr0), p6=[list(x) for x in p6s], couplings=e.barostat_state()["couplings"])
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


def barostat_rank(rank, world, port, steps, out):
    try:
        import torch
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from rxmd_amd.comm import TorchTransport
        tr = TorchTransport(mode="staged", device=torch.device("cuda", 0), capacity_doubles=1 << 20)
        out[rank] = barostat_run((2, 1, 1), rank, steps, attach=tr.attach)
        dist.barrier(); dist.destroy_process_group()
    except Exception:
        out[rank] = dict(error=traceback.format_exc())
