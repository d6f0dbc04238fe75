"""world_size-2/3 gloo tests of the N>1 plumbing on CPU: the transport callbacks the engine drives its six-stage
exchange with (C-ABI contract checked by rxmd_host_comm_selftest with host buffers), and the domain decomposition."""
import os
import numpy as np
import pytest

import oracle_api as oa
from rxmd_amd import system
import mr_worker
from ranks import run_ranks


@pytest.mark.parametrize("world", [2, 3])
def test_transport_contract_over_gloo(world):
    for r, (rc, nex, nar, err) in enumerate(run_ranks(mr_worker.transport_selftest, world, timeout=120, gpu=False)):
        assert rc == 0, (r, rc, err)
        assert nex == 6 and nar == 1


def test_domain_decomposition_matches_reference_rank_grid():
    """vprocs grid, per-rank atom sets and the six partners exactly as reference src/init.F90:74-100 / geninit.F90:495-527"""
    names, frac, lat = system.read_xyz(os.path.join(oa.INP, "rdx.xyz"))
    ff = os.path.join(oa.INP, "ffield_rdx")
    g = np.load(os.path.join(oa.GOLD, "rdx222_v222_tight.npz"))
    allg = []
    for r in range(8):
        lat_s, rec = system.geninit(ff, names, frac, lat, mc=(2, 2, 2), vprocs=(2, 2, 2), myid=r)
        gid = np.rint((rec[:, 7] - np.rint(rec[:, 7])) * 1e13).astype(np.int64)
        assert np.array_equal(gid, g["gid_%d" % r])          # the real MPI reference saw the same atoms on the same ranks, same order
        assert (rec[:, :3] > 0).all() and (rec[:, :3] <= 0.5 + 1e-12).all()
        allg.append(gid)
    assert np.array_equal(np.sort(np.concatenate(allg)), np.arange(1, 1345))
