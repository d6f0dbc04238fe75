"""Multi-rank runs of the HIP engine against the REAL MPI reference at the same vprocs (the reference's
forces depend on the decomposition, so N-rank results are compared with the MPI run, not with the 1-rank run).
All ranks share the single GPU of the test box; messages travel host-staged over gloo, so this exercises the engine's
staged exchange (ghost build, vector halos, force return, migration, all-reduces) exactly as the RCCL transport does."""
import os
import numpy as np
import pytest

import oracle_api as oa
import mr_worker
from ranks import run_ranks
from parity import _engine, _oracle, q_err, f_err, slab_system

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,steps,win", [("rdx222_v211_tight", 0, "1"), ("rdx222_v222_tight", 0, "1"), ("rdx222_v222_md3", 3, "1"), ("rdx222_v222_md3", 3, "0"),
                                            ("example2_v211_md3", 3, "1"), ("example2_v211_md3", 3, "0")])   # example2: the reference's examples/2-reaxff-dc (mc 4 3 5, -v 2 1 1, 2 ranks)
def test_vprocs_parity_vs_mpi_reference(case, steps, win, monkeypatch):
    """win "1": the default window pass; "0": the wavefront-per-row pass (RXMD_SPMV_WIN=0), which keeps the iteration-count gate of 25 % it had before
    the window pass existed.  The window pass stops the LAST step of example2 after 32 iterations where the reference's own run took 47 (its re-ordering
    spread is 31..39 of 35 at step 0): that the earlier exit is REAL(4) noise on the relative-change test of qeq.F90:115 and not another operator is what
    test_window_pass_and_row_pass_are_the_same_operator shows iteration by iteration on the Est trace; its gate here is wider for that reason only."""
    monkeypatch.setenv("RXMD_SPMV_WIN", win)
    g = np.load(os.path.join(oa.GOLD, case + ".npz"))
    vp = tuple(int(x) for x in g["vprocs"]); world = vp[0] * vp[1] * vp[2]
    res = run_ranks(mr_worker.engine_rank, world, case, vp, steps, timeout=600)
    for r, o in enumerate(res):
        assert o["err"] == "None"
        assert np.array_equal(o["gid"], g["gid_%d" % r])
        qref, fref = g["charge_%d" % r], g["force_%d" % r]
        assert q_err(o["q"], qref) <= 1e-6
        assert f_err(o["f"], fref) <= (1e-6 if steps == 0 else 1e-5)
        assert np.abs(o["pos"] - g["pos_%d" % r]).max() <= 1e-8
        # the exit iteration moves with the summation order (the reference itself goes 35 -> 31..39 under atom
        # re-ordering): same neighbourhood, not the same count; charges and forces above are the gate
        # (round 3: 32 against the reference's 47 in the last step of example2 with the window pass -- the relative-change test of qeq.F90:115
        #  fires by chance; the charges of that step agree to 1e-6 all the same)
        assert abs(o["iters"] - int(g["qeq_iters"][-1])) <= (0.25 if win == "0" else 0.4) * int(g["qeq_iters"][-1])
        assert o["nex"] > 0 and o["nar"] > 0


@pytest.mark.parametrize("case,steps", [("rdx222_v222_md3", 3), ("example2_v211_md3", 3)])
def test_direct_vector_halo_vs_mpi_reference(case, steps, monkeypatch):
    """RXMD_HALO_DIRECT=1: every ghost value of a QEq vector / charge halo comes straight from the rank that owns the atom (owner rank and
    owner index travel with the ghost build, one request phase per build, then ONE exchange with all peers per halo) instead of the
    reference's x -> y -> z forwarding (comm.F90:68-86).  8 ranks of a 2 x 2 x 2 grid have 7 distinct peers each; the messages go through
    the host-staged callbacks (np - 1 shifted send_recv rounds).  Same goldens of the real MPI reference as the staged halo: per-rank
    order, charges, forces, positions after 3 MD steps."""
    monkeypatch.setenv("RXMD_HALO_DIRECT", "1")
    test_vprocs_parity_vs_mpi_reference(case, steps, "1", monkeypatch)


@pytest.mark.parametrize("case,steps", [("rdx222_v222_md3", 3), ("example2_v211_md3", 3)])
def test_one_round_per_stage_between_ranks_vs_mpi_reference(case, steps, monkeypatch):
    """RXMD_NO_STAGE_PAIRS=1 between REAL ranks: ghost build, migration, vector halos and the force fold walk the six stages one message per
    round, as the reference does (comm.F90:68-86) -- 8 ranks with corner forwarding, 2 ranks with migration.  Same goldens of the real MPI
    reference and the same gates as the paired walk."""
    monkeypatch.setenv("RXMD_NO_STAGE_PAIRS", "1")
    test_vprocs_parity_vs_mpi_reference(case, steps, "1", monkeypatch)


def test_transport_without_exchange_known_vs_mpi_reference(monkeypatch):
    """A host whose rxmd_comm_ops has a null exchange_known (mr_worker hands the struct over that way): ghost build and migration keep their paired
    rounds (two `exchange` calls per round), vector halos and the force fold fall back to one `exchange` call per stage with the buffer capacity.
    2 ranks with migration, same golden and gates."""
    monkeypatch.setenv("MR_WORKER_NO_EXCHANGE_KNOWN", "1")
    test_vprocs_parity_vs_mpi_reference("example2_v211_md3", 3, "1", monkeypatch)


@pytest.mark.parametrize("case,steps,qeq_mode", [("rdx222_v211_tight", 0, 0), ("example2_v211_md3", 3, 1)])
def test_native_rccl_with_real_peers_vs_mpi_reference(case, steps, qeq_mode):
    """The native transport with REAL peers: one process per GPU, ncclSend/ncclRecv/ncclAllReduce between two MI355X (runs only on a
    box that shows at least two devices; the 1-GPU test boxes exercise the same code as a self loop and through the host-staged
    callbacks).  2 x 1 x 1 against the real-MPI reference at the same vprocs: per-rank local order, charges, forces, positions."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: the RCCL peer-to-peer path cannot run with both ranks on one device")
    g = np.load(os.path.join(oa.GOLD, case + ".npz"))
    vp = tuple(int(x) for x in g["vprocs"]); world = 2
    res = run_ranks(mr_worker.engine_rank_rccl, world, case, vp, steps, qeq_mode, timeout=900)
    for r, o in enumerate(res):
        assert np.array_equal(o["gid"], g["gid_%d" % r])
        qref, fref = g["charge_%d" % r], g["force_%d" % r]
        assert q_err(o["q"], qref) <= 1e-6
        assert f_err(o["f"], fref) <= (1e-6 if steps == 0 else 1e-5)
        assert np.abs(o["pos"] - g["pos_%d" % r]).max() <= 1e-8
        assert o["nghost"] > 0


@pytest.mark.parametrize("qeq_mode", [0, 1])
def test_a_rank_that_owns_no_atom(qeq_mode):
    """ragged decomposition: all 168 atoms in the lower half of the box, rank 1 of 2x1x1 is EMPTY (zero residents, ghosts only) and must
    still answer every exchange round and all-reduce; compared per rank with the multi-rank oracle, energies with the global sums"""
    ff, names, frac, lat = slab_system()
    lat_s, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), vprocs=(2, 1, 1))
    assert [len(r["type"]) for r in ranks] == [168, 0]
    o = oa.Oracle(ff, lat_s, ranks, vprocs=(2, 1, 1), QEq_tol=1e-12, NMAXQEq=2000, nbuffer=20000)
    o.qeq(); o.force(); pe_ref = o.energy()
    res = run_ranks(mr_worker.engine_rank_empty, 2, 0, qeq_mode, timeout=600)
    for r, x in enumerate(res):
        assert x["err"] == "None"
    assert res[0]["n0"] == 168 and res[1]["n0"] == 0 and len(res[1]["gid"]) == 0
    assert np.array_equal(res[0]["gid"], o.gids(0))
    qref, fref = o.charges(0), o.forces(0)
    assert q_err(res[0]["q"], qref) <= 1e-6
    assert f_err(res[0]["f"], fref) <= 1e-6
    pe = np.array(res[0]["pe"]) + np.array(res[1]["pe"])           # rank-local energies; the oracle reports the global sums
    assert max(abs(a - b) / abs(b) for a, b in zip(pe, pe_ref) if abs(b) > 1e-6) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("qeq_mode,overlap,direct", [(0, True, False), (1, True, False), (1, False, False), (1, True, True), (1, False, True)])
def test_native_rccl_transport_self_loop(qeq_mode, overlap, direct, monkeypatch):
    """The native transport (rccl_comm.hip: ncclSend/ncclRecv/ncclAllReduce on the engine's stream) on ONE GPU: a single rank is
    pushed through the staged six-stage exchange (RXMD_FORCE_STAGED) and every message through RCCL send/recv to itself
    (RXMD_FORCE_REMOTE) -- the code path of vprocs > 1 minus the wire.  Must reproduce the single-rank oracle trajectory."""
    monkeypatch.setenv("RXMD_FORCE_STAGED", "1")
    monkeypatch.setenv("RXMD_FORCE_REMOTE", "1")
    if not overlap:          # default: the (hs,ht) halo runs on a second stream under the interior rows of the matrix pass (qeq_mode 1)
        monkeypatch.setenv("RXMD_NO_HALO_OVERLAP", "1")
    if direct:               # the direct vector halo (one grouped RCCL exchange; here the only peer is the rank itself)
        monkeypatch.setenv("RXMD_HALO_DIRECT", "1")
    kw = dict(QEq_tol=1e-12, NMAXQEq=2000)
    e = _engine("rdx222", (2, 2, 2), qeq_mode=qeq_mode, **kw)
    e.init_rccl(e.rccl_unique_id(), 0, 1)
    o = _oracle("rdx222", (2, 2, 2), **kw)
    e.QEq(); e.FORCE(); o.qeq(); o.force()
    e.step(3); o.step(3)
    a = e.atoms()
    assert np.array_equal(a["gid"], o.gids())
    assert q_err(a["q"], o.charges()) <= 1e-6
    assert f_err(a["f"], o.forces()) <= 1e-6
    assert np.abs(a["pos"] - o.pos()).max() <= 1e-9
    e.close()


@pytest.mark.gpu
def test_pqeq_through_the_multi_rank_path_self_loop(monkeypatch):
    """PQEq on the vprocs > 1 code path (staged exchange + RCCL self send/recv): shell positions and charges travel as halos,
    the shell displacement migrates with its atom (14 doubles per record, comm.F90:153,165-167); against the clean oracle"""
    monkeypatch.setenv("RXMD_FORCE_STAGED", "1")
    monkeypatch.setenv("RXMD_FORCE_REMOTE", "1")
    kw = dict(QEq_tol=1e-12, NMAXQEq=2000)
    e = _engine("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP, qeq_mode=1, **kw)
    e.init_rccl(e.rccl_unique_id(), 0, 1)
    o = _oracle("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP, **kw); o.set_pqeq_clean(1)
    e.QEq(); e.FORCE(); o.qeq(); o.force()
    e.step(3); o.step(3)
    a = e.atoms()
    ie = np.argsort(a["gid"]); io = np.argsort(o.gids())
    assert np.abs(a["pos"][ie] - o.pos()[io]).max() <= 1e-9
    assert q_err(a["q"][ie], o.charges()[io]) <= 1e-6
    assert f_err(a["f"][ie], o.forces()[io]) <= 1e-6
    assert np.abs(e.shells()[ie] - o.spos()[io]).max() <= 1e-7
    e.close()


# ---- round 6: every MODE of the driver between DISTINCT ranks (until now only plain isQEq 1 had left a self loop) ---------------------------------
def _run_ranks(spec, world, timeout=900):
    res = run_ranks(mr_worker.engine_rank_mode, world, spec, timeout=timeout)
    for o in res:
        assert o["err"] == "None"
        assert o["nex"] > 0 and o["nar"] > 0 and o["nghost"] > 0
    return res


def _rank_errs(q, f, qref, fref):
    return q_err(q, qref), f_err(f, fref)


@pytest.mark.parametrize("vp,direct", [((2, 1, 1), False), ((2, 1, 1), True), ((2, 2, 2), False), ((2, 2, 2), True)])
def test_pqeq_between_ranks_vs_mpi_reference_and_clean_oracle(vp, direct, monkeypatch):
    """PQEq with shells crossing REAL rank boundaries (BASELINE configs[4] is PQEq on 8 GPUs): the SiC nanoparticle replicated to one
    particle per rank, 2 ranks on 2 x 1 x 1 and 8 on 2 x 2 x 2 (edge and corner ranks forward the shell halo x -> y -> z, comm.F90:68-86,
    129-131).  (i) the state after the pre-loop PQEq + FORCE against `mpiexec rxmd_mpi --pqeq` at the same vprocs (every shell on its core:
    the reference has no beyond-cut-off look-up there), per rank: local order, charges, forces <= 1e-6; (ii) 3 MD steps -- a plane of 36 atoms
    sits 3e-8 A inside the x boundary and MIGRATES to the other rank in the first step, taking its shell displacement along (14 doubles per
    MOVE record, comm.F90:153,165-167) -- against the multi-rank CLEAN oracle, per rank: local order, positions, charges,
    forces <= 1e-6, shell displacements <= 1e-7.  direct = RXMD_HALO_DIRECT=1 (every ghost value straight from its owner)."""
    if direct:
        monkeypatch.setenv("RXMD_HALO_DIRECT", "1")
    world = vp[0] * vp[1] * vp[2]
    case = "sicnp%d%d%d_v%d%d%d_pqeq_tight" % (vp + vp)
    g = np.load(os.path.join(oa.GOLD, case + ".npz"))
    res = _run_ranks(dict(case="sicnp", mc=vp, vp=vp, steps=3, pqeq=True), world)
    ff, names, frac, lat = oa.make_system("sicnp")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=vp, vprocs=vp)
    o = oa.Oracle(ff, lat2, ranks, vprocs=vp, pqeq=oa.PQEQ_SICNP, QEq_tol=1e-12, NMAXQEq=2000); o.set_pqeq_clean(1)
    o.qeq(); o.force()
    for r, x in enumerate(res):
        assert np.array_equal(x["gid0"], g["gid_%d" % r])
        dq, df = _rank_errs(x["q0"], x["f0"], g["charge_%d" % r], g["force_%d" % r])
        assert dq <= 1e-6 and df <= 1e-6, (r, dq, df)
        assert np.abs(x["shells0"] - o.spos(r)).max() <= 1e-9 and 0 < np.linalg.norm(x["shells0"], axis=1).max() <= 1e-3 * (1 + 1e-12)
    o.step(3)
    moved = 0
    for r, x in enumerate(res):
        assert np.array_equal(x["gid"], o.gids(r))
        moved += len(set(x["gid"]) - set(x["gid0"]))
        assert np.abs(x["pos"] - o.pos(r)).max() <= 1e-9
        dq, df = _rank_errs(x["q"], x["f"], o.charges(r), o.forces(r))
        assert dq <= 1e-6 and df <= 1e-6, (r, dq, df)
        assert np.abs(x["shells"] - o.spos(r)).max() <= 1e-7
        assert np.linalg.norm(x["shells"], axis=1).max() > 1e-3
    assert moved >= 36                                                   # shells did travel with migrating atoms


def test_pqeq_with_the_field_between_ranks_vs_clean_oracle():
    """rxmd.in `efield 1 0.05` on two ranks: the field on cores and shells, and LinearMomentum's per-type sums (main.F90:70-71,766-797)
    all-reduced between kick and drift of every step.  3 MD steps against the two-rank clean oracle (the per-rank local order also against the
    reference's own two-rank run; its charges and forces carry the beyond-cut-off artefact of INTEGRATION 5b #1 once shells have moved -- 176 stale
    look-ups in these 3 steps, |dq| 1.6e-2 between the faithful and the clean restatement, both pinned on CPU in tests/test_oracle_golden.py)."""
    vp = (2, 1, 1)
    g = np.load(os.path.join(oa.GOLD, "sicnp211_v211_pqeq_efieldx_md3.npz"))
    res = _run_ranks(dict(case="sicnp", mc=vp, vp=vp, steps=3, pqeq=True, efield=(1, 0.05)), 2)
    ff, names, frac, lat = oa.make_system("sicnp")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=vp, vprocs=vp)
    o = oa.Oracle(ff, lat2, ranks, vprocs=vp, pqeq=oa.PQEQ_SICNP, QEq_tol=1e-12, NMAXQEq=2000); o.set_efield(1, 0.05); o.set_pqeq_clean(1)
    o.qeq(); o.force(); o.step(3)
    for r, x in enumerate(res):
        assert np.array_equal(x["gid"], o.gids(r)) and np.array_equal(x["gid"], g["gid_%d" % r])
        assert np.abs(x["pos"] - o.pos(r)).max() <= 1e-9
        assert np.abs(x["v"] - o.vel(r)).max() <= 1e-9 * max(1.0, np.abs(o.vel(r)).max())
        dq, df = _rank_errs(x["q"], x["f"], o.charges(r), o.forces(r))
        assert dq <= 1e-6 and df <= 1e-6, (r, dq, df)
        assert np.abs(x["shells"] - o.spos(r)).max() <= 1e-7


@pytest.mark.parametrize("qeq_mode", [0, 1])
def test_extended_lagrangian_between_ranks_vs_mpi_reference(qeq_mode):
    """isQEq 2 on two ranks, 10 steps against `mpiexec -np 2 rxmd_mpi --isQEq 2`: one CG step per MD step from the mixed fictitious
    charges, qsfp / qsfv integrated by the step and carried by MODE_MOVE with their atom (comm.F90:159-163)"""
    g = np.load(os.path.join(oa.GOLD, "rdx222_v211_lex_md10.npz"))
    res = _run_ranks(dict(case="rdx222", mc=(2, 2, 2), vp=(2, 1, 1), steps=10, isQEq=2, qeq_mode=qeq_mode, kw=dict()), 2)
    for r, x in enumerate(res):
        assert np.array_equal(x["gid"], g["gid_%d" % r])
        assert np.abs(x["pos"] - g["pos_%d" % r]).max() <= 1e-9
        dq, df = _rank_errs(x["q"], x["f"], g["charge_%d" % r], g["force_%d" % r])
        assert dq <= 1e-6 and df <= 1e-6, (r, dq, df)


@pytest.mark.parametrize("mode,kw", [(5, dict(treq=300.0)), (7, dict(treq=300.0)), (8, dict(treq=300.0))])
def test_velocity_scaling_modes_between_ranks_vs_mpi_reference(mode, kw):
    """mdmode 5 / 7 / 8 on two ranks from the reference's own two-rank restart file (20 NVE steps), 7 steps with sstep 3, against the
    reference's per-rank dump of the last step: the kinetic energy, the per-element counts and energies and the centre-of-mass momentum
    are sums over BOTH ranks (MPI_ALLREDUCE, main.F90:699,738,783 -> Engine::thermostat / remove_momentum)"""
    g = np.load(os.path.join(oa.GOLD, "rdx222_v211_thermo%d.npz" % mode))
    res = _run_ranks(dict(case="rdx222", vp=(2, 1, 1), steps=7, restart="rdx222_v211_thermo%d" % mode, thermo=(mode, kw, 3)), 2)
    for r, x in enumerate(res):
        assert np.array_equal(x["gid"], g["gid_%d" % r])
        assert np.abs(x["pos"] - g["pos_%d" % r]).max() <= 1e-9
        dq, df = _rank_errs(x["q"], x["f"], g["charge_%d" % r], g["force_%d" % r])
        assert dq <= 1e-6 and df <= 1e-6, (r, dq, df)


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher around it (how the driver may call it; the reference is started as `mpirun -np N rxmd`,
    examples/2-reaxff-dc/Makefile): the script starts its two ranks itself as a child process before anything touches HIP, relays their JSON
    line and leaves with their exit code.  Both ranks share the one GPU of the test box (RXMD_BENCH_DEVICE), messages host-staged over gloo."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RXMD_BENCH_BACKEND="gloo", RXMD_BENCH_DEVICE="0", RXMD_SINGLE_STREAM="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--cells", "6", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.split("\n") if l.startswith("{")][-1]
    r = json.loads(line)
    assert r["n_gpus"] == 2 and r["config"]["ranks_in_communicator"] == 2
    assert r["config"]["atoms_total"] == 2 * 36288 and "vprocs 2x1x1" in r["config"]["parallelism"]
    pr = r["per_rank"]
    assert len(pr["natoms"]) == 2 and sum(pr["natoms"]) == 2 * 36288 and min(pr["nghost"]) > 0
    assert r["config"]["env"]["RXMD_BENCH_BACKEND"] == "gloo"
    assert r["value"] > 0 and abs(r["value"] * r["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert "cpu_baseline" not in r


def test_bench_launches_eight_ranks_on_the_2x2x2_grid_and_carries_the_cpu_baseline():
    """The 8-rank form of the line above (BASELINE configs[3]: vprocs 2 2 2): `bench.py --gpus 8 --cells 3`, eight ranks sharing the one GPU, gloo, no
    second stream.  The first 8-GPU run must not be the first time this launch path, the 2x2x2 rank grid and the per-rank record run at all.
    The parent times the reference on the host cores before it starts the ranks (the small sample here) and rank 0 prints it in the line."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RXMD_BENCH_BACKEND="gloo", RXMD_BENCH_DEVICE="0", RXMD_SINGLE_STREAM="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RXMD_BENCH_CPU_BASELINE_FILE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--cells", "3", "--steps", "2", "--warmup", "1", "--full", "--cpu-baseline-sample", "small"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([l for l in p.stdout.split("\n") if l.startswith("{")][-1])
    assert r["n_gpus"] == 8 and r["config"]["ranks_in_communicator"] == 8
    assert r["config"]["atoms_total"] == 8 * 4536 and "vprocs 2x2x2" in r["config"]["parallelism"]
    pr = r["per_rank"]
    for key in ("natoms", "nghost", "qeq_iters_total", "ms_halo_per_step", "ms_ghost_build_per_step", "place_ms_kept", "pass_ms_in_the_loop"):
        assert len(pr[key]) == 8, key
    assert sum(pr["natoms"]) == 8 * 4536 and min(pr["nghost"]) > 0
    assert len(set(pr["qeq_iters_total"])) == 1                      # the exit test is a global decision: every rank runs the same iterations
    if os.path.exists(os.path.join(root, "oracle", "_ref", "rxmd_omp")):
        cb = r["cpu_baseline"]
        assert cb["kind"] == "reference" and cb["value"] > 0 and cb["cores"] >= 1 and "parent process" in cb["measured_by"]

