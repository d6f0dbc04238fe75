"""The per-entry streams of the 10 A list laid out by PLACE (RXMD_STREAMS_BY_PLACE, default 1) against the atom layout (0).

A row of the streams (matrix values, window slots, 4-byte entries, PQEq's shell-core values) lies at the row's place in rows_sorted -- window group
x 16 + wavefront of the window pass -- instead of at its atom index; k_spmv_win then requests the row's first batch before it has read rows_sorted.
Entries, values, slots and their order within a row are the same, every product is added in the same order: everything the solver computes is the
same BITS in both layouts.  Forces, energies and stress are summed with floating-point atomics in FORCE and differ between two runs of ONE setting
in a few components; a force component is compared exactly unless two runs of the same setting disagree on it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_api as oa
from parity import q_err, f_err, perturbed_rdx, run, lattice_sequence, QTOL, FTOL, SWITCH, CLEAN

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def same_bits(a, b, keys=("it0", "est0", "q0", "rows0", "est", "q", "pos", "gid", "rows", "iters")):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def same_forces(on, off):
    """on, off: two runs of each setting.  A force component on which the two runs of ONE setting disagree is noise of the floating-point atomics of
    FORCE (hydrogen-bond acceptors, stress and energy sums); every other component is expected to be the same bits in both layouts.  WHICH components
    are noisy is itself drawn anew by every run (measured, RDX 6 x 6 x 6 behind QEq + FORCE: 4 of 108,864 components differ between two runs of one
    layout, 2 OTHER ones between the layouts -- and two runs of one layout masked by the other layout's pair fail the same way), so a component that
    differs between the layouts without having been caught as noisy is held to the yardstick the runs of one setting give: no further from the other
    layout than the largest difference seen between two runs of the same setting, and no more such components than a few per 10,000."""
    spread = max(float(np.abs(r[0][k] - r[1][k]).max()) for r in (on, off) for k in ("f0", "f"))      # (one yardstick from all four pairs of equal runs)
    for k in ("f0", "f"):
        noisy = (on[0][k] != on[1][k]) | (off[0][k] != off[1][k])
        differ = on[0][k] != off[0][k]
        unmasked = differ & ~noisy
        cross = float(np.abs(on[0][k] - off[0][k])[unmasked].max()) if unmasked.any() else 0.0
        print("%s: %d components differ between the layouts (%d of them not noisy within one, max |d| %.3e), %d are noisy within one (largest |d| between equal runs, both arrays: %.3e)" % (
            k, int(differ.sum()), int(unmasked.sum()), cross, int(noisy.sum()), spread))
        assert cross <= spread, k
        assert unmasked.mean() < 3e-4 and noisy.mean() < 3e-4, "forces that differ run to run in more than a few components are no yardstick"


_CACHE = {}


def rdx_runs(mc, monkeypatch):
    """two runs per layout of the perturbed RDX crystal, once per module"""
    if mc not in _CACHE:
        ff, lat, rec = perturbed_rdx(mc)
        _CACHE[mc] = {p: [run(ff, lat, rec, p, monkeypatch) for _ in range(2)] for p in (1, 0)}
    return _CACHE[mc]


@pytest.mark.parametrize("mc", [(2, 2, 2), (6, 6, 6)])
def test_layouts_agree_bit_for_bit(mc, monkeypatch):
    """RDX 2 x 2 x 2 (1,344 atoms: every row has ghost partners) and 6 x 6 x 6 (36,288 atoms: about a third of the rows have none, so the lean and the
    ghost-column bodies of the window pass both run), perturbed as in test_gpu_scale.py; 3 MD steps at QEq_tol 1e-7.  Est trace of the first and of the
    last QEq call (tap 13), iteration counts, charges, matrix row sums (tap 7), positions: the same bytes; forces: same_forces."""
    r = rdx_runs(mc, monkeypatch)
    on, off = r[1], r[0]
    for o in on:
        assert o["layout0"] == 1 and o["layout"] == 1 and o["stats"]["win_in_use"] == 1
    for o in off:
        assert o["layout0"] == 0 and o["layout"] == 0 and o["stats"]["win_in_use"] == 1
    assert len(on[0]["est"]) >= 2 and on[0]["iters"] > 3
    same_bits(on[0], on[1]); same_bits(off[0], off[1]); same_bits(on[0], off[0])
    same_forces(on, off)


def test_short_groups_and_unwritten_places_under_the_poison_pattern(monkeypatch):
    """RDX 6 x 6 x 6 with every buffer starting as 0xFF bytes (RXMD_POISON_ALLOC=1, read once per process: a child process runs streams_place_worker.py):
    the places of a short last group are never written, so they hold NaN values and 0xFFFF slots, and the window pass reads them like any row.  Finite
    results, equal to the unpoisoned run.  That the box HAS such places: the engine reports win_groups, and win_groups x 16 places > natoms rows means
    at least one group has a sentinel row (here every cell column of the grid ends in a short group unless its residents are a multiple of 16)."""
    ref = rdx_runs((6, 6, 6), monkeypatch)[1][0]
    assert ref["stats"]["win_groups"] * 16 > ref["stats"]["natoms"], (ref["stats"]["win_groups"], ref["stats"]["natoms"])
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "streams_place_poison_%d.npz" % os.getpid())
    env = dict(os.environ, RXMD_POISON_ALLOC="1")
    for k in CLEAN:
        env.pop(k, None)
    env[SWITCH] = "1"
    p = subprocess.run([sys.executable, os.path.join(HERE, "streams_place_worker.py"), out], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "PLACE-POISON-OK" in p.stdout
    try:
        w = dict(np.load(out))
    finally:
        if os.path.exists(out):
            os.remove(out)
    assert int(w["layout"]) == 1 and w["tap14"][0] == 1.0 and np.isnan(w["tap14"][1]) and int(w["win_groups"]) * 16 > len(w["q"])
    for k in ("est0", "q0", "rows0", "est", "q", "pos", "rows", "f0", "f"):
        assert np.isfinite(w[k]).all(), k
    for k in ("est0", "q0", "rows0", "est", "q", "pos", "rows"):
        assert w[k].tobytes() == np.asarray(ref[k]).tobytes(), k
    assert int(w["iters"]) == ref["iters"]
    assert f_err(w["f"], ref["f"]) <= 1e-12      # (atomics: a few components differ in the last bit run to run)


def test_more_places_than_rows_keeps_the_atom_layout(monkeypatch):
    """A gas: the perturbed RDX 2 x 2 x 2 box with its edges tripled (79 x 69 x 64 A, 1,344 atoms in ~195 cell columns of the grid, most of them one
    short group): win_groups x 16 places exceed the rows the streams were sized for -- min(nbuffer, n + n / 8 + 1024), Engine::set_atoms -- so the
    build keeps the atom layout although its windows are valid and the switch is on.  Same bits as with the switch off; a dense box on a fresh
    engine afterwards reports the place layout."""
    ff, lat, rec = perturbed_rdx((2, 2, 2), scale=3.0, sigma=0.1)
    on = [run(ff, lat, rec, 1, monkeypatch, nsteps=2) for _ in range(2)]
    off = [run(ff, lat, rec, 0, monkeypatch, nsteps=2) for _ in range(2)]
    st = on[0]["stats"]; n = st["natoms"]
    print("gas: win_groups %d natoms %d nbuffer %d cells10 %s win_in_use %d" % (st["win_groups"], n, st["nbuffer"], st["cells10"], st["win_in_use"]))
    assert st["win_groups"] * 16 > min(st["nbuffer"], n + n // 8 + 1024) and st["win_in_use"] == 1
    assert on[0]["layout0"] == 0 and on[0]["layout"] == 0 and off[0]["layout"] == 0
    same_bits(on[0], off[0]); same_forces(on, off)
    dense = rdx_runs((2, 2, 2), monkeypatch)[1][0]
    assert dense["layout0"] == 1 and dense["layout"] == 1


def test_row_stride_growth_keeps_layout_and_results(monkeypatch):
    """The SiC particle in a box widened 3 x along x: the row stride of the 10 A list, sized from the mean density, grows in the first build (the
    streams are allocated again and swept again).  The layout flag and the results of the grown engine against a fresh engine created with the final
    stride, and against the atom layout through the same growth: the same bits."""
    from rxmd_amd import system
    ff, names, frac, lat = oa.make_system("sicnp")
    lat3, rec = system.geninit(ff, names, frac, lat, mc=(1, 1, 1))
    lat_wide = list(lat3); lat_wide[0] *= 3.0
    rec2 = rec.copy(); rec2[:, 0] = rec2[:, 0] / 3.0
    rec2[:, 3:6] = np.random.default_rng(3).normal(0, 0.02, (len(rec2), 3))
    s0 = {}
    grown = run(ff, lat_wide, rec2, 1, monkeypatch, nsteps=2, before=lambda e, o: s0.update(stride=e.stats()["n10_stride"]))
    assert grown["stride"] > s0["stride"], (s0, grown["stride"])
    fresh = run(ff, lat_wide, rec2, 1, monkeypatch, nsteps=2, maxneighbs10=grown["stride"])
    atom = run(ff, lat_wide, rec2, 0, monkeypatch, nsteps=2)
    assert fresh["stride"] == grown["stride"] == atom["stride"]
    assert grown["layout0"] == grown["layout"] == fresh["layout0"] == fresh["layout"] and atom["layout"] == 0
    print("sicnp wide: stride %d -> %d, layout %d, win_in_use %d" % (s0["stride"], grown["stride"], grown["layout"], grown["stats"]["win_in_use"]))
    same_bits(grown, fresh); same_bits(grown, atom)
    assert f_err(grown["f"], fresh["f"]) <= 1e-12 and f_err(grown["f"], atom["f"]) <= 1e-12


def test_set_lattice_growth_of_the_window_groups_keeps_layout_and_results(monkeypatch):
    """RDX 2 x 2 x 2, then set_lattice to the expanded cell of parity.lattice_sequence (more cells on every axis: the
    window-group arrays are allocated again), then 2 steps.  Both layouts through the same call sequence: the same bits, the flag as set.  Against a
    fresh engine that starts in the expanded cell with the same normalised coordinates, both with converged charges (QEq_tol 1e-12): the parity
    tolerances of the suite (its positions are rnorm x lattice, the live engine's an affine map of its old ones: an ulp apart, which the REAL(4)
    rounding of r^2 in the matrix turns into 6e-8 of an entry where it flips)."""
    ff, lat, rec = perturbed_rdx((2, 2, 2))
    seq = {}

    def grow(e, o):
        e.QEq(); e.FORCE()
        o["cells_before"] = list(e.stats()["cells10"]); o["layout_before"] = e.stats()["streams_by_place"]
        seq.update(dict(lattice_sequence(list(e.lattice), e.cutoffs()[1])))
        e.set_lattice(seq["expanded"])
    on = run(ff, lat, rec, 1, monkeypatch, nsteps=2, before=grow)
    off = run(ff, lat, rec, 0, monkeypatch, nsteps=2, before=grow)
    assert all(a > b for a, b in zip(on["stats0"]["cells10"], on["cells_before"])), (on["cells_before"], on["stats0"]["cells10"])
    assert on["layout_before"] == on["layout0"] == on["layout"] == 1 and off["layout_before"] == off["layout0"] == off["layout"] == 0
    same_bits(on, off)
    assert f_err(on["f"], off["f"]) <= 1e-12
    # (measured at QEq_tol 1e-7, where the two stop on different iterates: q 2.3e-7, f 1.3e-6 -- hence converged charges on both sides for this comparison)
    tight = dict(QEq_tol=1e-12, NMAXQEq=2000)
    grown = run(ff, lat, rec, 1, monkeypatch, nsteps=2, before=grow, **tight)
    fresh = run(ff, list(seq["expanded"]), rec, 1, monkeypatch, nsteps=2, **tight)
    assert grown["layout"] == fresh["layout"] == 1 and np.array_equal(fresh["gid"], grown["gid"])
    print("grown against fresh: q %.2e f %.2e" % (q_err(grown["q"], fresh["q"]), f_err(grown["f"], fresh["f"])))
    assert q_err(grown["q"], fresh["q"]) <= QTOL and f_err(grown["f"], fresh["f"]) <= FTOL


@pytest.mark.parametrize("what", ["sicnp211-pqeq", "rdx222-f32", "rdx222-qeq-mode-0", "rdx666-staged-remote"])
def test_other_instances_of_the_pass(what, monkeypatch):
    """The other instances of k_spmv_win at their smallest shapes, layout on against off, Est traces and charges (and the rest of same_bits): the SiC
    particle 2 x 1 x 1 with PQEq (third stream hsc; its 4-byte entries are read by the shell update and ENbond_PQEq through rpos), the fp32 value stream
    on RDX 2 x 2 x 2, qeq_mode 0 (the gradient instances of the pass) on the same box, and the staged single-rank path through RCCL with the interior / boundary split of the pass on RDX 6 x 6 x 6."""
    from rxmd_amd import system
    kw = {}
    if what == "sicnp211-pqeq":
        ff, names, frac, lat0 = oa.make_system("sicnp")
        lat, rec = system.geninit(ff, names, frac, lat0, mc=(2, 1, 1))
        rec[:, 3:6] = np.random.default_rng(5).normal(0, 0.02, (len(rec), 3))
        kw = dict(pqeq=oa.PQEQ_SICNP, maxneighbs10=768)       # (a fixed row stride: the one sized from the mean density of a particle in vacuum is below the 384 entries the place layout asks for)
    elif what == "rdx222-f32":
        ff, lat, rec = perturbed_rdx((2, 2, 2)); kw = dict(bits=32)
    elif what == "rdx222-qeq-mode-0":
        ff, lat, rec = perturbed_rdx((2, 2, 2)); kw = dict(qeq_mode=0)       # (two matrix passes per iteration: the MODE_GRAD instances, atom-ordered tail)
    else:
        ff, lat, rec = perturbed_rdx((6, 6, 6)); kw = dict(env=(("RXMD_FORCE_STAGED", "1"), ("RXMD_FORCE_REMOTE", "1")), rccl=True)
    on = run(ff, lat, rec, 1, monkeypatch, nsteps=2, **kw)
    off = run(ff, lat, rec, 0, monkeypatch, nsteps=2, **kw)
    print(what, "layout", on["layout"], off["layout"], "win_in_use", on["stats"]["win_in_use"], "spmv_nstep", on["stats"]["spmv_nstep"], "boundary rows", on["stats"]["n_boundary_rows"])
    assert on["layout0"] == on["layout"] == 1 and off["layout0"] == off["layout"] == 0 and on["stats"]["win_in_use"] == 1
    if what == "rdx666-staged-remote":
        assert 0 < on["stats"]["n_boundary_rows"] < on["stats"]["natoms"]
    same_bits(on, off)
    assert f_err(on["f"], off["f"]) <= 1e-12
