"""rxmd_hip_get_bonds_device and rxmd_hip_get_pairs_device on DECOMPOSED boxes: every rank of a 2 x 1 x 1 or 2 x 2 x 2 grid exports its graphs with
global ids (tests/graph_worker.py: all ranks on GPU 0, messages host-staged over gloo, one file per rank) and the parent holds the union to
references that know nothing of the decomposition.  What a decomposed box adds to the single-rank tests (test_gpu_pair_graph.py,
test_gpu_bond_graph.py): global ids and positions of ghosts that came from another rank (in 2 x 2 x 2 forwarded x -> y -> z through a third one),
rows split into an interior and a boundary launch, a rank with no atom, the list of a QEq-only build, PQEq's longer list, a skewed cell.

Systems (the smallest that still decompose): rdx222 = RDX 2 x 2 x 2, 1,344 atoms, on both grids; the same with every atom displaced by N(0, 0.05 A)
(seed 2048) and velocities by global id (parity.mode_velocities, seed 7, sigma 0.05 as test_gpu_scale), three steps; parity.slab_system (rank 1
owns nothing); the SiC nanoparticle with PQEq, one particle per rank; triclinic MoS2 3 x 3 x 2; rdx222 with the fp32 matrix stream.  Seed 2048 was
picked on the CPU: the brute-force distances of the starting state keep 2.7e-5 / 1.0e-5 / 7.8e-7 A from 3.0 / 6.5 / 9.5 A, and on the multi-rank oracle 2 atoms
(2 x 1 x 1) and 3 atoms (2 x 2 x 2) change rank within the three steps -- seeds 2027..2032 with the same velocities move none at this size.
The edge counts of the perfect rdx222 are 8 x those of rdx168 (periodic replication; confirmed by the brute force on geninit's positions).

Frames: rxmd_hip_get_atoms returns Cartesian positions in the frame of the WHOLE box on every rank (set_atoms_rxff adds the domain origin before xs2xu;
the pos_<rank> goldens of the reference are in that frame too), so the parent adds no origin.  It wraps them into the box before the brute force,
whose image reach assumes one box: r' = r - H floor(H^-1 r), one more lattice vector of <= 60 A added per coordinate.

Bounds, and where they come from:
  * n = rint(H^-1 (vec - (pos[dst] - pos[src]))) and its distance from an integer: 1e-9, the bound of test_gpu_bond_graph._check_images (a coordinate
    carries ~1e-14 in normalised units; a wrong partner or image is off by ~1e-1).
  * the sorted (src, dst, n) of all ranks together against the brute force over the wrapped global positions: exact.  No brute-force distance may lie
    within 1e-8 A of r_cut (test_gpu_pair_graph._select).  The whole list (r_cut = 0) is held to the brute force at the taper cut-off, 10 A (PQEq 12.5 A).
  * vec against the brute-force vector: 1e-12 A, the derived bound of test_gpu_pair_graph.py: same magnitudes, one more origin added.
  * row counts of the whole list: equal to debug tap 6 and to tap 104 of the multi-rank oracle, rank by rank.
  * math.fsum row sums of hval against debug tap 7 and oracle tap 108: rtol 1e-12 (test_gpu_parity.py:81).  With the fp32 stream every value is one
    float rounding (relative 2^-24) from the oracle's double and all values of a row have one sign: rtol 2^-24 + 1e-12 against tap 108 there.
  * hval entry by entry: graph_support.check_hval_entries, 8 eps |h|, at most 2 entries matched at the neighbouring float; fp32 stream: exact.
    One of the four forms of the reference must hold ALL ranks of a system (one kernel build), and the 2 entries are counted over all its ranks.
    PQEq: row sums only.  MoS2: in a skewed box a ghost beyond the reference's QEq ghost shell is in the list but not in the QEq matrix (lists.hip: inq)
    and would be exported as 0; in this box at 2 x 1 x 1 no partner is such a ghost (none of the 239,112 entries is 0), so every entry is held to the
    table here as in the other systems, with no exemption.
  * bonds: src, dst, bo of a rank equal its own host list (bonds() + atoms()["gid"]) exactly, also with bo_min = 0.3; |sum bo3 - bo| <= 4 eps bo,
    bo3 >= 0, 0 < |vec| <= maxrc (test_gpu_bond_graph.py); every directed bond has its mirror on the rank that owns the partner, with the negated image
    and vec + mirror vec <= 1e-9 normalised.
  * the bond order of a bond and of its mirror are one formula evaluated in two frames: no number fixed in advance, the engine is allowed ten times
    the mismatch the multi-rank ORACLE shows between its own ranks (printed).
  * bond lists by global id against the multi-rank oracle: the rows of compare_bond_order_taps (test_gpu_parity.py) and its tolerance, 1e-10.
  * chi + H q = const from the matrix assembled over all ranks: no number fixed in advance, the rule of
    test_exported_matrix_is_the_qeq_operator_of_the_converged_charges (engine's charges: ten times the spread of the oracle's; printed).
  * a second pair of calls on one state returns the same bits (compared inside each rank).
"""
import json
import math
import os

import numpy as np
import pytest

import oracle_api as oa
import graph_worker
from ranks import run_ranks
from npt_reference import hmat
from parity import build_system
from graph_support import brute_force, _select, check_hval_entries, qeq_table, CUTS, EDGES, SENT_I, SENT_F, TIGHT

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
RDX222 = dict(case="rdx222", mc=(2, 2, 2))
SHAKEN = dict(RDX222, shaken=(2048, 0.05), v=(7, 0.05, 1344), steps=3)
SYSTEMS = {
    "rdx222-v211": dict(RDX222, vp=(2, 1, 1)),
    "rdx222-v222": dict(RDX222, vp=(2, 2, 2)),
    "rdx222-shaken-v211": dict(SHAKEN, vp=(2, 1, 1)),
    "rdx222-shaken-v222": dict(SHAKEN, vp=(2, 2, 2)),
    "slab-v211": dict(case="rdx168", slab=True, vp=(2, 1, 1)),
    "sicnp-pqeq-v211": dict(case="sicnp", mc=(2, 1, 1), vp=(2, 1, 1), pqeq=True),
    "mos2_tri324-v211": dict(case="mos2_tri324", mc=(3, 3, 2), vp=(2, 1, 1)),
    "rdx222-f32-v211": dict(RDX222, vp=(2, 1, 1), f32=True),
}
COUNTS = {                                         # directed edges at 3.0 / 6.5 / 9.5 A, from the brute force on the CPU
    "rdx222": tuple(8 * x for x in EDGES["rdx168"]),
    "rdx222-shaken": (13580, 157384, 492110),
}
assert COUNTS["rdx222"] == (13776, 157408, 491904)
CUTS_AFTER = tuple(6.5 + 1e-3 * k for k in range(5))   # after the steps: the first of these with no distance within 1e-8 A


def _cuts(spec):
    return CUTS + ((12.0,) if spec.get("pqeq") else ()) + (0.0,)


def _reach(spec):
    return 12.5 if spec.get("pqeq") else 10.0      # the taper cut-off: what the whole list holds (init.F90:28-43)


def _run(name, tmp_path):
    """one spawn of the system's ranks -> dict(spec, lat, ranks=[what rank r wrote], world)"""
    spec = dict(SYSTEMS[name], kw=TIGHT, dir=str(tmp_path))
    spec["cuts"] = _cuts(spec); spec["cuts_after"] = CUTS_AFTER
    vp = spec["vp"]; world = vp[0] * vp[1] * vp[2]
    run_ranks(graph_worker.graph_rank, world, spec, timeout=600)
    ranks = []
    for r in range(world):
        with np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) as f:
            ranks.append({k: f[k] for k in f.files})
        assert str(ranks[r]["transport_error"]) == "None" and (ranks[r]["transport"] > 0).all()
    ff, lat, recs, vs = build_system(spec)
    return dict(name=name, spec=spec, ff=ff, lat=lat, recs=recs, ranks=ranks, world=world)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """system name -> its run, spawned at the first request: the pair, bond and operator cases of a system share one spawn (and one oracle, kept in
    the run).  The cases of a system follow one another, so only the last run is kept: a run holds ~100 MB of edges.  Selecting or ordering the
    cases otherwise only spawns a system again, which the fixture says aloud."""
    kept = {}

    def get(name):
        if name not in kept:
            kept.clear()
            print("spawning the ranks of", name)
            kept[name] = _run(name, tmp_path_factory.mktemp(name))
        return kept[name]
    return get


def _oracle(run):
    """the multi-rank oracle of the system after QEq + FORCE, built once per run"""
    if "oracle" not in run:
        spec = run["spec"]
        kw = dict(TIGHT, nbuffer=20000) if spec.get("slab") else dict(TIGHT)
        o = oa.Oracle(run["ff"], run["lat"], run["recs"], vprocs=spec["vp"], pqeq=oa.PQEQ_SICNP if spec.get("pqeq") else None, **kw)
        if spec.get("pqeq"):
            o.set_pqeq_clean(1)
        o.qeq(); o.force()
        run["oracle"] = o
    return run["oracle"]


def _world(run, tag):
    """the box by global id from what the ranks report: wrapped positions, types, charges, owner rank, index on the owner"""
    gids = np.concatenate([x[tag + "gid"] for x in run["ranks"]])
    n = len(gids)
    assert np.array_equal(np.sort(gids), np.arange(1, n + 1)), "the ranks' residents are not the atoms of the box, each once"
    H = hmat(run["lat"]); Hi = np.linalg.inv(H)
    pos = np.zeros((n, 3)); typ = np.zeros(n, dtype=np.int64); q = np.zeros(n); owner = np.zeros(n, dtype=np.int64); loc = np.zeros(n, dtype=np.int64)
    for r, x in enumerate(run["ranks"]):
        g = x[tag + "gid"] - 1
        pos[g] = x[tag + "pos"]; typ[g] = x[tag + "type"]; q[g] = x[tag + "q"]; owner[g] = r; loc[g] = np.arange(len(g))
    pos = pos - np.floor(pos @ Hi.T) @ H.T
    return dict(n=n, H=H, Hi=Hi, pos=pos, type=typ, q=q, owner=owner, loc=loc)


def _images(w, s, d, vec):
    """n = rint(H^-1 (vec - (pos[dst] - pos[src]))) of edges given by global id, and the largest distance of the quotient from an integer"""
    frac = (vec - (w["pos"][d - 1] - w["pos"][s - 1])) @ w["Hi"].T
    n = np.rint(frac)
    return n.astype(np.int64), float(np.abs(frac - n).max(initial=0.0))


def _rank_pairs(x, key, r, w, label):
    """one rank's arrays of one call: count-only = fill, nothing written behind the count, src owned by this rank and in resident order"""
    cnt, E = int(x[key + "cnt"]), int(x[key + "E"])
    s, d, vec, hv = (x[key + k] for k in ("src", "dst", "vec", "hval"))
    assert cnt == E, "%s rank %d: the count-only call gives %d, the fill %d" % (label, r, cnt, E)
    assert len(s) == E + 3
    assert (s[E:] == SENT_I).all() and (d[E:] == SENT_I).all() and (vec[E:] == SENT_F).all() and (hv[E:] == SENT_F).all(), "written behind the count"
    s, d, vec, hv = s[:E], d[:E], vec[:E], hv[:E]
    assert (s >= 1).all() and (s <= w["n"]).all() and (d >= 1).all() and (d <= w["n"]).all(), "%s rank %d: a global id outside the box" % (label, r)
    assert (w["owner"][s - 1] == r).all(), "%s rank %d: src holds an atom of another rank" % (label, r)
    assert (np.diff(w["loc"][s - 1]) >= 0).all(), "%s rank %d: src is not in resident order" % (label, r)
    assert np.isfinite(vec).all() and np.isfinite(hv).all()
    return s, d, vec, hv


def check_pair_graph(run, tag, r_cut, bf, label):
    """checks 1-7 of one cut-off (r_cut 0: the whole list against the brute force at the taper cut-off) -> the ranks' (src, dst, vec, hval)"""
    w = _world(run, tag)
    key = "%spd%.3f_" % (tag, r_cut)
    per = [_rank_pairs(x, key, r, w, label) for r, x in enumerate(run["ranks"])]
    for r, x in enumerate(run["ranks"]):
        if len(x[tag + "gid"]) == 0:
            assert len(per[r][0]) == 0                                  # the empty rank: 0, and (above) nothing written
    s, d, vec = (np.concatenate([p[k] for p in per]) for k in range(3))
    assert len(np.unique(s)) == w["n"], "%s: an atom is src on no rank" % label      # (every atom of every system here has a partner within 3 A)
    n, off_int = _images(w, s, d, vec)
    ref_keys, ref_vec, gap = _select(bf, r_cut if r_cut > 0 else _reach(run["spec"]))
    keys = np.concatenate([s[:, None] - 1, d[:, None] - 1, n], axis=1)
    o = np.lexsort(keys.T[::-1])
    keys, vec_s = keys[o], vec[o]
    err = np.abs(vec_s - ref_vec).max() if len(keys) == len(ref_keys) and len(keys) else float("nan")
    print("%s r_cut %.3f: E %d = %s (brute force %d), smallest gap to the cut-off %.2e A, distance from a lattice vector (normalised) %.2e, max |vec - brute force| %.2e A"
          % (label, r_cut, len(s), " + ".join(str(len(p[0])) for p in per), len(ref_keys), gap, off_int, err))
    assert off_int <= 1e-9
    assert len(keys) == len(ref_keys)
    assert np.array_equal(keys, ref_keys), "the (src, dst, image) of all ranks together differ from the brute-force radius graph"
    assert err <= 1e-12
    return per


def _bf(run, tag, r_max):
    w = _world(run, tag)
    return brute_force(w["pos"], run["lat"], r_max)


def check_pairs(run):
    name, spec = run["name"], run["spec"]
    for x in run["ranks"]:
        assert list(x["codes"]) == [-1, -1, -1, -1, -1], "local indices / shift3 on a decomposed box: %s" % list(x["codes"])
        assert bool(x["refused_calls_wrote_nothing"]) and bool(x["s0_same_bits"])
    bf = _bf(run, "s0_", _reach(spec))
    w = _world(run, "s0_")
    per = {}
    for r_cut in _cuts(spec):
        per[r_cut] = check_pair_graph(run, "s0_", r_cut, bf, name)
    base = name[:-5].replace("-f32", "")
    if base in COUNTS:
        assert tuple(sum(len(p[0]) for p in per[c]) for c in CUTS) == COUNTS[base]
    o = _oracle(run)
    tab = None if spec.get("pqeq") else qeq_table(o, run["ff"])
    f32 = bool(spec.get("f32"))
    form, escapes, worst = None, 0, 0.0  # of the per-entry check of hval: one form and one escape count per SYSTEM
    for r, x in enumerate(run["ranks"]):
        n = len(x["s0_gid"])
        assert np.array_equal(x["s0_gid"], o.gids(r)), "rank %d: the resident order is not the oracle's" % r
        if f32:
            assert int(x["qeq_precision"][0]) == 32
        s, d, vec, hv = per[0.0][r]
        # a cut-off filters the whole list in order
        for r_cut in _cuts(spec)[:-1]:
            keep = np.linalg.norm(vec, axis=1) <= r_cut
            for got, ref in zip(per[r_cut][r], (s, d, vec, hv)):
                assert np.array_equal(got, ref[keep]), "rank %d: the list at %.1f A is not the whole list filtered" % (r, r_cut)
        # the list of the QEq call alone
        for r_cut in (6.5, 0.0):
            q = "q_pd%.3f_" % r_cut
            E = int(x[q + "E"])
            assert int(x[q + "cnt"]) == E == len(per[r_cut][r][0])
            for k, ref in zip(("src", "dst", "vec", "hval"), per[r_cut][r]):
                assert np.array_equal(x[q + k][:E], ref), "rank %d: %s after QEq alone differs from that after FORCE (r_cut %.1f)" % (r, k, r_cut)
        if n == 0:
            continue
        cnt = np.bincount(w["loc"][s - 1], minlength=n)
        assert np.array_equal(cnt, x["s0_dbg6"].astype(np.int64)), "rank %d: row counts differ from tap 6" % r
        assert np.array_equal(cnt, o.get(104, r)[:n].astype(np.int64)), "rank %d: row counts differ from the oracle's tap 104" % r
        assert len(s) == json.loads(str(x["s0_stats"]))["nnz10"]
        off = np.concatenate([[0], np.cumsum(cnt)])
        rows = np.array([math.fsum(hv[off[i]:off[i + 1]]) for i in range(n)])
        t7, t108 = x["s0_dbg7"], o.get(108, r)[:n]
        e7, e108 = np.abs(rows / t7 - 1).max(), np.abs(rows / t108 - 1).max()
        print("%s rank %d: %d rows, whole list %d, row sums of hval vs tap 7: max rel %.2e, vs the oracle's tap 108: max rel %.2e" % (name, r, n, len(s), e7, e108))
        assert np.allclose(rows, t7, rtol=1e-12, atol=0.0)
        assert np.allclose(rows, t108, rtol=(2.0 ** -24 if f32 else 0.0) + 1e-12, atol=0.0)
        if tab is not None:
            e_r, esc_r, form_r = check_hval_entries(vec, hv, w["type"][s - 1], w["type"][d - 1], tab, "%s rank %d" % (name, r), f32=f32, form=form)
            assert form in (None, form_r)
            form, escapes, worst = form_r, escapes + esc_r, max(worst, e_r)
    if tab is not None:
        print("%s: hval entry by entry, all ranks: max %.2f eps |h| with the products contracted %s on every rank, entries matched at the neighbouring float %d"
              % (name, worst, form, escapes))
        assert escapes <= 2, "%d entries of the system matched only at the neighbouring float" % escapes
    if spec.get("steps"):
        check_pairs_after_steps(run)


def check_pairs_after_steps(run):
    name = run["name"]
    moved = sum(len(set(x["s1_gid"]) - set(x["s0_gid"])) for x in run["ranks"])
    print("%s: atoms that changed rank within %d steps: %d" % (name, run["spec"]["steps"], moved))
    assert moved >= 1
    assert all(bool(x["s1_same_bits"]) for x in run["ranks"])
    bf = _bf(run, "s1_", max(CUTS_AFTER) + 1e-3)
    gaps = [np.abs(bf[2] - c).min() for c in CUTS_AFTER]
    ok = [c for c, g in zip(CUTS_AFTER, gaps) if g > 1e-8]
    assert ok, "a distance within 1e-8 A of every one of %s" % (CUTS_AFTER,)
    check_pair_graph(run, "s1_", ok[0], bf, name + " after the steps")


# ---- bonds ---------------------------------------------------------------------------------------------------------------------------------
def _mirror_mismatch(edges):
    """edges: (src gid, dst gid, bo) of every directed bond of the box -> the largest |bo(i -> j) - bo(j -> i)|; a pair bonded through several images
    is compared as sorted lists"""
    by = {}
    for s, d, b in zip(*edges):
        by.setdefault((int(s), int(d)), []).append(float(b))
    worst = 0.0
    for (s, d), v in by.items():
        m = by.get((d, s))
        assert m is not None and len(m) == len(v), "bond (%d, %d) has no mirror" % (s, d)
        worst = max(worst, float(np.abs(np.sort(v) - np.sort(m)).max()))
    return worst


def _oracle_edges(o, world):
    S, D, B = [], [], []
    for r in range(world):
        n = len(o.gids(r))
        if n == 0:
            continue
        nbr, bo = o.bonds(r)
        cnt = o.get(103, r)[:n].astype(np.int64)
        gidG = o.get(106, r).astype(np.int64)
        mask = np.arange(nbr.shape[1])[None, :] < cnt[:, None]
        S.append(np.repeat(gidG[:n], cnt)); D.append(gidG[nbr[:n][mask] - 1]); B.append(bo[:n][mask])
    return np.concatenate(S), np.concatenate(D), np.concatenate(B)


def check_bond_graph(run, tag, label):
    """checks 1-5 of one state -> (src, dst, bo) of all ranks"""
    w = _world(run, tag)
    S, D, B, V, N = [], [], [], [], []
    for r, x in enumerate(run["ranks"]):
        for bo_min in (0.0, 0.3):
            k = "%sbd%.1f_" % (tag, bo_min)
            cnt, E = int(x[k + "cnt"]), int(x[k + "E"])
            s, d, b, parts, vec = (x[k + a] for a in ("src", "dst", "bo", "bo3", "vec"))
            assert cnt == E and len(s) == E + 3
            assert (s[E:] == SENT_I).all() and (d[E:] == SENT_I).all() and all((a[E:] == SENT_F).all() for a in (b, parts, vec)), "written behind the count"
            s, d, b, parts, vec = s[:E], d[:E], b[:E], parts[:E], vec[:E]
            h = "%shost%.1f_" % (tag, bo_min)
            assert E == len(x[h + "bo"]), "%s rank %d: %d bonds on the device, %d in the host list (bo_min %.1f)" % (label, r, E, len(x[h + "bo"]), bo_min)
            assert np.array_equal(s, x[h + "src"]) and np.array_equal(d, x[h + "dst"]) and np.array_equal(b, x[h + "bo"]), \
                "%s rank %d: the device graph differs from the host list (bo_min %.1f)" % (label, r, bo_min)
            if bo_min:
                assert (b >= bo_min).all() and (len(x[tag + "gid"]) == 0 or 0 < E < int(x["%sbd0.0_E" % tag]))
                continue
            assert (w["owner"][s - 1] == r).all() and (d >= 1).all() and (d <= w["n"]).all()
            if E == 0:
                assert len(x[tag + "gid"]) == 0
                continue
            length = np.linalg.norm(vec, axis=1)
            maxrc = float(x["maxrc"])
            print("%s rank %d: directed bonds %d, parts min %.3e, |sum - bo| / bo max %.2e, |vec| in [%.4f, %.4f], maxrc %.4f"
                  % (label, r, E, parts.min(), (np.abs(parts.sum(axis=1) - b) / np.maximum(b, 1e-300)).max(), length.min(), length.max(), maxrc))
            assert np.isfinite(parts).all() and (parts >= 0.0).all()
            assert (np.abs(parts.sum(axis=1) - b) <= 4 * EPS * b).all()
            assert (length > 0.0).all() and (length <= maxrc).all()
            S.append(s); D.append(d); B.append(b); V.append(vec)
    s, d, b, vec = (np.concatenate(a) for a in (S, D, B, V))
    n, off_int = _images(w, s, d, vec)
    edges = {}
    for k in range(len(s)):
        edges[(int(s[k]), int(d[k]), int(n[k, 0]), int(n[k, 1]), int(n[k, 2]))] = k
    assert len(edges) == len(s), "two bonds with the same ends and image"
    worst = 0.0
    for (i, j, n0, n1, n2), k in edges.items():
        m = edges.get((j, i, -n0, -n1, -n2))       # (src is owned by the rank that exported the edge: the mirror is on the owner of j)
        assert m is not None, "%s: bond (%d, %d) through image (%d, %d, %d) has no mirror on the rank that owns %d" % (label, i, j, n0, n1, n2, j)
        worst = max(worst, float(np.abs((vec[k] + vec[m]) @ w["Hi"].T).max()))
    print("%s: directed bonds of all ranks %d, through an image %d, distance from a lattice vector (normalised) %.2e, vec + mirror vec (normalised) %.2e"
          % (label, len(s), int((n != 0).any(axis=1).sum()), off_int, worst))
    assert off_int <= 1e-9 and worst <= 1e-9
    return s, d, b


def check_bonds(run):
    name, spec = run["name"], run["spec"]
    assert all(bool(x["s0_same_bits"]) and bool(x.get("s1_same_bits", True)) for x in run["ranks"])     # (the second pair of calls covers the bond calls too)
    edges = check_bond_graph(run, "s0_", name)
    o = _oracle(run)
    mm_engine, mm_oracle = _mirror_mismatch(edges), _mirror_mismatch(_oracle_edges(o, run["world"]))
    print("%s: largest |bo(i -> j) - bo(j -> i)|: engine %.3e, oracle %.3e" % (name, mm_engine, mm_oracle))
    assert mm_engine <= 10.0 * mm_oracle
    # the lists by global id against the oracle's, row by row as compare_bond_order_taps does
    worst = 0.0
    for r, x in enumerate(run["ranks"]):
        n = len(x["s0_gid"])
        assert np.array_equal(x["s0_gid"], o.gids(r))
        if n == 0:
            continue
        cnt, pg, bo = x["s0_hb_cnt"], x["s0_hb_pg"], x["s0_hb_bo"]
        onbr, obo = o.bonds(r)
        gidG = o.get(106, r).astype(np.int64)
        assert np.array_equal(cnt, o.get(103, r)[:n].astype(cnt.dtype)), "rank %d: bond counts differ from the oracle's" % r
        for i in range(n):
            c = int(cnt[i])
            ge, go = pg[i, :c], gidG[onbr[i, :c] - 1]
            ie, io = np.lexsort((bo[i, :c], ge)), np.lexsort((obo[i, :c], go))
            assert np.array_equal(ge[ie], go[io]), "rank %d atom %d: partners differ from the oracle's" % (r, i)
            worst = max(worst, float(np.abs(bo[i, :c][ie] - obo[i, :c][io]).max(initial=0.0)))
    print("%s: bond orders against the multi-rank oracle: max abs %.2e" % (name, worst))
    assert worst <= 1e-10
    if spec.get("steps"):
        assert sum(len(set(x["s1_gid"]) - set(x["s0_gid"])) for x in run["ranks"]) >= 1
        check_bond_graph(run, "s1_", name + " after the steps")


# ---- the operator across ranks ---------------------------------------------------------------------------------------------------------------
def check_operator(run):
    """chi + H q is one number on every atom at the solution of QEq; H = eta on the diagonal + the values of ALL ranks' whole lists"""
    import ctypes as C
    from rxmd_amd import _lib
    w = _world(run, "s0_")
    o = _oracle(run)
    info = np.zeros(64)
    _lib.load().rxmd_host_ffield_table(str(run["ff"]).encode(), None, 6, info.ctypes.data_as(C.c_void_p), 64)
    nso = int(info[0])
    chi, eta = info[5:5 + nso][w["type"] - 1], info[5 + nso:5 + 2 * nso][w["type"] - 1]
    key = "s0_pd%.3f_" % 0.0
    s, d, h = (np.concatenate([x[key + k][:int(x[key + "E"])] for x in run["ranks"]]) for k in ("src", "dst", "hval"))
    q_oracle = np.zeros(w["n"])
    for r in range(run["world"]):
        q_oracle[o.gids(r) - 1] = o.charges(r)

    def spread(q):
        mu = chi + eta * q + np.bincount(s - 1, weights=h * q[d - 1], minlength=w["n"])
        return mu.max() - mu.min(), mu.mean()

    s_engine, mu_engine = spread(w["q"])
    s_oracle, mu_oracle = spread(q_oracle)
    print("%s: spread of chi + H q over the atoms: engine's charges %.3e, oracle's charges %.3e (mean %.6f / %.6f)" % (run["name"], s_engine, s_oracle, mu_engine, mu_oracle))
    assert s_oracle < 1e-3 * abs(mu_oracle), "the matrix of all ranks together is not the operator the oracle's charges solve"
    assert s_engine <= 10.0 * s_oracle


PARTS = {"pairs": check_pairs, "bonds": check_bonds, "operator": check_operator}
CASES = [(n, p) for n in SYSTEMS for p in (("pairs", "bonds", "operator") if n == "rdx222-v222" else ("pairs", "bonds"))]


@pytest.mark.parametrize("name,part", CASES, ids=["%s-%s" % c for c in CASES])
def test_graphs_of_a_decomposed_box(name, part, runs):
    PARTS[part](runs(name))
