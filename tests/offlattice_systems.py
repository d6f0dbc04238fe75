"""The off-lattice systems of test_gpu_offlattice.py and of the CPU regime test in test_oracle_golden.py (TEST INFRASTRUCTURE).

One recipe: the crystal as geninit lays it out, the three edges multiplied by `scale` (the angles stay), every atom displaced by
N(0, sigma) per component from default_rng(7), wrapped back into [0, 1); velocities N(0, 0.1) drawn from the same generator after the
displacements.  The last columns were measured on the oracle at step 0 (they are asserted as inequalities by the regime gates):

  name        case, mc            scale  sigma  atoms  longest bond list   atoms > 12 / 15 / 24 bonds   longest 10 A row
  rdx-dense   rdx222, (2,2,2)     0.85   0.1    1344   20                  454 / 278 / 0                722
  rdx-denser  rdx222, (2,2,2)     0.75   0.1    1344   25                  953 / 828 / 6                1048
  rdx-shaken  rdx222, (2,2,2)     1.0    0.3    1344   13                  8 / 0 / 0                    450
  rdx-dilute  rdx222, (2,2,2)     1.6    0.1    1344   4 (one atom: none)  -                            114 (shortest 93)
  ice-dense   ice644, (6,4,4)     0.75   0.1    2304   14                  297 / 0 / 0                  852
  ice-dilute  ice644, (6,4,4)     1.5    0.1    2304   3 (shortest 1)      -                            112
  rdx-trap    rdx222, (2,2,2)     0.70   0.1    1344   more than the reference's MAXNEIGHBS = 30: "overflow of max # in neighbor list"
"""
import numpy as np

import oracle_api as oa

SEED = 7
MAXN10 = 2000                     # the oracle's 10 A row capacity: the dense boxes need more than its default 1500
SYSTEMS = {
    "rdx-dense": ("rdx222", (2, 2, 2), 0.85, 0.1),
    "rdx-denser": ("rdx222", (2, 2, 2), 0.75, 0.1),
    "rdx-shaken": ("rdx222", (2, 2, 2), 1.0, 0.3),
    "rdx-dilute": ("rdx222", (2, 2, 2), 1.6, 0.1),
    "ice-dense": ("ice644", (6, 4, 4), 0.75, 0.1),
    "ice-dilute": ("ice644", (6, 4, 4), 1.5, 0.1),
    "rdx-trap": ("rdx222", (2, 2, 2), 0.70, 0.1),
}
NAMES = [k for k in SYSTEMS if k != "rdx-trap"]
# the property each case exists for, from the ORACLE's lists: (key, comparison, bound); keys as returned by regime()
GATES = {
    "rdx-dense": [("max_nb", ">", 15), ("n_gt12", ">", 100), ("max_n10", ">", 512)],
    "rdx-denser": [("max_nb", ">", 24), ("n_gt12", ">", 100), ("max_n10", ">", 1024)],
    "rdx-shaken": [("max_nb", ">", 12)],
    "rdx-dilute": [("n_nobond", ">=", 1), ("max_n10", "<", 128)],
    "ice-dense": [("n_gt12", ">", 100), ("max_n10", ">", 512)],
    "ice-dilute": [("max_n10", "<", 128)],
}


def build(name, shift=0.0):
    """-> (ffield, lattice, ranks (one rank), v).  shift: every coordinate moved by up to that many Angstrom (the oracle's self-spread runs)"""
    case, mc, scale, sigma = SYSTEMS[name]
    ff, names, frac, lat = oa.make_system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=mc)
    lat2 = [lat2[0] * scale, lat2[1] * scale, lat2[2] * scale] + list(lat2[3:6])
    rng = np.random.default_rng(SEED)
    n = len(ranks[0]["type"])
    rn = ranks[0]["rnorm"] + rng.normal(0, sigma, (n, 3)) / np.asarray(lat2[:3])
    rn = rn - np.floor(rn)
    v = rng.normal(0, 0.1, (n, 3))
    if shift:
        rn = rn + np.random.default_rng(SEED + 1).uniform(-shift, shift, (n, 3)) / np.asarray(lat2[:3])
        rn = rn - np.floor(rn)
    ranks[0]["rnorm"] = rn
    return ff, lat2, ranks, v


def oracle(name, shift=0.0, with_v=False, **kw):
    ff, lat2, ranks, v = build(name, shift)
    kw.setdefault("maxn10", MAXN10)
    return oa.Oracle(ff, lat2, ranks, v0=[v] if with_v else None, **kw)


def regime(o):
    """what the gates read, from an oracle whose lists are built (after qeq() and force())"""
    n = len(o.gids())
    nb = o.get(103)[:n].astype(int); n10 = o.get(104)[:n].astype(int)
    return dict(natoms=n, max_nb=int(nb.max()), min_nb=int(nb.min()), n_nobond=int((nb == 0).sum()), n_gt12=int((nb > 12).sum()),
                n_gt15=int((nb > 15).sum()), n_gt24=int((nb > 24).sum()), max_n10=int(n10.max()), min_n10=int(n10.min()))


def check_gates(name, r):
    for key, op, bound in GATES[name]:
        ok = {">": r[key] > bound, ">=": r[key] >= bound, "<": r[key] < bound}[op]
        assert ok, "%s left its regime: %s = %d, needs %s %d" % (name, key, r[key], op, bound)
