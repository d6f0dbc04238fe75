#!/usr/bin/env python3
"""Generate the fixtures of the single-precision QEq matrix stream: tests/golden/{rdx168,ice644}_f32matrix_tight.npz.

TEST INFRASTRUCTURE.  The mode `rxmd_hip_set_qeq_precision(h, 32)` rounds every value of the 10 A matrix ONCE to REAL(4) where the list
sweep forms it; everything else stays double.  The fixed point of that rounded matrix is computed here by the plain-C oracle with the same
single rounding: oracle/ is copied to a temporary directory, the ONE assignment of a matrix value in the copy

    HES(r, i, cnt) = (1.0 - drtb) * T[itb] + drtb * T[itb + 1];        ->  HES(r, i, cnt) = (double)(float)(...);

is replaced (exactly one replacement, asserted), the copy is built there, and tests/oracle_api.py is pointed at it before its first
lib() call.  Nothing under oracle/ changes.

Each fixture: gid, q, f, pe[14], Est after QEq + FORCE at QEq_tol 1e-12 / NMAXQEq 2000.  rdx168 also: positions, charges and
E_tot = KE + PE(0) after 40 steps from rest.
Usage: python tests/golden/make_f32_matrix_golden.py
"""
import os, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

OLD = "HES(r, i, cnt) = (1.0 - drtb) * T[itb] + drtb * T[itb + 1];"
NEW = "HES(r, i, cnt) = (double)(float)((1.0 - drtb) * T[itb] + drtb * T[itb + 1]);"
CASES = [("rdx168", (1, 1, 1), 40), ("ice644", (6, 4, 4), 0)]
KW = dict(QEq_tol=1e-12, NMAXQEq=2000)


def rounded_oracle_root(tmp):
    """a copy of oracle/ under tmp whose matrix values are rounded to REAL(4), built; returns the directory that stands in for the repository root"""
    dst = os.path.join(tmp, "oracle")
    os.makedirs(dst)
    for name in ("Makefile", "rxmd_oracle.c"):
        shutil.copy(os.path.join(ROOT, "oracle", name), os.path.join(dst, name))
    src = os.path.join(dst, "rxmd_oracle.c")
    text = open(src).read()
    assert text.count(OLD) == 1, "expected exactly one assignment of a matrix value, found %d" % text.count(OLD)
    open(src, "w").write(text.replace(OLD, NEW))
    subprocess.check_call(["make", "-C", dst, "oracle"])
    return tmp


def main():
    tmp = tempfile.mkdtemp(prefix="f32matrix_")
    try:
        import oracle_api as oa
        assert oa._lib is None, "oracle_api has loaded a library already"
        oa.ROOT = rounded_oracle_root(tmp)
        for case, mc, nsteps in CASES:
            ff, names, frac, lat = oa.make_system(case)
            lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=mc)
            o = oa.Oracle(ff, lat2, ranks, **KW)
            it = o.qeq(); o.force()
            out = dict(gid=o.gids(), q=o.charges(), f=o.forces(), pe=o.energy(), Est=o.trace()[-1, 0], iters=it)
            if nsteps:
                o.step(nsteps)
                out.update(md_steps=nsteps, md_gid=o.gids(), md_pos=o.pos(), md_q=o.charges(), md_Etot=o.kinetic() + o.energy()[0])
            path = os.path.join(HERE, "%s_f32matrix_tight.npz" % case)
            np.savez_compressed(path, **out)
            print("%s: %d atoms, %d CG iterations, Est %.12f, PE %.9f -> %s (%d bytes)" % (case, len(out["gid"]), it, out["Est"], out["pe"][0], os.path.basename(path), os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
