"""Run by test_gpu_streams_by_place.py in a process of its own with RXMD_POISON_ALLOC=1 (read once per process): the perturbed RDX 6 x 6 x 6 run of that
module with the streams laid out by place, its results written to the .npz named on the command line."""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import pytest
from parity import perturbed_rdx, run

assert os.environ.get("RXMD_POISON_ALLOC") == "1"
mp = pytest.MonkeyPatch()
try:
    ff, lat, rec = perturbed_rdx((6, 6, 6))
    r = run(ff, lat, rec, 1, mp)
finally:
    mp.undo()
np.savez(sys.argv[1], layout=r["layout"], tap14=r["tap14"], win_groups=r["stats"]["win_groups"], iters=r["iters"],
         **{k: r[k] for k in ("est0", "q0", "rows0", "est", "q", "pos", "rows", "f0", "f")})
print("PLACE-POISON-OK")
