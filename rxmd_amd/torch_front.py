"""ReaxFF energy, forces and charges as functions of a torch CUDA tensor.

`ReaxFF` owns an `RxmdEngine` and hands it the addresses of torch tensors (RxmdEngine.evaluate_device ->
rxmd_hip_evaluate_device): positions never cross to the host, the engine joins torch's current stream with
an event on either side.  `energy(pos)` is a `torch.autograd.Function` whose gradient is minus the force, so
a bias potential, an integrator or a correction model written in torch composes with it.

    model = ReaxFF(ffield, lattice, types)
    out = model.evaluate(pos)           # dict(energy, forces, charges, pe, virial)
    e = model(pos); e.backward()        # pos.grad == -forces

Single rank, plain QEq (isQEq 0 or 1).  No second derivatives, no gradient with respect to the lattice.
This module imports torch; `import rxmd_amd` does not import it.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .engine import RxmdEngine


def _check_pos(pos, natoms, device):
    """ValueError unless pos is a float64 CUDA tensor [natoms, 3] on `device`; touches no GPU"""
    if not isinstance(pos, torch.Tensor):
        raise ValueError("pos must be a torch.Tensor, got %s" % type(pos).__name__)
    if pos.dtype != torch.float64:
        raise ValueError("pos must be float64, got %s" % pos.dtype)
    if pos.dim() != 2 or pos.shape[0] != natoms or pos.shape[1] != 3:
        raise ValueError("pos must have shape [%d, 3], got %s" % (natoms, list(pos.shape)))
    if not pos.is_cuda or pos.device != device:
        raise ValueError("pos must be a CUDA tensor on %s, got one on %s" % (device, pos.device))


class _Energy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, model):
        out = model.evaluate(pos.detach())
        ctx.save_for_backward(out["forces"])
        return out["energy"]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        (forces,) = ctx.saved_tensors
        return -forces * grad_output, None


class ReaxFF:
    """types: int tensor or array [N] of ffield atom types (1..nso), moved to the device once; gid: optional int64 global ids (default
    1..N); engine_kw: the keywords of RxmdEngine (isQEq, QEq_tol, NMAXQEq, device, ...)"""

    def __init__(self, ffield, lattice, types, gid=None, **engine_kw):
        self.engine = RxmdEngine(ffield, lattice, **engine_kw)      # RxmdError(-6) without a GPU, before torch is asked for one
        self.device = torch.device("cuda", int(engine_kw.get("device", 0)))
        self.set_atoms(types, gid)

    def set_atoms(self, types, gid=None):
        """replace the atom list (order, types, global ids).  The first evaluate sizes the engine; later lists may be shorter or longer within
        that capacity (RxmdError -3 above it)"""
        as_dev = lambda a, dt: (a.detach() if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a))).to(dtype=dt, device=self.device).contiguous()
        types = as_dev(types, torch.int32)
        gid = None if gid is None else as_dev(gid, torch.int64)
        if types.dim() != 1 or types.shape[0] < 1 or (gid is not None and gid.shape != types.shape):
            raise ValueError("types must be one-dimensional and not empty, and gid must match it")
        self.types, self.gid, self.natoms = types, gid, int(types.shape[0])

    def evaluate(self, pos, q0=None):
        """QEq + FORCE at pos [N, 3] (float64, CUDA, anywhere in space; not modified).  q0: start charges [N] (isQEq = 0: the charges used); None:
        the previous call's solution.  -> energy (0-dim device tensor), forces [N, 3], charges [N] (fresh device tensors), pe[14], virial[6] (CPU)"""
        _check_pos(pos, self.natoms, self.device)
        if q0 is not None:
            if not isinstance(q0, torch.Tensor) or q0.dtype != torch.float64 or q0.shape != (self.natoms,) or q0.device != self.device:
                raise ValueError("q0 must be a float64 CUDA tensor of shape [%d] on %s" % (self.natoms, self.device))
            q0 = q0.detach().contiguous()
        p = pos.detach().contiguous()
        with torch.cuda.device(self.device):
            forces = torch.empty((self.natoms, 3), dtype=torch.float64, device=self.device)
            charges = torch.empty(self.natoms, dtype=torch.float64, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            pe, vir = self.engine.evaluate_device(self.natoms, self.types.data_ptr(), p.data_ptr(), forces.data_ptr(), charges.data_ptr(),
                                                  gid_ptr=0 if self.gid is None else self.gid.data_ptr(), q_in_ptr=0 if q0 is None else q0.data_ptr(), stream=stream)
            energy = torch.tensor(pe[0], dtype=torch.float64, device=self.device)
        return dict(energy=energy, forces=forces, charges=charges, pe=torch.from_numpy(pe), virial=torch.from_numpy(vir))

    def energy(self, pos):
        """potential energy as a differentiable function of pos: d energy / d pos = -forces (first derivatives only)"""
        return _Energy.apply(pos, self)

    __call__ = energy

    def set_lattice(self, lat):
        self.engine.set_lattice(lat)

    def close(self):
        self.engine.close()
