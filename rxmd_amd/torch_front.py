"""ReaxFF energy, forces and charges as functions of a torch CUDA tensor.

`ReaxFF` owns an `RxmdEngine` and hands it the addresses of torch tensors (RxmdEngine.evaluate_device ->
rxmd_hip_evaluate_device): positions never cross to the host, the engine joins torch's current stream with
an event on either side.  `energy(pos)` is a `torch.autograd.Function` whose gradient is minus the force, so
a bias potential, an integrator or a correction model written in torch composes with it.

    model = ReaxFF(ffield, lattice, types)
    out = model.evaluate(pos)           # dict(energy, forces, charges, pe, virial)
    e = model(pos); e.backward()        # pos.grad == -forces
    g = model.bond_graph(bo_min=0.3)    # dict(edge_index [2, E], bond_order [E], edge_vec [E, 3]) of the last evaluate, device tensors

The bond-order graph (`bond_graph`, or `evaluate(pos, bond_graph=bo_min)`) is what FORCE left in the engine's bond tables, compacted on the device
(RxmdEngine.bonds_device -> rxmd_hip_get_bonds_device).  It is NOT differentiable: bond orders and bond vectors come out as constants.

Single rank, plain QEq (isQEq 0 or 1).  No second derivatives, no gradient with respect to the lattice.
This module imports torch; `import rxmd_amd` does not import it.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .engine import RxmdEngine


def _check_bo_min(bo_min):
    """ValueError unless bo_min is a real number (a bool is not); touches no GPU"""
    if isinstance(bo_min, (bool, np.bool_)) or not isinstance(bo_min, (int, float, np.integer, np.floating)):
        raise ValueError("bo_min must be a real number, got %s" % type(bo_min).__name__)
    return float(bo_min)


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

    def evaluate(self, pos, q0=None, bond_graph=None):
        """QEq + FORCE at pos [N, 3] (float64, CUDA, anywhere in space; not modified).  q0: start charges [N] (isQEq = 0: the charges used); None:
        the previous call's solution.  -> energy (0-dim device tensor), forces [N, 3], charges [N] (fresh device tensors), pe[14], virial[6] (CPU).
        bond_graph = <number>: also "bonds" = self.bond_graph(bo_min=<number>), the bond-order graph of this call (constants: not differentiable)"""
        _check_pos(pos, self.natoms, self.device)
        if bond_graph is not None:
            bond_graph = _check_bo_min(bond_graph)
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
        out = dict(energy=energy, forces=forces, charges=charges, pe=torch.from_numpy(pe), virial=torch.from_numpy(vir))
        if bond_graph is not None:
            out["bonds"] = self.bond_graph(bo_min=bond_graph)
        return out

    def bond_graph(self, bo_min=0.0, components=False):
        """The bond-order graph of the last evaluate / energy call (RxmdError -7 before the first, or after set_lattice), as fresh tensors on the
        model's device, produced on torch's current stream:
            edge_index [2, E] int64    (src, dst) in the caller's atom order; directed: a bond appears once from each end (`src < dst` keeps one)
            bond_order [E]    float64  the corrected total bond order BO(0); every entry of the engine's bond lists with bond_order >= bo_min
            edge_vec   [E, 3] float64  r_dst - r_src through the right periodic image: the bond vector itself, wherever in space pos was given
            bond_order_parts [E, 3]    with components=True: sigma, pi, double-pi (they sum to bond_order)
        Edges are ordered by src, then by the engine's list order.  Count, allocate exactly, fill: two short device passes, one host wait each.

        NOT differentiable: these are constants, no gradient reaches pos through them.  For differentiable bond lengths recover the integer image
        shift once and recompute in torch (H = the lattice vectors as columns):
            src, dst = g["edge_index"]
            shift = torch.round((g["edge_vec"] - (pos[dst] - pos[src])) @ torch.linalg.inv(H).T)       # [E, 3] integers, constants
            d = (pos[dst] - pos[src] + shift @ H.T).norm(dim=1)                                       # differentiable in pos"""
        bo_min = _check_bo_min(bo_min)
        if not isinstance(components, (bool, np.bool_)):
            raise ValueError("components must be a bool, got %s" % type(components).__name__)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            E = self.engine.bonds_device(0, 0, 0, 0, bo_min=bo_min, stream=stream)
            kw = dict(device=self.device)
            edge = torch.empty((2, E), dtype=torch.int64, **kw)
            bo = torch.empty(E, dtype=torch.float64, **kw)
            vec = torch.empty((E, 3), dtype=torch.float64, **kw)
            parts = torch.empty((E, 3), dtype=torch.float64, **kw) if components else None
            if E > 0:
                got = self.engine.bonds_device(E, edge[0].data_ptr(), edge[1].data_ptr(), bo.data_ptr(), bo3_ptr=parts.data_ptr() if components else 0,
                                               vec_ptr=vec.data_ptr(), bo_min=bo_min, stream=stream)
                assert got == E, "the bond tables changed between the count and the fill"
        out = dict(edge_index=edge, bond_order=bo, edge_vec=vec)
        if components:
            out["bond_order_parts"] = parts
        return out

    def energy(self, pos):
        """potential energy as a differentiable function of pos: d energy / d pos = -forces (first derivatives only)"""
        return _Energy.apply(pos, self)

    __call__ = energy

    def set_lattice(self, lat):
        self.engine.set_lattice(lat)

    def close(self):
        self.engine.close()
