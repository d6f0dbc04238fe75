"""ReaxFF energy, forces and charges as functions of a torch CUDA tensor.

`ReaxFF` owns an `RxmdEngine` and hands it the addresses of torch tensors (RxmdEngine.evaluate_device ->
rxmd_hip_evaluate_device): positions never cross to the host, the engine joins torch's current stream with
an event on either side.  `energy(pos)` is a `torch.autograd.Function` whose gradient is minus the force, so
a bias potential, an integrator or a correction model written in torch composes with it.

    model = ReaxFF(ffield, lattice, types)
    out = model.evaluate(pos)           # dict(energy, forces, charges, pe, virial)
    e = model(pos); e.backward()        # pos.grad == -forces
    g = model.bond_graph(bo_min=0.3)    # dict(edge_index [2, E], bond_order [E], edge_vec [E, 3]) of the last evaluate, device tensors

    b = model.bond_orders(pos, bo_min=0.3)   # the same graph of a fresh evaluate, DIFFERENTIABLE in pos (with energy, forces, charges)
    p = model.pair_graph(6.0, pos=pos)       # the radius graph of the last evaluate: dict(edge_index [2, E], shifts [E, 3], vec [E, 3]), vec
                                             # differentiable in pos by plain autograd; values=True adds h [E], the QEq matrix value per edge

The bond-order graph (`bond_graph`, or `evaluate(pos, bond_graph=bo_min)`) is what FORCE left in the engine's bond tables, compacted on the device
(RxmdEngine.bonds_device -> rxmd_hip_get_bonds_device).  From those two calls it is NOT differentiable: bond orders and bond vectors come out as
constants.  `bond_orders(pos)` returns the same arrays as outputs of one `torch.autograd.Function` whose backward is the engine's vector-Jacobian
product (RxmdEngine.bonds_vjp_device -> rxmd_hip_bonds_vjp_device): a restraint on a bond order or a coordination number, a reaction-coordinate
loss or a model trained on bond orders sends its gradient to pos.  The backward reads the engine's state of that evaluation, so it has to run
before the model evaluates again (RuntimeError otherwise).

Single rank, plain QEq (isQEq 0 or 1).  No second derivatives, no gradient with respect to the lattice.
This module imports torch; `import rxmd_amd` does not import it.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .engine import RxmdEngine


def _check_real(name, v):
    """ValueError unless v is a real number (a bool is not) -> float(v); touches no GPU"""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a real number, got %s" % (name, type(v).__name__))
    return float(v)


def _check_bool(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s must be a bool, got %s" % (name, type(v).__name__))


def _check_bo_min(bo_min):
    return _check_real("bo_min", bo_min)


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


class _BondOrders(torch.autograd.Function):
    """one evaluate + one graph extraction; outputs: energy, bond_order, edge_vec, bond_order_parts (None without components) -- differentiable --
    and edge_index, forces, charges (constants).  backward: -forces g_E + the engine's VJP of (g_bo, g_parts, g_vec); an output the loss did not
    use arrives as None and goes to the engine as NULL"""

    @staticmethod
    def forward(ctx, pos, model, bo_min, components, q0):
        out = model.evaluate(pos.detach(), q0=q0)
        g = model.bond_graph(bo_min=bo_min, components=components)
        ctx.model, ctx.bo_min, ctx.serial = model, bo_min, model._evaluations
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(out["forces"])
        ctx.mark_non_differentiable(g["edge_index"], out["forces"], out["charges"])
        return out["energy"], g["bond_order"], g["edge_vec"], g.get("bond_order_parts"), g["edge_index"], out["forces"], out["charges"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_energy, g_bo, g_vec, g_parts, *unused):
        model = ctx.model
        if ctx.serial != model._evaluations:
            raise RuntimeError("the engine no longer holds the state these bond orders came from (evaluate / energy / bond_orders / set_lattice ran on "
                               "the model since): call backward before the next evaluation")
        (forces,) = ctx.saved_tensors
        grad = None if g_energy is None else -forces * g_energy
        given = [None if g is None else g.to(torch.float64).contiguous() for g in (g_bo, g_parts, g_vec)]
        E = next((int(g.shape[0]) for g in given if g is not None), 0)
        if E > 0:
            with torch.cuda.device(model.device):
                gpos = torch.empty((model.natoms, 3), dtype=torch.float64, device=model.device)
                ptr = [0 if g is None else g.data_ptr() for g in given]
                model.engine.bonds_vjp_device(E, gpos.data_ptr(), grad_bo_ptr=ptr[0], grad_bo3_ptr=ptr[1], grad_vec_ptr=ptr[2], bo_min=ctx.bo_min,
                                              stream=torch.cuda.current_stream(model.device).cuda_stream)
            grad = gpos if grad is None else grad + gpos
        return grad, None, None, None, None


class ReaxFF:
    """types: int tensor or array [N] of ffield atom types (1..nso), moved to the device once; gid: optional int64 global ids (default
    1..N); engine_kw: the keywords of RxmdEngine (isQEq, QEq_tol, NMAXQEq, device, ...)"""

    _evaluations = 0      # evaluations (and lattice changes) so far: a backward of bond_orders checks that the engine still holds its state

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
        self._evaluations += 1
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

        NOT differentiable: these are constants, no gradient reaches pos through them (bond_orders(pos) returns the same graph with gradients).  For
        differentiable bond lengths alone, recover the integer image shift once and recompute in torch (H = the lattice vectors as columns):
            src, dst = g["edge_index"]
            shift = torch.round((g["edge_vec"] - (pos[dst] - pos[src])) @ torch.linalg.inv(H).T)       # [E, 3] integers, constants
            d = (pos[dst] - pos[src] + shift @ H.T).norm(dim=1)                                       # differentiable in pos"""
        bo_min = _check_bo_min(bo_min)
        _check_bool("components", components)
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

    def cell(self):
        """the lattice vectors of the engine's box as the ROWS of a [3, 3] float64 tensor on the model's device (a constant)"""
        la, lb, lc, al, be, ga = self.engine.lattice
        ca, cb, cg, sg = (np.cos(np.radians(al)), np.cos(np.radians(be)), np.cos(np.radians(ga)), np.sin(np.radians(ga)))
        h2 = lc * np.sqrt(1.0 - ca * ca - cb * cb - cg * cg + 2.0 * ca * cb * cg) / sg
        rows = [[la, 0.0, 0.0], [lb * cg, lb * sg, 0.0], [lc * cb, lc * (ca - cb * cg) / sg, h2]]      # GetBoxParams, init.F90:610-633
        return torch.tensor(rows, dtype=torch.float64, device=self.device)

    def pair_graph(self, r_cut, pos=None, values=False, cell=None):
        """The radius graph of the last evaluate / energy call -- the engine's own 10 A list, every pair with |vec| <= r_cut through every periodic
        image within reach (r_cut <= 0: the whole list; above the taper cut-off, 10 A: RxmdError -1; RxmdError -7 before the first evaluate or
        after set_lattice) -- as fresh tensors on the model's device, produced on torch's current stream:
            edge_index [2, E] int64    (src, dst) in the caller's atom order; directed, and one edge per image: in a small box a pair repeats
            shifts     [E, 3] int64    the image n of dst: vec = pos[dst] - pos[src] + n @ cell (cell: lattice vectors as rows)
            vec        [E, 3] float64  r_dst - r_src through that image
            h          [E]    float64  with values=True: the QEq matrix value of the pair (edge_index + h = the off-diagonal part of the QEq operator
                                       as a COO matrix; its diagonal is the ffield's eta)
        Edges are ordered by src, then by the engine's list order.  Count, allocate exactly, fill: two device passes, one host wait each.
        Without pos: shifts refer to the engine's wrapped positions and every tensor is a constant.  With pos = the tensor of the last evaluate
        (anywhere in space, possibly requiring grad): shifts are re-expressed for those coordinates -- n' = rint((vec - (pos[dst] - pos[src])) cell^-1),
        an exact integer recovery -- and vec is RETURNED AS pos[dst] - pos[src] + n' @ cell, computed in torch: differentiable in pos, and in `cell`
        when that is given as a [3, 3] tensor (default: the engine's lattice, a constant), by plain autograd.  edge_index, shifts and h are constants:
        which pairs are selected is not differentiated, and h carries no gradient (no dH/dr)."""
        r_cut = _check_real("r_cut", r_cut)
        _check_bool("values", values)
        if pos is not None:
            _check_pos(pos, self.natoms, self.device)
        if cell is not None and (not isinstance(cell, torch.Tensor) or cell.dtype != torch.float64 or cell.shape != (3, 3) or cell.device != self.device):
            raise ValueError("cell must be a float64 tensor of shape [3, 3] on %s (lattice vectors as rows)" % self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            E = self.engine.pairs_device(0, 0, 0, r_cut=r_cut, stream=stream)
            kw = dict(device=self.device)
            edge = torch.empty((2, E), dtype=torch.int64, **kw)
            shift32 = torch.empty((E, 3), dtype=torch.int32, **kw)
            vec = torch.empty((E, 3), dtype=torch.float64, **kw)
            h = torch.empty(E, dtype=torch.float64, **kw) if values else None
            if E > 0:
                got = self.engine.pairs_device(E, edge[0].data_ptr(), edge[1].data_ptr(), shift_ptr=shift32.data_ptr(), vec_ptr=vec.data_ptr(),
                                               h_ptr=h.data_ptr() if values else 0, r_cut=r_cut, stream=stream)
                assert got == E, "the 10 A list changed between the count and the fill"
            shifts = shift32.to(torch.int64)
            if pos is not None:
                c = self.cell() if cell is None else cell
                d = pos[edge[1]] - pos[edge[0]]
                shifts = torch.round((vec - d.detach()) @ torch.linalg.inv(c.detach())).to(torch.int64)
                vec = d + shifts.to(torch.float64) @ c
        out = dict(edge_index=edge, shifts=shifts, vec=vec)
        if values:
            out["h"] = h
        return out

    def bond_orders(self, pos, bo_min=0.0, components=False, q0=None):
        """One evaluate at pos and the bond-order graph of it, differentiable in pos -> dict of
            energy           0-dim, differentiable (d energy / d pos = -forces)
            edge_index       [2, E] int64, a constant: which entries are selected (bond_order >= bo_min) is not differentiated
            bond_order       [E], edge_vec [E, 3], and with components=True bond_order_parts [E, 3] (sigma, pi, double-pi): differentiable
            forces [N, 3], charges [N]   constants, as from evaluate
        in the layout of bond_graph.  The derivative of a corrected bond order reaches through the neighbour shells of both atoms; it comes from the
        engine (rxmd_hip_bonds_vjp_device), first derivatives only.  A coordination number is `torch.zeros(N).index_add(0, edge_index[0], bond_order)`.
        backward() must run before the next evaluate / energy / bond_orders / set_lattice on this model: the engine keeps ONE state, and a backward
        that finds another raises RuntimeError -- nothing is evaluated again behind the caller's back."""
        _check_pos(pos, self.natoms, self.device)
        bo_min = _check_bo_min(bo_min)
        _check_bool("components", components)
        energy, bo, vec, parts, edge, forces, charges = _BondOrders.apply(pos, self, bo_min, bool(components), q0)
        out = dict(energy=energy, edge_index=edge, bond_order=bo, edge_vec=vec, forces=forces, charges=charges)
        if components:
            out["bond_order_parts"] = parts
        return out

    def energy(self, pos):
        """potential energy as a differentiable function of pos: d energy / d pos = -forces (first derivatives only)"""
        return _Energy.apply(pos, self)

    __call__ = energy

    def set_lattice(self, lat):
        self._evaluations += 1
        self.engine.set_lattice(lat)

    def close(self):
        self.engine.close()
