"""``MolecularForceBatch`` -- the harmonic bonds and Lennard-Jones pairs of B independent small systems in ONE kernel launch.

The reference's driver builds every run from the cavity force plus ``hoomd.md.bond.Harmonic`` and
``hoomd.md.pair.LJ(mode='shift')`` over a neighbour list that excludes bonded pairs (examples/05_advanced_run.py:556-596).
This class is those two forces (``cavmd_molecular_compute``; the arithmetic and the summation order are spelled out in
include/cavmd.h) for systems of at most 2048 particles, where every particle looks at every other one out of LDS and no
neighbour list is needed.  Its force arrays are further forces of the integrator's items::

    molecular = MolecularForceBatch(sysdefs, bonds, bond_typeid, harmonic={0: dict(k=0.73204, r0=2.281655158)},
                                    lj={("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=15.0)})
    integrator = VerletBatch(cavity, velocities, extra_forces=[[f] for f in molecular.forces])
    with torch.cuda.graph(graph):
        integrator.step_one(); cavity.compute(); molecular.compute(); integrator.step_two()

Type pairs that are not listed do not interact (the driver switches every pair with the photon 'L' off).  Electrostatics are
``CoulombForceBatch``'s, a further force array of the same integrator.  The expressions restate HOOMD-blue 4.x from knowledge; parity with HOOMD-blue itself is not pinned.  No CPU
fallback: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._force_batch import ForceBatchBase


class MolecularForceBatch(ForceBatchBase):
    """sysdefs: the systems (positions, type ids and boxes are taken from them; all on one GPU, all with the same type
    names); bonds: per system an (n_b, 2) integer array (or None); bond_typeid: per system the (n_b,) bond types;
    harmonic: {bond type: dict(k=, r0=)}; lj: {(type a, type b): dict(epsilon=, sigma=, r_cut=)}, types by name or id, each
    pair listed once; mode: "shift" (the pair energy is 0 at r_cut, as the driver sets) or "none".  ``compute`` is ONE
    kernel; column 3 of a force array is the particle's share of the bond plus pair energy."""

    def __init__(self, sysdefs, bonds, bond_typeid, harmonic, lj, mode: str = "shift"):
        pds = self._systems(sysdefs)
        if mode not in ("shift", "none"):
            raise ValueError("mode is 'shift' or 'none'")
        self._need_gpu(pds, lambda pd: (pd.getPositions(),), "position")
        self._one_device(pds)
        B = len(pds)
        bonds = [None] * B if bonds is None else list(bonds)
        bond_typeid = [None] * B if bond_typeid is None else list(bond_typeid)
        if len(bonds) != B or len(bond_typeid) != B:
            raise ValueError(f"bonds and bond_typeid: one array per system ({B})")
        types = pds[0].types
        if any(pd.types != types for pd in pds):
            raise ValueError("all systems of one batch share their type names")

        def type_id(t) -> int:
            return types.index(t) if isinstance(t, str) else int(t)

        self.params = _capi.molecular_params(
            len(types), {int(t): (p["k"], p["r0"]) for t, p in harmonic.items()},
            {(type_id(a), type_id(b)): (p["epsilon"], p["sigma"], p["r_cut"]) for (a, b), p in lj.items()}, shift=(mode == "shift"))
        sizes = self._allocate(pds)
        items = []
        for k, pd in enumerate(pds):
            b = np.zeros((0, 2), dtype=np.int64) if bonds[k] is None else np.asarray(bonds[k], dtype=np.int64).reshape(-1, 2)
            t = np.zeros(0, dtype=np.int64) if bond_typeid[k] is None else np.asarray(bond_typeid[k], dtype=np.int64).reshape(-1)
            if len(t) != len(b):
                raise ValueError(f"system {k}: {len(b)} bonds but {len(t)} bond types")
            if len(b) and (b.min() < 0 or b.max() >= 2**32 or t.min() < 0):
                raise ValueError(f"system {k}: negative bond index or type")
            triples = np.concatenate([b, t[:, None]], axis=1).astype(np.uint32)
            n = sizes[k]
            items.append(_capi.molecular_item(n, pd.getPositions().data_ptr() if n else 0,
                                              self._force[k].data_ptr() if n else 0, pd.getGlobalBox().getL(), triples))
        self._open(self._device, lambda ws: _capi.Molecular(ws, self.params, items))

    @property
    def molecular(self) -> _capi.Molecular:
        return self._handle
