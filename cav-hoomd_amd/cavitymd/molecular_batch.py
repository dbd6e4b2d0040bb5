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
import torch

from . import _capi
from ._device import stream_handle


class MolecularForceBatch:
    """sysdefs: the systems (positions, type ids and boxes are taken from them; all on one GPU, all with the same type
    names); bonds: per system an (n_b, 2) integer array (or None); bond_typeid: per system the (n_b,) bond types;
    harmonic: {bond type: dict(k=, r0=)}; lj: {(type a, type b): dict(epsilon=, sigma=, r_cut=)}, types by name or id, each
    pair listed once; mode: "shift" (the pair energy is 0 at r_cut, as the driver sets) or "none"."""

    def __init__(self, sysdefs, bonds, bond_typeid, harmonic, lj, mode: str = "shift"):
        self._sysdefs = list(sysdefs)
        if not self._sysdefs:
            raise ValueError("a batch needs at least one system")
        if mode not in ("shift", "none"):
            raise ValueError("mode is 'shift' or 'none'")
        pds = [s.getParticleData() for s in self._sysdefs]
        for pd in pds:
            pos = pd.getPositions()
            if not isinstance(pos, torch.Tensor) or pos.device.type != "cuda":
                raise RuntimeError("MolecularForceBatch needs the position arrays in GPU memory; no CPU fallback exists in this "
                                   "package")
        dev = pds[0].device
        if any(pd.device != dev for pd in pds):
            raise ValueError("all systems of one batch live on one device")
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
        self._device = dev
        self._dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        sizes = [pd.getN() for pd in pds]
        self._sizes = sizes
        # one allocation behind all force arrays: the energy is then one segmented sum
        self._pool = torch.zeros((max(sum(sizes), 1), 4), dtype=torch.float64, device=dev)
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._force = [self._pool[int(starts[k]):int(starts[k + 1])] for k in range(B)]
        self._lengths = torch.tensor(sizes, dtype=torch.int64, device=dev)
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
        self._ws = _capi.Workspace(1, device=self._dev_index)
        self._molecular = _capi.Molecular(self._ws, self.params, items)
        self.n_systems = B
        torch.cuda.current_stream(dev).synchronize()   # the zeroed pool is there before any stream computes

    def __len__(self) -> int:
        return self.n_systems

    def _need(self):
        if self._molecular is None:
            raise RuntimeError("MolecularForceBatch used after close()")

    def compute(self, timestep: int = 0, stream=None) -> None:
        """ONE kernel on ``stream`` (default: torch's current stream): every entry of every system's force array.  May be
        captured.  ``timestep`` is accepted for signature compatibility with ``CavityForceBatch.compute``; it is not used."""
        self._need()
        self._molecular.compute(stream_handle(stream, self._device))

    @property
    def forces(self):
        """Per-system (N_k, 4) float64 device tensors: force in columns 0-2, the particle's share of the potential energy
        in column 3."""
        return list(self._force)

    def potential_energy(self) -> torch.Tensor:
        """(B,) device tensor: bond plus pair energy of every system, the sum of its ``.w`` column, ordered on torch's current
        stream (the kernel keeps no totals across workgroups)."""
        self._need()
        w = self._pool[:sum(self._sizes), 3]
        if len(set(self._sizes)) == 1 and self._sizes[0] > 0:
            return w.reshape(self.n_systems, self._sizes[0]).sum(dim=1)
        return torch.segment_reduce(w.contiguous(), "sum", lengths=self._lengths)

    @property
    def molecular(self) -> _capi.Molecular:
        return self._molecular

    def close(self) -> None:
        if getattr(self, "_molecular", None) is not None:
            self._molecular.close()
        if getattr(self, "_ws", None) is not None:
            self._ws.close()
        self._molecular = self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
