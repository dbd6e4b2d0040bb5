"""What ``MolecularForceBatch`` and ``CoulombForceBatch`` share: the checks on their systems, the one allocation behind their
force arrays, and the life of their library handle.  A subclass keeps its constructor's own arguments, builds its items
between ``_allocate`` and ``_open``, and names its handle's public attribute."""
from __future__ import annotations

import numpy as np
import torch

from ._device import HandleOwner, one_device, stream_handle


class ForceBatchBase(HandleOwner):
    def _systems(self, sysdefs):
        """The particle data of ``sysdefs`` (kept alive here); an empty batch raises."""
        self._sysdefs = list(sysdefs)
        if not self._sysdefs:
            raise ValueError("a batch needs at least one system")
        return [s.getParticleData() for s in self._sysdefs]

    def _need_gpu(self, pds, arrays, what: str) -> None:
        """``arrays(pd)``, the tensors the kernels read, are in GPU memory; ``what`` names them in the message."""
        for pd in pds:
            for t in arrays(pd):
                if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
                    raise RuntimeError(f"{type(self).__name__} needs the {what} arrays in GPU memory; no CPU fallback exists in "
                                       "this package")

    def _one_device(self, pds) -> None:
        self._device = one_device(pds, "batch")

    def _allocate(self, pds):
        """The force arrays, views of one allocation (the energy is then one segmented sum); returns the sizes."""
        sizes = [pd.getN() for pd in pds]
        self._sizes = sizes
        self._pool = torch.zeros((max(sum(sizes), 1), 4), dtype=torch.float64, device=self._device)
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._force = [self._pool[int(starts[k]):int(starts[k + 1])] for k in range(len(sizes))]
        self._lengths = torch.tensor(sizes, dtype=torch.int64, device=self._device)
        return sizes

    def _open(self, device, make_handle) -> None:
        """``make_handle(workspace)`` creates the library object over the items."""
        super()._open(device, make_handle)
        self.n_systems = len(self._sizes)
        torch.cuda.current_stream(self._device).synchronize()   # the zeroed pool is there before any stream computes

    def __len__(self) -> int:
        return self.n_systems

    def compute(self, timestep: int = 0, stream=None) -> None:
        """The object's launches on ``stream`` (default: torch's current stream): every entry of every system's force array.
        May be captured.  ``timestep`` is accepted for signature compatibility with ``CavityForceBatch.compute``; it is not
        used."""
        self._need().compute(stream_handle(stream, self._dev_index))

    @property
    def forces(self):
        """Per-system (N_k, 4) float64 device tensors: force in columns 0-2, the particle's share of the potential energy
        in column 3."""
        return list(self._force)

    def potential_energy(self) -> torch.Tensor:
        """(B,) device tensor: the energy of every system, the sum of its ``.w`` column, ordered on torch's current stream
        (the kernels keep no totals across workgroups)."""
        self._need()
        return self._pool_energy(self._pool)

    def _pool_energy(self, pool) -> torch.Tensor:
        """the per-system sums of the ``.w`` column of one allocation laid out like ``_pool``"""
        w = pool[:sum(self._sizes), 3]
        if len(set(self._sizes)) == 1 and self._sizes[0] > 0:
            return w.reshape(self.n_systems, self._sizes[0]).sum(dim=1)
        return torch.segment_reduce(w.contiguous(), "sum", lengths=self._lengths)
