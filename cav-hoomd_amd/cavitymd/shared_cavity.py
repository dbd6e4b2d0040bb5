"""``SharedCavityForceBatch`` -- several systems of a batch coupled to ONE cavity mode, in two kernel launches.

Collective coupling is what cavity MD is run for: one photon coordinate feels the summed dipole of many molecular cells, so
the Rabi splitting grows with the number of cells.  The cells are small periodic systems with their own boxes, bonds, LJ and
Ewald sums -- the systems of a batch -- and the cavity term is the only force that crosses their boundaries::

    cavity = SharedCavityForceBatch([cell_0, ..., cell_5], cavity_of=[0, 0, 0, 1, 1, 1], params=params)
    cavity.compute()                 # two launches, asynchronous, capturable
    cavity.forces[k]                 # (N_k, 4) device tensor of cell k
    cavity.energies()                # (n_cavities, 3): harmonic, coupling, dipole-self per cavity
    cavity.cell_dipoles              # (B, 3) device tensor: every cell's own dipole

Exactly one system of each cavity, its carrier, holds a particle of the type named ``L``; the photon is the carrier's first
particle of that type (``carriers=`` names the carriers instead, e.g. one that has lost its photon).  A cavity of one cell is ``CavityForceBatch``'s evaluation of that cell, bit
for bit.  ``BatchRecorder``, ``BatchEnergyLedger`` and ``BatchThermalizer`` take the object where they take a
``CavityForceBatch``: the carrier's result block holds the cavity's energies, the other members' hold zero, so the sum of
``universe_total`` over a cavity's members is the cavity's conserved energy (no member is conserved on its own).

There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import HandleOwner, stream_handle
from .batch import _as_params


class _DeviceArray:
    """memory of the library's as a ``__cuda_array_interface__`` exporter (float64, C order)"""

    def __init__(self, ptr: int, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2,
                                         "strides": None}


class SharedCavityForceBatch(HandleOwner):
    """B systems (``SystemDefinition``s whose arrays live on one GPU) in ``max(cavity_of) + 1`` cavities; ``params`` is one
    parameter set ({omegac, couplstr, phmass} or ``_capi.Params``) or one per CAVITY; ``carriers``: None (the systems that hold
    a particle of type 'L' when the object is built) or the system index of each cavity's carrier.  Owns the workspace, the
    library object and the force arrays."""

    def __init__(self, sysdefs, cavity_of, params, carriers=None):
        self._sysdefs = list(sysdefs)
        if not self._sysdefs:
            raise ValueError("a batch needs at least one system")
        self._cavity_of = [int(c) for c in cavity_of]
        if len(self._cavity_of) != len(self._sysdefs) or min(self._cavity_of) < 0:
            raise ValueError("cavity_of: one cavity id >= 0 per system")
        n_cavities = max(self._cavity_of) + 1
        if isinstance(params, (dict, _capi.Params)):
            params = [params] * n_cavities
        params = list(params)
        if len(params) != n_cavities:
            raise ValueError("params: one parameter set, or one per cavity")
        self._params = [_as_params(p) for p in params]
        pds = [s.getParticleData() for s in self._sysdefs]
        dev = pds[0].device
        if dev.type != "cuda" or any(pd.device != dev for pd in pds):
            raise RuntimeError("SharedCavityForceBatch requires every system's particle data in the memory of one GPU (got "
                               f"'{dev}'); no CPU fallback exists in this package")
        self._device = dev
        self._carriers = ({k for k, pd in enumerate(pds) if self._holds_photon(pd)} if carriers is None
                          else {int(k) for k in carriers})
        self._force = [torch.empty((pd.getN(), 4), dtype=torch.float64, device=dev) for pd in pds]
        self._open(dev, lambda ws: _capi.SharedCavity(ws, [self._item(k) for k in range(len(pds))]))
        self._cell_dipoles = torch.as_tensor(_DeviceArray(self._handle.cell_dipoles_device_ptr(), (len(pds), 4)), device=dev)
        torch.cuda.current_stream(dev).synchronize()

    @staticmethod
    def _holds_photon(pd) -> bool:
        try:
            L_typeid = pd.getTypeByName("L")
        except RuntimeError:
            return False
        if pd.getN() == 0:
            return False
        tags = pd.getPositions()[:, 3].cpu().numpy().view(np.uint64) & 0xFFFFFFFF
        return bool((tags == L_typeid).any())

    def _item(self, k: int, cavity=None) -> _capi.SharedCavityItem:
        pd = self._sysdefs[k].getParticleData()
        L_typeid = -1       # a member that is not its cavity's carrier names no photon type
        if k in self._carriers:
            try:
                L_typeid = pd.getTypeByName("L")
            except RuntimeError:
                raise ValueError(f"system {k} is a carrier but has no particle type named 'L'") from None
        n = pd.getN()
        if self._force[k].shape[0] != n:
            self._force[k] = torch.empty((n, 4), dtype=torch.float64, device=self._device)
        cavity = self._cavity_of[k] if cavity is None else int(cavity)
        if not 0 <= cavity < len(self._params):
            raise ValueError(f"system {k}: no parameters for cavity {cavity}")
        return _capi.shared_cavity_item(n, pd.getPositions().data_ptr(), pd.getCharges().data_ptr(), pd.getImages().data_ptr(),
                                        self._force[k].data_ptr(), pd.getGlobalBox().getL(), L_typeid, self._params[cavity], cavity)

    def __len__(self) -> int:
        return len(self._sysdefs)

    # -- following the systems ------------------------------------------------------------------------------------
    def refresh(self, indices=None, cavity_of=None) -> None:
        """Re-register systems whose box or arrays changed, or that move to another cavity (``cavity_of``: {system: cavity}
        or one id per system) -- ``cavmd_shared_cavity_set_items``, which synchronises the stream of the last evaluation and
        validates the whole table, so systems that change cavities together go in one call.  Default: all systems."""
        new = dict(enumerate(cavity_of)) if cavity_of is not None and not isinstance(cavity_of, dict) else dict(cavity_of or {})
        idx = sorted(set(range(len(self)) if indices is None else (int(i) for i in indices)) | {int(k) for k in new})
        if not idx:
            return
        first, last = idx[0], idx[-1]
        items = [self._item(k, new.get(k)) for k in range(first, last + 1)]     # one contiguous range: one validation
        self._need().set_items(first, items)
        for k, c in new.items():
            self._cavity_of[int(k)] = int(c)

    # -- the per-step entry point ---------------------------------------------------------------------------------
    def compute(self, timestep: int = 0, stream=None) -> None:
        """Enqueue the TWO kernels that evaluate every cavity, on ``stream`` (default: torch's current stream).  ``timestep``
        is accepted for signature compatibility with ``CavityForceBatch.compute`` only; it is not used."""
        self._need().compute(stream_handle(stream, self._dev_index))

    # -- results --------------------------------------------------------------------------------------------------
    @property
    def forces(self):
        """Per-system (N_k, 4) float64 device tensors laid out like HOOMD's ``m_force``."""
        return list(self._force)

    @property
    def cell_dipoles(self) -> torch.Tensor:
        """(B, 3) float64 device tensor, a view of the library's array: every system's own dipole d_c of the last evaluation
        (ordered after it on the stream it ran on)."""
        self._need()
        return self._cell_dipoles[:, :3]

    @property
    def n_cavities(self) -> int:
        return self._need().count()

    @property
    def carriers(self):
        """The system index of each cavity's carrier."""
        h = self._need()
        return [h.carrier(c) for c in range(h.count())]

    @property
    def cavity_of(self):
        return list(self._cavity_of)

    def last_sequence(self) -> int:
        return self._need().last_sequence()

    def results(self, stream=None):
        """The B result blocks of the last evaluation, after a wait for ``stream`` (default: torch's current stream)."""
        return self._need().results(stream_handle(stream, self._dev_index))

    def energies(self, stream=None):
        """(n_cavities, 3) array of the last evaluation: harmonic, coupling, dipole-self energy per cavity (its carrier's)."""
        res = self.results(stream)
        return np.array([res[k].energy[:] for k in self.carriers], dtype=np.float64).reshape(-1, 3)

    @property
    def batch(self) -> _capi.SharedCavity:
        return self._handle

    def close(self) -> None:
        self._cell_dipoles = None
        super().close()
