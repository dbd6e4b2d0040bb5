"""``CavityForceBatch`` -- many independent small systems evaluated by ONE kernel launch.

The reference's production workload is N = 501 particles run as 500 independent replicas: a loop over replica ids in one
process, or one SLURM array task per replica (examples/05_advanced_run.py:1336-1351, 1570-1612; submit.sh:3).  One such
system is a single 256-thread workgroup on the GPU -- one CU of 256.  A caller that holds several replicas on one GPU
registers them once as a batch (``cavmd_batch_create``) and evaluates all of them with one launch, one workgroup per
system; every system's forces and result block are, bit for bit, what ``CavityForceComputeHIP`` gives for it alone::

    batch = CavityForceBatch([sysdef_1, ..., sysdef_B], params)      # params: one dict or B dicts {omegac, couplstr, phmass}
    history = batch.history()
    for step in range(n_steps):
        batch.compute()                                               # one launch, asynchronous
        history.record(step)
        for timestep, energies in history.drain():                    # energies: (B, 3), every recorded step but the newest
            ...
    batch.forces[k]                                                   # (N_k, 4) device tensor of system k

There is no CPU fallback.
"""
from __future__ import annotations

from collections import deque

import torch

from . import _capi
from ._capi import CavmdError
from ._device import HandleOwner, stream_handle


def _as_params(p) -> _capi.Params:
    if isinstance(p, _capi.Params):
        return p
    return _capi.make_params(p["omegac"], p["couplstr"], p.get("phmass", 1.0))


class BatchEnergyHistory:
    """``EnergyHistory`` (history.py) for a batch: rows ``(timestep, energies)`` with ``energies`` a ``(B, 3)`` array
    (harmonic, coupling, dipole-self per system), read from the batch's result ring one step late so that the host never
    waits for the evaluation it has just enqueued.  ``batch`` is anything with ``last_sequence()`` and
    ``energies_at(sequence)``.  A step whose slot has been reused or whose evaluation failed raises :class:`CavmdError`
    once; rows read before it are returned by the next ``drain()`` / ``flush()``."""

    def __init__(self, batch):
        self._batch = batch
        self._pending = deque()  # (timestep, sequence), oldest first
        self._rows = []

    def record(self, timestep: int) -> None:
        """Note that the evaluation enqueued last belongs to ``timestep``.  Call after each ``compute()``."""
        self._pending.append((int(timestep), int(self._batch.last_sequence())))

    def __len__(self) -> int:
        return len(self._pending) + len(self._rows)

    def _read(self, keep: int):
        while len(self._pending) > keep:
            timestep, seq = self._pending[0]
            try:
                e = self._batch.energies_at(seq)
            except CavmdError:
                self._pending.popleft()  # reported once, here
                raise
            self._pending.popleft()
            self._rows.append((timestep, e))
        rows, self._rows = self._rows, []
        return rows

    def drain(self):
        """Rows of every recorded step except the newest, oldest first; they are forgotten."""
        return self._read(1)

    def flush(self):
        """Rows of every recorded step, the newest included (waits for it); the history is then empty."""
        return self._read(0)


class CavityForceBatch(HandleOwner):
    """B systems (``SystemDefinition``s whose arrays live on one GPU), one launch per ``compute()``.  Owns the workspace,
    the batch and the force arrays."""

    def __init__(self, sysdefs, params, history_depth: int = 64):
        self._sysdefs = list(sysdefs)
        if not self._sysdefs:
            raise ValueError("a batch needs at least one system")
        if isinstance(params, (dict, _capi.Params)):
            params = [params] * len(self._sysdefs)
        params = list(params)
        if len(params) != len(self._sysdefs):
            raise ValueError("params: one parameter set, or one per system")
        self._params = [_as_params(p) for p in params]
        pds = [s.getParticleData() for s in self._sysdefs]
        dev = pds[0].device
        if dev.type != "cuda" or any(pd.device != dev for pd in pds):
            raise RuntimeError("CavityForceBatch requires every system's particle data in the memory of one GPU (got "
                               f"'{dev}'); no CPU fallback exists in this package")
        self._device = dev
        self._force = [torch.empty((pd.getN(), 4), dtype=torch.float64, device=dev) for pd in pds]
        self._open(dev, lambda ws: _capi.Batch(ws, [self._item(k) for k in range(len(pds))], history_depth))

    def _item(self, k: int) -> _capi.BatchItem:
        pd = self._sysdefs[k].getParticleData()
        try:
            L_typeid = pd.getTypeByName("L")
        except RuntimeError:
            L_typeid = -1  # no type named 'L': matches no particle, the no-photon path (as CavityForceComputeHIP)
        n = pd.getN()
        if self._force[k].shape[0] != n:
            self._force[k] = torch.empty((n, 4), dtype=torch.float64, device=self._device)
        return _capi.batch_item(n, pd.getPositions().data_ptr(), pd.getCharges().data_ptr(), pd.getImages().data_ptr(),
                                self._force[k].data_ptr(), pd.getGlobalBox().getL(), L_typeid, self._params[k])

    def __len__(self) -> int:
        return len(self._sysdefs)

    # -- following the systems ------------------------------------------------------------------------------------
    def refresh(self, indices=None) -> None:
        """Re-register systems whose box, arrays or parameters changed (``cavmd_batch_set_items``; synchronises the
        stream of the last evaluation).  Default: all."""
        idx = range(len(self)) if indices is None else sorted(int(i) for i in indices)
        for k in idx:
            self._need().set_items(k, [self._item(k)])

    def setParams(self, k: int, omegac: float, couplstr: float, phmass: float = 1.0) -> None:
        self._params[k] = _capi.make_params(omegac, couplstr, phmass)
        self.refresh([k])

    # -- the per-step entry point ---------------------------------------------------------------------------------
    def compute(self, timestep: int = 0, stream=None) -> None:
        """Enqueue ONE kernel that evaluates every system, on ``stream`` (default: torch's current stream).  ``timestep`` is
        accepted for signature compatibility with ``CavityForceComputeHIP.compute`` only; it is not used."""
        self._need().compute(stream_handle(stream, self._dev_index))

    # -- results --------------------------------------------------------------------------------------------------
    @property
    def forces(self):
        """Per-system (N_k, 4) float64 device tensors laid out like HOOMD's ``m_force``."""
        return list(self._force)

    def last_sequence(self) -> int:
        return self._need().last_sequence()

    def energies(self):
        """(B, 3) array of the last evaluation: harmonic, coupling, dipole-self energy per system."""
        import numpy as np
        return np.array([r.energy[:] for r in self._need().results()], dtype=np.float64).reshape(len(self), 3)

    def energies_at(self, sequence: int):
        return self._need().energies_at(sequence)

    def results(self):
        return self._need().results()

    def results_at(self, sequence: int):
        return self._need().results_at(sequence)

    def history(self, depth=None) -> BatchEnergyHistory:
        """Record-then-drain bookkeeping over this batch's result ring.  ``depth`` (if given) must not exceed the ring the
        batch was created with (``history_depth``): that many steps may be recorded between drains."""
        if depth is not None and int(depth) > self._need().history_depth:
            raise ValueError(f"history depth {depth} exceeds the batch's result ring ({self._need().history_depth}); "
                             "create the batch with a larger history_depth")
        return BatchEnergyHistory(self)

    @property
    def batch(self) -> _capi.Batch:
        return self._handle
