"""``BatchRecorder`` -- the per-step observables of B independent small systems, appended by ONE kernel launch per step to a
time series in device memory.

What the reference's trackers write every step for every replica -- ``EnergyTracker`` (src/cavitymd/analysis.py:425-),
``CavityModeTracker`` (:1285-1417), ``DipoleAutocorrelation`` (:1424-) and the reduction of ``AdaptiveTimestepUpdater``
(src/cavitymd/simulation.py:66-92) -- is one 128-byte row per system here (``cavmd_record``): the three cavity energies, the
total dipole, the photon position, the cavity mode's kinetic energy and temperature, the group's kinetic energy and
``S = sum |F_i| / m_i``.  The write position lives on the device, so ``record()`` captured into a graph next to
``CavityForceBatch.compute`` and ``BussiReservoirBatch.step_async`` appends a NEW row on every replay::

    recorder = BatchRecorder(forces, velocities, net_forces=forces.forces)
    with torch.cuda.graph(graph):
        forces.compute()
        recorder.record()
        thermostat.step_async()
    for _ in range(steps):
        graph.replay()
    series = recorder.read()              # (B, steps) structured array, one copy, behind one synchronisation
    series["energy"][:, :, 0]             # harmonic energy of every system at every step

There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import Checkpointable, HandleOwner, device_tensor, member_indices, stream_handle
from .utils import PhysicalConstants


def _device_tensor(t, what: str):
    return device_tensor(t, "BatchRecorder", what, note=" (HOOMD Scalar4)")


class _SeriesRecorder(HandleOwner, Checkpointable):
    """What ``BatchRecorder`` and ``BatchFieldRecorder`` share: the stream a read waits for and the default window of
    ``read()``.  A subclass opens its recorder and sets ``n_systems``, ``capacity`` and ``_record_dtype`` (a function that
    gives the numpy dtype of one row)."""

    def _read_stream(self, stream) -> int:
        """The stream a read synchronises.  Default: the whole device first (a graph replays on the stream it is launched
        on, which need not be the one ``record`` was captured on), then torch's current stream."""
        if stream is None:
            torch.cuda.synchronize(self._device)
        return stream_handle(stream, self._dev_index)

    def rows(self, stream=None) -> np.ndarray:
        """Rows written per system since creation / reset, behind a synchronisation (see ``read``)."""
        return self._need().rows(self._read_stream(stream))

    def _read(self, first, count, stream) -> np.ndarray:
        """first=None: the oldest row still held; count=None: up to the last row every system has."""
        recorder = self._need()
        handle = self._read_stream(stream)
        if first is None or count is None:
            rows = recorder.rows(handle)
            if first is None:
                first = max(int(rows.max()) - self.capacity, 0)
            if count is None:
                count = int(rows.min()) - int(first)
            if count <= 0:
                return np.zeros((self.n_systems, 0), dtype=self._record_dtype())
        return recorder.read(handle, 0, self.n_systems, int(first), int(count))

    def reset(self, stream=None) -> None:
        """Zero every system's counters (a field recorder's references with them), ordered on ``stream`` (default: torch's
        current stream)."""
        self._need().reset(stream_handle(stream, self._dev_index))

    @property
    def recorder(self):
        return self._handle


class BatchRecorder(_SeriesRecorder):
    """force_batch: the ``CavityForceBatch`` whose result blocks are recorded; velocities: one (N_k, 4) device tensor per
    system (mass in column 3), or None per system; net_forces: the same for the net force (None: ``force_mass_sum`` is 0);
    members: None, or per system None / an index array of the group ``kinetic_energy`` covers.  An item keeps its last
    ``capacity`` rows; every ``period``-th ``record()`` writes one."""
    _record_dtype = staticmethod(_capi.record_dtype)

    def __init__(self, force_batch, velocities, net_forces=None, members=None, capacity: int = 4096, period: int = 1,
                 kB: float = PhysicalConstants.KB_HARTREE_PER_K):
        velocities = list(velocities)
        for what, arrays in (("velocity", velocities), ("net-force", [] if net_forces is None else list(net_forces))):
            for t in arrays:
                if t is not None:
                    _device_tensor(t, what)   # CPU tensors are refused before anything else is looked at
        B = len(force_batch)
        net_forces = [None] * B if net_forces is None else list(net_forces)
        members = [None] * B if members is None else list(members)
        if len(velocities) != B or len(net_forces) != B or len(members) != B:
            raise ValueError(f"velocities, net_forces and members: one entry per system of the force batch ({B})")
        sizes = force_batch.batch.sizes
        dev = None
        for k, (v, f) in enumerate(zip(velocities, net_forces)):
            for t, what in ((v, "velocity"), (f, "net-force")):
                if t is None:
                    continue
                _device_tensor(t, what)
                dev = t.device if dev is None else dev
                if t.device != dev:
                    raise ValueError("all systems of one recorder live on one device")
                if t.shape[0] != sizes[k]:
                    raise ValueError(f"system {k}: the {what} array has {t.shape[0]} rows, the force batch evaluates {sizes[k]}")
        if dev is None:
            dev = force_batch.forces[0].device
            if dev.type != "cuda":
                raise RuntimeError("BatchRecorder needs its arrays in GPU memory; no CPU fallback exists in this package")
        self._force_batch = force_batch
        self._velocities, self._net_forces, self._members = velocities, net_forces, []
        results = force_batch.batch.results_device_ptr()
        result_bytes = 192
        items = []
        for k in range(B):
            v, f, m = velocities[k], net_forces[k], members[k]
            n = int(sizes[k])
            if m is None:
                mt, n_members = None, (n if v is not None else 0)
            else:
                mt, n_members = member_indices(m, n, dev)
            self._members.append(mt)
            items.append(_capi.recorder_item(results + result_bytes * k,
                                             v.data_ptr() if (v is not None and n) else 0,
                                             f.data_ptr() if (f is not None and n) else 0,
                                             mt.data_ptr() if (mt is not None and n_members) else 0,
                                             n if (v is not None and f is not None) else 0, n_members))
        self._open(dev, lambda ws: _capi.Recorder(ws, items, capacity, period, kB))
        self.n_systems = B
        self.capacity, self.period = int(capacity), int(period)
        self._stream = 0
        torch.cuda.current_stream(dev).synchronize()   # the member lists are on the device before any stream records

    def record(self, stream=None) -> None:
        """ONE kernel launch on ``stream`` (default: torch's current stream): nothing is waited for; may be captured."""
        recorder = self._need()
        handle = stream_handle(stream, self._dev_index)
        recorder.record(handle)
        self._stream = handle

    def read(self, first=None, count=None, stream=None) -> np.ndarray:
        """Structured array of shape (B, n), dtype mirroring ``cavmd_record``: rows first .. first + count - 1 (0-based count
        of recorded rows) of every system.  Default: everything still held.  Waits for the device (or, if given, for
        ``stream`` only); works the same before, between and after the replays of a graph, never inside a capture."""
        return self._read(first, count, stream)
