"""``BatchFieldRecorder`` -- the density field rho(k) of B independent small systems, its correlation F(k,t) with each
system's stored reference fields and the reference bookkeeping, appended by ONE kernel launch per step to a time series in
device memory.

What the reference's ``FieldAutocorrelationTracker`` (src/cavitymd/analysis.py:260-418) does every step for every replica is
one 160-byte row per system here (``cavmd_field_record``): ``F[r]`` against every stored reference, ``rho2`` (the lag-0 value),
how many references the row was correlated with and whether it took one.  Write position and references live on the device,
so ``record()`` captured into a graph next to ``CavityForceBatch.compute``, ``BatchRecorder.record`` and
``BussiReservoirBatch.step_async`` appends a NEW row on every replay and takes references when they are due::

    fields = BatchFieldRecorder(positions, kmag=1.0, reference_interval=10000)
    with torch.cuda.graph(graph):
        forces.compute()
        recorder.record()
        fields.record()
        thermostat.step_async()
    for _ in range(steps):
        graph.replay()
    series = fields.read()                # (B, steps) structured array, one copy, behind one synchronisation
    series["F"][:, :, 0]                  # F(k,t) of every system against its first reference

``reference_interval`` counts recorded rows.  The reference's time-based ``reference_interval_ps`` under an adaptive timestep
is the caller's policy: keep a uint32 tensor of B words on the device, set a word when that replica's clock passes its next
reference time, and hand the tensor to ``record(take_reference=...)``; it is read when the kernel runs.  That clock exists
on the device since ``StepDraw``: ``elapsed`` of its state (``cavmd_draw_state_device_ptr``) is the sum of every dt handed out.

There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import device_tensor, one_device, stream_handle
from .recorder import _SeriesRecorder
from .observables import generate_fibonacci_sphere


class BatchFieldRecorder(_SeriesRecorder):
    """positions: one (N_k, 3) or (N_k, 4) device tensor of WRAPPED positions per system (HOOMD's Scalar4 pos is (N, 4)).
    wavevectors: (n_k, 3), ONE set for all systems; default ``kmag * generate_fibonacci_sphere(num_wavevectors)``, the
    reference tracker's.  An item keeps its last ``capacity`` rows; every ``period``-th ``record()`` writes one; at most
    ``max_references`` reference fields per system, a new one every ``reference_interval`` recorded rows (0: only the first)
    or when asked through ``take_reference``.  The defaults are the reference tracker's."""
    _record_dtype = staticmethod(_capi.field_record_dtype)

    def __init__(self, positions, wavevectors=None, kmag: float = 1.0, num_wavevectors: int = 50, capacity: int = 4096,
                 period: int = 1, max_references: int = 10, reference_interval: int = 10000):
        positions = list(positions)
        for t in positions:   # CPU tensors are refused before anything else is looked at
            device_tensor(t, "BatchFieldRecorder", "position", (3, 4), " (WRAPPED positions)")
        if not positions:
            raise ValueError("BatchFieldRecorder needs at least one system")
        dev = one_device(positions, "field recorder")
        if wavevectors is None:
            wavevectors = float(kmag) * generate_fibonacci_sphere(int(num_wavevectors))
        self.wavevectors = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
        self._positions = positions
        items = [_capi.field_item(t.data_ptr() if t.shape[0] else 0, t.shape[1] * 8, t.shape[0]) for t in positions]
        self._open(dev, lambda ws: _capi.FieldRecorder(ws, items, self.wavevectors, capacity, period, max_references,
                                                       reference_interval))
        self.n_systems = len(positions)
        self.n_k = self._handle.n_k
        self.capacity, self.period = int(capacity), int(period)
        self.max_references, self.reference_interval = int(max_references), int(reference_interval)
        self._take = None

    def record(self, stream=None, take_reference=None) -> None:
        """ONE kernel launch on ``stream`` (default: torch's current stream): nothing is waited for; may be captured.
        take_reference: None, or a uint32 / int32 device tensor of B words read when the kernel RUNS (so a captured call
        sees what the tensor holds at each replay): non-zero asks that system to take a reference at this call."""
        recorder = self._need()
        ptr = 0
        if take_reference is not None:
            t = take_reference
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
                raise RuntimeError("take_reference must live in GPU memory; no CPU fallback exists in this package")
            if t.dtype not in (torch.int32, torch.uint32) or t.dim() != 1 or t.shape[0] != self.n_systems \
                    or not t.is_contiguous():
                raise ValueError("take_reference: a contiguous int32 / uint32 tensor with one word per system")
            self._take = t   # kept alive for the kernel (and for the graph that captured it)
            ptr = t.data_ptr()
        recorder.record(stream_handle(stream, self._dev_index), ptr)

    def read(self, first=0, count=None, stream=None) -> np.ndarray:
        """Structured array of shape (B, n), dtype mirroring ``cavmd_field_record``: rows first .. first + count - 1 (0-based
        count of recorded rows) of every system; ``first=None`` starts at the oldest row still held.  Waits for the device
        (or, if given, for ``stream`` only); works the same before, between and after the replays of a graph."""
        return self._read(first, count, stream)

    def fields(self, item: int, stream=None):
        """(rho_now, rho_refs, ref_rows) of one system: the field of its last recorded call (complex, (n_k,)), its stored
        reference fields ((n_refs, n_k)) and the row each was taken at -- what a checkpoint of the tracker needs."""
        return self._need().read_fields(self._read_stream(stream), int(item))
