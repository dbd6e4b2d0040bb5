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

``period`` counts calls and ``reference_interval`` counts recorded rows.  Under an adaptive timestep the reference tracker
goes by TIME instead (``--fkt-output-period-ps`` and ``--fkt-ref-interval``, its "PREFERRED for adaptive mode" rule,
src/cavitymd/analysis.py:366-378), and so does this class once ``set_time_rule`` was called with the ``StepDraw`` whose
``elapsed`` is every system's clock on the device::

    fields = BatchFieldRecorder(positions, kmag=1.0, reference_interval=0)
    fields.set_time_rule(draw, time_interval=period, reference_time_interval=ref_period)      # BEFORE the capture
    ...
    series = fields.read()
    series["time"]                        # the clock of every row
    fields.lag_times(series)              # (B, n, max_references): time of the row minus time of the reference's row

A row is then written on a system's first ``record()`` and whenever its clock has moved by ``time_interval`` since its last
row; a reference is taken (after the correlation, as always) with the first row, when ``take_reference`` asks, and whenever
the clock has moved by ``reference_time_interval`` since the system's last reference of any cause.  A system at rest behind
its end time (``StepDraw.set_end_time``) writes nothing more.  ``take_reference`` stays for any other policy of the caller's.

There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _capi
from ._device import device_tensor, one_device, stream_handle
from .recorder import _SeriesRecorder
from .observables import generate_fibonacci_sphere


def _record_dtype() -> np.dtype:
    """cavmd_field_record's dtype with ``time`` as one more field, at the offset of ``reserved``"""
    base = _capi.field_record_dtype()
    return np.dtype({"names": list(base.names) + ["time"], "formats": [base.fields[n][0] for n in base.names] + [np.dtype("<f8")],
                     "offsets": [base.fields[n][1] for n in base.names] + [base.fields["reserved"][1]], "itemsize": base.itemsize})


_RECORD_DTYPE = _record_dtype()


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
        (or, if given, for ``stream`` only); works the same before, between and after the replays of a graph.  ``time`` is
        the record's ``reserved`` double under its name: the system's clock at the row under a time rule, 0 without one."""
        return self._read(first, count, stream).view(_RECORD_DTYPE)

    def set_time_rule(self, clock, time_interval, reference_time_interval=None) -> None:
        """clock: the ``StepDraw`` of the same B systems (its ``elapsed`` is read on the device when the kernel runs), or a
        contiguous (B,) float64 device tensor of clocks.  time_interval: a row whenever a system's clock has moved by this much
        since its last row (the recorder must have ``period == 1``); None or 0 switches the rule off.
        reference_time_interval: None or 0 keeps ``reference_interval`` (recorded rows); otherwise a reference whenever the
        clock has moved by this much since the system's last reference.  Set it BEFORE ``record()`` is captured: the rule is
        frozen into a captured launch.  Never inside a capture."""
        on = bool(time_interval)
        ptr = stride = 0
        if on:
            if isinstance(clock, torch.Tensor):
                if clock.device.type != "cuda":
                    raise RuntimeError("BatchFieldRecorder.set_time_rule needs the clocks in GPU memory; no CPU fallback exists "
                                       "in this package")
                if clock.dtype != torch.float64 or clock.shape != (self.n_systems,) or not clock.is_contiguous():
                    raise ValueError(f"a clock tensor must be a contiguous ({self.n_systems},) float64 tensor")
                ptr, stride = clock.data_ptr(), 8
            else:
                if getattr(clock, "n_systems", None) != self.n_systems:
                    raise ValueError(f"BatchFieldRecorder.set_time_rule: the clock of the same {self.n_systems} systems")
                ptr = clock._need().state_device_ptr() + _capi.DrawState.elapsed.offset
                stride = ctypes.sizeof(_capi.DrawState)
        self._need().set_time_rule(ptr, stride, float(time_interval) if on else 0.0,
                                   float(reference_time_interval) if (on and reference_time_interval) else 0.0)
        self._clock = clock if on else None   # kept alive for the kernel

    def lag_times(self, series) -> np.ndarray:
        """(B, n, max_references) float64: for every row of ``series`` (what ``read()`` gave) and every reference it was
        correlated with, ``time`` of the row minus ``time`` of the row that took the reference (that row has
        ``took_reference`` and ``n_references == r``); NaN where a row has no such reference.  Raises where the row that took a
        reference a later row of ``series`` is correlated with is not in ``series`` (it has left the ring, or the slice starts
        behind it)."""
        B, n = series.shape
        out = np.full((B, n, self.max_references), np.nan)
        for b in range(B):
            ref_time = {}
            for j in range(n):
                row = series[b, j]
                for r in range(int(row["n_references"])):
                    if r not in ref_time:
                        raise ValueError(f"system {b}: the row that took reference {r} is not among the rows given")
                    out[b, j, r] = row["time"] - ref_time[r]
                if row["took_reference"]:
                    ref_time[int(row["n_references"])] = float(row["time"])
        return out

    def fields(self, item: int, stream=None):
        """(rho_now, rho_refs, ref_rows) of one system: the field of its last recorded call (complex, (n_k,)), its stored
        reference fields ((n_refs, n_k)) and the row each was taken at -- what a checkpoint of the tracker needs."""
        return self._need().read_fields(self._read_stream(stream), int(item))
