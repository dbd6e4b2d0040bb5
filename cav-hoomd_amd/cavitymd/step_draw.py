"""``StepDraw`` -- the step inputs of B independent small systems drawn on the device, ONE kernel launch per step.

``VerletBatch.draw_inputs`` and ``BussiReservoirBatch.draw_inputs`` fill their ``inputs`` tables with a string of torch
launches whose gamma sampler takes no generator, and with a dt the host supplies.  This class fills both tables with one
kernel of the library (``cavmd_draw_fill``; the arithmetic is spelled out in include/cavmd.h): Philox4x32-10 variates keyed by
``seed`` and counted on the device, so that a run can be repeated and a graph replay draws fresh ones, and a dt that is either
fixed or the rule of the reference's ``AdaptiveTimestepUpdater`` (src/cavitymd/simulation.py:57-92) taken on the device from
the ``force_mass_sum`` a ``BatchRecorder`` wrote last.  The elapsed time of every system is kept next to it (``state()``).
It is the Coulomb example's step with the two ``draw_inputs`` calls replaced by one ``fill()``::

    draw = StepDraw(seed, integrator, thermostat, dt=dt, gamma=gamma, kT=kT)               # a fixed dt
    draw = StepDraw(seed, integrator, thermostat, recorder, dt=dt, gamma=gamma, kT=kT,     # dt = sqrt(tolerance / S)
                    tolerance=1e-3, dt_min=0.1, dt_max=50.0)
    with torch.cuda.graph(graph):
        draw.fill()
        integrator.step_one(); forces.compute(); coulomb.compute(); integrator.step_two()
        recorder.record(); thermostat.step_async()
    for _ in range(steps):
        graph.replay()
    draw.state()["elapsed"]                                  # per system, in the units of dt

The integrator and the thermostat are unchanged, and their own ``draw_inputs`` / ``set_inputs`` keep working.  The
thermostat's ``kT`` may be a callable of the timestep for ``BussiReservoirBatch.draw_inputs``; here it is one number per
system, fixed when the object is built: a callable raises.  ``elapsed`` and ``tolerance_time_constant`` are in the units of
dt; the conversion to ps is the caller's.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import Checkpointable, HandleOwner, one_device, per_system, stream_handle

_ROW_BYTES = 64
_RECORD_BYTES = 128


def _state_dtype() -> np.dtype:
    """cavmd_draw_state's dtype with ``finished`` as one more field, at the offset of reserved[0]"""
    base = _capi.draw_state_dtype()
    names = list(base.names) + ["finished"]
    return np.dtype({"names": names, "formats": [base.fields[n][0] for n in base.names] + [np.dtype("<u8")],
                     "offsets": [base.fields[n][1] for n in base.names] + [base.fields["reserved"][1]], "itemsize": base.itemsize})


_STATE_DTYPE = _state_dtype()


def _inputs_of(owner, what: str):
    """The (B, 8) float64 device tensor a destination stands for: the ``inputs`` of a batch object, or the tensor itself."""
    t = getattr(owner, "inputs", owner)
    if t is None:
        raise RuntimeError(f"StepDraw: the {what} has no inputs yet (attach() it first)")
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"StepDraw needs the {what}'s input rows in GPU memory; no CPU fallback exists in this package")
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 8 or not t.is_contiguous():
        raise ValueError(f"the {what}'s inputs must be a contiguous (B, 8) float64 tensor")
    return t


class StepDraw(HandleOwner, Checkpointable):
    """seed: 0 .. 2**64 - 1, the generator's key; integrator: a ``VerletBatch`` (or its ``inputs`` tensor) or None;
    thermostat: an attached ``BussiReservoirBatch`` (or its ``inputs`` tensor) or None -- at least one of the two;
    recorder: the ``BatchRecorder`` whose last row gives S, required with ``tolerance``.

    dt, gamma, kT: what ``VerletBatch.draw_inputs`` takes, one number or one per system (dt: the fixed dt, or with
    ``tolerance`` the dt while nothing is recorded).  set_T, tau, dof: the thermostat's kT, tau and translational degrees of
    freedom, one number or one per system; default: those of the ``BussiReservoirBatch`` given.
    tolerance: None (a fixed dt) or the target of dt = sqrt(tolerance / S); tolerance_initial and tolerance_time_constant
    ramp it as target - (target - initial) exp(-elapsed / time_constant) (time constant 0: no ramp); dt_min, dt_max clamp
    the adaptive dt."""

    def __init__(self, seed, integrator=None, thermostat=None, recorder=None, dt=0.0, gamma=0.0, kT=0.0, set_T=None, tau=None,
                 dof=None, tolerance=None, tolerance_initial=None, tolerance_time_constant=0.0, dt_min=0.0, dt_max=None):
        if integrator is None and thermostat is None:
            raise ValueError("StepDraw: an integrator, a thermostat or both")
        tables = [(_inputs_of(x, what), what) for x, what in ((integrator, "integrator"), (thermostat, "thermostat"))
                  if x is not None]          # CPU tensors are refused before anything else is looked at
        dev = one_device([t for t, _ in tables], "draw object")
        B = int(tables[0][0].shape[0])
        if any(int(t.shape[0]) != B for t, _ in tables):
            raise ValueError("StepDraw: the integrator and the thermostat hold different numbers of systems")
        verlet_rows = _inputs_of(integrator, "integrator") if integrator is not None else None
        bussi_rows = _inputs_of(thermostat, "thermostat") if thermostat is not None else None
        if thermostat is not None:
            set_T = getattr(thermostat, "_kT", None) if set_T is None else set_T
            tau = getattr(thermostat, "_tau", None) if tau is None else tau
            dof = getattr(thermostat, "_dof", None) if dof is None else dof
            if set_T is None or tau is None or dof is None:
                raise ValueError("StepDraw: set_T, tau and dof are needed with a bare thermostat table")
        columns = {}
        for name, value in (("dt", dt), ("gamma", gamma), ("kT", kT), ("set_T", 0.0 if set_T is None else set_T),
                            ("tau", 0.0 if tau is None else tau), ("dof", 0.0 if dof is None else dof),
                            ("tolerance", 0.0 if tolerance is None else tolerance),
                            ("tolerance_initial", (0.0 if tolerance is None else tolerance) if tolerance_initial is None
                             else tolerance_initial),
                            ("tolerance_time_constant", tolerance_time_constant), ("dt_min", dt_min),
                            ("dt_max", np.finfo(np.float64).max if dt_max is None else dt_max)):
            values = per_system(value, B, name, callables=True)
            if any(callable(v) for v in values):
                raise TypeError(f"StepDraw: {name} is one number per system here, not a callable of the timestep")
            columns[name] = [float(v) for v in values]
        records = rows = capacity = 0
        if tolerance is not None:
            if recorder is None or getattr(recorder, "n_systems", None) != B:
                raise ValueError(f"StepDraw: tolerance= needs the BatchRecorder of the same {B} systems")
            records, rows = recorder.recorder.device_ptr()
            capacity = int(recorder.capacity)
        items = []
        for k in range(B):
            items.append(_capi.draw_item(
                verlet_rows.data_ptr() + _ROW_BYTES * k if verlet_rows is not None else 0,
                bussi_rows.data_ptr() + _ROW_BYTES * k if bussi_rows is not None else 0,
                **{name: columns[name][k] for name in columns},
                records_ptr=records + _RECORD_BYTES * capacity * k if records else 0, rows_ptr=rows + 8 * k if records else 0,
                capacity=capacity))
        self._kept = (integrator, thermostat, recorder, verlet_rows, bussi_rows)   # the tables outlive the launches
        self.seed = int(seed)
        self._open(dev, lambda ws: _capi.Draw(ws, self.seed, items))
        self.n_systems = B
        self.adaptive = tolerance is not None
        self._stream = 0
        torch.cuda.current_stream(dev).synchronize()   # the states are zero before any stream fills

    def fill(self, stream=None) -> None:
        """ONE kernel launch on ``stream`` (default: torch's current stream): every system's rows, counters and dt.  Nothing
        is waited for; may be captured, and a replay draws a new block."""
        draw = self._need()
        handle = stream_handle(stream, self._dev_index)
        draw.fill(handle)
        self._stream = handle

    def state(self, stream=None) -> np.ndarray:
        """Per-system ``draws``, ``dt``, ``elapsed``, ``tolerance``, ``exhausted``, ``finished`` (1 while the system rests
        behind its end time; the first of the three ``reserved`` words, under its name).  Default: waits for the whole device
        (a graph replays on the stream it is launched on), then reads; never inside a capture."""
        draw = self._need()
        if stream is None:
            torch.cuda.synchronize(self._device)
        return draw.read(stream_handle(stream, self._dev_index)).view(_STATE_DTYPE)

    def set_end_time(self, t_end) -> None:
        """The end of the run by every system's own clock: one number, or one per system, in the units of ``elapsed``; None
        or 0: no end.  From the ``fill()`` that finds ``elapsed >= t_end`` on, a system is at rest: its rows carry dt = 0 and
        ``skip``, so the integrator, the bath and the thermostat leave it untouched, it draws no block and its clock stands
        still -- the reference's ``ElapsedTimeTracker`` (src/cavitymd/analysis.py:1230-1259), per system and without a
        read-back.  The last step is not clamped onto t_end.  A larger t_end given later lets a system go on, bit for bit as if
        it had had that end time from the start.  Call it before ``fill()`` is captured: a graph captured before the FIRST
        call keeps launching the kernel that knows no end times; later calls change values a captured launch reads.  Waits
        for the stream of the last ``fill()``; never inside a capture."""
        values = per_system(0.0 if t_end is None else t_end, self.n_systems, "t_end")
        self._need().set_end(0, [0.0 if v is None else float(v) for v in values])

    def finished(self, stream=None) -> np.ndarray:
        """(B,) bool: which systems rest behind their end time.  Waits as ``state()`` does."""
        return self.state(stream)["finished"] != 0

    def n_finished(self, stream=None) -> int:
        """How many systems rest behind their end time: one synchronisation and one small copy (``run_until_finished``)."""
        draw = self._need()
        if stream is None:
            torch.cuda.synchronize(self._device)
        return draw.finished(stream_handle(stream, self._dev_index))

    def reset(self, stream=None) -> None:
        """Zero every system's counters, ordered on ``stream`` (default: torch's current stream): the next ``fill`` draws the
        first block again and ``elapsed`` restarts at 0."""
        self._need().reset(stream_handle(stream, self._dev_index))

    @property
    def draw(self) -> _capi.Draw:
        return self._handle
