"""``VerletBatch`` -- the velocity-Verlet step of B independent small systems, each half-step ONE kernel launch.

The reference has no integrator of its own: its driver gives the molecules to HOOMD-blue's ``ConstantVolume`` method and the
one cavity particle to HOOMD-blue's ``Langevin`` method (``--molecular-bath bussi --cavity-bath langevin``, the default of
examples/05_advanced_run.py:652, 677).  This class is the two half-steps of those methods (``cavmd_verlet_step_one`` /
``cavmd_verlet_step_two``; the arithmetic is spelled out in include/cavmd.h) on the arrays a ``CavityForceBatch`` already
evaluates, so that a captured graph of this package's kernels alone advances a trajectory::

    integrator = VerletBatch(forces, velocities, langevin_index=500)
    forces.compute(); integrator.prime()                  # a = F / m once, as HOOMD does at the start of a run
    with torch.cuda.graph(graph):
        integrator.draw_inputs(dt, gamma, kT)             # or set_inputs(...) in stream order before each replay
        integrator.step_one()                             # v += a dt / 2; x += v dt; wrap
        forces.compute()
        integrator.step_two()                             # a = F / m (+ the cavity particle's bath); v += a dt / 2
        recorder.record(); thermostat.draw_inputs(0, dt); thermostat.step_async()

The step's inputs live in a ``(B, 8)`` float64 DEVICE tensor, ``inputs`` (row = dt, gamma, sqrt(6 gamma kT / dt), three
variates uniform in [-1, 1), skip flag, one reserved word), read by both kernels when they run.  ``draw_inputs`` uses torch's
generator, not HOOMD's RandomGenerator: the variates are not bit-comparable with a HOOMD run; everything after the draw is.
The Langevin bath of this class acts on at most one particle per system; ``LangevinBathBatch`` (bath_batch.py) supplies step two
with a bath on any set of particles.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import Checkpointable, HandleOwner, StepInputs, device_tensor, per_system, stream_handle


class VerletBatch(HandleOwner, Checkpointable):
    """force_batch: the ``CavityForceBatch`` whose systems are integrated (positions, images and boxes are taken from its
    system definitions, its force arrays are the first force of every system); velocities: one (N_k, 4) device tensor per
    system (mass in column 3); extra_forces: None, or per system a list of up to three more (N_k, 4) force tensors, summed
    after the cavity force in list order; langevin_index: None, one index, or one per system (None / -1: no bath);
    net_forces: allocate ``net_forces`` and have step two (and ``prime``) write the summed force there."""

    def __init__(self, force_batch, velocities, extra_forces=None, langevin_index=None, net_forces: bool = False):
        velocities = list(velocities)
        for v in velocities:
            device_tensor(v, "VerletBatch", "velocity")   # CPU tensors are refused before anything else is looked at
        B = len(force_batch)
        if len(velocities) != B:
            raise ValueError(f"velocities: one entry per system of the force batch ({B})")
        extra_forces = [None] * B if extra_forces is None else list(extra_forces)
        if len(extra_forces) != B:
            raise ValueError("extra_forces: None, or one list per system")
        extra_forces = [[] if e is None else list(e) for e in extra_forces]
        langevin = [-1 if i is None else int(i) for i in per_system(langevin_index, B, "langevin_index")]
        sysdefs = force_batch._sysdefs
        forces = force_batch.forces
        dev = velocities[0].device if B else None
        self.accel, self.net_forces, items = [], ([] if net_forces else None), []
        for k in range(B):
            pd = sysdefs[k].getParticleData()
            n = pd.getN()
            v = velocities[k]
            if v.device != dev or pd.device != dev:
                raise ValueError("all systems of one integrator live on one device")
            if v.shape[0] != n:
                raise ValueError(f"system {k}: the velocity array has {v.shape[0]} rows, the force batch evaluates {n}")
            if len(extra_forces[k]) > 3:
                raise ValueError(f"system {k}: at most three extra force arrays")
            for f in extra_forces[k]:
                if device_tensor(f, "VerletBatch", "force").shape[0] != n or f.device != dev:
                    raise ValueError(f"system {k}: an extra force array does not match the system")
            a = torch.zeros((n, 3), dtype=torch.float64, device=dev)
            self.accel.append(a)
            net = None
            if net_forces:
                net = torch.zeros((n, 4), dtype=torch.float64, device=dev)
                self.net_forces.append(net)
            flist = [forces[k]] + extra_forces[k]
            items.append(_capi.verlet_item(n, pd.getPositions().data_ptr() if n else 0, pd.getImages().data_ptr() if n else 0,
                                           v.data_ptr() if n else 0, a.data_ptr() if n else 0,
                                           [f.data_ptr() if n else 0 for f in flist], net.data_ptr() if (net is not None and n) else 0,
                                           pd.getGlobalBox().getL(), langevin[k]))
        self._force_batch, self._velocities, self._extra = force_batch, velocities, extra_forces
        self._open(dev, lambda ws: _capi.Verlet(ws, items))
        self.n_systems = B
        self._step_inputs = StepInputs(B, dev, skip_column=6)
        self.inputs = self._step_inputs.tensor
        self._stream = 0
        self._kick_tables = {}   # pointers of a kick's force arrays -> (their device table, the arrays): kick_table
        torch.cuda.current_stream(dev).synchronize()   # accel, inputs and the states are zero before any stream steps

    # -- the step's inputs -------------------------------------------------------------------------------------------------
    def _rows(self, dt, gamma, kT, uniforms=None) -> np.ndarray:
        """(B, 8) host rows made by cavmd_verlet_input_make; dt, gamma, kT: one number or one per system."""
        B = self.n_systems
        dts, gammas, kTs = (per_system(x, B, name) for x, name in ((dt, "dt"), (gamma, "gamma"), (kT, "kT")))
        u = np.zeros((B, 3)) if uniforms is None else np.asarray(uniforms, dtype=np.float64)
        if u.shape != (B, 3):
            raise ValueError(f"uniforms must have shape ({B}, 3)")
        rows = (_capi.VerletInput * max(B, 1))()
        for i in range(B):
            rows[i] = _capi.verlet_input_make(dts[i], gammas[i], kTs[i], u[i])
        return np.frombuffer(rows, dtype=np.float64).reshape(-1, 8)[:B].copy()

    def set_inputs(self, dt, gamma=0.0, kT=0.0, uniforms=None) -> None:
        """uniforms: None (no bath: zeros) or a (B, 3) host array of variates in [-1, 1).  The rows reach ``inputs`` with one
        asynchronous copy on the current stream."""
        self._need()
        self._step_inputs.upload(self._rows(dt, gamma, kT, uniforms))

    def draw_inputs(self, dt, gamma, kT, generator=None) -> None:
        """Fills ``inputs`` ON THE DEVICE, in stream order, with no host wait: the variates as ``2 * torch.rand - 1``, the rest
        from host arithmetic (uploaded only when it changes).  Capturable together with the two half-steps."""
        self._need()
        const = self._rows(dt, gamma, kT)
        u = torch.rand((self.n_systems, 3), dtype=torch.float64, device=self._device, generator=generator)
        self._step_inputs.fill_constants(const)
        self.inputs[:, 3:6] = 2.0 * u - 1.0

    # -- the launches ------------------------------------------------------------------------------------------------------
    def _launch(self, call, stream, *args) -> None:
        verlet = self._need()
        handle = stream_handle(stream, self._dev_index)
        call(verlet, handle, *args)
        self._stream = handle

    def prime(self, stream=None) -> None:
        """ONE kernel: ``accel`` = F / m from the force arrays as they are (after a ``force_batch.compute()``)."""
        self._launch(_capi.Verlet.accelerations, stream)

    def step_one(self, stream=None) -> None:
        """ONE kernel: v += (a / 2) dt, x += dt v, one wrap per axis with the image following.  May be captured."""
        self._launch(_capi.Verlet.step_one, stream, self.inputs.data_ptr())

    def step_two(self, stream=None) -> None:
        """ONE kernel: F = sum of the force arrays (+ the bath on the Langevin particle), a = F / m, v += (a / 2) dt."""
        self._launch(_capi.Verlet.step_two, stream, self.inputs.data_ptr())

    def kick_table(self, forces) -> torch.Tensor:
        """The device table of B force pointers ``kick`` hands to its kernel, built once per list of arrays and kept alive
        here with the arrays.  forces: a list of B (N_k, 4) device tensors (None: that system is left alone), or an object
        with ``.forces``.  A new table is an upload from the host: not during a stream capture (``kick`` the same arrays once
        before capturing, or call this)."""
        self._need()
        flist = list(getattr(forces, "forces", forces))
        if len(flist) != self.n_systems:
            raise ValueError(f"forces: one array per system ({self.n_systems})")
        ptrs = []
        for k, f in enumerate(flist):
            n = self._velocities[k].shape[0]
            if f is None or n == 0:
                ptrs.append(0)
                continue
            if device_tensor(f, "VerletBatch", "force").shape != (n, 4) or f.dtype != torch.float64 or not f.is_contiguous() \
                    or f.device != self._device:
                raise ValueError(f"system {k}: the kick's force array is a contiguous ({n}, 4) float64 tensor on the "
                                 "integrator's device")
            ptrs.append(f.data_ptr())
        tables = self._kick_tables
        key = tuple(ptrs)
        if key not in tables:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("VerletBatch.kick: the pointer table of these force arrays is not on the device yet; call "
                                   "kick_table(forces) before the capture")
            table = torch.zeros(max(len(ptrs), 1), dtype=torch.int64, device=self._device)
            table[:len(ptrs)] = torch.from_numpy(np.array(ptrs, dtype=np.uint64).view(np.int64).copy()).to(self._device)
            torch.cuda.current_stream(self._device).synchronize()
            tables[key] = (table, flist)
        return tables[key][0]

    def kick(self, forces, weight, inputs=None, stream=None) -> None:
        """ONE kernel: v += (f / m) (weight dt) with a force that is none of the integrator's own arrays, and nothing else
        written -- the outer half-kicks of the impulse multiple-time-step scheme, ``kick(coulomb.long, n / 2)`` before and
        after n plain steps.  forces: as for ``kick_table``; inputs: a (B, 8) device tensor of input rows, default
        ``inputs``.  Pointers and rows are read when the kernel runs.  May be captured once the table exists."""
        table = self.kick_table(forces)
        rows = self.inputs if inputs is None else inputs
        if rows.shape != (self.n_systems, 8) or rows.dtype != torch.float64 or rows.device != self._device or not rows.is_contiguous():
            raise ValueError(f"inputs: a contiguous ({self.n_systems}, 8) float64 tensor on the integrator's device")
        self._launch(_capi.Verlet.kick, stream, rows.data_ptr(), table.data_ptr(), float(weight))

    def state(self, stream=None) -> np.ndarray:
        """Per-system counters (``steps``, ``out_of_box``, ``langevin_reservoir``).  Default: waits for the whole device (a
        graph replays on the stream it is launched on), then reads; never inside a capture."""
        verlet = self._need()
        if stream is None:
            torch.cuda.synchronize(self._device)
        return verlet.read(stream_handle(stream, self._dev_index))

    def reset(self, stream=None) -> None:
        """Zero every system's counters, ordered on ``stream`` (default: torch's current stream)."""
        self._need().reset(stream_handle(stream, self._dev_index))

    def _state_tensors(self) -> dict:
        """``accel`` (after a step with a bath it holds the random force and cannot be recomputed), ``inputs`` and, if there,
        ``net_forces``: what ``state_dict`` saves next to the integrator's counters"""
        own = {"accel": self.accel, "inputs": self.inputs}
        if self.net_forces is not None:
            own["net_forces"] = self.net_forces
        return own

    @property
    def verlet(self) -> _capi.Verlet:
        return self._handle
