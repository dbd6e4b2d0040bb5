"""``BussiReservoirBatch`` -- the Bussi reservoir thermostat of B independent small systems, stepped by ONE kernel launch.

The reference's production workload is N = 501 particles run as 500 independent replicas, every one of them thermostatted
each step (src/BussiReservoirThermostat.h:43-98, 177-225).  ``thermostats.BussiReservoir.step_async`` costs two launches per
system and cannot be captured into a graph; this class registers the velocity arrays of all systems once
(``cavmd_bussi_batch_create``) and steps them with one kernel, one workgroup per system (``cavmd_bussi_batch_step``).  Per
system the velocities and counters are bit for bit those of ``BussiReservoir.step_async`` with the same variates.

The step's random inputs live in a ``(B, 8)`` float64 DEVICE tensor, ``inputs`` (row = normal variate, gamma variate,
c = exp(-dt / tau), kT, skip flag, 3 reserved words), which the kernel reads when it runs.  So a step captured into a CUDA/HIP
graph stays stochastic as long as the caller refreshes ``inputs`` in stream order between replays: with ``set_inputs`` (host
variates, one asynchronous copy) or with ``draw_inputs`` (drawn on the device, no host round trip).

``draw_inputs`` uses torch's generator, not HOOMD's RandomGenerator: variate GENERATION is not bit-comparable with a HOOMD
run (as for ``BussiReservoir``); everything after the draw is.  Translational degrees of freedom only; rotational ones stay
on ``BussiReservoir.step``.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _capi
from ._device import Checkpointable, HandleOwner, StepInputs, device_tensor, member_indices, one_device, per_system, stream_handle


class BussiReservoirBatch(HandleOwner, Checkpointable):
    _unusable = "used before attach()"

    def __init__(self, kT, tau=0.0):
        self.kT = kT    # a number, a callable of the timestep, or one of either per system
        self.tau = tau  # a number or one per system
        self.inputs = None
        self._stream = 0

    # -- attachment ----------------------------------------------------------------------------------------------------------
    def attach(self, velocities, translational_dof, members=None) -> None:
        """velocities: list of contiguous (N_i, 4) float64 device tensors (HOOMD Scalar4, mass in column 3), kept alive here;
        translational_dof: one number or one per system; members: None, or per system None / an index array of the group."""
        velocities = list(velocities)
        if not velocities:
            raise ValueError("BussiReservoirBatch.attach: no systems")
        for v in velocities:
            device_tensor(v, "BussiReservoirBatch", "velocity", note=" (HOOMD Scalar4, mass in .w)")
        B = len(velocities)
        dev = one_device(velocities, "batch")
        self._dof = [float(d) for d in per_system(translational_dof, B, "translational_dof")]
        self._kT = per_system(self.kT, B, "kT", callables=True)
        self._tau = [float(t) for t in per_system(self.tau, B, "tau")]
        members = [None] * B if members is None else list(members)
        if len(members) != B:
            raise ValueError("members: None, or one entry per system")
        self._members, items = [], []
        for v, m, dof in zip(velocities, members, self._dof):
            if m is None:
                mt, n = None, int(v.shape[0])
            else:
                mt, n = member_indices(m, v.shape[0], dev)
            self._members.append(mt)
            items.append(_capi.bussi_batch_item(v.data_ptr() if v.shape[0] else 0,
                                                mt.data_ptr() if (mt is not None and n) else 0, n, dof))
        self._velocities = velocities
        self.detach()
        self._open(dev, lambda ws: _capi.BussiBatch(ws, items))
        self.n_systems = B
        self._step_inputs = StepInputs(B, dev, skip_column=4)
        self.inputs = self._step_inputs.tensor
        self._dof_dev = torch.tensor(self._dof, dtype=torch.float64, device=dev)
        self._shape = torch.clamp((self._dof_dev - 1.0) / 2.0, min=0.5)   # gamma shape where dof > 1; unused elsewhere
        self._has_normal = self._dof_dev != 0
        self._has_gamma = self._dof_dev > 1.0
        torch.cuda.current_stream(dev).synchronize()

    def detach(self) -> None:
        self.close()
        self.inputs = None

    def _set_T(self, timestep: int):
        return [float(k(timestep)) if callable(k) else float(k) for k in self._kT]

    # -- the step's inputs -------------------------------------------------------------------------------------------------
    def set_inputs(self, timestep: int, deltaT: float, variates) -> None:
        """variates: (B, 2) host array {normal, gamma} per system.  Rows are made by cavmd_bussi_batch_input_make (the c of
        cavmd_bussi_step_device) and reach ``inputs`` with one asynchronous copy on the current stream."""
        self._need()
        v = np.asarray(variates, dtype=np.float64)
        if v.shape != (self.n_systems, 2):
            raise ValueError(f"variates must have shape ({self.n_systems}, 2)")
        rows = (_capi.BussiBatchInput * self.n_systems)()
        lib = _capi.load()
        for i, (T, tau) in enumerate(zip(self._set_T(timestep), self._tau)):
            _capi.check(lib.cavmd_bussi_batch_input_make(float(deltaT), T, tau, float(v[i, 0]), float(v[i, 1]),
                                                         ctypes.byref(rows[i])), "cavmd_bussi_batch_input_make")
        self._step_inputs.upload(np.frombuffer(rows, dtype=np.float64).reshape(self.n_systems, 8))

    def draw_inputs(self, timestep: int, deltaT: float, generator=None) -> None:
        """Fills ``inputs`` ON THE DEVICE, in stream order, with no host wait: normal variates from torch.randn, gamma variates
        of shape (dof - 1) / 2 from torch's gamma sampler where dof > 1 (0 elsewhere; nothing "drawn" for dof == 0), c and kT
        from host arithmetic.  torch's generator, not HOOMD's RandomGenerator.  (The gamma sampler has no generator argument in
        torch: `generator` seeds the normal draw only.)  Capturable together with ``step_async``."""
        self._need()
        dev = self.inputs.device
        B = self.n_systems
        T = self._set_T(timestep)
        const = np.zeros((B, 8))
        for i in range(B):
            row = _capi.bussi_batch_input_make(deltaT, T[i], self._tau[i], 0.0, 0.0)
            const[i, 2], const[i, 3] = row.c, row.set_T
            const[i, 4] = np.array([row.skip], dtype=np.uint64).view(np.float64)[0]
        normal = torch.randn(B, dtype=torch.float64, device=dev, generator=generator)
        gamma = torch._standard_gamma(self._shape)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        self._step_inputs.fill_constants(const)                 # c, kT, skip
        self.inputs[:, 0] = torch.where(self._has_normal, normal, zero)
        self.inputs[:, 1] = torch.where(self._has_gamma, gamma, zero)

    # -- one step of every system ------------------------------------------------------------------------------------------
    def step_async(self, stream=None) -> None:
        """ONE kernel launch: kinetic energy -> alpha -> counters -> velocities *= alpha for every system, from ``inputs`` as
        it is when the kernel runs.  Nothing is waited for; may be captured into a graph."""
        batch = self._need()
        handle = stream_handle(stream, self._dev_index)
        batch.step(handle, self.inputs.data_ptr())
        self._stream = handle

    def device_state(self):
        """Per-system counters after the last enqueued step (waits for that step's stamps, nothing else).  Raises
        CavmdError(CAVMD_ERR_BAD_PARAMS) once after a step that was refused for zero kinetic energy."""
        return self._need().read()

    def _field(self, name: str) -> np.ndarray:
        if self._handle is None:
            return np.zeros(0)
        states, _ = self._handle.read(raise_refused=False)
        return np.array([getattr(s, name) for s in states], dtype=np.float64)

    # -- the reference's loggable quantities, one entry per system -------------------------------------------------------------
    @property
    def reservoir_energy_translational(self) -> np.ndarray:
        return self._field("reservoir_translational")

    @property
    def reservoir_energy_rotational(self) -> np.ndarray:
        return np.zeros_like(self.reservoir_energy_translational)

    @property
    def total_reservoir_energy(self) -> np.ndarray:
        return self.reservoir_energy_translational + self.reservoir_energy_rotational

    @property
    def instantaneous_reservoir_translational(self) -> np.ndarray:
        return self._field("instantaneous_translational")

    @property
    def instantaneous_reservoir_rotational(self) -> np.ndarray:
        return np.zeros_like(self.instantaneous_reservoir_translational)

    @property
    def instantaneous_reservoir_total(self) -> np.ndarray:
        return self.instantaneous_reservoir_translational + self.instantaneous_reservoir_rotational

    def _state_tensors(self) -> dict:
        """the input rows: what ``state_dict`` saves next to the per-system counters"""
        return {"inputs": self.inputs}

    def reset_reservoir_energy(self) -> None:
        self._need().reset(self._stream)
