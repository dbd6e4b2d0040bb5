"""``LangevinBathBatch`` -- a Langevin bath on any set of particles of B independent small systems, drawn inside step two.

The reference's driver has three choices for ``--molecular-bath`` (examples/05_advanced_run.py:649-666): ``bussi`` is
``BussiReservoirBatch``, ``none`` is a plain ``VerletBatch``, and ``langevin`` is HOOMD-blue's ``Langevin`` method on every
molecular particle with ``tally_reservoir_energy=True``.  This class is the third.  It is created from a ``VerletBatch`` and
its ``step_two()`` takes the place of the integrator's in a step (``cavmd_bath_step_two``; the arithmetic is spelled out in
include/cavmd.h): ONE kernel, in which every coupled particle draws its three variates from a seeded, counter-based generator
(Philox4x32-10, counted on the device, so that a run can be repeated and a graph replay draws fresh ones).  The variates
never touch memory and nothing new is launched.  The captured step of ``--molecular-bath langevin --cavity-bath langevin``,
the cavity particle simply carrying its own gamma in ``gammas``::

    gammas = [torch.full((n,), gamma_molecular, dtype=torch.float64, device="cuda") for n in sizes]
    for g in gammas:
        g[-1] = gamma_cavity                                # the photon is the last particle of its system
    integrator = VerletBatch(forces, velocities, net_forces=True)
    draw = StepDraw(seed, integrator, recorder=recorder, dt=dt, tolerance=1e-3, dt_min=0.1, dt_max=50.0)
    bath = LangevinBathBatch(integrator, gammas, kT, seed)
    forces.compute(); integrator.prime()
    with torch.cuda.graph(graph):
        draw.fill()                                          # 1. the step's dt (the bath needs no variates from it)
        integrator.step_one()                                # 2.
        forces.compute(); molecular.compute()                # 3. the forces
        bath.step_two()                                      # 4. in place of integrator.step_two()
        recorder.record()                                    # 5.
    for _ in range(steps):
        graph.replay()
    bath.state()["reservoir"]                                # per system: HOOMD's reservoir energy of the method

The net force that step two writes carries no bath term, so the adaptive dt's ``force_mass_sum`` excludes the bath, as the
reference's does.  System i draws under the key ``(seed + 0x9E3779B97F4A7C15 * (i + 1)) mod 2**64`` (``seeds=`` overrides it,
one key per system): its variates do not depend on its place in a batch.  A particle named by the integrator's
``langevin_index`` whose row carries a non-zero gamma keeps the ROW's bath and takes none from here.

The limits.  The variates are Philox with the counter layout published in include/cavmd.h, not HOOMD's RandomGenerator: no
draw is bit-comparable with a HOOMD run; everything after the draw is held to the header's expressions.  Rotational degrees of
freedom and triclinic boxes are out of scope.  Close the bath before its integrator.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import Checkpointable, HandleOwner, per_system, stream_handle


def _gamma_tensor(g, k: int):
    if not isinstance(g, torch.Tensor) or g.device.type != "cuda":
        raise RuntimeError("LangevinBathBatch needs the gamma arrays in GPU memory; no CPU fallback exists in this package")
    if g.dtype != torch.float64 or g.dim() != 1 or not g.is_contiguous():
        raise ValueError(f"system {k}: gammas must be a contiguous (N,) float64 tensor, or None")
    return g


class LangevinBathBatch(HandleOwner, Checkpointable):
    """integrator: the ``VerletBatch`` whose second half-step this object supplies; gammas: per system a ``(N_k,)`` float64
    device tensor of frictions (a particle with gamma 0, or beyond the tensor's end, is not coupled), or None for no bath on
    that system; kT: one number, or one per system; seed: 0 .. 2**64 - 1; seeds: None, or one Philox key per system."""

    def __init__(self, integrator, gammas, kT, seed=0, seeds=None):
        gammas = list(gammas)
        for k, g in enumerate(gammas):
            if g is not None:
                _gamma_tensor(g, k)               # CPU tensors are refused before anything else is looked at
        verlet = integrator._need()               # a closed integrator raises
        B = integrator.n_systems
        if len(gammas) != B:
            raise ValueError(f"gammas: one entry per system of the integrator ({B})")
        self.seed = int(seed)
        if not 0 <= self.seed < 2**64:
            raise ValueError("seed: 0 .. 2**64 - 1")
        self._kTs = [float(x) for x in per_system(kT, B, "kT")]
        self.keys = ([_capi.bath_item_key(self.seed, i) for i in range(B)] if seeds is None
                     else [int(x) for x in per_system(seeds, B, "seeds")])
        if any(not 0 <= key < 2**64 for key in self.keys):
            raise ValueError("seeds: 0 .. 2**64 - 1")
        self._integrator = integrator
        self._device, self._dev_index = integrator._device, integrator._dev_index
        self._gammas = gammas                      # the arrays outlive the launches
        self._handle = _capi.Bath(verlet, self._items(0, gammas))
        self.n_systems = B
        self._stream = 0
        torch.cuda.current_stream(self._device).synchronize()   # the states are zero before any stream steps

    def _items(self, first: int, gammas):
        items = []
        for k, g in enumerate(gammas, start=first):
            n = 0 if g is None else int(g.shape[0])
            if g is not None and g.device != self._device:
                raise ValueError("all systems of one bath live on the integrator's device")
            items.append(_capi.bath_item(g.data_ptr() if n else 0, n, self._kTs[k], self.keys[k]))
        return items

    def step_two(self, stream=None) -> None:
        """ONE kernel on ``stream`` (default: torch's current stream), in place of ``integrator.step_two()``: F = sum of the
        force arrays, the bath on every coupled particle, a = F / m, v += (a / 2) dt.  May be captured; a replay draws anew."""
        bath = self._need()
        handle = stream_handle(stream, self._dev_index)
        bath.step_two(handle, self._integrator.inputs.data_ptr())
        self._stream = self._integrator._stream = handle

    def state(self, stream=None) -> np.ndarray:
        """Per-system ``draws``, ``coupled``, ``reservoir``.  Default: waits for the whole device (a graph replays on the
        stream it is launched on), then reads; never inside a capture."""
        bath = self._need()
        if stream is None:
            torch.cuda.synchronize(self._device)
        return bath.read(stream_handle(stream, self._dev_index))

    def reset(self, stream=None) -> None:
        """Zero every system's counters, ``draws`` included, ordered on ``stream`` (default: torch's current stream): the
        same variates come again."""
        self._need().reset(stream_handle(stream, self._dev_index))

    def set_gammas(self, first: int, gammas) -> None:
        """Replace the gamma arrays of systems ``first`` .. ``first + len(gammas) - 1`` (None: no bath) after waiting for the
        last step's stream; never inside a capture.  The systems' counters are kept."""
        bath = self._need()
        gammas = list(gammas)
        if first < 0 or first + len(gammas) > self.n_systems or not gammas:
            raise ValueError("set_gammas: systems outside the batch")
        for k, g in enumerate(gammas, start=first):
            if g is not None:
                _gamma_tensor(g, k)
        bath.set_items(first, self._items(first, gammas))
        self._gammas[first:first + len(gammas)] = gammas

    @property
    def bath(self) -> _capi.Bath:
        return self._handle
