"""``BatchThermalizer`` -- the start of B independent small systems in ONE launch: seeded momenta and the photon's placement.

The reference's driver does two things before its first step, both on the host (examples/05_advanced_run.py):
``thermalize_system`` (:710-750) calls ``thermalize_particle_momenta(kT, filter=Type(['O', 'N']))`` on the molecules and draws
a separate normal velocity for the cavity particle, and ``add_cavity_particle`` (:455-494) places the photon at ``q = 0`` or,
with ``--finite-q``, at ``-d g / omegac**2`` with the z component zeroed, adds a thermal spread ``sqrt(kT / omegac**2)`` where
``g != 0``, wraps the position and sets the image flags.  This class does both for every system with one kernel
(``cavmd_thermalize_run``; the arithmetic is spelled out in include/cavmd.h), reading the molecular dipole where it lives: in
the result block of the ``CavityForceBatch``.  It is seeded and counted like ``LangevinBathBatch``: system i draws under the key
``(seed + 0x9E3779B97F4A7C15 * (i + 1)) mod 2**64`` (``seeds=`` overrides it, one key per system), so its start does not
depend on its place in a batch, and the call counter lives on the device, so a captured ``thermalize()`` draws a new block
with every replay.  The order of a start -- a moved photon makes the earlier forces stale::

    cavity = CavityForceBatch(sysdefs, params)
    thermalizer = BatchThermalizer(velocities, kT, seed, cavity=cavity, place_photon=True, finite_q=True)
    cavity.compute()                                     # 1. the molecular dipole of every system
    thermalizer.thermalize()                             # 2. velocities, the photon's velocity, position and image
    cavity.compute(); molecular.compute()                # 3. the forces of the state the run starts from
    integrator.prime()                                   # 4. a = F / m
    thermalizer.state()["thermalised"]                   # per system: the particles that received a velocity

Without ``members`` every particle but the photon receives a velocity (every particle where there is no ``cavity`` or its
result names no photon); ``zero_momentum`` then shares the total momentum out, as HOOMD-blue's
``thermalize_particle_momenta`` does.  The photon's velocity carries no momentum term (the driver's :729).

The limits.  The variates are Philox with the counter layout published in include/cavmd.h, not HOOMD's RandomGenerator and not
numpy's: no start is bit-comparable with a HOOMD run; the momentum rule restates HOOMD-blue 4.x from knowledge and parity with
it is pinned by nothing; everything after the draw is held to the header's expressions.  Angular momenta and triclinic boxes
are out of scope.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import Checkpointable, HandleOwner, device_tensor, one_device, per_system, stream_handle

_RESULT_BYTES = 192


class BatchThermalizer(HandleOwner, Checkpointable):
    """velocities: one ``(N_k, 4)`` float64 device tensor per system, mass in column 3; kT: one number, or one per system;
    seed: 0 .. 2**64 - 1; members: None, or per system None / an index array of the particles that receive a velocity (an
    index at or beyond N_k is skipped and counted); zero_momentum: take the total momentum out of them; cavity: the
    ``CavityForceBatch`` of the same systems, which supplies positions, images, boxes, params and result blocks;
    place_photon / finite_q: place the photon at ``q = 0`` or at the displaced equilibrium (both need ``cavity``);
    photon_velocity: draw the photon's velocity (it has one only with ``cavity``); seeds: None, or one Philox key per system."""

    def __init__(self, velocities, kT, seed=0, members=None, zero_momentum=True, cavity=None, place_photon=False, finite_q=False,
                 photon_velocity=True, seeds=None):
        velocities = list(velocities)
        for v in velocities:
            device_tensor(v, "BatchThermalizer", "velocity")    # CPU tensors are refused before anything else is looked at
        B = len(velocities)
        if B == 0:
            raise ValueError("a thermalizer needs at least one system")
        if cavity is not None and len(cavity) != B:
            raise ValueError(f"velocities: one entry per system of the cavity batch ({len(cavity)})")
        if (place_photon or finite_q) and cavity is None:
            raise ValueError("place_photon and finite_q need the cavity batch: it holds the photon and the dipole")
        dev = one_device(velocities, "thermalizer")
        members = [None] * B if members is None else list(members)
        if len(members) != B:
            raise ValueError(f"members: one entry per system ({B})")
        self.seed = int(seed)
        if not 0 <= self.seed < 2**64:
            raise ValueError("seed: 0 .. 2**64 - 1")
        self._kTs = [float(x) for x in per_system(kT, B, "kT")]
        self.keys = ([_capi.bath_item_key(self.seed, i) for i in range(B)] if seeds is None
                     else [int(x) for x in per_system(seeds, B, "seeds")])
        if any(not 0 <= key < 2**64 for key in self.keys):
            raise ValueError("seeds: 0 .. 2**64 - 1")
        self._flags = dict(zero_momentum=bool(zero_momentum), place_photon=bool(place_photon), finite_q=bool(finite_q),
                           photon_velocity=bool(photon_velocity))
        self._velocities, self._cavity = velocities, cavity   # the arrays outlive the launches
        self._members = []
        for k, m in enumerate(members):
            if m is None:
                self._members.append(None)
                continue
            idx = np.ascontiguousarray(m, dtype=np.uint32).reshape(-1)
            host = idx if idx.size else np.zeros(1, dtype=np.uint32)   # an element behind the pointer: an empty list is not
            held = torch.from_numpy(host.view(np.int32).copy()).to(dev)  # the default set
            self._members.append((held, int(idx.size)))
        if cavity is not None:
            sizes = cavity.batch.sizes
            for k, v in enumerate(velocities):
                if v.shape[0] != sizes[k]:
                    raise ValueError(f"system {k}: the velocity array has {v.shape[0]} rows, the cavity batch evaluates {sizes[k]}")
        self._open(dev, lambda ws: _capi.Thermalize(ws, self._items(range(B))))
        self.n_systems = B
        self._stream = 0
        torch.cuda.current_stream(dev).synchronize()   # the member lists are on the device before any stream runs

    def _items(self, systems):
        flags = ((_capi.THERMALIZE_ZERO_MOMENTUM if self._flags["zero_momentum"] else 0)
                 | (_capi.THERMALIZE_PLACE_PHOTON if self._flags["place_photon"] else 0)
                 | (_capi.THERMALIZE_FINITE_Q if self._flags["finite_q"] else 0)
                 | (_capi.THERMALIZE_PHOTON_VELOCITY if self._flags["photon_velocity"] else 0))
        cavity = self._cavity
        results = cavity.batch.results_device_ptr() if cavity is not None else 0
        items = []
        for k in systems:
            v, m = self._velocities[k], self._members[k]
            n = int(v.shape[0])
            args = dict(vel_ptr=v.data_ptr() if n else 0, N=n, kT=self._kTs[k], seed=self.keys[k], flags=flags)
            if m is not None:
                args.update(members_ptr=m[0].data_ptr(), n_members=m[1])
            if cavity is not None:
                pd = cavity._sysdefs[k].getParticleData()
                args.update(pos_ptr=pd.getPositions().data_ptr() if n else 0, image_ptr=pd.getImages().data_ptr() if n else 0,
                            result_ptr=results + _RESULT_BYTES * k, box_L=pd.getGlobalBox().getL(), params=cavity._params[k])
                if not n:   # an empty system has no arrays to place a photon in; the kernel leaves it untouched
                    args["flags"] = flags & ~(_capi.THERMALIZE_PLACE_PHOTON | _capi.THERMALIZE_FINITE_Q)
            items.append(_capi.thermalize_item(**args))
        return items

    def thermalize(self, stream=None) -> None:
        """ONE kernel on ``stream`` (default: torch's current stream): every system's velocities, momentum, photon and
        counters.  Nothing is waited for.  May be captured; a replay draws anew."""
        handle = stream_handle(stream, self._dev_index)
        self._need().run(handle)
        self._stream = handle

    def state(self, stream=None) -> np.ndarray:
        """Per-system ``draws``, ``thermalised``, ``skipped``, ``momentum`` and ``photon``.  Default: waits for the whole
        device (a graph replays on the stream it is launched on), then reads; never inside a capture."""
        handle = self._need()
        if stream is None:
            torch.cuda.synchronize(self._device)
        return handle.read(stream_handle(stream, self._dev_index))

    def reset(self, stream=None) -> None:
        """Zero every system's counters, ``draws`` included, ordered on ``stream`` (default: torch's current stream): the
        same variates come again."""
        self._need().reset(stream_handle(stream, self._dev_index))

    def update(self, kT=None, zero_momentum=None, place_photon=None, finite_q=None, photon_velocity=None) -> None:
        """Replace what is given (``cavmd_thermalize_set_items`` on every system) after waiting for the last launch's stream;
        never inside a capture.  The counters are kept, and a ``thermalize()`` captured earlier follows the new values."""
        handle = self._need()
        kTs, flags = list(self._kTs), dict(self._flags)
        if kT is not None:
            kTs = [float(x) for x in per_system(kT, self.n_systems, "kT")]
        for name, value in (("zero_momentum", zero_momentum), ("place_photon", place_photon), ("finite_q", finite_q),
                            ("photon_velocity", photon_velocity)):
            if value is not None:
                flags[name] = bool(value)
        if (flags["place_photon"] or flags["finite_q"]) and self._cavity is None:
            raise ValueError("place_photon and finite_q need the cavity batch: it holds the photon and the dipole")
        old = self._kTs, self._flags
        self._kTs, self._flags = kTs, flags
        try:
            handle.set_items(0, self._items(range(self.n_systems)))
        except Exception:
            self._kTs, self._flags = old
            raise

    @property
    def thermalizer(self) -> _capi.Thermalize:
        return self._handle
