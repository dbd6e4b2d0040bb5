"""``BatchEnergyLedger`` -- every term of the conserved energy of B independent small systems, appended by ONE kernel launch
per step to a time series in device memory.

What the reference's ``EnergyTracker`` (src/cavitymd/analysis.py:425-1046) writes per output step -- the potential of every
force, the three cavity energies, the molecular, cavity and total kinetic energy, the system total, the reservoir energy of
every bath and ``universe_total_energy``, the column it marks ``[CONSERVED]`` -- is one 192-byte row per system here
(``cavmd_ledger_row``).  The kernel reads the ``.w`` column of the force arrays, the result blocks, the velocities and the
baths' reservoirs where they live on the device, when it runs; the write position lives on the device too, so ``record()``
captured into a graph appends a NEW row on every replay::

    ledger = BatchEnergyLedger(cavity, velocities, terms=[molecular, coulomb],
                               reservoirs=[("bussi", thermostat), ("langevin", integrator)], capacity=steps)
    with torch.cuda.graph(graph):
        integrator.step_one()
        cavity.compute(); molecular.compute(); coulomb.compute()
        integrator.step_two()
        ledger.record()                   # one kernel: one row per system
        thermostat.step_async()
    for _ in range(steps):
        graph.replay()
    series = ledger.read()                # (B, steps) structured array, one copy, behind one synchronisation
    series["universe_total"]              # the conserved quantity of every system at every step
    series["bussi"]                       # = series["reservoir"][:, :, 0]

Each potential term is a fixed-order compensated sum within 2 ulp of the exact one; ``kinetic_group`` and ``kinetic_cavity``
have the bits of ``BatchRecorder``'s ``kinetic_energy`` and ``cavity_kinetic``; every total is the expression listed in
include/cavmd.h, one rounding per operation.  One ``.w`` per force array: the reference's ``harmonic`` / ``lj`` columns are
not split (create two force batches for that); ``ewald_short`` / ``ewald_long`` are the two arrays of a split
``CoulombForceBatch``, ``terms=[("ewald_short", coulomb.short), ("ewald_long", coulomb.long)]``.

There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _capi
from ._device import device_tensor, member_indices, stream_handle
from .recorder import _SeriesRecorder
from .utils import PhysicalConstants

MAX_TERMS = MAX_RESERVOIRS = 4
_RESULT_BYTES = 192   # sizeof(cavmd_result)


def _device_tensor(t, what: str):
    return device_tensor(t, "BatchEnergyLedger", what, note=" (HOOMD Scalar4)")


def _named(entries, default: str):
    """[(name, object)] of entries given as objects or as (name, object) pairs"""
    out = []
    for k, e in enumerate(entries):
        if isinstance(e, tuple) and len(e) == 2 and isinstance(e[0], str):
            out.append(e)
        else:
            out.append((f"{default}{k}", e))
    return out


def _reservoir_addresses(obj, B: int):
    """The device address of system i's reservoir double, for i < B; the object whose memory that is."""
    from .bath_batch import LangevinBathBatch
    from .integrator_batch import VerletBatch
    from .thermostat_batch import BussiReservoirBatch
    for cls, struct, field in ((BussiReservoirBatch, _capi.BussiDeviceState, "reservoir_translational"),
                               (VerletBatch, _capi.VerletState, "langevin_reservoir"),
                               (LangevinBathBatch, _capi.BathState, "reservoir")):
        if isinstance(obj, cls):
            if obj.n_systems != B:
                raise ValueError(f"a {cls.__name__} of {obj.n_systems} systems as the reservoir of a ledger of {B}")
            base = obj._need().state_device_ptr() + getattr(struct, field).offset
            stride = ctypes.sizeof(struct)
            return [base + stride * i for i in range(B)]
    if isinstance(obj, torch.Tensor):
        if obj.device.type != "cuda":
            raise RuntimeError("BatchEnergyLedger needs the reservoir arrays in GPU memory; no CPU fallback exists in this package")
        if obj.dtype != torch.float64 or obj.shape != (B,) or not obj.is_contiguous():
            raise ValueError(f"a reservoir tensor must be a contiguous ({B},) float64 tensor")
        return [obj.data_ptr() + 8 * i for i in range(B)]
    raise TypeError("a reservoir is a BussiReservoirBatch, a VerletBatch, a LangevinBathBatch or a (B,) float64 device tensor")


class BatchEnergyLedger(_SeriesRecorder):
    """cavity: the ``CavityForceBatch`` whose result blocks hold the three cavity energies and the photon's index, or None
    (no cavity); velocities: one (N_k, 4) device tensor per system (mass in column 3), or None per system; terms: up to four
    force batches (anything with ``.forces``) or lists of one (N_k, 4) tensor per system, whose ``.w`` is summed; reservoirs:
    up to four ``BussiReservoirBatch``, ``VerletBatch`` or ``LangevinBathBatch`` objects or (B,) float64 device tensors; terms
    and reservoirs may be given as (name, object) pairs, and ``read()`` has the columns under those names as well; members:
    None (every particle that is not of the cavity's type 'L', the cavity particle's kinetic energy being added to the
    total), or per system None / an index array of the group ``kinetic_group`` covers; dof: the degrees of freedom of
    ``temperature``, one number or one per system (default 3 * n_members); clock: a ``StepDraw`` whose elapsed time becomes
    ``time``, or None; add_cavity_kinetic: whether ``kinetic_total`` adds the cavity particle's kinetic energy to the group's
    (default: only where ``members`` is left to its default, a group given by the caller may hold that particle already).
    An item keeps its last ``capacity`` rows; every ``period``-th ``record()`` writes one."""
    _record_dtype = staticmethod(_capi.ledger_row_dtype)

    def __init__(self, cavity, velocities, terms=(), reservoirs=(), members=None, dof=None, clock=None, capacity: int = 4096,
                 period: int = 1, kB: float = PhysicalConstants.KB_HARTREE_PER_K, add_cavity_kinetic=None):
        velocities = list(velocities)
        for v in velocities:
            if v is not None:
                _device_tensor(v, "velocity")          # CPU tensors are refused before anything else is looked at
        B = len(velocities)
        if B == 0:
            raise ValueError("a ledger needs at least one system")
        if cavity is not None and len(cavity) != B:
            raise ValueError(f"velocities: one entry per system of the force batch ({len(cavity)})")
        terms, reservoirs = _named(list(terms), "term"), _named(list(reservoirs), "reservoir")
        if len(terms) > MAX_TERMS or len(reservoirs) > MAX_RESERVOIRS:
            raise ValueError(f"at most {MAX_TERMS} terms and {MAX_RESERVOIRS} reservoirs")
        term_arrays = []
        for name, t in terms:
            arrays = list(t.forces if hasattr(t, "forces") else t)
            if len(arrays) != B:
                raise ValueError(f"term {name!r}: one force array per system ({B})")
            for f in arrays:
                _device_tensor(f, "force")
            term_arrays.append(arrays)
        dev = next((t.device for t in velocities + [f for arrays in term_arrays for f in arrays] if t is not None), None)
        if dev is None:
            if cavity is None:
                raise ValueError("a ledger without velocities, terms and cavity has nothing to read")
            dev = cavity.forces[0].device
        sizes = []
        for k in range(B):
            ns = {int(t.shape[0]) for t in [velocities[k]] + [arrays[k] for arrays in term_arrays] if t is not None}
            if cavity is not None:
                ns.add(int(cavity.batch.sizes[k]))
            if len(ns) > 1:
                raise ValueError(f"system {k}: its arrays have {sorted(ns)} rows")
            if any(t is not None and t.device != dev for t in [velocities[k]] + [arrays[k] for arrays in term_arrays]):
                raise ValueError("all systems of one ledger live on one device")
            sizes.append(ns.pop() if ns else 0)
        default_group = members is None and cavity is not None
        if add_cavity_kinetic is None:
            add_cavity_kinetic = default_group
        members = [None] * B if members is None else list(members)
        if len(members) != B:
            raise ValueError("members: None, or one entry per system")
        if default_group:
            members = [self._not_the_cavity(cavity, k) for k in range(B)]
        reservoir_ptrs = [_reservoir_addresses(obj, B) for _, obj in reservoirs]
        time_ptrs = [0] * B
        if clock is not None:
            if clock.n_systems != B:
                raise ValueError(f"a clock of {clock.n_systems} systems for a ledger of {B}")
            base = clock._need().state_device_ptr() + _capi.DrawState.elapsed.offset
            time_ptrs = [base + ctypes.sizeof(_capi.DrawState) * i for i in range(B)]
        results = cavity.batch.results_device_ptr() if cavity is not None else 0
        # everything whose memory the kernel reads stays alive with the ledger
        self._kept = (cavity, velocities, term_arrays, [obj for _, obj in terms], [obj for _, obj in reservoirs], clock)
        dofs = [None] * B if dof is None else ([float(dof)] * B if np.isscalar(dof) else [float(d) for d in dof])
        if len(dofs) != B:
            raise ValueError(f"dof: one value, or one per system ({B})")
        self._members, items = [], []
        for k in range(B):
            v, n = velocities[k], sizes[k]
            if members[k] is None:
                mt, n_members = None, (n if v is not None else 0)
            else:
                mt, n_members = member_indices(members[k], n, dev)
            self._members.append(mt)
            items.append(_capi.ledger_item(
                results + _RESULT_BYTES * k if cavity is not None else 0, v.data_ptr() if (v is not None and n) else 0,
                mt.data_ptr() if (mt is not None and n_members) else 0, n_members, n,
                [arrays[k].data_ptr() for arrays in term_arrays] if n else [], [ptrs[k] for ptrs in reservoir_ptrs],
                time_ptrs[k], 3.0 * n_members if dofs[k] is None else dofs[k], 1 if add_cavity_kinetic else 0))
        self.term_names = tuple(name for name, _ in terms)
        self.reservoir_names = tuple(name for name, _ in reservoirs)
        self._named_dtype = self._dtype_with_names()
        self._open(dev, lambda ws: _capi.Ledger(ws, items, capacity, period, kB))
        self.n_systems = B
        self.capacity, self.period = int(capacity), int(period)
        self._stream = 0
        torch.cuda.current_stream(dev).synchronize()   # the member lists are on the device before any stream records

    @staticmethod
    def _not_the_cavity(cavity, k: int):
        """indices of the particles of system k whose type is not 'L' (None: all of them)"""
        pd = cavity._sysdefs[k].getParticleData()
        try:
            L_typeid = pd.getTypeByName("L")
        except RuntimeError:
            return None
        tags = pd.getPositions()[:, 3].cpu().numpy().view(np.uint64) & 0xFFFFFFFF
        return np.flatnonzero(tags != L_typeid)

    def _dtype_with_names(self) -> np.dtype:
        """cavmd_ledger_row's dtype with one more field per named term and reservoir, at that column's own offset"""
        base = _capi.ledger_row_dtype()
        names, formats, offsets = list(base.names), [base.fields[n][0] for n in base.names], [base.fields[n][1] for n in base.names]
        for column, given in (("potential", self.term_names), ("reservoir", self.reservoir_names)):
            for k, name in enumerate(given):
                if name in names:
                    raise ValueError(f"the name {name!r} is a column of the row already, or was given twice")
                names.append(name)
                formats.append(np.dtype("<f8"))
                offsets.append(base.fields[column][1] + 8 * k)
        return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": base.itemsize})

    def record(self, stream=None) -> None:
        """ONE kernel launch on ``stream`` (default: torch's current stream): nothing is waited for; may be captured."""
        ledger = self._need()
        handle = stream_handle(stream, self._dev_index)
        ledger.record(handle)
        self._stream = handle

    def read(self, first=None, count=None, stream=None) -> np.ndarray:
        """Structured array of shape (B, n) with the columns of ``cavmd_ledger_row`` and, under the names given, those of the
        terms and reservoirs: rows first .. first + count - 1 (0-based count of recorded rows) of every system.  Default:
        everything still held.  Waits for the device (or, if given, for ``stream`` only); works the same before, between and
        after the replays of a graph, never inside a capture."""
        return self._read(first, count, stream).view(self._named_dtype)

    def set_time_rule(self, time_interval, max_time=None) -> None:
        """Rows by every system's own clock instead of by calls -- the reference's ``--energy-output-period-ps`` and
        ``--max-energy-output-time`` (``EnergyTracker``, src/cavitymd/analysis.py:692-701) under an adaptive dt: a system
        writes a row on its first ``record()`` and then whenever its clock has moved by ``time_interval`` since its last
        row, and none once the clock is past ``max_time`` (None or 0: no last time).  The clock is the ``clock=`` the ledger
        was built with, in its units; the ledger must have ``period == 1``.  ``time_interval`` None or 0 switches the rule
        off.  Set it BEFORE ``record()`` is captured: the rule is frozen into a captured launch.  A system at rest behind its
        end time (``StepDraw.set_end_time``) stops writing rows by itself.  Never inside a capture."""
        if self._kept[-1] is None and time_interval:
            raise ValueError("BatchEnergyLedger.set_time_rule needs the clock= the ledger is built with")
        self._need().set_time_rule(0.0 if time_interval is None else float(time_interval), 0.0 if max_time is None else float(max_time))

    @property
    def ledger(self):
        return self._handle
