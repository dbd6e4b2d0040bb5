"""``CoulombForceBatch`` -- the Ewald Coulomb forces of B independent small systems in TWO kernel launches.

The reference's driver adds the pair of forces returned by ``make_pppm_coulomb_forces`` over the bond-excluding neighbour list
(examples/05_advanced_run.py:598-608): HOOMD-blue's PPPM, a mesh approximation of the Ewald sum.  For systems of at most 2048
particles the sum itself is cheaper than a mesh, so this class is the Ewald sum (``cavmd_coulomb_compute``; the expressions are
spelled out in include/cavmd.h): real space over all pairs out of LDS, reciprocal space as a direct sum over the kept
k-vectors -- with one sincos per (particle, k), or with ``reciprocal="factored"`` from per-axis phase factors.  It is the
twin of ``MolecularForceBatch``, and its force arrays are further forces of the integrator's items::

    coulomb = CoulombForceBatch(sysdefs, exclusions=bonds, r_cut=12.0, accuracy=1e-6)
    integrator = VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(molecular.forces, coulomb.forces)])
    with torch.cuda.graph(graph):
        integrator.step_one(); cavity.compute(); molecular.compute(); coulomb.compute(); integrator.step_two()

The reference treats electrostatics as two forces (``short, long = make_pppm_coulomb_forces(...)``) and logs an energy column
for each.  ``split=True`` gives the batch a second set of arrays and evaluates the sum in those two groups
(``cavmd_mts_coulomb_compute_parts``): ``forces`` are then the SHORT part (the erfc terms inside the cut-off), ``forces_long`` the
LONG part (the exclusion partners' erf terms, the reciprocal sum, the self and background terms), and ``compute(parts=...)``
evaluates "both", "short" or "long".  ``short`` and ``long`` are small objects with ``.forces`` for ``VerletBatch`` force
slots, ``VerletBatch.kick`` and ``BatchEnergyLedger(terms=[("ewald_short", c.short), ("ewald_long", c.long)])``.  Evaluating
the long part every n-th step and kicking with it is the impulse multiple-time-step scheme
(examples/mts/batch_mts_coulomb_in_one_graph.py); it is defined for a dt that stays the same through an outer step.

Parity with HOOMD-blue's PPPM is not pinned: what separates the two is PPPM's discretisation error.  No CPU fallback: CPU
tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import stream_handle
from ._force_batch import ForceBatchBase


class CoulombPart:
    """One part of a split batch: ``forces``, per system an (N_k, 4) float64 device tensor (``.w``: the particle's share of
    the part's energy).  Keeps the batch alive."""

    def __init__(self, batch, name: str, forces):
        self.batch, self.name, self._forces = batch, name, forces

    @property
    def forces(self):
        return list(self._forces)

    def __len__(self) -> int:
        return len(self._forces)


class CoulombForceBatch(ForceBatchBase):
    """sysdefs: the systems (positions, charges -- ``getCharges()`` -- and boxes are taken from them; all on one GPU);
    exclusions: per system an (n, 2) integer array of pairs whose Coulomb interaction is removed (the bonds), or None;
    r_cut: the real-space cut-off, at most half the shortest box length; then either ``accuracy`` (kappa and k_cut follow from
    ``cavmd_coulomb_parameters``) or both ``kappa`` and ``k_cut``.  ``reciprocal``: "direct" (one sincos per particle and
    k-vector) or "factored" (per-axis phase factors, ``cavmd_ewald_set_reciprocal``; same expressions, results within the
    rounding bound, not the same bits).  ``compute`` is TWO kernels; column 3 of a force array is the particle's share of the
    Coulomb energy.  ``split``: the object owns a second set of arrays, ``forces_long``, and ``compute`` evaluates the SHORT
    part into ``forces`` (one kernel) and the LONG part into ``forces_long`` (two), together or one at a time."""

    def __init__(self, sysdefs, exclusions, r_cut, accuracy=None, kappa=None, k_cut=None, reciprocal="direct", split=False):
        if reciprocal not in _capi.EWALD_RECIPROCAL:
            raise ValueError(f"reciprocal: one of {sorted(_capi.EWALD_RECIPROCAL)}, not {reciprocal!r}")
        pds = self._systems(sysdefs)
        self._need_gpu(pds, lambda pd: (pd.getPositions(), pd.getCharges()), "position and charge")
        if (accuracy is None) == (kappa is None or k_cut is None) or (accuracy is not None and (kappa is not None or k_cut is not None)):
            raise ValueError("give either accuracy or both kappa and k_cut")
        if accuracy is not None:
            kappa, k_cut = _capi.coulomb_parameters(r_cut, accuracy)
        self.r_cut, self.kappa, self.k_cut = float(r_cut), float(kappa), float(k_cut)
        self._one_device(pds)
        B = len(pds)
        exclusions = [None] * B if exclusions is None else list(exclusions)
        if len(exclusions) != B:
            raise ValueError(f"exclusions: one array per system ({B})")
        sizes = self._allocate(pds)
        self._charges = []
        items = []
        for k, pd in enumerate(pds):
            e = np.zeros((0, 2), dtype=np.int64) if exclusions[k] is None else np.asarray(exclusions[k], dtype=np.int64).reshape(-1, 2)
            if len(e) and (e.min() < 0 or e.max() >= 2**32):
                raise ValueError(f"system {k}: negative exclusion index")
            q = pd.getCharges()
            if q.dtype != torch.float64 or not q.is_contiguous():
                raise ValueError(f"system {k}: charges are a contiguous float64 tensor")
            self._charges.append(q)
            n = sizes[k]
            items.append(_capi.coulomb_item(n, pd.getPositions().data_ptr() if n else 0, q.data_ptr() if n else 0,
                                            self._force[k].data_ptr() if n else 0, pd.getGlobalBox().getL(), self.kappa, self.r_cut,
                                            self.k_cut, e))
        self.k_counts = []
        for k, it in enumerate(items):
            try:
                self.k_counts.append(_capi.coulomb_k_count(it))
            except _capi.CavmdError as e:
                if e.status == _capi.CAVMD_ERR_CAPACITY and sizes[k] <= _capi.COULOMB_MAX_ITEM_N:
                    raise ValueError(f"system {k}: k_cut = {self.k_cut:.4g} keeps more than {_capi.COULOMB_MAX_K} k-vectors in its box; "
                                     "ask for a coarser accuracy or a larger r_cut") from e
                raise
        self._boxes = [tuple(float(l) for l in pd.getGlobalBox().getL()) for pd in pds]
        self._open(self._device, lambda ws: _capi.Coulomb(ws, items))
        self.split = bool(split)
        try:
            self.set_reciprocal(reciprocal)
            if self.split:
                self._pool_long = torch.zeros_like(self._pool)
                starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
                self._force_long = [self._pool_long[int(starts[k]):int(starts[k + 1])] for k in range(B)]
                torch.cuda.current_stream(self._device).synchronize()
                self._need().set_long_forces([f.data_ptr() if n else 0 for f, n in zip(self._force_long, sizes)])
                self.short = CoulombPart(self, "short", self._force)
                self.long = CoulombPart(self, "long", self._force_long)
        except Exception:
            self.close()
            raise

    @property
    def coulomb(self) -> _capi.Coulomb:
        return self._handle

    def compute(self, timestep: int = 0, stream=None, parts=None) -> None:
        """Not split: today's TWO kernels, the whole sum into ``forces`` (``parts`` raises).  Split: ``parts`` is "both" (the
        default; three kernels), "short" (one kernel, writes ``forces``) or "long" (two kernels, writes ``forces_long``).  May
        be captured; ``timestep`` is not used."""
        if not self.split:
            if parts is not None:
                raise ValueError("parts: the batch was not created with split=True")
            return super().compute(timestep, stream)
        parts = "both" if parts is None else parts
        if parts not in _capi.COULOMB_PARTS:
            raise ValueError(f"parts: one of {sorted(_capi.COULOMB_PARTS)}, not {parts!r}")
        self._need().compute_parts(stream_handle(stream, self._dev_index), _capi.COULOMB_PARTS[parts])

    @property
    def forces_long(self):
        """Split batches only: per-system (N_k, 4) float64 device tensors of the LONG part."""
        if not self.split:
            raise AttributeError("forces_long: the batch was not created with split=True")
        return list(self._force_long)

    def potential_energy(self) -> torch.Tensor:
        """(B,) device tensor: the Coulomb energy of every system; for a split batch the sum of both parts' ``.w``."""
        e = super().potential_energy()
        return e + self._pool_energy(self._pool_long) if self.split else e

    @property
    def reciprocal(self) -> str:
        """"direct" or "factored": how ``compute`` obtains cos(k.x) and sin(k.x)."""
        method = self._need().reciprocal
        return next(name for name, value in _capi.EWALD_RECIPROCAL.items() if value == method)

    def set_reciprocal(self, name: str) -> None:
        """Selects the reciprocal-space method of later ``compute`` calls (a launch already captured keeps its own).  Not during
        a stream capture.  A system whose k-vectors reach beyond the factored method's per-axis limit raises ValueError and
        leaves the method as it was."""
        if name not in _capi.EWALD_RECIPROCAL:
            raise ValueError(f"reciprocal: one of {sorted(_capi.EWALD_RECIPROCAL)}, not {name!r}")
        try:
            self._need().set_reciprocal(_capi.EWALD_RECIPROCAL[name])
        except _capi.CavmdError as e:
            if e.status != _capi.CAVMD_ERR_CAPACITY:
                raise
            max_m = _capi.ewald_order()[2]
            for k, box in enumerate(self._boxes):
                for axis, length in zip("xyz", box):
                    M = int(self.k_cut * length / (2.0 * np.pi)) if self._sizes[k] else 0
                    if M > max_m:
                        raise ValueError(f"system {k}: the k-vectors reach M = {M} along {axis}, beyond the factored method's "
                                         f"{max_m}; use reciprocal='direct'") from e
            raise
