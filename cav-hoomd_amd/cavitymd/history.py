"""``EnergyHistory`` -- per-step cavity energies without making the host wait for the step it just enqueued.

The reference's ``EnergyTracker`` (src/cavitymd/analysis.py:775-799) and ``CavityModeTracker`` (:1356-1359) call the three
energy getters after EVERY step.  A getter can only answer once its evaluation has finished, so each call drains the queue
and the next step is launched into an idle GPU.  Every evaluation also publishes its result into its own slot of a ring
(``cavmd_result_at``, the tunable ``"result_history"``, default 64 slots), so a tracker can note which evaluation belongs
to which timestep and read it one step later, while the next evaluation runs::

    history = EnergyHistory(compute)        # a CavityForceComputeHIP (or anything with the same three methods)
    for step in range(n_steps):
        compute.compute(step)
        history.record(step)
        for timestep, e_h, e_c, e_d in history.drain():   # every recorded step but the newest
            ...
    rows = history.flush()                  # the rest, the newest included

The rows are exactly what the synchronous getters would have returned right after each step, one step later.
"""
from __future__ import annotations

from collections import deque

from ._capi import CavmdError


class EnergyHistory:
    """Rows ``(timestep, E_harmonic, E_coupling, E_dipole_self)`` of recorded steps, read from the result history of
    ``compute`` (``lastSequence()`` / ``getEnergiesAt(sequence)``).

    A step whose slot has been reused (more than ``"result_history"`` steps recorded and not drained) or whose
    evaluation failed raises :class:`CavmdError` with the library's status; it is reported once, never skipped
    silently, and rows read before it are returned by the next ``drain()`` / ``flush()``."""

    def __init__(self, compute):
        self._compute = compute
        self._pending = deque()  # (timestep, sequence), oldest first
        self._rows = []          # rows already read, not yet handed out (a read after them raised)

    def record(self, timestep: int) -> None:
        """Note that the evaluation enqueued last belongs to ``timestep``.  Call after each ``compute(timestep)``."""
        self._pending.append((int(timestep), int(self._compute.lastSequence())))

    def __len__(self) -> int:
        return len(self._pending) + len(self._rows)

    def _read(self, keep: int):
        while len(self._pending) > keep:
            timestep, seq = self._pending[0]
            if seq == 0:
                e = (0.0, 0.0, 0.0)  # nothing evaluated yet: what the reference's getters return before the first step
            else:
                try:
                    e = self._compute.getEnergiesAt(seq)
                except CavmdError:
                    self._pending.popleft()  # reported once, here
                    raise
            self._pending.popleft()
            self._rows.append((timestep, float(e[0]), float(e[1]), float(e[2])))
        rows, self._rows = self._rows, []
        return rows

    def drain(self):
        """Rows of every recorded step except the newest, oldest first; they are forgotten.  While the newest
        evaluation is still running these reads do not wait for it."""
        return self._read(1)

    def flush(self):
        """Rows of every recorded step, the newest included (waits for it); the history is then empty."""
        return self._read(0)
