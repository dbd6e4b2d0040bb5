"""A numpy restatement of the run clock's rules (include/cavmd.h, "the run clock"): the end time of cavmd_draw_fill (item 4a of
the draw contract), the time rule of cavmd_ledger_record and the time rule of cavmd_field_recorder_record.  Built on
tests/draw_mirror.py and tests/trajectory_mirror.py by
import: the draw of an item that is not at rest IS draw_mirror.step, and the decision of one ledger call IS
trajectory_mirror.Item.call (the trajectory's rule 2) with the last time held in front of it.  Written from the header's text;
tests/test_runclock_abi.py holds it against hand-worked cases and against the two mirrors where no rule is set."""
import numpy as np

import draw_mirror
import trajectory_mirror

STATE_FIELDS = ("draws", "dt", "elapsed", "tolerance", "exhausted")


def new_state(n):
    st = draw_mirror.new_state(n)
    st["finished"] = np.zeros(n, dtype=np.uint64)
    return st


def at_rest(elapsed, t_end):
    """t_end > 0 and elapsed >= t_end, as IEEE comparisons: a NaN clock never finishes"""
    elapsed, t_end = np.asarray(elapsed, dtype=np.float64), np.asarray(t_end, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (t_end > 0.0) & (elapsed >= t_end)


def rest_rows(it):
    """the rows of items at rest: what the two input makers give for dt = 0 with every variate +0"""
    B = len(it["gamma"])
    one = np.ones(B, dtype=np.uint64).view(np.float64)
    verlet, bussi = np.zeros((B, 8)), np.zeros((B, 8))
    verlet[:, 1], verlet[:, 6] = it["gamma"], one
    bussi[:, 2] = np.where(it["tau"] != 0.0, 1.0, 0.0)          # exp(-0 / tau)
    bussi[:, 3], bussi[:, 4] = it["set_T"], one
    return verlet, bussi


def draw_step(seed, it, st, adaptive, recorded, S, t_end, tolerance=None):
    """One launch of an object with end times t_end ((B,), +0: none) -> (verlet, bussi, new state, info) as draw_mirror.step,
    the state with `finished`, info with `rest` (which items were at rest in this call); the bounds of an item at rest are 0."""
    rest = at_rest(st["elapsed"], t_end)
    verlet, bussi, new, info = draw_mirror.step(seed, it, {k: st[k] for k in STATE_FIELDS}, adaptive, recorded, S, tolerance)
    rv, rb = rest_rows(it)
    verlet[rest], bussi[rest] = rv[rest], rb[rest]
    for name in STATE_FIELDS:
        new[name] = np.where(rest, st[name], new[name])
    new["finished"] = rest.astype(np.uint64)
    info = {k: np.where(rest, np.zeros_like(v), v) for k, v in info.items()}
    info["rest"] = rest
    return verlet, bussi, new, info


class LedgerItem:
    """the four counter words of one ledger item and, beside them, last_time"""

    def __init__(self):
        self.words = trajectory_mirror.Item()
        self.last_time = 0.0

    def reset(self):
        self.words.reset()
        self.last_time = 0.0

    @property
    def counters(self):
        w = self.words
        return w.rows, w.calls, w.phase, w.slot

    def call(self, capacity: int, period: int, time_interval: float, max_time: float, time):
        """One cavmd_ledger_record for this item; `time` is what *d_time holds (None: d_time is NULL, legal without a rule
        only).  Returns None where no row is written, else dict(call, row, time, slot)."""
        w = self.words
        if time_interval == 0.0:                                 # no rule: every period-th call, last_time is not touched
            return w.call(capacity, period, 0.0, time, False)
        assert period == 1 and time is not None
        with np.errstate(invalid="ignore"):
            if max_time > 0.0 and bool(np.float64(time) > np.float64(max_time)):
                w.calls += 1                                     # past the last time: the call is counted, nothing else moves
                return None
        w.last_time = self.last_time
        head = w.call(capacity, 1, time_interval, time, False)
        if head is not None:
            self.last_time = head["time"]
        return head


class FieldItem:
    """the six counter words of one field-recorder item, the rows its references were taken at and, beside them, last_time and
    last_reference_time.  Restates the decisions of one cavmd_field_recorder_record call from include/cavmd.h: whether the row
    is written, and whether it takes a reference (after the correlation)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.rows = self.calls = self.phase = self.slot = self.refs = self.last_ref = 0
        self.ref_rows = []
        self.last_time = self.last_reference_time = 0.0

    @property
    def counters(self):
        return self.rows, self.calls, self.phase, self.slot, self.refs, self.last_ref

    def call(self, capacity: int, period: int, interval: int, max_refs: int, time_interval: float, ref_time_interval: float,
             time, asked: bool):
        """Returns None where no row is written, else dict(call, row, slot, n_references, took_reference, time)."""
        timed = time_interval > 0.0
        self.calls += 1
        with np.errstate(invalid="ignore"):
            if timed:
                assert period == 1
                due_row = self.rows == 0 or bool(np.float64(time) - np.float64(self.last_time) >= np.float64(time_interval))
            else:
                self.phase += 1
                due_row = self.phase >= period
            if not due_row:
                return None
            if timed and ref_time_interval > 0.0:                # in place of the row count
                by_interval = bool(np.float64(time) - np.float64(self.last_reference_time) >= np.float64(ref_time_interval))
            else:
                by_interval = interval > 0 and self.rows - self.last_ref >= interval
        take = self.refs < max_refs and (self.refs == 0 or by_interval or bool(asked))
        head = dict(call=self.calls, row=self.rows, slot=self.slot, n_references=self.refs, took_reference=bool(take),
                    time=float(time) if timed else 0.0)
        if take:
            self.ref_rows.append(self.rows)
            self.last_ref = self.rows
            self.refs += 1
            if timed:
                self.last_reference_time = float(time)           # whatever the cause of the reference
        self.rows += 1
        self.slot = self.rows % capacity
        self.phase = 0
        if timed:
            self.last_time = float(time)
        return head
