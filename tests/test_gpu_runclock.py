"""The run clock on the device: cavmd_draw_fill with end times, cavmd_ledger_record and cavmd_field_recorder_record under their
time rules, against the numpy restatement of the rules (tests/runclock_mirror.py) -- bit for bit where tests/test_gpu_step_draw.py is bit for bit, inside the
draw mirror's own bounds elsewhere; then the whole captured step of tests/checkpoint_runs.py with items at rest: at rest means at
rest, a raised end time continues bit for bit, replays equal eager steps, a graph captured before the rules keeps the old
behaviour, a run saved with items at rest resumes in fresh objects; the refusals that need a live object; run_until_finished;
the example.  Every index the new code forms is an item index below n_items, checked on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
import runclock_mirror as mirror
from abi_support import ROOT
from cavitymd import _capi
from checkpoint_runs import Run
from gpu_support import same as _same
from gpu_support import stream as _stream
from test_gpu_ledger import KB, Sys
from test_gpu_step_draw import MODES, SENTINEL, Tables, _plain_items, _ragged_table

pytestmark = pytest.mark.gpu

INV = _capi.CAVMD_ERR_INVALID_VALUE
NEVER = 1e30


def _state(draw):
    s = draw.read(_stream())
    out = {name: s[name].copy() for name in mirror.STATE_FIELDS}
    out["finished"], out["reserved"] = s["reserved"][:, 0].copy(), s["reserved"][:, 1:].copy()
    return out


def _refused(call, *args):
    with pytest.raises(_capi.CavmdError) as e:
        call(*args)
    assert e.value.status == INV
    return True


# ---- 1. the draw kernel with end times against the mirror ----------------------------------------------------------------------
def test_draw_with_end_times_equals_the_mirror():
    """600 items (lanes 256 and 512 are crossed) in both dt modes, six launches; t_end per item drawn from {none, passed after 1
    call, passed after 3 calls, never}, and on fixed-mode items the two edges: elapsed == t_end after one call (at rest in call
    2) and t_end one ulp above that (not at rest in call 2)."""
    B, SEED = 600, 0x9E3779B97F4A7C15
    rng = np.random.default_rng(31)
    it, adaptive, mode, launches = _ragged_table(B, rng)
    launches = launches + launches
    dest = (np.arange(B) // len(MODES)) % 3
    to_verlet, to_bussi = dest != 1, dest != 0
    # the clocks of a run without end times, from the mirror alone (a ramped tolerance differs from the device's by ulps: the
    # end times below sit half a step away from every clock value)
    st, clocks = mirror.new_state(B), []
    for recorded, S in launches[:3]:
        _, _, st, _ = mirror.draw_step(SEED, it, st, adaptive, recorded, S, np.zeros(B))
        clocks.append(st["elapsed"].copy())
    kind = rng.integers(0, 4, B)
    t_end = np.select([kind == 0, kind == 1, kind == 2], [0.0, 0.5 * clocks[0], 0.5 * (clocks[1] + clocks[2])], NEVER)
    plain = np.flatnonzero(mode == MODES.index("fixed"))
    equal, ulp_above = plain[0::2], plain[1::2]
    t_end[equal] = it["dt_initial"][equal]
    t_end[ulp_above] = np.nextafter(it["dt_initial"][ulp_above], np.inf)
    kind[plain] = 4
    assert (t_end >= 0).all() and len(equal) > 5 and len(ulp_above) > 5

    t = Tables(B)
    ws = _capi.Workspace(1)
    draw = _capi.Draw(ws, SEED, [t.item(k, it, adaptive, to_verlet[k], to_bussi[k]) for k in range(B)])
    draw.set_end(0, t_end)
    st = mirror.new_state(B)
    first_rest = np.zeros(B, dtype=np.int64)                                 # the 1-based launch that found the item at rest
    left_out = 0
    for launch, (recorded, S) in enumerate(launches, 1):
        t.plant(recorded, S)
        t.verlet.fill_(SENTINEL)
        t.bussi.fill_(SENTINEL)
        draw.fill(_stream())
        dev = _state(draw)
        verlet, bussi = t.verlet.cpu().numpy(), t.bussi.cpu().numpy()
        want_v, want_b, new, info = mirror.draw_step(SEED, it, st, adaptive, recorded, S, t_end, tolerance=dev["tolerance"])
        rest = info["rest"]
        first_rest[rest & (first_rest == 0)] = launch
        # the integrator row: every word bit for bit; a NULL destination's row is untouched
        assert _same(verlet[to_verlet], want_v[to_verlet]) and (verlet[~to_verlet] == SENTINEL).all()
        # the thermostat row: bit for bit where the draw test is (and the whole row of an item at rest), else inside the bound
        got, want = bussi[to_bussi], want_b[to_bussi]
        assert (bussi[~to_bussi] == SENTINEL).all()
        assert _same(got[:, 3:], want[:, 3:])
        exact_c = (~adaptive | rest)[to_bussi]
        assert _same(got[exact_c, 2], want[exact_c, 2])
        assert (np.abs(got[:, 2] - want[:, 2]) <= info["c_bound"][to_bussi]).all()
        assert (np.abs(got[:, 0] - want[:, 0]) <= info["normal_bound"][to_bussi]).all()
        check = ~info["gamma_ambiguous"][to_bussi]
        left_out += int((~check).sum())
        assert (np.abs(got[:, 1] - want[:, 1]) <= info["gamma_bound"][to_bussi])[check].all()
        assert _same(got[rest[to_bussi]], want[rest[to_bussi]])
        # the state: an item at rest keeps every word (no block consumed: `draws` stands), `finished` says which
        assert (dev["draws"] == new["draws"]).all() and _same(dev["dt"], new["dt"]) and _same(dev["elapsed"], new["elapsed"])
        assert (dev["finished"] == new["finished"]).all() and (dev["reserved"] == 0).all() and (dev["exhausted"] == 0).all()
        ramp = adaptive & (it["tol_time_constant"] != 0.0) & ~rest
        quiet = ~ramp
        own = np.where(rest, st["tolerance"], info["own_tolerance"])
        assert _same(dev["tolerance"][quiet], own[quiet])
        assert (np.abs(dev["tolerance"] - info["own_tolerance"])[ramp] <= info["tolerance_bound"][ramp]).all()
        assert (dev["draws"][rest] == st["draws"][rest]).all()
        assert draw.finished(_stream()) == int(rest.sum())
        st = new
        st["tolerance"] = dev["tolerance"].copy()                            # (a ramped one is the device's, as the mirror took it)
    moving = clocks[0] > 0.0                                                 # dt = 0 items never pass a positive end time
    print("first launch at rest, by kind:", {k: np.unique(first_rest[kind == k]).tolist() for k in range(5)},
          "; gamma draws left out:", left_out)
    assert (first_rest[kind == 0] == 0).all() and (first_rest[kind == 3] == 0).all()
    assert (first_rest[(kind == 1) & moving] == 2).all() and ((kind == 1) & moving).sum() > 50
    assert (first_rest[(kind == 1) & ~moving] == 0).all()
    three = (kind == 2) & (clocks[2] > clocks[1])
    assert (first_rest[three] == 4).all() and three.sum() > 50
    assert (first_rest[equal] == 2).all() and (first_rest[ulp_above] == 3).all()
    assert left_out * 1000 <= B * len(launches)
    for lanes in (slice(250, 262), slice(506, 518)):                         # both lane boundaries have items at rest and moving
        assert 0 < (first_rest[lanes] != 0).sum() < 12
    # reset zeroes the flag with the rest of the state; the end times are kept
    draw.reset(_stream())
    assert not any(_state(draw)[name].any() for name in ("draws", "elapsed", "finished"))
    draw.close()
    ws.close()


def _draw_only(B, seed, t_end):
    rng = np.random.default_rng(8)
    it, adaptive = _plain_items(B, rng)
    adaptive[::2] = True
    it["tol_target"][:] = 1e-3
    it["tol_initial"][:] = 1e-4
    it["tol_time_constant"][::4] = 300.0
    it["dt_min"][:], it["dt_max"][:] = 0.5, 50.0
    t = Tables(B)
    t.plant(np.full(B, 3, dtype=np.uint64), 1e-3 / rng.uniform(2.0, 6.0, B) ** 2)
    ws = _capi.Workspace(1)
    draw = _capi.Draw(ws, seed, [t.item(k, it, adaptive) for k in range(B)])
    if t_end is not None:
        draw.set_end(0, t_end)
    torch.cuda.synchronize()
    return t, ws, draw


def test_twenty_replays_equal_twenty_eager_launches():
    B, REPLAYS = 70, 20
    t_end = np.random.default_rng(1).choice([0.0, 7.0, 31.0, NEVER], B)      # dt is 2 .. 6: some rest early, some late, some never
    logs, states = [], []
    for captured in (False, True):
        t, ws, draw = _draw_only(B, 77, t_end)
        log = torch.zeros((REPLAYS, 2, B, 8), dtype=torch.float64, device="cuda")
        graph = None
        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                draw.fill(_stream())
            assert not _state(draw)["draws"].any()                           # capturing ran nothing
        for r in range(REPLAYS):
            graph.replay() if captured else draw.fill(_stream())
            log[r, 0].copy_(t.verlet)
            log[r, 1].copy_(t.bussi)
        states.append(draw.read(_stream()))
        logs.append(log.cpu().numpy())
        del graph
        draw.close()
        ws.close()
    assert _same(logs[0], logs[1]) and states[0].tobytes() == states[1].tobytes()
    finished = states[0]["reserved"][:, 0]
    assert 0 < finished.sum() < B and (states[0]["draws"][finished == 1] < REPLAYS).all()
    assert (states[0]["draws"][finished == 0] == REPLAYS).all()


# ---- 2. the whole captured step with items at rest (tests/checkpoint_runs.py) ---------------------------------------------------
T1 = [5.0, NEVER, 7.0, NEVER]        # systems 0 (N = 17) and 2 (N = 433) finish early; 1 (N = 55) and 3 (empty) keep going
T2 = [12.0, NEVER, 14.0, NEVER]        # above 5 + dt_max and 7 + dt_max: both have steps left to make
LEDGER_INTERVAL = 3.0
FIELD_INTERVAL, FIELD_REF_INTERVAL = 2.5, 9.0
FIRST, REST, MORE = 16, 14, 30       # dt >= 0.5: at most 14 steps to 7.0, so FIRST replays bring both to rest
PER_ITEM = ("position", "image", "velocity", "accel", "net_force")
STATES = ("state.integrator", "state.thermostat", "state.draw", "integrator.inputs", "thermostat.inputs")


class StepRun(Run):
    """checkpoint_runs.Run -- B = 4 systems of N = 17, 55, 433 and 0 (the issue's "four diatomic systems of N = 17" grown to the
    sizes the checkpoint tests use, the empty one included) under {fill, step one, cavity, molecular, Coulomb, step two with
    the cavity particle's Langevin row, recorder, ledger, field recorder, trajectory, Bussi thermostat} -- with a field recorder
    of period 1, which its time rule needs.  The states a test of this section covers are therefore the integrator's (with its
    Langevin reservoir), the thermostat's and the draw object's; a LangevinBathBatch is not in this step (its kernel obeys
    `skip` as step two does: tests/test_gpu_bath_batch.py)."""

    def __init__(self, field_capacity: int = 4):
        super().__init__()
        self.fields.close()
        positions = [s.getParticleData().getPositions() for s in self.sysdefs]
        self.fields = cavitymd.BatchFieldRecorder(positions, num_wavevectors=5, capacity=field_capacity, period=1, max_references=3,
                                                  reference_interval=3)
        self.objects["fields"] = self.fields
        self.checkpoint = cavitymd.BatchCheckpoint(self.sysdefs, self.velocities, self.objects)

    def set_rules(self, t_end):
        self.draw.set_end_time(t_end)
        self.ledger.set_time_rule(LEDGER_INTERVAL)
        self.fields.set_time_rule(self.draw, FIELD_INTERVAL, FIELD_REF_INTERVAL)


def _ruled(t_end, rules_before_capture=True, capture=True):
    run = StepRun()
    if rules_before_capture:
        run.set_rules(t_end)
    if capture:
        run.capture()
    return run


def _of_item(obs: dict, k: int, B: int = 4) -> dict:
    """what belongs to system k alone: its arrays, its slice of every state and input table, its timed series"""
    out = {name: obs[f"{name}.{k}"] for name in PER_ITEM}
    for name in STATES:
        size = len(obs[name]) // B
        out[name] = obs[name][k * size:(k + 1) * size]
    for series in ("ledger", "trajectory", "fields"):
        out["rows." + series] = obs["rows." + series][8 * k:8 * k + 8]
        out["read." + series] = obs[f"read.{series}.{k}"]
    out["fields"] = obs[f"fields.{k}"]                                       # the last field, the references and their rows
    return out


def _differ(a: dict, b: dict):
    assert a.keys() == b.keys()
    return [key for key in a if a[key] != b[key]]


@pytest.fixture(scope="module")
def runs():
    """A: T1, observed after FIRST, FIRST + REST (saved there) and FIRST + REST + MORE replays, then T2 and MORE replays again;
    R: no rule at all, FIRST + REST replays; D: T2 from the start, as many replays as A made in all."""
    out = {}
    a = _ruled(T1)
    a.replay(FIRST)
    out["a_first"] = a.observe()
    a.replay(REST)
    out["a_rest"] = a.observe()
    out["a_saved"] = a.checkpoint.state()
    a.replay(MORE)
    out["a_more"] = a.observe()
    a.draw.set_end_time(T2)                                                  # between two replays of the same graph
    a.replay(MORE)
    out["a_resumed"] = a.observe()
    out["a_draws"] = a.draw.state()["draws"].copy()
    a.close()
    r = StepRun()
    r.capture()
    r.replay(FIRST + REST)
    out["r"] = r.observe()
    r.close()
    d = _ruled(T2)
    d.replay(FIRST + REST + 2 * MORE)
    out["d"] = d.observe()
    d.close()
    return out


def test_at_rest_means_at_rest(runs):
    first, rest, plain = runs["a_first"], runs["a_rest"], runs["r"]
    draw = np.frombuffer(rest["state.draw"], dtype=_capi.draw_state_dtype())
    assert draw["reserved"][:, 0].tolist() == [1, 0, 1, 0] and (draw["elapsed"][[0, 2]] >= [5.0, 7.0]).all()
    assert (draw["draws"][[0, 2]] < FIRST).all() and draw["draws"][[1, 3]].tolist() == [FIRST + REST] * 2
    for k in (0, 2):                                                         # REST more replays: not a bit of them has moved
        assert not _differ(_of_item(first, k), _of_item(rest, k)), k
        assert np.frombuffer(rest["rows.ledger"], dtype=np.uint64)[k] >= 2   # (they wrote rows while they ran)
    for k in (1, 3):                                                         # the others ran on ...
        assert _differ(_of_item(first, k), _of_item(rest, k)), k
    # ... as in a batch that knows no end times.  (Not "a batch that never held the resting ones": the generator's counter holds
    # the item index, so a batch without items 0 and 2 draws other variates for the two that are left.  Items do not read each
    # other, so the same batch without any end time is the run they must equal.)
    for k in (1, 3):
        got, want = _of_item(rest, k), _of_item(plain, k)
        for name in ("state.draw", "rows.ledger", "read.ledger", "rows.fields", "read.fields", "fields"):   # (plain: every call)
            got.pop(name), want.pop(name)
        assert not _differ(got, want), k
        a, b = (np.frombuffer(o["state.draw"], dtype=_capi.draw_state_dtype())[k] for o in (rest, plain))
        assert all(a[n].tobytes() == b[n].tobytes() for n in mirror.STATE_FIELDS)
    # the recorder keeps writing a row per call for every item (the adaptive dt reads its last row)
    assert np.frombuffer(rest["rows.recorder"], dtype=np.uint64).tolist() == [FIRST + REST] * 4


def test_timed_ledger_rows_in_the_full_step(runs):
    """every row sits at least the interval behind the one before it, the first at the first call; an item at rest writes none"""
    obs = runs["a_more"]
    rows = np.frombuffer(obs["rows.ledger"], dtype=np.uint64)
    assert rows[0] == np.frombuffer(runs["a_first"]["rows.ledger"], dtype=np.uint64)[0]
    for k in range(4):
        held = np.frombuffer(obs[f"read.ledger.{k}"], dtype=_capi.ledger_row_dtype())
        assert len(held) == min(int(rows[k]), 8) and (np.diff(held["time"]) >= LEDGER_INTERVAL).all(), k
        assert (np.diff(held["call"].astype(np.int64)) >= 1).all()
    assert rows[3] == 1 + (FIRST + REST + MORE - 1) // 2                     # the empty system: dt = 2 throughout, a row every 2nd call


def test_a_raised_end_time_continues_bit_for_bit(runs):
    resumed, fresh = runs["a_resumed"], runs["d"]
    draw = np.frombuffer(resumed["state.draw"], dtype=_capi.draw_state_dtype())
    assert draw["reserved"][:, 0].tolist() == [1, 0, 1, 0] and (draw["elapsed"][[0, 2]] >= [12.0, 14.0]).all()
    assert _differ(_of_item(runs["a_more"], 0), _of_item(resumed, 0))        # it did go on
    for k in (0, 2):
        got, want = _of_item(resumed, k), _of_item(fresh, k)
        for name in ("read.ledger", "read.trajectory", "read.fields"):       # rows carry the call that wrote them: compared below
            got.pop(name), want.pop(name)
        assert not _differ(got, want), k
        for series, held, dtype in (("ledger", 8, _capi.ledger_row_dtype()), ("trajectory", 4, None),
                                    ("fields", 4, _capi.field_record_dtype())):
            a, b = resumed[f"read.{series}.{k}"], fresh[f"read.{series}.{k}"]
            n = min(int(np.frombuffer(fresh["rows." + series], dtype=np.uint64)[k]), held)
            assert n > 0 and len(a) == len(b) and len(a) % n == 0
            if dtype is None:                                                # a frame: the header's first word is the call
                dtype = np.dtype([("call", "<u8"), ("rest", "V%d" % (len(a) // n - 8))])
            a, b = (np.frombuffer(x, dtype=dtype).copy() for x in (a, b))
            assert (a["call"] >= b["call"]).all() and (a["call"] > b["call"]).any()   # calls went by while it rested
            a["call"] = b["call"] = 0
            assert a.tobytes() == b.tobytes(), (k, series)
    for k in (1, 3):                                                         # never at rest: the same run, call numbers included
        assert not _differ(_of_item(resumed, k), _of_item(fresh, k)), k


def test_replays_equal_eager_steps_with_the_rules_on(runs):
    eager = _ruled(T1, capture=False)
    for _ in range(FIRST + REST):
        eager.step()
    got = eager.observe()
    eager.close()
    assert not _differ(got, runs["a_rest"])


def test_a_graph_captured_before_the_rules_keeps_the_old_behaviour(runs):
    run = _ruled(T1, rules_before_capture=False)
    run.set_rules(T1)                                                        # after the capture: the captured launches are the old kernels
    run.replay(FIRST + REST)
    got = run.observe()
    assert not _differ(got, runs["r"])
    run.step()                                                               # a launch made now is the new one: system 0 is past 5.0
    assert run.draw.finished().tolist() == [True, False, True, False]
    run.close()


def test_a_run_saved_with_items_at_rest_resumes_in_fresh_objects(runs):
    fresh = _ruled(T1, capture=False)                                        # the same constructors, the rules set again
    fresh.checkpoint.load_state(runs["a_saved"])
    assert not _differ(fresh.observe(), runs["a_rest"])
    assert fresh.draw.finished().tolist() == [True, False, True, False]      # `finished` travels with the draw state
    fresh.capture()
    fresh.replay(MORE)
    got = fresh.observe()
    fresh.close()
    assert not _differ(got, runs["a_more"])
    # a ledger blob taken under the rule is refused by a ledger without one, and the reverse
    plain = StepRun()
    timed_blob = runs["a_saved"]["object.ledger.snapshot"]
    plain_blob = plain.ledger.recorder.snapshot_save(_stream())
    assert len(timed_blob) == len(plain_blob) + 32                           # last_time: 4 doubles
    assert _refused(plain.ledger.recorder.snapshot_load, _stream(), timed_blob)
    plain.ledger.set_time_rule(LEDGER_INTERVAL)
    assert _refused(plain.ledger.recorder.snapshot_load, _stream(), plain_blob)
    plain.ledger.recorder.snapshot_load(_stream(), timed_blob)
    plain.ledger.set_time_rule(0.0)                                          # off again: the third section is gone, the header the old one
    again = plain.ledger.recorder.snapshot_save(_stream())
    assert len(again) == len(plain_blob) and again.tobytes()[:64] == plain_blob.tobytes()[:64]
    # the same for the field recorder: two time words per item behind the five sections
    timed_blob = runs["a_saved"]["object.fields.snapshot"]
    plain_blob = plain.fields.recorder.snapshot_save(_stream())
    assert len(timed_blob) == len(plain_blob) + 64                           # last_time and last_reference_time: 8 doubles
    assert _refused(plain.fields.recorder.snapshot_load, _stream(), timed_blob)
    plain.fields.set_time_rule(plain.draw, FIELD_INTERVAL)
    assert _refused(plain.fields.recorder.snapshot_load, _stream(), plain_blob)
    plain.fields.recorder.snapshot_load(_stream(), timed_blob)
    plain.fields.set_time_rule(None, 0.0)
    again = plain.fields.recorder.snapshot_save(_stream())
    assert len(again) == len(plain_blob) and again.tobytes()[:64] == plain_blob.tobytes()[:64]
    plain.close()


def test_timed_field_rows_in_the_full_step(runs):
    """rows at least the interval apart with their clock in `time`, references by time, lag times from what is stored"""
    obs = runs["a_more"]
    rows = np.frombuffer(obs["rows.fields"], dtype=np.uint64)
    assert rows[0] == np.frombuffer(runs["a_first"]["rows.fields"], dtype=np.uint64)[0]      # at rest: none since
    for k in range(4):
        held = np.frombuffer(obs[f"read.fields.{k}"], dtype=cavitymd.field_recorder._RECORD_DTYPE)
        assert len(held) == min(int(rows[k]), 4) and (np.diff(held["time"]) >= FIELD_INTERVAL).all() and (held["time"] > 0).all(), k
    run = StepRun(field_capacity=16)                                         # six replays write six rows at the most
    run.set_rules(T1)
    run.capture()
    run.replay(6)                                                            # dt >= 0.5 after a first step of 2: a second row by now
    series = run.fields.read()
    lags = run.fields.lag_times(series)
    assert series.shape[1] >= 2 and (series["took_reference"][:, 0] == 1).all() and (lags[:, 0, 0] != lags[:, 0, 0]).all()
    assert _same(lags[:, 1:, 0], series["time"][:, 1:] - series["time"][:, :1])
    with pytest.raises(ValueError, match="not among the rows"):
        run.fields.lag_times(series[:, 1:])
    run.close()


# ---- 3. the ledger's rule on planted clocks ---------------------------------------------------------------------------------------
def _blob_words(blob, B, capacity):
    """(counters (4, B), last_time (B,) or None) of a ledger's snapshot blob"""
    counters = np.frombuffer(blob[64:64 + 32 * B].tobytes(), dtype=np.uint64).reshape(4, B)
    pad = lambda n: (n + 15) // 16 * 16
    at = 64 + pad(32 * B) + pad(B * capacity * 192)
    return counters, (np.frombuffer(blob[at:at + 8 * B].tobytes(), dtype=np.float64) if len(blob) > at else None)


def test_ledger_rows_by_time_equal_the_mirror():
    """B = 5 systems of N = 0, 1, 256, 257, 600; 40 calls, the clocks advanced by unequal steps; every edge planted once on
    system 2: t - last_time equal to the interval and one ulp below, t equal to max_time and one ulp above, a NaN clock.  An
    untimed ledger over the same items records every call: a row written under the rule holds the bytes of its row."""
    CALLS, CAPACITY, INTERVAL, MAX_TIME = 40, 64, 0.75, 24.0
    rng = np.random.default_rng(12)
    sizes = (0, 1, 256, 257, 600)
    systems = [Sys(n, "first" if n else None, "all", 2 if n else 0, rng) for n in sizes]
    B = len(systems)
    ws = _capi.Workspace(1)
    fb = _capi.Batch(ws, [s.force_item() for s in systems])
    res = fb.results_device_ptr()
    clock = torch.zeros(B, dtype=torch.float64, device="cuda")
    reservoir = torch.zeros(B, dtype=torch.float64, device="cuda")
    items = [s.ledger_item(res + 192 * k, (reservoir.data_ptr() + 8 * k,), clock.data_ptr() + 8 * k, 3.0, 1) for k, s in enumerate(systems)]
    timed, plain = _capi.Ledger(ws, items, CAPACITY, 1, KB), _capi.Ledger(ws, items, CAPACITY, 1, KB)
    timed.set_time_rule(INTERVAL, MAX_TIME)
    fb.compute(_stream())
    steps = rng.uniform(0.05, 0.6, (CALLS, B)) * np.array([1.0, 0.5, 1.0, 1.0, 3.0])   # system 4 passes max_time on its way
    times = np.cumsum(steps, axis=0)
    # the edges, on system 2 (rows follow one another there at calls that this schedule fixes): row 0 at call 1 (t = 1.0);
    # call 2 one ulp below the interval, call 3 equal to it; later a NaN; at the end max_time itself; system 3 ends one ulp above
    times[:, 2] = 1.0 + np.cumsum(np.full(CALLS, 0.5))
    times[0, 2] = 1.0
    times[1, 2] = np.nextafter(1.75, 0.0)
    times[2, 2] = 1.75
    times[10, 2] = np.nan
    times[-1, 2] = MAX_TIME                                                  # due (the row before it is 3 or more back), and allowed
    times[-3:, 3] = [21.0, 21.2, np.nextafter(MAX_TIME, np.inf)]             # due by the interval, and one ulp past max_time
    mirrors = [mirror.LedgerItem() for _ in range(B)]
    written = [[] for _ in range(B)]                                         # per system the heads of its rows
    hit = dict.fromkeys(("due", "not_due", "equal", "ulp_below", "nan", "at_max", "past_max"), 0)
    for call in range(CALLS):
        clock.copy_(torch.from_numpy(times[call]))
        reservoir.copy_(torch.from_numpy(rng.normal(size=B)))                # every call's row differs from the last
        timed.record(_stream())
        plain.record(_stream())
        for k in range(B):
            t = times[call, k]
            head = mirrors[k].call(CAPACITY, 1, INTERVAL, MAX_TIME, t)
            if head is not None:
                written[k].append(head)
            hit["due" if head is not None else "not_due"] += 1
            if k == 2:
                hit["ulp_below"] += call == 1 and head is None
                hit["equal"] += call == 2 and head is not None
                hit["nan"] += call == 10 and head is None
                hit["at_max"] += call == CALLS - 1 and head is not None
            if k == 3 and call == CALLS - 1:
                assert t - mirrors[3].last_time >= INTERVAL                  # the interval alone would have written a row
                hit["past_max"] += head is None
        rows = timed.rows(_stream())
        assert rows.tolist() == [len(w) for w in written], call
        counters, last_time = _blob_words(timed.snapshot_save(_stream()), B, CAPACITY)
        assert counters.T.tolist() == [list(m.counters) for m in mirrors], call
        assert _same(last_time, [m.last_time for m in mirrors]), call
        every = plain.read(_stream(), 0, B, 0, call + 1)
        for k in range(B):
            if not written[k]:
                continue
            got = timed.read(_stream(), k, 1, 0, len(written[k]))[0]
            assert got["call"].tolist() == [h["call"] for h in written[k]] and _same(got["time"], [h["time"] for h in written[k]])
            assert got.tobytes() == every[k][[h["call"] - 1 for h in written[k]]].tobytes(), (call, k)
    assert all(n > 0 for n in hit.values()) and hit["equal"] == hit["ulp_below"] == hit["nan"] == hit["at_max"] == hit["past_max"] == 1, hit
    assert written[4][-1]["time"] <= MAX_TIME < times[-6, 4]                 # system 4 stopped writing where it passed max_time
    # the rule off again: every call records, last_time stands; reset zeroes it
    timed.set_time_rule(0.0)
    timed.record(_stream())
    assert timed.rows(_stream()).tolist() == [len(w) + 1 for w in written]
    timed.set_time_rule(INTERVAL)
    counters, last_time = _blob_words(timed.snapshot_save(_stream()), B, CAPACITY)
    assert _same(last_time, [m.last_time for m in mirrors])
    timed.reset(_stream())
    counters, last_time = _blob_words(timed.snapshot_save(_stream()), B, CAPACITY)
    assert not counters.any() and _same(last_time, np.zeros(B))
    for led in (timed, plain):
        led.close()
    fb.close()
    ws.close()


# ---- 3b. the field recorder's rule on planted clocks -------------------------------------------------------------------------------
def _F(ref, cur):
    """include/cavmd.h: (sum over k ascending of (a_r a + b_r b)) / n_k, one rounding per operation, from +0"""
    acc = np.float64(0.0)
    for k in range(len(cur)):
        acc = acc + (np.float64(ref[k].real) * np.float64(cur[k].real) + np.float64(ref[k].imag) * np.float64(cur[k].imag))
    return acc / np.float64(len(cur))


def test_field_rows_and_references_by_time_equal_the_mirror():
    """B = 5 systems of N = 0, 1, 256, 257, 600, n_k = 3, max_references = 3; 40 calls with new positions and unequally advanced
    clocks every call.  Three recorders over the same positions: `plain` (period 1, its stored field of every call is rho of that
    call), `by_time` (rows and references by time) and `by_rows` (rows by time, reference_time_interval 0: a reference every 2
    recorded rows).  After every call the series, the six counters, both time words and the stored references of the two timed
    ones against the mirror; F and rho2 are the header's expression on plain's fields, bit for bit.  At calls 3 to 5 every system is
    asked for a reference: it moves last_reference_time."""
    CALLS, CAPACITY, N_K, REFS, INTERVAL, REF_INTERVAL = 40, 64, 3, 3, 0.75, 4.0
    rng = np.random.default_rng(21)
    sizes = (0, 1, 256, 257, 600)
    B = len(sizes)
    positions = [torch.zeros((n, 4), dtype=torch.float64, device="cuda") for n in sizes]
    kvec = rng.normal(size=(N_K, 3))
    clock = torch.zeros(B, dtype=torch.float64, device="cuda")
    take = torch.zeros(B, dtype=torch.int32, device="cuda")
    ws = _capi.Workspace(1)
    items = [_capi.field_item(p.data_ptr() if n else 0, 32, n) for p, n in zip(positions, sizes)]
    plain = _capi.FieldRecorder(ws, items, kvec, CAPACITY, 1, 1, 0)
    by_time = _capi.FieldRecorder(ws, items, kvec, CAPACITY, 1, REFS, 0)
    by_rows = _capi.FieldRecorder(ws, items, kvec, CAPACITY, 1, REFS, 2)
    by_time.set_time_rule(clock.data_ptr(), 8, INTERVAL, REF_INTERVAL)
    by_rows.set_time_rule(clock.data_ptr(), 8, INTERVAL, 0.0)
    rules = {"by_time": (by_time, 0, REF_INTERVAL), "by_rows": (by_rows, 2, 0.0)}
    times = np.cumsum(rng.uniform(0.05, 0.6, (CALLS, B)) * np.array([1.0, 0.5, 1.0, 2.0, 3.0]), axis=0)
    times[:, 2] = 1.0 + 0.5 * np.arange(CALLS)                               # system 2: the edges, as in the ledger's test
    times[1, 2], times[2, 2], times[10, 2] = np.nextafter(1.75, 0.0), 1.75, np.nan
    mirrors = {name: [mirror.FieldItem() for _ in range(B)] for name in rules}
    written = {name: [[] for _ in range(B)] for name in rules}               # per system (head, rho of the call)
    ref_fields = {name: [[] for _ in range(B)] for name in rules}
    hit = dict.fromkeys(("row", "no_row", "ref_by_time", "ref_by_rows", "ref_forced", "full", "ulp_below", "equal", "nan"), 0)
    dtype = cavitymd.field_recorder._RECORD_DTYPE
    for call in range(CALLS):
        for p, n in zip(positions, sizes):
            p.copy_(torch.from_numpy(np.concatenate([rng.uniform(-20.0, 20.0, (n, 3)), np.full((n, 1), np.nan)], axis=1)))
        clock.copy_(torch.from_numpy(times[call]))
        take.fill_(1 if call in (2, 3, 4) else 0)
        for rec in (plain, by_time, by_rows):
            rec.record(_stream(), take.data_ptr())
        rho = [plain.read_fields(_stream(), k)[0] for k in range(B)]
        for name, (rec, interval, ref_interval) in rules.items():
            for k in range(B):
                m = mirrors[name][k]
                head = m.call(CAPACITY, 1, interval, REFS, INTERVAL, ref_interval, times[call, k], call in (2, 3, 4))
                hit["row" if head else "no_row"] += 1
                if k == 2 and name == "by_time":
                    hit["ulp_below"] += call == 1 and head is None
                    hit["equal"] += call == 2 and head is not None
                    hit["nan"] += call == 10 and head is None
                if head is None:
                    continue
                head["F"] = [_F(f, rho[k]) for f in ref_fields[name][k]]
                head["rho2"], head["rho"] = _F(rho[k], rho[k]), rho[k].copy()
                if head["took_reference"]:
                    ref_fields[name][k].append(rho[k].copy())
                    hit["ref_forced" if call in (2, 3, 4) else "ref_by_time" if name == "by_time" else "ref_by_rows"] += head["row"] > 0
                hit["full"] += head["n_references"] == REFS
                written[name][k].append(head)
            blob = rec.snapshot_save(_stream())
            counters = np.frombuffer(blob[64:64 + 48 * B].tobytes(), dtype=np.uint64).reshape(6, B)
            words = np.frombuffer(blob[-16 * B:].tobytes(), dtype=np.float64).reshape(2, B)
            assert counters.T.tolist() == [list(m.counters) for m in mirrors[name]], (name, call)
            assert _same(words[0], [m.last_time for m in mirrors[name]]) and _same(words[1], [m.last_reference_time for m in mirrors[name]])
            for k in range(B):
                heads = written[name][k]
                got = rec.read(_stream(), k, 1, 0, len(heads))[0].view(dtype)
                assert got["call"].tolist() == [h["call"] for h in heads] and _same(got["time"], [h["time"] for h in heads])
                assert got["n_references"].tolist() == [h["n_references"] for h in heads]
                assert got["took_reference"].tolist() == [int(h["took_reference"]) for h in heads]
                assert _same(got["rho2"], [h["rho2"] for h in heads])
                assert _same(got["F"], [h["F"] + [0.0] * (16 - len(h["F"])) for h in heads]), (name, call, k)
                now, refs, ref_rows = rec.read_fields(_stream(), k)
                assert ref_rows.tolist() == mirrors[name][k].ref_rows and _same(refs.view(np.float64), np.array(ref_fields[name][k]).view(np.float64).reshape(len(ref_rows), -1))
                assert _same(now.view(np.float64), heads[-1]["rho"].view(np.float64))     # the field of the last RECORDED call
    assert all(n > 0 for n in hit.values()) and hit["ulp_below"] == hit["equal"] == hit["nan"] == 1, hit
    # an untimed recorder's `time` stays +0; reset zeroes both time words
    assert _same(plain.read(_stream(), 0, B, 0, CALLS).view(dtype)["time"], np.zeros((B, CALLS)))
    by_time.reset(_stream())
    blob = by_time.snapshot_save(_stream())
    assert not np.frombuffer(blob[64:64 + 48 * B].tobytes(), dtype=np.uint64).any() and not np.frombuffer(blob[-16 * B:].tobytes(), dtype=np.uint64).any()
    # the refusals that need a live object
    for args in ((0, 8, 1.0, 0.0), (clock.data_ptr() + 4, 8, 1.0, 0.0), (clock.data_ptr(), 4, 1.0, 0.0), (clock.data_ptr(), 12, 1.0, 0.0),
                 (clock.data_ptr(), 8, -1.0, 0.0), (clock.data_ptr(), 8, float("nan"), 0.0), (clock.data_ptr(), 8, 1.0, float("inf")),
                 (clock.data_ptr(), 8, 1.0, -1.0), (clock.data_ptr(), 8, 0.0, 1.0)):
        assert _refused(by_time.set_time_rule, *args), args
    period2 = _capi.FieldRecorder(ws, items, kvec, CAPACITY, 2, REFS, 0)
    assert _refused(period2.set_time_rule, clock.data_ptr(), 8, 1.0, 0.0)    # created with period != 1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        by_time.record(_stream(), 0)
        assert _refused(by_time.set_time_rule, clock.data_ptr(), 8, 1.0, 0.0)
    torch.cuda.synchronize()
    del graph
    for rec in (period2, by_rows, by_time, plain):
        rec.close()
    ws.close()


# ---- 4. refusals that need a live object ------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    B = 3
    t, ws, draw = _draw_only(B, 5, None)
    lib = ws._lib
    for bad in (-1.0, float("nan"), float("inf"), -1e-300):
        assert _refused(draw.set_end, 1, [2.0, bad])
    assert _refused(draw.set_end, B, [1.0]) and _refused(draw.set_end, 1, [1.0] * B) and _refused(draw.set_end, 0, [])
    assert lib.cavmd_runclock_draw_set_end(draw.handle, 0, 1, None) == INV
    assert lib.cavmd_runclock_draw_finished(draw.handle, None, None) == INV
    draw.fill(_stream())
    assert draw.finished(_stream()) == 0                                     # nothing above took effect: the old kernel ran
    draw.set_end(1, [1e-9])
    draw.set_end(0, [-0.0])                                                  # -0 is none
    draw.fill(_stream())
    draw.fill(_stream())
    assert draw.read(_stream())["reserved"][:, 0].tolist() == [0, 1, 0]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        draw.fill(_stream())
        assert _refused(draw.set_end, 0, [1.0])                              # the object's last stream is being captured
        assert _refused(draw.finished, _stream())
    torch.cuda.synchronize()
    draw.set_end(0, [1.0])
    del graph
    draw.close()
    # the ledger
    rng = np.random.default_rng(3)
    s = Sys(20, "first", "all", 1, rng)
    fb = _capi.Batch(ws, [s.force_item()])
    clock = torch.zeros(1, dtype=torch.float64, device="cuda")
    with_clock = s.ledger_item(fb.results_device_ptr(), (), clock.data_ptr(), 3.0, 1)
    without = s.ledger_item(fb.results_device_ptr(), (), 0, 3.0, 1)
    led = _capi.Ledger(ws, [with_clock], 4, 1, KB)
    for interval, max_time in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, -1.0), (1.0, float("nan")),
                               (1.0, float("inf")), (0.0, 5.0)):
        assert _refused(led.set_time_rule, interval, max_time)
    led.set_time_rule(1.0, 5.0)
    assert _refused(led.set_items, 0, [without])                             # under the rule an item needs its clock
    led.set_items(0, [with_clock])
    led.set_time_rule(0.0)
    led.set_items(0, [without])
    assert _refused(led.set_time_rule, 1.0, 0.0)                             # an item without d_time
    period2 = _capi.Ledger(ws, [with_clock], 4, 2, KB)
    assert _refused(period2.set_time_rule, 1.0, 0.0)                         # created with period != 1
    period2.set_time_rule(0.0)
    led.set_items(0, [with_clock])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        led.record(_stream())
        assert _refused(led.set_time_rule, 1.0, 0.0)
    torch.cuda.synchronize()
    led.set_time_rule(1.0, 0.0)
    del graph
    for obj in (period2, led, fb):
        obj.close()
    ws.close()


# ---- 5. run_until_finished ----------------------------------------------------------------------------------------------------------
def test_run_until_finished_on_the_device():
    """fixed dt per system, so the call that puts each to rest is known: ceil(t_end / dt) steps, then the fill that finds it"""
    B, T_END = 5, 10.0
    dts = [0.5, 1.0, 3.0, 0.25, 2.0]
    integrator = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    draw = cavitymd.StepDraw(3, integrator=integrator, dt=dts)
    draw.set_end_time(T_END)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        draw.fill()
    last = int(np.ceil(T_END / min(dts))) + 1                                # 41: the fill that finds the slowest clock at 10.0
    assert cavitymd.run_until_finished(graph.replay, draw, check_every=16) == 48 >= last
    state = draw.state()
    assert state["draws"].tolist() == [20, 10, 4, 40, 5] and state["finished"].all() and (state["elapsed"] >= T_END).all()
    assert state["elapsed"].tolist() == [10.0, 10.0, 12.0, 10.0, 10.0]       # no clamping of the last step
    assert cavitymd.run_until_finished(graph.replay, draw) == 0              # all at rest: not one replay more
    draw.set_end_time([20.0, 10.0, 12.0, None, 0])                           # systems 3 and 4: no end any more
    assert cavitymd.run_until_finished(graph.replay, draw, check_every=7, max_replays=30) == 30
    state = draw.state()
    assert state["finished"].tolist() == [1, 1, 1, 0, 0] and state["draws"].tolist() == [40, 10, 4, 70, 35]
    draw.set_end_time(T_END)
    draw.reset()
    assert cavitymd.run_until_finished(graph.replay, draw, check_every=41) == 41 == last
    assert cavitymd.run_until_finished(graph.replay, draw, check_every=5, max_replays=3) == 0
    del graph
    draw.close()


# ---- 6. the example -------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_to_its_end_time():
    example = os.path.join(ROOT, "examples", "run_clock", "batch_run_to_end_time.py")
    done = subprocess.run([sys.executable, example, "2", "60", "10"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "B=2: t_end 60.0" in done.stdout and "replica 1:" in done.stdout and "energy rows per replica" in done.stdout, done.stdout
    assert "F(k,t) rows per replica" in done.stdout, done.stdout
