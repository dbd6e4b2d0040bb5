"""cavmd_trajectory / BatchTrajectoryRecorder on the device: frames of a batch written by ONE kernel per call, against the numpy
restatement of the contract (tests/trajectory_mirror.py), bit for bit -- the whole ring and the five counter words are compared,
so a byte written outside the target slot, or inside it where the contract writes nothing, fails the comparison."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
import trajectory_mirror as mirror
from cavitymd import _capi, synthetic
from abi_support import ROOT
from gpu_support import stream as _stream

pytestmark = pytest.mark.gpu

INV, CAP = _capi.CAVMD_ERR_INVALID_VALUE, _capi.CAVMD_ERR_CAPACITY
FILL = 0xAB                                     # what the ring holds before a test's first call
TAG_BITS, MASS_BITS = 0x4142434445464748, 0x4152535455565758      # pos.w and vel.w of every particle: never copied
HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=8.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=8.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=8.0)}


def _expect_status(status, call, *args):
    with pytest.raises(_capi.CavmdError) as e:
        call(*args)
    assert e.value.status == status, (call, args, e.value.status)


def _f64(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


class Sys:
    """one system: host arrays and their device copies"""

    def __init__(self, n, rng, k=0, with_vel=True):
        self.N = n
        self.box = (8.0 + k, 10.0, 12.5)
        self.pos = np.empty((n, 4))
        self.pos[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * np.array(self.box)
        self.pos[:, 3] = _f64(TAG_BITS)
        self.vel = np.empty((n, 4))
        self.vel[:, :3] = rng.normal(0.0, 1e-3, (n, 3))
        self.vel[:, 3] = _f64(MASS_BITS)
        self.image = rng.integers(-5, 6, (n, 3)).astype(np.int32)
        self.with_vel = with_vel

    def upload(self):
        self.d_pos, self.d_vel = torch.from_numpy(self.pos).cuda(), torch.from_numpy(self.vel).cuda()
        self.d_image = torch.from_numpy(self.image).cuda()
        return self

    def item(self, time_ptr=0):
        n = self.N
        return _capi.trajectory_item(self.d_pos.data_ptr() if n else 0, self.d_image.data_ptr() if n else 0,
                                     self.d_vel.data_ptr() if (n and self.with_vel) else 0, time_ptr, self.box, n)

    def frame(self, lay, old, head):
        return mirror.frame_bytes(lay, old, head, self.box, self.pos, self.vel if (self.with_vel and self.N) else None, self.image)


def _device_view(ptr, shape, typestr):
    class View:
        __cuda_array_interface__ = {"data": (ptr, False), "shape": shape, "typestr": typestr, "strides": None, "version": 2}
    return torch.as_tensor(View(), device="cuda")


class Ring:
    """the object's ring and counters, viewed where they live (cavmd_trajectory_device_ptr), and their mirror on the host"""

    def __init__(self, traj, B, fill=FILL):
        self.B, self.capacity, self.lay = B, traj.capacity, mirror.layout(traj.max_N, traj.format)
        series, rows = traj.device_ptr()
        self.series = _device_view(series, (B, traj.capacity, self.lay["frame_bytes"]), "|u1")
        self.counters = _device_view(rows, (5, B), "<i8")
        torch.cuda.synchronize()
        assert not self.series.any() and not self.counters.any()                # zero at creation
        self.series.fill_(fill)
        torch.cuda.synchronize()
        self.want = np.full((B, traj.capacity, self.lay["frame_bytes"]), fill, dtype=np.uint8)
        self.items = [mirror.Item() for _ in range(B)]
        self.heads = [[] for _ in range(B)]

    def call(self, systems, period, interval, times=None, forced=None):
        """the mirror's call; returns the items that recorded"""
        recorded = []
        for k, s in enumerate(systems):
            head = self.items[k].call(self.capacity, period, interval, None if times is None else times[k],
                                      bool(forced[k]) if forced is not None else False)
            if head is not None:
                self.want[k, head["slot"]] = s.frame(self.lay, self.want[k, head["slot"]], head)
                self.heads[k].append(head)
                recorded.append(k)
        return recorded

    def got(self):
        torch.cuda.synchronize()
        return self.series.cpu().numpy()

    def assert_equal(self, where):
        got = self.got()
        if got.tobytes() != self.want.tobytes():
            bad = np.argwhere(got != self.want)
            raise AssertionError((where, "first differing (item, slot, byte)", bad[0].tolist(), "of", len(bad)))
        c = self.counters.cpu().numpy()
        want = np.array([[it.rows for it in self.items], [it.calls for it in self.items], [it.phase for it in self.items],
                         [it.slot for it in self.items],
                         [int(np.float64(it.last_time).view(np.uint64)) for it in self.items]], dtype=np.uint64)
        assert c.tobytes() == want.tobytes(), (where, c, want)


# ---- 1. one ragged batch, both formats ---------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 501, 511, 512, 513, 1023, 1024, 1025, 2049, 4097)
MAX_N = 4097
NO_VEL = SIZES.index(7)
BIG, MID = SIZES.index(4097), SIZES.index(513)
EDGES = (float("nan"), float("inf"), float("-inf"), -0.0, 1e-40, 2.0 ** -150, 1e39)


def _ragged(rng):
    systems = [Sys(n, rng, k, with_vel=(k != NO_VEL)) for k, n in enumerate(SIZES)]
    for j, value in enumerate(EDGES):                                          # each edge once in a position, once in a velocity
        systems[BIG].pos[10 + 37 * j, j % 3] = value
        systems[MID].vel[3 + 71 * j, (j + 1) % 3] = value
    systems[BIG].image[5] = (-2 ** 31, 2 ** 31 - 1, 0)
    systems[MID].image[512] = (2 ** 31 - 1, 0, -2 ** 31)
    return [s.upload() for s in systems]


@pytest.mark.parametrize("fmt", (_capi.TRAJECTORY_F64, _capi.TRAJECTORY_F32), ids=("f64", "f32"))
def test_one_ragged_batch_equals_the_mirror_bit_for_bit(fmt):
    rng = np.random.default_rng(20261020)
    systems = _ragged(rng)
    B = len(systems)
    ws = _capi.Workspace(1)
    traj = _capi.Trajectory(ws, [s.item() for s in systems], MAX_N, fmt, 2, 1, 0.0)
    assert traj.launch_order == sorted(range(B), key=lambda i: -SIZES[i]) != list(range(B))
    lay = traj.layout
    assert {name: int(getattr(lay, name)) for name, _ in _capi.TrajectoryLayout._fields_} == mirror.layout(MAX_N, fmt)
    ring = Ring(traj, B)
    for call in range(2):                                                       # slot 0, then slot 1
        traj.record(_stream())
        assert ring.call(systems, 1, 0.0) == list(range(B))
        ring.assert_equal(("call", call + 1))
    assert list(traj.rows(_stream())) == [2] * B
    frames = traj.read(_stream(), 0, B, 0, 2)
    assert frames.tobytes() == ring.want.tobytes()
    e = np.float64 if fmt == _capi.TRAJECTORY_F64 else np.float32
    for k, s in enumerate(systems):
        f = frames[k, 1]
        assert (int(f["call"]), int(f["row"]), float(f["time"]), int(f["N"]), int(f["reserved"])) == (2, 1, 0.0, s.N, 0)
        assert int(f["flags"]) == (0 if (k == NO_VEL or s.N == 0) else _capi.TRAJECTORY_HAS_VELOCITIES)
        assert tuple(f["box"]) == s.box
        with np.errstate(over="ignore", under="ignore"):
            assert f["position"][:s.N].tobytes() == s.pos[:, :3].astype(e).tobytes()
            want_v = s.vel[:, :3] if (k != NO_VEL) else np.zeros((s.N, 3))
            assert f["velocity"][:s.N].tobytes() == want_v.astype(e).tobytes()
        assert f["image"][:s.N].tobytes() == s.image.tobytes()
    # the planted values, counted in what the device wrote
    for section, k in (("position", BIG), ("velocity", MID)):
        x = frames[k, 0][section][:SIZES[k]]
        if fmt == _capi.TRAJECTORY_F64:
            counts = (np.isnan(x).sum(), (x == np.inf).sum(), (x == -np.inf).sum(), ((x == 0) & np.signbit(x)).sum(),
                      (x == 1e-40).sum(), (x == 2.0 ** -150).sum(), (x == 1e39).sum())
            assert counts == (1, 1, 1, 1, 1, 1, 1), (section, counts)
        else:
            tiny = np.float32(1e-40)
            assert 0 < tiny < np.finfo(np.float32).tiny and int(tiny.view(np.uint32)) == 71362        # a subnormal, kept
            counts = (np.isnan(x).sum(), (x == np.inf).sum(), (x == -np.inf).sum(), ((x == 0) & np.signbit(x)).sum(),
                      (x == tiny).sum(), ((x == 0) & ~np.signbit(x)).sum())
            assert counts == (1, 2, 1, 1, 1, 1), (section, counts)              # 1e39 -> +inf; 2^-150 -> +0 (a tie, to even)
    assert frames[BIG, 0]["image"][5].tolist() == [-2 ** 31, 2 ** 31 - 1, 0]
    assert frames[MID, 0]["image"][512].tolist() == [2 ** 31 - 1, 0, -2 ** 31]
    # pos.w and vel.w appear nowhere: not as they are, not converted
    blob = ring.got().reshape(-1)
    assert blob.size % 8 == 0
    for bits in (TAG_BITS, MASS_BITS):
        assert not (blob.view("<u8") == np.uint64(bits)).any()
        assert np.isfinite(np.float32(_f64(bits))) and not (blob.view("<u4") == np.float32(_f64(bits)).view(np.uint32)).any()
    traj.close()
    ws.close()


# ---- 2. the call rule ------------------------------------------------------------------------------------------------------------
def test_step_rule_with_take_words_over_40_calls():
    rng = np.random.default_rng(7)
    systems = [Sys(n, rng, k).upload() for k, n in enumerate((5, 0, 300))]
    B, CALLS = 3, 40
    ws = _capi.Workspace(1)
    traj = _capi.Trajectory(ws, [s.item() for s in systems], 300, _capi.TRAJECTORY_F32, 64, 3, 0.0)
    ring = Ring(traj, B)
    take = torch.zeros(B, dtype=torch.int32, device="cuda")
    schedule = np.zeros((CALLS, B), dtype=np.int32)
    schedule[3, 0] = schedule[4, 0] = 1            # right after a due call, and again
    schedule[8, 1] = 7                             # on a due call (call 9): forced and due; any non-zero word counts
    schedule[20:23, 2] = 1
    schedule[39, :] = 1
    for c in range(CALLS):
        take.copy_(torch.from_numpy(schedule[c]))
        traj.record(_stream(), 0 if (c % 5 == 0 and not schedule[c].any()) else take.data_ptr())     # NULL: nobody is forced
        ring.call(systems, 3, 0.0, forced=schedule[c])
        assert list(traj.rows(_stream())) == [it.rows for it in ring.items], c
    assert take.cpu().numpy().tolist() == schedule[-1].tolist()                  # the word is only read
    ring.assert_equal("step rule")
    rows = [it.rows for it in ring.items]
    assert rows[0] > 13 and all(it.calls == CALLS for it in ring.items)
    for k in range(B):
        f = traj.read(_stream(), k, 1, 0, rows[k])[0]
        assert [(int(x["call"]), int(x["row"]), int(x["flags"]) & 1) for x in f] == \
            [(h["call"], h["row"], int(h["forced"])) for h in ring.heads[k]], k
    assert [h["call"] for h in ring.heads[0]][:5] == [3, 4, 5, 8, 11]
    traj.close()
    ws.close()


def test_time_rule_over_40_calls():
    rng = np.random.default_rng(8)
    systems = [Sys(n, rng, k).upload() for k, n in enumerate((65, 0, 257, 3))]
    B, CALLS, T = 4, 40, 0.25
    times = np.zeros((CALLS, B))
    times[:, 0] = 0.5 + 0.125 * np.arange(CALLS)                                 # exact: due on every second call, by equality
    t1, last = [0.5], 0.5
    for c in range(1, CALLS):                                                    # one ulp below the interval, then exactly on it
        if c % 2:
            t1.append(math.nextafter(last + T, 0.0))
        else:
            last += T
            t1.append(last)
    times[:, 1] = t1
    times[:, 2] = np.cumsum(rng.uniform(0.0, 0.2, CALLS))
    times[10:13, 2] = np.nan                                                     # a NaN time is never due
    times[:, 3] = 1e3 + np.cumsum(rng.uniform(0.0, 0.3, CALLS))
    forced = np.zeros((CALLS, B), dtype=np.int32)
    forced[11, 2] = 1                                                            # forced at a NaN time: last_time becomes NaN ...
    forced[20, 2] = 1                                                            # ... and nothing is due until the next forced frame
    forced[5, 0] = 1                                                             # a forced frame moves last_time
    clock = torch.zeros(B, dtype=torch.float64, device="cuda")
    take = torch.zeros(B, dtype=torch.int32, device="cuda")
    ws = _capi.Workspace(1)
    traj = _capi.Trajectory(ws, [s.item(clock.data_ptr() + 8 * k) for k, s in enumerate(systems)], 257, _capi.TRAJECTORY_F64, 64, 1, T)
    ring = Ring(traj, B)
    for c in range(CALLS):
        clock.copy_(torch.from_numpy(times[c]))
        take.copy_(torch.from_numpy(forced[c]))
        traj.record(_stream(), take.data_ptr())
        ring.call(systems, 1, T, times=times[c], forced=forced[c])
        assert list(traj.rows(_stream())) == [it.rows for it in ring.items], c
    ring.assert_equal("time rule")
    calls = [[h["call"] for h in heads] for heads in ring.heads]
    assert calls[0][:6] == [1, 3, 5, 6, 8, 10]                                   # equality is due; the forced frame shifts the rest
    assert calls[1] == [1] + list(range(3, CALLS + 1, 2))                        # one ulp below is not
    assert 12 in calls[2] and 21 in calls[2] and not any(12 < c < 21 for c in calls[2])
    for k in range(B):
        f = traj.read(_stream(), k, 1, 0, ring.items[k].rows)[0]
        assert [(int(x["call"]), int(x["row"]), int(x["flags"]) & 1) for x in f] == \
            [(h["call"], h["row"], int(h["forced"])) for h in ring.heads[k]], k
        assert f["time"].tobytes() == np.array([h["time"] for h in ring.heads[k]]).tobytes()
    # reset zeroes the five counters: the next call records at once
    traj.reset(_stream())
    for it in ring.items:
        it.reset()
    clock.copy_(torch.from_numpy(times[0]))
    take.zero_()
    traj.record(_stream(), take.data_ptr())
    assert ring.call(systems, 1, T, times=times[0]) == list(range(B))
    ring.assert_equal("after reset")
    traj.close()
    ws.close()


def test_ring_of_four_keeps_the_last_four_of_eleven():
    rng = np.random.default_rng(9)
    systems = [Sys(n, rng, k).upload() for k, n in enumerate((40, 7))]
    ws = _capi.Workspace(1)
    traj = _capi.Trajectory(ws, [s.item() for s in systems], 40, _capi.TRAJECTORY_F32, 4, 1, 0.0)
    ring = Ring(traj, 2)
    _expect_status(_capi.CAVMD_ERR_NOT_COMPUTED, traj.read, _stream(), 0, 2, 0, 1)
    for c in range(11):
        systems[0].d_pos[:, 0].add_(1.0)                                         # every frame differs
        systems[0].pos[:, 0] += 1.0
        traj.record(_stream())
        ring.call(systems, 1, 0.0)
    ring.assert_equal("ring")
    assert list(traj.rows(_stream())) == [11, 11]
    for first in range(7):
        _expect_status(_capi.CAVMD_ERR_EXPIRED, traj.read, _stream(), 0, 2, first, 1)
    _expect_status(INV, traj.read, _stream(), 0, 2, 11, 1)
    _expect_status(INV, traj.read, _stream(), 0, 2, 8, 4)
    last = traj.read(_stream(), 0, 2, 7, 4)                                      # slots 3, 0, 1, 2: two runs of the ring
    assert last["call"].tolist() == [[8, 9, 10, 11]] * 2 and last["row"].tolist() == [[7, 8, 9, 10]] * 2
    assert last.tobytes() == ring.want[:, [3, 0, 1, 2]].tobytes()
    traj.close()
    ws.close()


# ---- 3. own slot only -------------------------------------------------------------------------------------------------------------
def test_a_call_writes_its_own_slots_and_nothing_else():
    rng = np.random.default_rng(10)
    systems = [Sys(n, rng, k).upload() for k, n in enumerate((501, 33, 0, 256))]
    B = 4
    ws = _capi.Workspace(1)
    traj = _capi.Trajectory(ws, [s.item() for s in systems], 501, _capi.TRAJECTORY_F32, 3, 2, 0.0)
    ring = Ring(traj, B)
    before = ring.got()
    traj.record(_stream())                                                       # call 1 of period 2: nobody records
    assert ring.call(systems, 2, 0.0) == []
    assert ring.got().tobytes() == before.tobytes()                              # no series byte changed
    ring.assert_equal("a call that does not record")
    take = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device="cuda")
    traj.reset(_stream())
    for it in ring.items:
        it.reset()
    traj.record(_stream(), take.data_ptr())                                      # call 1 again, item 1 forced
    assert ring.call(systems, 2, 0.0, forced=[0, 1, 0, 0]) == [1]
    after = ring.got()
    changed = np.argwhere(after != before)
    assert len(changed) and set(map(tuple, changed[:, :2])) == {(1, 0)}          # item 1, slot 0 and nothing else
    ring.assert_equal("one forced item")
    before = after
    traj.record(_stream())                                                       # call 2: items 0, 2, 3 are due; item 1's phase restarted
    assert ring.call(systems, 2, 0.0) == [0, 2, 3]
    after = ring.got()
    assert set(map(tuple, np.argwhere(after != before)[:, :2])) == {(0, 0), (2, 0), (3, 0)}
    ring.assert_equal("three due items")
    # inside a target slot: behind a section's padded end the bytes stay what they were
    lay = ring.lay
    end = lay["position_offset"] + mirror.pad16(3 * 33 * 4)
    assert (after[1, 0, end:lay["velocity_offset"]] == FILL).all() and (after[2, 0, 64:] == FILL).all()
    traj.close()
    ws.close()


# ---- 4. replay ---------------------------------------------------------------------------------------------------------------------
def _system_of(cfg):
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"], cfg["box"],
                                           device="cuda")
    return cavitymd.SystemDefinition(pd)


def _empty_like(cfg):
    return dict(cfg, position=np.zeros((0, 3)), typeid=np.zeros(0, dtype=np.int32), charge=np.zeros(0),
                image=np.zeros((0, 3), dtype=np.int32))


def _velocities(cfg, rng, kT=3.167e-4):
    n = len(cfg["typeid"])
    mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
    v = rng.normal(size=(n, 3)) * np.sqrt(kT / mass)[:, None]
    return torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda()


def _clocked_run(captured: bool, steps: int):
    """Systems of N = 65, 501 and 0 under {draw, step one, cavity, step two, record} with a StepDraw clock: dt 0.5, 0.25 and
    0.5 against a time interval of 0.5, so system 0 records on every call and system 1 on every second one."""
    rng = np.random.default_rng(12)
    cfgs = [synthetic.diatomic_box(64, 1, box_length=30.0), synthetic.config1(seed=2)]
    cfgs.append(_empty_like(cfgs[0]))
    sysdefs = [_system_of(c) for c in cfgs]
    velocities = [_velocities(c, rng) for c in cfgs]
    cavity = cavitymd.CavityForceBatch(sysdefs, cfgs[0]["params"])
    integrator = cavitymd.VerletBatch(cavity, velocities)
    draw = cavitymd.StepDraw(0x1234, integrator, dt=[0.5, 0.25, 0.5])
    trajectory = cavitymd.BatchTrajectoryRecorder(cavity, velocities, capacity=32, time_interval=0.5, clock=draw, dtype="f64")
    cavity.compute()
    integrator.prime()

    def step():
        draw.fill()
        integrator.step_one()
        cavity.compute()
        integrator.step_two()
        trajectory.record()

    torch.cuda.synchronize()
    if captured:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        assert list(trajectory.rows()) == [0, 0, 0]                               # a capture runs nothing
        for r in range(steps):
            graph.replay()
            if r == steps // 2:                                                   # a read between replays disturbs nothing
                assert int(trajectory.rows()[0]) == r + 1
    else:
        for _ in range(steps):
            step()
    rows = trajectory.rows()
    frames = [trajectory.trajectory.read(0, k, 1, 0, int(rows[k]))[0] for k in range(3)]
    elapsed = draw.state()["elapsed"].copy()
    trajectory.close()
    draw.close()
    integrator.close()
    cavity.close()
    return rows, frames, elapsed


def test_a_replayed_graph_records_the_frames_of_the_eager_steps():
    STEPS = 30
    rows_e, eager, t_e = _clocked_run(False, STEPS)
    rows_g, replayed, t_g = _clocked_run(True, STEPS)
    assert list(rows_e) == list(rows_g) == [30, 15, 30] and t_e.tobytes() == t_g.tobytes()
    for k in range(3):
        assert replayed[k].tobytes() == eager[k].tobytes(), k
    assert replayed[0]["call"].tolist() == list(range(1, 31)) == replayed[2]["call"].tolist()
    assert replayed[1]["call"].tolist() == list(range(1, 31, 2))
    assert replayed[0]["time"].tolist() == [0.5 * c for c in range(1, 31)]
    assert replayed[1]["time"].tolist() == [0.25 * c for c in range(1, 31, 2)]
    assert replayed[0]["N"].tolist() == [65] * 30 and replayed[2]["N"].tolist() == [0] * 30
    assert (replayed[0]["flags"] == _capi.TRAJECTORY_HAS_VELOCITIES).all() and (replayed[2]["flags"] == 0).all()
    for k in (0, 1):                                                              # the systems move: every frame differs
        n = int(replayed[k]["N"][0])
        assert len({f["position"][:n].tobytes() for f in replayed[k]}) == len(replayed[k])
        assert len({f["velocity"][:n].tobytes() for f in replayed[k]}) == len(replayed[k])


# ---- 5. set_items -------------------------------------------------------------------------------------------------------------------
def test_set_items_swaps_arrays_refuses_a_larger_system_and_a_capture():
    rng = np.random.default_rng(13)
    systems = [Sys(300, rng, 0).upload(), Sys(40, rng, 1).upload()]
    smaller, larger = Sys(20, rng, 2).upload(), Sys(301, rng, 3).upload()
    ws = _capi.Workspace(1)
    traj = _capi.Trajectory(ws, [s.item() for s in systems], 300, _capi.TRAJECTORY_F64, 4, 1, 0.0)
    ring = Ring(traj, 2)
    traj.record(_stream())
    ring.call(systems, 1, 0.0)
    ring.assert_equal("before")
    _expect_status(CAP, traj.set_items, 1, [larger.item()])                       # N > max_N
    _expect_status(CAP, traj.set_items, 0, [smaller.item(), larger.item()])       # refused at its second item: nothing changed
    _expect_status(INV, traj.set_items, 2, [smaller.item()])
    assert traj.sizes == [300, 40]
    traj.record(_stream())
    ring.call(systems, 1, 0.0)
    ring.assert_equal("after the refusals")
    traj.set_items(1, [smaller.item()])                                           # other arrays, a smaller N: counters and ring kept
    systems[1] = smaller
    assert traj.sizes == [300, 20] and list(traj.rows(_stream())) == [2, 2]
    ring.assert_equal("after set_items")
    traj.record(_stream())
    ring.call(systems, 1, 0.0)
    ring.assert_equal("the swapped item")
    f = traj.read(_stream(), 1, 1, 0, 3)[0]
    assert f["N"].tolist() == [40, 40, 20] and f["call"].tolist() == [1, 2, 3] and tuple(f["box"][2]) == smaller.box
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        traj.record(_stream())
        _expect_status(INV, traj.set_items, 1, [systems[1].item()])               # refused during a capture
        _expect_status(INV, traj.rows, _stream())
    graph.replay()
    ring.call(systems, 1, 0.0)
    ring.assert_equal("a replay after the refusal")
    # a time rule refuses an item without a clock, at creation and in set_items
    clock = torch.zeros(2, dtype=torch.float64, device="cuda")
    _expect_status(INV, _capi.Trajectory, ws, [s.item() for s in systems], 300, _capi.TRAJECTORY_F64, 4, 1, 0.5)
    timed = _capi.Trajectory(ws, [s.item(clock.data_ptr() + 8 * k) for k, s in enumerate(systems)], 300, _capi.TRAJECTORY_F64, 4, 1, 0.5)
    _expect_status(INV, timed.set_items, 0, [systems[0].item()])
    timed.close()
    traj.close()
    ws.close()


# ---- 6. restore ---------------------------------------------------------------------------------------------------------------------
def test_restore_puts_a_frame_back_and_the_run_repeats_bit_for_bit():
    rng = np.random.default_rng(14)
    cfgs = [synthetic.diatomic_box(64, 3, box_length=30.0), synthetic.diatomic_lattice(4, 8.0, seed=4)]      # N = 65 and 129
    sysdefs = [_system_of(c) for c in cfgs]
    assert [s.getParticleData().getN() for s in sysdefs] == [65, 129]
    velocities = [_velocities(c, rng) for c in cfgs]
    bonds, bond_typeid = zip(*[synthetic.diatomic_bonds(c) for c in cfgs])
    cavity = cavitymd.CavityForceBatch(sysdefs, cfgs[0]["params"])
    molecular = cavitymd.MolecularForceBatch(sysdefs, list(bonds), list(bond_typeid), harmonic=HARMONIC, lj=LJ)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m] for m in molecular.forces])
    trajectory = cavitymd.BatchTrajectoryRecorder(cavity, velocities, capacity=4, period=1000, dtype="f64")
    lossy = cavitymd.BatchTrajectoryRecorder(cavity, velocities, capacity=4, dtype="f32")
    integrator.set_inputs(2.0)                                                    # NVE: a fixed dt, no bath

    def forces():
        cavity.compute()
        molecular.compute()

    def run(steps):
        for _ in range(steps):
            integrator.step_one()
            forces()
            integrator.step_two()

    def state():
        torch.cuda.synchronize()
        return [(s.getParticleData().getPositions().cpu().numpy().tobytes(), s.getParticleData().getImages().cpu().numpy().tobytes(),
                 v.cpu().numpy().tobytes()) for s, v in zip(sysdefs, velocities)]

    forces()
    integrator.prime()
    run(10)
    trajectory.record(force=True)
    lossy.record()
    kept_at_10 = state()
    run(10)
    final = state()
    assert final != kept_at_10
    with pytest.raises(RuntimeError, match="f64"):
        lossy.restore()
    trajectory.restore()
    assert state() == kept_at_10                                                  # x, y, z, images and velocities; tags and masses kept
    forces()
    integrator.prime()
    run(10)
    assert state() == final
    # systems=: one system alone goes back
    trajectory.restore(row=0, systems=[1])
    now = state()
    assert now[1] == kept_at_10[1] and now[0] == final[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="captured"):
            trajectory.restore()
        trajectory.record()
    # the hand-over: GSD's chunk names and types, and the unwrapped positions
    chunks = trajectory.gsd_chunks(1, 0)
    assert chunks["particles/N"].tolist() == [129] and chunks["configuration/step"].tolist() == [1]
    assert chunks["particles/position"].dtype == np.float32 and chunks["particles/position"].shape == (129, 3)
    assert chunks["particles/image"].dtype == np.int32 and chunks["particles/velocity"].shape == (129, 3)
    assert chunks["particles/typeid"].tolist() == cfgs[1]["typeid"].tolist()
    assert chunks["configuration/box"].tolist() == [32.0, 32.0, 32.0, 0.0, 0.0, 0.0]
    frames = trajectory.read()
    assert frames.shape == (2, 1) and frames["position"].shape == (2, 1, 129, 3) and frames["image"].dtype == np.int32
    un = trajectory.unwrapped(frames)
    assert un.dtype == np.float64 and np.array_equal(
        un[1, 0], frames["position"][1, 0] + frames["image"][1, 0] * np.array([32.0, 32.0, 32.0]))
    both = lossy.read()
    assert both["position"].dtype == np.float32
    assert both["position"][1, 0].tobytes() == frames["position"][1, 0].astype(np.float32).tobytes()
    for obj in (lossy, trajectory, integrator, molecular, cavity):
        obj.close()


# ---- 7. the example ---------------------------------------------------------------------------------------------------------------
def test_the_example_runs():
    """examples/trajectory/batch_trajectory_in_one_graph.py, small: 2 systems, 60 replays, an output period of 10 (the adaptive dt
    stays between 0.5 and 10, so every system writes its first frame on call 1 and at least two more)"""
    done = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trajectory", "batch_trajectory_in_one_graph.py"), "2", "60", "10"],
                          cwd=ROOT, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
    out = done.stdout
    assert done.returncode == 0, out
    print(out)
    frames = re.search(r"frames per system (\d+) \.\. (\d+)", out)
    assert frames is not None and 3 <= int(frames.group(1)) <= int(frames.group(2)) <= 60 * 10 // 10 + 2, out
    assert "written by calls [1, " in out and "particles/position float32[433, 3]" in out and "particles/image int32[433, 3]" in out, out
    gap = re.search(r"smallest gap (\S+) \(output period 10\.0\)", out)
    assert gap is not None and float(gap.group(1)) >= 10.0, out
