"""The recorder (cavmd_recorder_*, cavitymd.BatchRecorder) on the GPU: one launch appends one 128-byte row per system to a time
series in device memory, also when that launch is replayed from a graph.

Equivalences asserted (include/cavmd.h), per item and recorded row, bit for bit:
  energy, total_dipole, q, eval_sequence   the bytes of that evaluation's cavmd_result
  cavity_kinetic, cavity_temperature       cavmd_cavity_mode's out[0], out[3]; cavity_kinetic + energy[0] its out[2]; the same
                                           expression in numpy float64 scalars (one rounding per operation)
  kinetic_energy, force_mass_sum           cavmd_kinetic_energy / cavmd_force_mass_sum for that item alone (the device has at
                                           least 64 compute units: MI355X has 256)
Against the executed reference (tests/golden/reference_python_golden.npz) the tolerances are those of
tests/test_gpu_reference_golden.py: rel 1e-14 cavity mode, rel 1e-13 kinetic energy, S and the dt rule."""
import csv
import ctypes
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi, observables as prod, synthetic
from gpu_support import same as _same
from gpu_support import stream as _stream

pytestmark = pytest.mark.gpu
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
KB = cavitymd.PhysicalConstants.KB_HARTREE_PER_K
L_TYPEID = 1
BOX = (40.0, 41.0, 42.0)
FLOAT_COLUMNS = ("energy", "total_dipole", "q", "cavity_kinetic", "cavity_temperature", "kinetic_energy", "force_mass_sum",
                 "reserved")


def _cavity_mode_numpy(vel_row, kB):
    """cavity_mode_kernel's expressions in float64 scalars: one rounding per operation, hence the same bits."""
    vx, vy, vz, m = (np.float64(x) for x in vel_row)
    ke = np.float64(0.5) * m * ((vx * vx + vy * vy) + vz * vz)
    return ke, (np.float64(2.0) / np.float64(3.0)) * ke / np.float64(kB)


class Sys:
    """One system of a ragged batch: HOOMD-layout device arrays, a photon at a chosen place (or none), a member list."""

    def __init__(self, N, photon, members, rng):
        self.N = N
        typeid = np.zeros(N, dtype=np.int32)
        if photon is not None and N:
            typeid[{"first": 0, "middle": N // 2, "last": N - 1}[photon]] = L_TYPEID
        self.photon = int(np.flatnonzero(typeid == L_TYPEID)[0]) if (typeid == L_TYPEID).any() else -1
        pos = np.zeros((N, 4))
        pos[:, :3] = rng.uniform(-0.5, 0.5, (N, 3)) * np.array(BOX)
        pos[:, 3] = cavitymd.state.type_tag_as_double(typeid)
        chg = rng.uniform(-1.0, 1.0, N)
        if self.photon >= 0:
            chg[self.photon] = 0.0
        vel = np.zeros((N, 4))
        vel[:, 3] = rng.uniform(0.5, 30.0, N)
        net = np.zeros((N, 4))
        self.pos = torch.from_numpy(pos).cuda()
        self.chg = torch.from_numpy(chg).cuda()
        self.img = torch.from_numpy(rng.integers(-2, 3, (N, 3)).astype(np.int32)).cuda()
        self.frc = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        self.scratch = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        self.vel = torch.from_numpy(vel).cuda()
        self.net = torch.from_numpy(net).cuda()
        if members == "all" or N == 0:
            self.members, self.n_members = None, N
        elif members == "sorted":
            idx = np.flatnonzero(typeid != L_TYPEID)
            self.members, self.n_members = torch.from_numpy(idx.astype(np.int32)).cuda(), len(idx)
        else:   # unsorted and sparse: a shuffled third of the particles
            idx = rng.permutation(N)[:max(N // 3, 1)]
            self.members, self.n_members = torch.from_numpy(idx.astype(np.int32)).cuda(), len(idx)
        self.params = _capi.make_params(0.0091, 1e-3, 1.0)

    def move(self, gen):
        """positions, velocities and net forces change (on the device, in stream order); masses and type tags stay"""
        if self.N == 0:
            return
        self.pos[:, :3].add_(torch.randn((self.N, 3), dtype=torch.float64, device="cuda", generator=gen) * 1e-2)
        self.vel[:, :3] = torch.randn((self.N, 3), dtype=torch.float64, device="cuda", generator=gen) * 1e-3
        self.net[:, :3] = torch.randn((self.N, 3), dtype=torch.float64, device="cuda", generator=gen) * 1e-2

    def force_item(self):
        ptr = (lambda t: t.data_ptr()) if self.N else (lambda t: 0)
        return _capi.batch_item(self.N, ptr(self.pos), ptr(self.chg), ptr(self.img), ptr(self.frc), BOX, L_TYPEID, self.params)

    def recorder_item(self, result_ptr, vel=True, net=True):
        return _capi.recorder_item(result_ptr, self.vel.data_ptr() if (vel and self.N) else 0,
                                   self.net.data_ptr() if (net and self.N) else 0,
                                   self.members.data_ptr() if (self.members is not None and self.n_members) else 0,
                                   self.N, self.n_members)


def _ragged(rng):
    spec = [(0, None, "all"), (1, "first", "all"), (1, None, "all"), (255, "first", "all"), (256, "middle", "sorted"),
            (257, "last", "sparse"), (501, "last", "all"), (501, "middle", "sorted"), (501, None, "sparse"),
            (501, "first", "sparse"), (1023, "middle", "all"), (1024, "last", "sorted"), (1024, None, "all"),
            (1025, "first", "sparse"), (1025, "last", "all"), (4096, "middle", "sorted"), (4096, None, "sparse"),
            (4096, "first", "all"), (65536, "last", "all"), (65536, "middle", "sparse"), (65536, None, "sorted")]
    return [Sys(N, photon, members, rng) for N, photon, members in spec]


def _recorder(ws, fb, systems, capacity, period=1, **kw):
    res = fb.results_device_ptr()
    return _capi.Recorder(ws, [s.recorder_item(res + 192 * k, **kw) for k, s in enumerate(systems)], capacity, period, KB)


def _expected_row(s, result, single, call, small_ws=None):
    """The row of one item from the single paths (per-item calls on a workspace of its own) and numpy."""
    row = np.zeros((), dtype=_capi.record_dtype())
    row["call"], row["eval_sequence"] = call, result.sequence
    row["energy"], row["total_dipole"], row["q"] = result.energy[:], result.total_dipole[:], result.q[:]
    assert result.photon_idx == s.photon
    if s.photon >= 0:
        ke, T = _cavity_mode_numpy(s.vel[s.photon].cpu().numpy(), KB)
        row["cavity_kinetic"], row["cavity_temperature"] = ke, T
        if small_ws is not None and s.N <= 1024:
            # the single workspace evaluates this N with the kernel the batch runs: same block, then cavmd_cavity_mode
            small_ws.compute_hoomd(_stream(), s.N, s.pos.data_ptr(), s.chg.data_ptr(), s.img.data_ptr(), BOX, L_TYPEID,
                                   s.params, s.scratch.data_ptr())
            out = small_ws.cavity_mode(_stream(), s.vel.data_ptr(), KB)
            assert _same(out[0], ke) and _same(out[3], T) and _same(out[1], result.energy[0])
            assert _same(out[2], np.float64(ke) + np.float64(result.energy[0]))
    if s.N:
        row["kinetic_energy"] = single.kinetic_energy(_stream(), s.vel.data_ptr(),
                                                      s.members.data_ptr() if s.members is not None else None, s.n_members)
        row["force_mass_sum"] = single.force_mass_sum(_stream(), s.N, s.net.data_ptr(), s.vel.data_ptr())
    return row


def _assert_rows_equal(got, want, where, skip=()):
    for name in got.dtype.names:
        if name in skip:
            continue
        a, b = got[name], want[name]
        same = np.array_equal(a, b) if a.dtype.kind == "u" else _same(a, b)
        assert same, (where, name, a, b)


# ---- 1. a ragged batch against the single paths, bit for bit --------------------------------------------------------------
def test_ragged_batch_is_bit_equal_to_the_single_paths_over_40_steps():
    STEPS = 40
    rng = np.random.default_rng(2024)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    systems = _ragged(rng)
    B = len(systems)
    ws = _capi.Workspace(1)
    assert ws.device_info()["compute_units"] >= 64
    single = _capi.Workspace(65536)
    small_ws = _capi.Workspace(1024)
    fb = _capi.Batch(ws, [s.force_item() for s in systems])
    rec = _recorder(ws, fb, systems, capacity=64)
    assert rec.launch_order == sorted(range(B), key=lambda i: -max(systems[i].N, systems[i].n_members))
    want = np.zeros((B, STEPS), dtype=_capi.record_dtype())
    for step in range(STEPS):
        for s in systems:
            s.move(gen)
        fb.compute(_stream())
        rec.record(_stream())
        torch.cuda.synchronize()
        results = fb.results()
        for k, s in enumerate(systems):
            want[k, step] = _expected_row(s, results[k], single, step + 1, small_ws)
    assert list(rec.rows(_stream())) == [STEPS] * B
    got = rec.read(_stream(), 0, B, 0, STEPS)
    assert got.shape == (B, STEPS)
    for k in range(B):
        _assert_rows_equal(got[k], want[k], f"item {k} (N = {systems[k].N})")
    # the columns are alive: sums differ from step to step, a photon has a temperature, an empty item has zeros everywhere
    for k, s in enumerate(systems):
        if s.N > 1:
            assert len(set(got[k]["kinetic_energy"])) == STEPS and len(set(got[k]["force_mass_sum"])) == STEPS and \
                (got[k]["kinetic_energy"] > 0).all() and (got[k]["force_mass_sum"] > 0).all()
        assert (got[k]["cavity_temperature"] > 0).all() == (s.photon >= 0)
        assert not got[k]["reserved"].any()
    assert not any(got[0][name].any() for name in FLOAT_COLUMNS)
    # a part of the series: items 3 .. 7, rows 10 .. 19
    part = rec.read(_stream(), 3, 5, 10, 10)
    assert part.tobytes() == np.ascontiguousarray(got[3:8, 10:20]).tobytes()
    rec.close()
    fb.close()
    for w in (ws, single, small_ws):
        w.close()


# ---- 2. the executed reference in one launch -------------------------------------------------------------------------------
def test_the_executed_reference_in_one_launch(golden_dir):
    """cavity_mode/{0,1,2}, kinetic/{0,1,2} and adaptive_dt/{0,1,2} of tests/golden/reference_python_golden.npz, built into
    systems as tests/test_gpu_reference_golden.py does, as items of ONE recorder and one record call."""
    with np.load(os.path.join(golden_dir, "reference_python_golden.npz")) as z:
        gold = {k: z[k] for k in z.files}
    omegac, gcoup, m = 0.25, 1e-3, 2.0
    K = m * omegac * omegac
    prm = _capi.make_params(omegac, gcoup, m)
    keep, fitems, ritems, checks = [], [], [], []
    empty = _capi.batch_item(0, 0, 0, 0, 0, (1e3, 1e3, 1e3), 2, prm)

    def dev(a, dtype=np.float64):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
        keep.append(t)
        return t

    for i in range(3):      # CavityModeTracker: the photon alone at q with 0.5 K q^2 = the fixture's harmonic energy
        g = {k: gold[f"cavity_mode/{i}/{k}"] for k in ("typeid", "mass", "velocity", "harmonic_energy", "properties")}
        n = len(g["mass"])
        where = int(np.flatnonzero(g["typeid"] == 2)[0])
        pos = np.zeros((n, 4))
        pos[where, 0] = np.sqrt(2.0 * float(g["harmonic_energy"]) / K)
        pos[:, 3] = cavitymd.state.type_tag_as_double(g["typeid"])
        frc = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
        keep.append(frc)
        fitems.append(_capi.batch_item(n, dev(pos).data_ptr(), dev(np.zeros(n)).data_ptr(),
                                       dev(np.zeros((n, 3)), np.int32).data_ptr(), frc.data_ptr(), (1e3, 1e3, 1e3), 2, prm))
        vel4 = dev(np.concatenate([g["velocity"], g["mass"][:, None]], axis=1))
        ritems.append((vel4.data_ptr(), 0, 0, 0, n))
        checks.append(("cavity_mode", g["properties"]))
    for i in range(3):      # EnergyTracker's kinetic energies: the molecular group through an index list, and all particles
        g = {k: gold[f"kinetic/{i}/{k}"] for k in ("typeid", "mass", "velocity", "molecular", "cavity")}
        n = len(g["mass"])
        vel4 = dev(np.concatenate([g["velocity"], g["mass"][:, None]], axis=1))
        mol = dev(np.flatnonzero(g["typeid"] != 2), np.int32)
        cav = dev(np.flatnonzero(g["typeid"] == 2)[:1], np.int32)
        for members, n_members, want, rel in ((mol, mol.numel(), g["molecular"][0], 1e-13), (cav, 1, float(g["cavity"]), 1e-15),
                                              (None, n, g["molecular"][0] + float(g["cavity"]), 1e-13)):
            fitems.append(empty)
            ritems.append((vel4.data_ptr(), 0, members.data_ptr() if members is not None else 0, 0, n_members))
            checks.append(("kinetic", (float(want), rel)))
    for i in range(3):      # AdaptiveTimestepUpdater: S over the sum of the force objects, dt = sqrt(tol / S)
        g = {k: gold[f"adaptive_dt/{i}/{k}"] for k in ("mass", "force_a", "force_b", "error_tolerance", "dt")}
        n = len(g["mass"])
        net = np.zeros((n, 4))
        net[:, :3] = g["force_a"] + g["force_b"]
        vel4 = np.zeros((n, 4))
        vel4[:, 3] = g["mass"]
        fitems.append(empty)
        ritems.append((dev(vel4).data_ptr(), dev(net).data_ptr(), 0, n, 0))
        checks.append(("adaptive_dt", (float(g["error_tolerance"]), float(g["dt"]))))
    ws = _capi.Workspace(1)
    fb = _capi.Batch(ws, fitems)
    res = fb.results_device_ptr()
    rec = _capi.Recorder(ws, [_capi.recorder_item(res + 192 * k, v, f, mem, N, nm) for k, (v, f, mem, N, nm) in enumerate(ritems)],
                         4, 1, KB)
    fb.compute(_stream())
    rec.record(_stream())                                                     # ONE launch for all fifteen
    rows = rec.read(_stream(), 0, len(ritems), 0, 1)[:, 0]
    for row, (kind, want) in zip(rows, checks):
        if kind == "cavity_mode":
            ke, pe, T = float(row["cavity_kinetic"]), float(row["energy"][0]), float(row["cavity_temperature"])
            print(f"cavity mode: KE {ke!r} / {want[0]!r}, PE {pe!r} / {want[1]!r}, T {T!r} / {want[3]!r}")
            assert ke == pytest.approx(want[0], rel=1e-14) and T == pytest.approx(want[3], rel=1e-14)
            assert pe == pytest.approx(want[1], rel=1e-14, abs=0)
            assert ke + pe == pytest.approx(want[2], rel=1e-14)
        elif kind == "kinetic":
            print(f"kinetic energy: {float(row['kinetic_energy'])!r} / {want[0]!r}")
            assert float(row["kinetic_energy"]) == pytest.approx(want[0], rel=want[1])
        else:
            tol, dt = want
            S = float(row["force_mass_sum"])
            print(f"S: {S!r} / {tol / dt**2!r}")
            assert S == pytest.approx(tol / dt**2, rel=1e-13)
            assert prod.adaptive_timestep(tol, S) == pytest.approx(dt, rel=1e-13)
    rec.close()
    fb.close()
    ws.close()


# ---- 3. a replay appends ---------------------------------------------------------------------------------------------------
def _replica_run(captured: bool, B: int, steps: int):
    """B replicas of N = 501: force batch + recorder + thermostat batch per step, positions moved in place between the steps;
    eager, or as replays of one captured graph.  Same seeds, same initial state, same sequence either way."""
    rng = np.random.default_rng(5)
    sysdefs, velocities = [], []
    for k in range(B):
        cfg = synthetic.config1(seed=k + 1)
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        v = np.ones((pd.getN(), 4))
        v[:, :3] = rng.normal(0.0, 1e-3, (pd.getN(), 3))
        velocities.append(torch.from_numpy(v).cuda())
    moves = [torch.from_numpy(rng.normal(0.0, 1e-3, (steps, 501, 3))).cuda() for _ in range(B)]
    variates = np.stack([rng.standard_normal((steps, B)), rng.gamma(749.5, size=(steps, B))], axis=2)
    forces = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    recorder = cavitymd.BatchRecorder(forces, velocities, net_forces=forces.forces, capacity=256)
    thermostat = cavitymd.BussiReservoirBatch(kT=1e-6, tau=0.5)
    thermostat.attach(velocities, translational_dof=3.0 * 501 - 3.0)
    positions = [s.getParticleData().getPositions() for s in sysdefs]

    def advance(r):
        for k in range(B):
            positions[k][:, :3].add_(moves[k][r])                           # in place, on the stream the step goes to
        thermostat.set_inputs(r, 0.005, variates[r])

    torch.cuda.synchronize()
    if captured:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            forces.compute(0)
            recorder.record()
            thermostat.step_async()
        assert list(recorder.rows()) == [0] * B                              # a capture runs nothing
        for r in range(steps):
            advance(r)
            graph.replay()
            if r == steps // 2:                                              # a read between replays disturbs nothing
                assert list(recorder.rows()) == [r + 1] * B
        with pytest.raises(_capi.CavmdError) as e:                           # nothing existing changed: no ring under replay
            forces.energies_at(1)
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    else:
        for r in range(steps):
            advance(r)
            forces.compute(0)
            recorder.record()
            thermostat.step_async()
    rows = recorder.rows()
    series = recorder.read()
    final_v = [v.cpu().numpy().tobytes() for v in velocities]
    recorder.close()
    thermostat.detach()
    forces.close()
    return rows, series, final_v


def test_a_replayed_graph_appends_a_new_row_every_time():
    B, REPLAYS = 6, 200
    rows_e, eager, v_e = _replica_run(False, B, REPLAYS)
    rows_g, replayed, v_g = _replica_run(True, B, REPLAYS)
    assert list(rows_e) == [REPLAYS] * B and list(rows_g) == [REPLAYS] * B
    assert eager.shape == replayed.shape == (B, REPLAYS)
    for k in range(B):
        assert list(replayed[k]["call"]) == list(range(1, REPLAYS + 1))
        assert list(eager[k]["eval_sequence"]) == list(range(1, REPLAYS + 1))
        assert len(set(replayed[k]["eval_sequence"])) == 1                  # frozen at capture: diagnostic only
        _assert_rows_equal(replayed[k], eager[k], f"system {k}", skip=("eval_sequence",))
        # the series is a series: every step saw other positions and other velocities
        for name in ("kinetic_energy", "force_mass_sum", "cavity_kinetic"):
            assert len(set(replayed[k][name])) == REPLAYS, name
        assert len({e.tobytes() for e in replayed[k]["energy"]}) == REPLAYS
    assert v_e == v_g


# ---- 4. ring and period ------------------------------------------------------------------------------------------------------
def test_ring_period_reset_set_items_and_lifetime():
    rng = np.random.default_rng(3)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    systems = [Sys(501, "last", "all", rng), Sys(300, "first", "sorted", rng), Sys(1500, None, "sparse", rng)]
    B = len(systems)
    ws = _capi.Workspace(1)
    single = _capi.Workspace(4096)
    fb = _capi.Batch(ws, [s.force_item() for s in systems])
    rec = _recorder(ws, fb, systems, capacity=8, period=3)
    with pytest.raises(_capi.CavmdError) as e:
        rec.read(_stream(), 0, B, 0, 1)
    assert e.value.status == _capi.CAVMD_ERR_NOT_COMPUTED
    assert ws._lib.cavmd_destroy(ws.handle) == _capi.CAVMD_ERR_INVALID_VALUE       # refused while the recorder lives
    want = {}
    for call in range(1, 51):
        for s in systems:
            s.move(gen)
        fb.compute(_stream())
        rec.record(_stream())
        if call % 3 == 0:
            torch.cuda.synchronize()
            results = fb.results()
            want[call // 3 - 1] = [_expected_row(s, results[k], single, call) for k, s in enumerate(systems)]
    assert list(rec.rows(_stream())) == [16] * B                             # calls 3, 6, ..., 48
    got = rec.read(_stream(), 0, B, 8, 8)
    for k in range(B):
        assert list(got[k]["call"]) == list(range(27, 49, 3))
        for j in range(8):
            _assert_rows_equal(got[k][j], want[8 + j][k], (k, 8 + j))
    assert rec.read(_stream(), 1, 1, 15, 1)[0, 0].tobytes() == got[1, 7].tobytes()
    for first, count, status in ((7, 1, _capi.CAVMD_ERR_EXPIRED), (7, 9, _capi.CAVMD_ERR_EXPIRED), (0, 16, _capi.CAVMD_ERR_EXPIRED),
                                 (16, 1, _capi.CAVMD_ERR_INVALID_VALUE), (15, 2, _capi.CAVMD_ERR_INVALID_VALUE),
                                 (8, 0, _capi.CAVMD_ERR_INVALID_VALUE)):
        with pytest.raises(_capi.CavmdError) as e:
            rec.read(_stream(), 0, B, first, count)
        assert e.value.status == status, (first, count)
    for first_item, n_items in ((B, 1), (0, B + 1), (0, 0)):
        with pytest.raises(_capi.CavmdError) as e:
            rec.read(_stream(), first_item, n_items, 8, 1)
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    # set_items keeps counters and series: item 0 now records system 1's arrays, rows go on from 16 (calls 51 and 54)
    res = fb.results_device_ptr()
    rec.set_items(0, [systems[1].recorder_item(res + 192 * 1)])
    assert list(rec.rows(_stream())) == [16] * B
    assert rec.read(_stream(), 0, B, 8, 8).tobytes() == got.tobytes()
    for call in range(51, 55):
        fb.compute(_stream())
        rec.record(_stream())
    assert list(rec.rows(_stream())) == [18] * B
    last = rec.read(_stream(), 0, B, 17, 1)[:, 0]
    assert list(last["call"]) == [54] * B
    _assert_rows_equal(last[0], last[1], "item 0 follows its new row of the table")
    records_ptr, rows_ptr = rec.device_ptr()
    assert records_ptr and rows_ptr and records_ptr % 16 == 0
    # reset: counters to zero, the next row is row 0 written by call 3
    rec.reset(_stream())
    assert list(rec.rows(_stream())) == [0] * B
    with pytest.raises(_capi.CavmdError) as e:
        rec.read(_stream(), 0, B, 0, 1)
    assert e.value.status == _capi.CAVMD_ERR_NOT_COMPUTED
    for call in range(1, 4):
        fb.compute(_stream())
        rec.record(_stream())
    assert list(rec.rows(_stream())) == [1] * B and list(rec.read(_stream(), 0, B, 0, 1)[:, 0]["call"]) == [3] * B
    rec.close()
    fb.close()
    assert ws._lib.cavmd_destroy(ctypes.c_void_p(0)) == 0
    ws.close()                                                                 # now it goes
    single.close()


# ---- 5. independence -------------------------------------------------------------------------------------------------------
def _series(systems, perm, steps, vel_off=(), net_off=()):
    """Record `steps` calls over the systems in the order `perm`; returns rows indexed by SYSTEM."""
    ws = _capi.Workspace(1)
    ordered = [systems[i] for i in perm]
    fb = _capi.Batch(ws, [s.force_item() for s in ordered])
    res = fb.results_device_ptr()
    rec = _capi.Recorder(ws, [s.recorder_item(res + 192 * k, vel=perm[k] not in vel_off, net=perm[k] not in net_off)
                              for k, s in enumerate(ordered)], 16, 1, KB)
    for step in range(steps):
        for s in systems:                                                      # the same motion whatever the order
            s.pos[:, :3].mul_(1.0 + 1e-3)
            s.vel[:, :3].mul_(1.0 - 1e-3)
            s.net[:, :3].mul_(1.0 + 2e-3)
        fb.compute(_stream())
        if step == steps - 1:
            torch.cuda.synchronize()
            before = [(s.vel.clone(), s.net.clone(), s.pos.clone(), s.frc.clone()) for s in systems]
            blocks = bytes(fb.results())
        rec.record(_stream())
    got = rec.read(_stream(), 0, len(perm), 0, steps)
    # nothing outside the series is written
    for s, (v, f, p, frc) in zip(systems, before):
        for a, b in ((s.vel, v), (s.net, f), (s.pos, p), (s.frc, frc)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert bytes(fb.results()) == blocks
    rec.close()
    fb.close()
    ws.close()
    out = np.zeros_like(got)
    for k, i in enumerate(perm):
        out[i] = got[k]
    return out


def test_items_are_independent_and_columns_without_arrays_are_zero():
    STEPS = 5
    sizes = [(501, "last", "all"), (1, "first", "all"), (2049, "middle", "sparse"), (501, None, "sorted"), (0, None, "all"),
             (1024, "first", "all"), (700, "last", "sparse")]

    def fresh():
        rng = np.random.default_rng(17)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        systems = [Sys(*spec, rng) for spec in sizes]
        for s in systems:
            s.move(gen)
        return systems

    B = len(sizes)
    base = _series(fresh(), list(range(B)), STEPS)
    perm = [int(i) for i in np.random.default_rng(1).permutation(B)]
    assert perm != list(range(B))
    assert _series(fresh(), perm, STEPS).tobytes() == base.tobytes()           # permuting the items permutes the series
    # without velocities: the three velocity columns and S are zero; without net forces: S alone; the others untouched
    got = _series(fresh(), list(range(B)), STEPS, vel_off=(2,), net_off=(5,))
    for k in range(B):
        for name in got.dtype.names:
            zeroed = (k == 2 and name in ("cavity_kinetic", "cavity_temperature", "kinetic_energy", "force_mass_sum")) or \
                (k == 5 and name == "force_mass_sum")
            if zeroed:
                assert not got[k][name].any() and base[k][name].all(), (k, name)
            else:
                assert got[k][name].tobytes() == base[k][name].tobytes(), (k, name)


# ---- 6. one record is one dispatch ------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import numpy as np
import torch
import cavitymd
from cavitymd import synthetic
rng = np.random.default_rng(1)
sysdefs, vels = [], []
for k in range(8):
    cfg = synthetic.config1(seed=k + 1)
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                           cfg["box"], device="cuda")
    sysdefs.append(cavitymd.SystemDefinition(pd))
    v = np.ones((501, 4)); v[:, :3] = rng.normal(0, 1e-3, (501, 3))
    vels.append(torch.from_numpy(v).cuda())
forces = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
rec = cavitymd.BatchRecorder(forces, vels, net_forces=forces.forces, capacity=128)
forces.compute(0)
for step in range(100):
    rec.record()
series = rec.read()
assert series.shape == (8, 100) and list(rec.rows()) == [100] * 8
print("CHILD-OK")
"""


@pytest.mark.skipif(shutil.which("rocprofv3") is None, reason="rocprofv3 is not installed")
def test_one_record_is_one_dispatch(tmp_path):
    """100 record calls of an 8-system recorder in a fresh child process under a kernel trace: 100 dispatches of
    recorder_batch_kernel, none of the single paths' kernels."""
    child = tmp_path / "recorder_child.py"
    child.write_text(CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "cav-hoomd_amd")))
    out = tmp_path / "trace"
    run = subprocess.run(["timeout", "-k", "10", "480", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
                          str(out), "--", sys.executable, str(child)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "CHILD-OK" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    stats = glob.glob(os.path.join(str(out), "**", "*kernel_stats.csv"), recursive=True)
    assert stats, os.listdir(str(out))
    calls = {}
    for path in stats:
        for row in csv.DictReader(open(path)):
            calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    recorded = sum(v for k, v in calls.items() if "recorder_batch_kernel" in k)
    single = sum(v for k, v in calls.items() if "kinetic_fused_kernel" in k or "force_mass_fused_kernel" in k
                 or "cavity_mode_kernel" in k)
    print(f"\ndispatches: recorder_batch_kernel {recorded}, single-path kernels {single}")
    assert recorded == 100 and single == 0, calls
