"""The velocity-Verlet step of a batch of independent small systems, one launch per half-step (cavmd_verlet_*,
cavitymd.VerletBatch) on the GPU.  Run with `-m gpu` on an MI355X.

The contract is the list of expressions in include/cavmd.h (HOOMD-blue's ConstantVolume half-steps plus its Langevin bath on
one particle).  This file carries a numpy mirror of it -- numpy element-wise operations round once each and do not fuse -- and
every "bit for bit" check compares uint64 views:
  1. one ragged batch against the mirror, with particles placed on every edge of the wrap;
  2. {step one, force batch, step two} replayed from a graph against the same steps enqueued eagerly;
  3. the batch form of tests/test_gpu_dynamics.py::test_thousand_step_velocity_verlet against a CPU twin with the oracle's forces;
  4. the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi, synthetic
from gpu_support import bits as _u64
from gpu_support import same as _same
from gpu_support import stream as _stream
from verlet_mirror import mirror_accelerations, mirror_step_one, mirror_step_two

pytestmark = pytest.mark.gpu

INV = _capi.CAVMD_ERR_INVALID_VALUE


def _rows_array(rows) -> np.ndarray:
    """a list of VerletInput -> (B, 8) float64 holding their bytes"""
    arr = (_capi.VerletInput * len(rows))(*rows)
    return np.frombuffer(bytes(arr), dtype=np.float64).reshape(len(rows), 8).copy()


# ---- 1. one ragged batch --------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 255, 256, 257, 501, 1024, 1025, 2049, 511, 512, 513)     # step two's tile is 512 particles
EDGES = ("at_hi", "at_lo", "above_hi", "below_lo", "far_outside")


def _edge_target(edge, L):
    hi = L * 0.5
    return {"at_hi": hi, "at_lo": -hi, "above_hi": np.nextafter(hi, np.inf), "below_lo": np.nextafter(-hi, -np.inf),
            "far_outside": hi + 1.5 * L}[edge]


def _ragged_system(k, n, rng, dt):
    """Host arrays of item k.  Particle p < 5 lands, on axis c, on edge (p + c) % 5 after the drift: its mass is 2, its summed
    force 4 per component and its velocity 0, so a = 2, the kicked velocity is dt and the drift dt * dt, all exact for the
    power-of-two dt used here.  (A one-particle system can hit three of the five edges, one per axis.)"""
    box = (8.0, 10.0 + 2.0 * (k % 2), 12.0)
    n_forces = (1, 2, 4)[k % 3]
    pos = np.zeros((max(n, 1), 4))
    pos[:, :3] = rng.uniform(-0.5, 0.5, (pos.shape[0], 3)) * np.array(box)
    pos[:, 3] = cavitymd.state.type_tag_as_double(rng.integers(0, 3, pos.shape[0]))
    pos[0, 3] = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]      # a NaN payload must survive too
    vel = np.zeros((pos.shape[0], 4))
    vel[:, :3] = rng.normal(0.0, 3.0, (pos.shape[0], 3))                                 # fast: many ordinary wraps
    vel[:, 3] = rng.uniform(0.5, 20.0, pos.shape[0])
    image = rng.integers(-3, 4, (pos.shape[0], 3)).astype(np.int32)
    forces = [rng.normal(0.0, 5.0, (pos.shape[0], 4)) for _ in range(n_forces)]
    for p in range(min(n, 5)):
        vel[p] = (0.0, 0.0, 0.0, 2.0)
        for f in forces:
            f[p, :3] = 0.0
        forces[0][p, :3] = 4.0
        for c in range(3):
            pos[p, c] = _edge_target(EDGES[(p + c) % 5], box[c]) - dt * dt
    return {"N": n, "box": box, "pos": pos[:n], "vel": vel[:n], "image": image[:n], "forces": [f[:n] for f in forces],
            "net": np.full((n, 4), 7.0) if k % 2 == 0 else None, "accel": np.full((n, 3), -3.0),
            "langevin": (-1 if n == 0 else (0, n - 1, -1)[k % 3]), "steps": 0, "out_of_box": 0, "reservoir": np.float64(0.0)}


def _to_device(s):
    d = {name: torch.from_numpy(np.ascontiguousarray(s[name])).cuda() for name in ("pos", "vel", "image", "accel")}
    d["forces"] = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in s["forces"]]
    d["net"] = None if s["net"] is None else torch.from_numpy(s["net"].copy()).cuda()
    return d


def _item(s, d):
    n = s["N"]
    return _capi.verlet_item(n, d["pos"].data_ptr() if n else 0, d["image"].data_ptr() if n else 0,
                             d["vel"].data_ptr() if n else 0, d["accel"].data_ptr() if n else 0,
                             [f.data_ptr() if n else 0 for f in d["forces"]],
                             d["net"].data_ptr() if (d["net"] is not None and n) else 0, s["box"], s["langevin"])


def _device_bytes(d):
    out = {name: d[name].cpu().numpy().tobytes() for name in ("pos", "vel", "image", "accel")}
    out["net"] = b"" if d["net"] is None else d["net"].cpu().numpy().tobytes()
    return out


def _assert_equals_mirror(s, d, state, where):
    for name in ("pos", "vel", "accel"):
        assert _same(d[name].cpu().numpy(), s[name]), (where, name)
    assert np.array_equal(d["image"].cpu().numpy(), s["image"]), where
    if s["net"] is not None:
        assert _same(d["net"].cpu().numpy(), s["net"]), (where, "net")
    assert (int(state["steps"]), int(state["out_of_box"])) == (s["steps"], s["out_of_box"]), where
    assert _same(state["langevin_reservoir"], s["reservoir"]), where


def test_one_ragged_batch_equals_the_mirror_bit_for_bit():
    rng = np.random.default_rng(20241018)
    SKIPPED = SIZES.index(257)
    dts = [(0.5, 0.25, 0.125)[k % 3] for k in range(len(SIZES))]
    systems = [_ragged_system(k, n, rng, dts[k]) for k, n in enumerate(SIZES)]
    assert sorted(len(s["forces"]) for s in systems if s["N"]) == [1, 1, 1, 2, 2, 2, 2, 4, 4, 4, 4]
    dev = [_to_device(s) for s in systems]
    ws = _capi.Workspace(1)
    batch = _capi.Verlet(ws, [_item(s, d) for s, d in zip(systems, dev)])
    assert batch.launch_order == sorted(range(len(SIZES)), key=lambda i: -SIZES[i]) != list(range(len(SIZES)))
    initial = [_device_bytes(d) for d in dev]
    tags = [_u64(s["pos"][:, 3]).copy() for s in systems]
    masses = [_u64(s["vel"][:, 3]).copy() for s in systems]
    torch.cuda.synchronize()

    # a = F / m, as HOOMD does once at the start of a run: no input row, nothing counted
    batch.accelerations(_stream())
    for s in systems:
        mirror_accelerations(s)
    state = batch.read(_stream())
    for k, (s, d) in enumerate(zip(systems, dev)):
        _assert_equals_mirror(s, d, state[k], ("accelerations", k))
    primed = [_device_bytes(d) for d in dev]
    assert primed[0] == initial[0]                                           # N = 0: nothing is touched

    hit = [[set() for _ in range(3)] for _ in systems]
    for step in range(2):
        rows = []
        for k, s in enumerate(systems):
            gamma = 0.0 if k == 6 else 0.01 * (k + 1)                         # item 6 names a Langevin particle but has no bath
            dt = 0.0 if k == SKIPPED else dts[k]
            rows.append(_capi.verlet_input_make(dt, gamma, 3.0e-4, rng.uniform(-1.0, 1.0, 3)))
        assert rows[SKIPPED].skip != 0 and sum(r.skip != 0 for r in rows) == 1
        d_rows = torch.from_numpy(_rows_array(rows)).cuda()
        batch.step_one(_stream(), d_rows.data_ptr())
        for k, s in enumerate(systems):
            def classify(c, x, lo, hi, L, k=k):
                p = np.arange(min(len(x), 5))
                for name, sel in (("at_hi", x[p] == hi), ("at_lo", x[p] == lo), ("above_hi", x[p] == np.nextafter(hi, np.inf)),
                                  ("below_lo", x[p] == np.nextafter(lo, -np.inf)), ("far_outside", x[p] >= hi + L)):
                    if sel.any():
                        hit[k][c].add(name)
            mirror_step_one(s, rows[k], classify if step == 0 else None)
        state = batch.read(_stream())
        for k, (s, d) in enumerate(zip(systems, dev)):
            _assert_equals_mirror(s, d, state[k], ("step one", step, k))
        batch.step_two(_stream(), d_rows.data_ptr())
        for k, s in enumerate(systems):
            mirror_step_two(s, rows[k])
        state = batch.read(_stream())
        for k, (s, d) in enumerate(zip(systems, dev)):
            _assert_equals_mirror(s, d, state[k], ("step two", step, k))
            assert np.array_equal(_u64(d["pos"].cpu().numpy()[:, 3]), tags[k]), k      # pos.w and vel.w keep their bits
            assert np.array_equal(_u64(d["vel"].cpu().numpy()[:, 3]), masses[k]), k

    # every edge was hit on every axis (a one-particle system: one edge per axis), and behaved as the contract says
    for k, s in enumerate(systems):
        if k == SKIPPED or s["N"] == 0:
            assert hit[k] == [set(), set(), set()]
        elif s["N"] >= 5:
            assert all(h == set(EDGES) for h in hit[k]), (k, hit[k])
        else:
            assert [h for h in hit[k]] == [{EDGES[c]} for c in range(3)], (k, hit[k])
    for k, s in enumerate(systems):
        if s["N"] >= 5 and k != SKIPPED:
            assert s["out_of_box"] >= 3 and s["steps"] == 2, k                # the far particle of each axis: counted, not repaired
    assert [s["langevin"] for s in systems] == [-1, 0, -1, 0, 256, -1, 0, 1024, -1, 0, 511, -1]  # first, last, none
    assert [k for k, s in enumerate(systems) if s["reservoir"] != 0.0] == [1, 3, 7, 9, 10]  # 4 is skipped, 6 has gamma == 0
    # the skipped item and the empty item: byte-identical to what they were after `accelerations`
    for k in (SKIPPED, 0):
        assert _device_bytes(dev[k]) == primed[k], k
        assert state[k].tobytes() == bytes(32)
    for name in ("pos", "vel", "image"):
        assert primed[SKIPPED][name] == initial[SKIPPED][name]
    batch.close()
    ws.close()


def test_a_nan_coordinate_is_counted_not_repaired():
    n = 300
    pos = np.zeros((n, 4))
    pos[7, 1] = np.nan
    pos[299, 2] = np.inf
    vel = np.ones((n, 4))
    s = {"N": n, "box": (8.0, 8.0, 8.0), "pos": pos, "vel": vel, "image": np.zeros((n, 3), dtype=np.int32),
         "forces": [np.zeros((n, 4))], "net": None, "accel": np.zeros((n, 3)), "langevin": -1}
    d = _to_device(s)
    ws = _capi.Workspace(1)
    batch = _capi.Verlet(ws, [_item(s, d)])
    rows = torch.from_numpy(_rows_array([_capi.verlet_input_make(0.5)])).cuda()
    batch.step_one(_stream(), rows.data_ptr())
    state = batch.read(_stream())
    got = d["pos"].cpu().numpy()
    assert int(state[0]["out_of_box"]) == 2 and np.isnan(got[7, 1]) and np.isinf(got[299, 2])     # inf - L stays outside
    assert np.array_equal(got[:7, :3], np.full((7, 3), 0.5))
    batch.close()
    ws.close()


# ---- 2. capture ---------------------------------------------------------------------------------------------------------------
def _replicas(seeds, rng_seed=42):
    """config-1 systems with masses and velocities drawn as tests/test_gpu_dynamics.py draws them"""
    out = []
    for seed in seeds:
        cfg = synthetic.config1(seed=seed)
        n = len(cfg["charge"])
        rng = np.random.default_rng(rng_seed)
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
        v0 = rng.normal(size=(n, 3)) * np.sqrt(3.167e-4 / mass)[:, None]
        out.append({"cfg": cfg, "N": n, "mass": mass, "v0": v0})
    return out


def _build(replicas, langevin_index=None, net_forces=False):
    sysdefs, velocities = [], []
    for r in replicas:
        cfg = r["cfg"]
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        velocities.append(torch.from_numpy(np.concatenate([r["v0"], r["mass"][:, None]], axis=1)).cuda())
    forces = cavitymd.CavityForceBatch(sysdefs, [r["cfg"]["params"] for r in replicas])
    integrator = cavitymd.VerletBatch(forces, velocities, langevin_index=langevin_index, net_forces=net_forces)
    return sysdefs, velocities, forces, integrator


def _snapshot(sysdefs, velocities, integrator):
    torch.cuda.synchronize()
    out = []
    for k, sd in enumerate(sysdefs):
        pd = sd.getParticleData()
        out.append((pd.getPositions().cpu().numpy().tobytes(), pd.getImages().cpu().numpy().tobytes(),
                    velocities[k].cpu().numpy().tobytes(), integrator.accel[k].cpu().numpy().tobytes()))
    return out


def test_captured_step_replays_like_the_eager_one():
    B, REPLAYS = 3, 200
    replicas = _replicas([11, 12, 13])
    photon = [int(np.flatnonzero(r["cfg"]["typeid"] == 2)[0]) for r in replicas]
    assert photon == [500] * B
    rng = np.random.default_rng(5)
    built = [_build(replicas, langevin_index=photon) for _ in range(2)]       # fresh copies of the same state
    rows = np.zeros((REPLAYS, B, 8))
    for r in range(REPLAYS):
        rows[r] = _rows_array([_capi.verlet_input_make(rng.uniform(2.0, 6.0), 1e-3, 3.167e-4, rng.uniform(-1.0, 1.0, 3))
                               for _ in range(B)])
    assert len(set(rows[:, :, 0].ravel().tolist())) == REPLAYS * B            # dt varies per replay and per item
    d_rows = torch.from_numpy(rows).cuda()
    for _, _, forces, integrator in built:
        forces.compute()
        integrator.prime()
    torch.cuda.synchronize()

    # eager
    sysdefs, velocities, forces, integrator = built[0]
    for r in range(REPLAYS):
        integrator.inputs.copy_(d_rows[r])
        integrator.step_one()
        forces.compute()
        integrator.step_two()
    want = _snapshot(sysdefs, velocities, integrator)
    want_state = integrator.state()

    # captured: the input rows rewritten in stream order before every replay
    sysdefs, velocities, forces, integrator = built[1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        integrator.step_one()
        forces.compute()
        integrator.step_two()
    assert integrator.state()["steps"].tolist() == [0] * B                    # capturing ran nothing
    for r in range(REPLAYS):
        integrator.inputs.copy_(d_rows[r])
        graph.replay()
    assert _snapshot(sysdefs, velocities, integrator) == want
    state = integrator.state()
    assert state.tobytes() == want_state.tobytes()
    assert state["steps"].tolist() == [REPLAYS] * B and state["out_of_box"].tolist() == [0] * B
    assert np.all(state["langevin_reservoir"] != 0.0)
    # a replay after a reset counts from 0
    integrator.reset()
    integrator.inputs.copy_(d_rows[0])
    graph.replay()
    state = integrator.state()
    assert state["steps"].tolist() == [1] * B and state["out_of_box"].tolist() == [0] * B
    for _, _, forces, integrator in built:
        integrator.close()
        forces.close()


# ---- 3. trajectory --------------------------------------------------------------------------------------------------------------
def _cpu_twin(r, ref, oracle_mod, dt, steps):
    """The contract expressions on the host with the oracle's forces; -> wrapped pos, image, vel, last energies, wrap events"""
    cfg = r["cfg"]
    n, L = r["N"], np.asarray(cfg["box"], dtype=np.float64)
    p = cfg["params"]
    prm = ref.make_params(p["omegac"], p["couplstr"], p["phmass"])
    s = {"N": n, "box": tuple(L), "pos": np.concatenate([cfg["position"], np.zeros((n, 1))], axis=1),
         "vel": np.concatenate([r["v0"], r["mass"][:, None]], axis=1), "image": np.array(cfg["image"], dtype=np.int32),
         "net": None, "langevin": -1, "steps": 0, "out_of_box": 0, "reservoir": np.float64(0.0)}

    def force():
        out = ref.compute(oracle_mod.pack_pos(s["pos"][:, :3], cfg["typeid"]), cfg["charge"], s["image"], cfg["box"], 2, prm)
        f = np.zeros((n, 4))
        f[:, :3] = out["force"][:, :3]
        return [f], out["energies"]

    row = _capi.verlet_input_make(dt)
    s["forces"], E = force()
    mirror_accelerations(s)
    events = 0
    for _ in range(steps):
        before = s["image"].copy()
        mirror_step_one(s, row)
        events += int(np.count_nonzero(s["image"] != before))
        s["forces"], E = force()
        mirror_step_two(s, row)
    return s, np.asarray(E), events


def test_thousand_captured_steps_of_two_replicas(ref, oracle_mod):
    dt, steps = 5.0, 1000
    replicas = _replicas([1, 2])
    B = len(replicas)
    sysdefs, velocities, forces, integrator = _build(replicas)
    recorder = cavitymd.BatchRecorder(forces, velocities, capacity=steps // 10, period=10)
    integrator.set_inputs(dt)
    forces.compute()
    integrator.prime()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        integrator.step_one()
        forces.compute()
        integrator.step_two()
        recorder.record()
    for _ in range(steps):
        graph.replay()
    state = integrator.state()
    series = recorder.read()
    assert series.shape == (B, steps // 10) and series["call"][0].tolist() == list(range(10, steps + 1, 10))
    assert state["steps"].tolist() == [steps] * B and state["out_of_box"].tolist() == [0] * B
    for k, r in enumerate(replicas):
        cfg = r["cfg"]
        L = np.asarray(cfg["box"], dtype=np.float64)
        twin, Ec, events = _cpu_twin(r, ref, oracle_mod, dt, steps)
        pd = sysdefs[k].getParticleData()
        pos, img = pd.getPositions().cpu().numpy(), pd.getImages().cpu().numpy()
        vg = velocities[k].cpu().numpy()[:, :3]
        r0 = cfg["position"] + cfg["image"] * L[None, :]
        rg = pos[:, :3] + img * L[None, :]
        rc = twin["pos"][:, :3] + twin["image"] * L[None, :]
        vc = twin["vel"][:, :3]
        moved = np.flatnonzero((img != cfg["image"]).any(axis=1))
        print(f"\nseed {cfg['seed']}: {events} wrap events on the host, {len(moved)} particles with a changed image, photon "
              f"image {img[500].tolist()} from {np.asarray(cfg['image'])[500].tolist()}; max |dr| {np.abs(rg - rc).max():.3e} of "
              f"{np.abs(rc - r0).max():.3e}, max |dv| {np.abs(vg - vc).max():.3e} of {np.abs(vc).max():.3e}")
        # GPU trajectory == the twin's, at the tolerances of test_thousand_step_velocity_verlet
        assert np.abs(rg - rc).max() <= 1e-9 * np.abs(rc - r0).max()
        assert np.abs(vg - vc).max() <= 1e-9 * np.abs(vc).max()
        assert np.array_equal(img, twin["image"])
        # energy from the recorder's rows: bounded oscillation, no drift
        H = series["kinetic_energy"][k] + series["energy"][k].sum(axis=1)
        scale = abs(Ec).max() + 0.5 * float((r["mass"] * (vc ** 2).sum(axis=1)).sum())
        print(f"    H oscillation {np.abs(H - H[0]).max() / scale:.3e}, drift {abs(H[-20:].mean() - H[:20].mean()) / scale:.3e} "
              "(of scale)")
        assert np.abs(H - H[0]).max() <= 5e-3 * scale
        assert abs(H[-20:].mean() - H[:20].mean()) <= 5e-4 * scale
        # the workload itself exercises the wrap and the force kernel's unwrap of what the integrator wrote
        assert twin["out_of_box"] == 0
        assert len(moved) >= 10 and 500 in moved
    recorder.close()
    integrator.close()
    forces.close()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    replicas = _replicas([3])
    sysdefs, velocities, forces, integrator = _build(replicas, net_forces=True)
    v = integrator.verlet
    lib = v._lib
    rows = integrator.inputs
    for call in (lib.cavmd_verlet_step_one, lib.cavmd_verlet_step_two):
        for bad in (0, rows.data_ptr() + 4):
            assert call(v.handle, None, ctypes.c_void_p(bad)) == INV
    integrator.set_inputs(5.0)
    forces.compute()
    integrator.prime()
    assert _same(integrator.net_forces[0].cpu().numpy(), forces.forces[0].cpu().numpy())   # one force array: the sum is that array
    item = [_capi.verlet_item(501, sysdefs[0].getParticleData().getPositions().data_ptr(),
                              sysdefs[0].getParticleData().getImages().data_ptr(), velocities[0].data_ptr(),
                              integrator.accel[0].data_ptr(), [forces.forces[0].data_ptr()], 0, (40.0, 40.0, 40.0))]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        integrator.step_one()
        with pytest.raises(_capi.CavmdError) as e:                             # the stream of the last launch is capturing
            v.set_items(0, item)
        assert e.value.status == INV
        with pytest.raises(_capi.CavmdError) as e:
            v.read(_stream())
        assert e.value.status == INV
    v.set_items(0, item)                                                       # outside the capture it goes through
    with pytest.raises(_capi.CavmdError):
        v.set_items(1, item)                                                   # leaves the batch
    assert v.state_device_ptr() % 8 == 0 and v.state_device_ptr() == v.state_device_ptr()
    # destroying the workspace before its integrator is an error, and harmless
    assert lib.cavmd_destroy(integrator._ws.handle) == INV
    integrator.step_one()
    integrator.step_two()
    assert integrator.state()["steps"].tolist() == [1]
    integrator.close()
    forces.close()
