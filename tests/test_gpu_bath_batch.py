"""A Langevin bath on any set of particles of a batch, drawn in step two (cavmd_bath_*, cavitymd.LangevinBathBatch) on the GPU.
Run with `-m gpu` on an MI355X.

The contract is the list of expressions in include/cavmd.h; tests/bath_mirror.py restates it in element-wise numpy, and every
"bit for bit" check compares uint64 views:
  1. one ragged batch against the mirror over three steps, every gamma pattern planted and counted;
  2. a system's bytes do not depend on its place in a batch or on the run;
  3. items without a bath get the bytes cavmd_verlet_step_two gives them;
  4. {step one, force batch, bath step two} replayed from a graph against the same steps enqueued eagerly;
  5. the bath IS a thermostat: the systems of tests/bath_twin.py, stepped from one graph, inside the host twin's band;
  6. the refusals and the lifetime rules."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bath_mirror as mirror
import bath_twin as twin
import cavitymd
from cavitymd import _capi, synthetic
from gpu_support import bits as _u64
from gpu_support import same as _same
from gpu_support import stream as _stream
from verlet_mirror import mirror_accelerations, mirror_step_one

pytestmark = pytest.mark.gpu

INV = _capi.CAVMD_ERR_INVALID_VALUE
EPS = 2.0 ** -52


def _rows_array(rows) -> np.ndarray:
    arr = (_capi.VerletInput * len(rows))(*rows)
    return np.frombuffer(bytes(arr), dtype=np.float64).reshape(len(rows), 8).copy()


def _system(n, rng, n_forces=1, net=True, langevin=-1):
    """host arrays of one system, as tests/verlet_mirror.py takes them"""
    pos = np.zeros((n, 4))
    pos[:, :3] = rng.uniform(-5.0, 5.0, (n, 3))
    pos[:, 3] = cavitymd.state.type_tag_as_double(rng.integers(0, 3, n))
    vel = np.zeros((n, 4))
    vel[:, :3] = rng.normal(0.0, 0.02, (n, 3))
    vel[:, 3] = rng.uniform(0.5, 20.0, n)
    return {"N": n, "box": (40.0, 42.0, 44.0), "pos": pos, "vel": vel, "image": rng.integers(-3, 4, (n, 3)).astype(np.int32),
            "forces": [rng.normal(0.0, 1e-3, (n, 4)) for _ in range(n_forces)], "net": np.full((n, 4), 7.0) if net else None,
            "accel": np.full((n, 3), -3.0), "langevin": langevin, "steps": 0, "out_of_box": 0, "reservoir": np.float64(0.0)}


def _bath(gamma, kT, seed):
    return {"gamma": None if gamma is None else np.array(gamma, dtype=np.float64), "kT": kT, "seed": seed, "draws": 0, "coupled": 0,
            "reservoir": np.float64(0.0)}


def _to_device(s, b):
    d = {name: torch.from_numpy(np.ascontiguousarray(s[name])).cuda() for name in ("pos", "vel", "image", "accel")}
    d["forces"] = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in s["forces"]]
    d["net"] = None if s["net"] is None else torch.from_numpy(s["net"].copy()).cuda()
    d["gamma"] = None if b["gamma"] is None else torch.from_numpy(b["gamma"].copy()).cuda()
    return d


def _item(s, d):
    n = s["N"]
    return _capi.verlet_item(n, d["pos"].data_ptr() if n else 0, d["image"].data_ptr() if n else 0,
                             d["vel"].data_ptr() if n else 0, d["accel"].data_ptr() if n else 0,
                             [f.data_ptr() if n else 0 for f in d["forces"]],
                             d["net"].data_ptr() if (d["net"] is not None and n) else 0, s["box"], s["langevin"])


def _bath_item(b, d):
    if b["gamma"] is None:
        return _capi.bath_item(0, 0, b["kT"], b["seed"])
    return _capi.bath_item(d["gamma"].data_ptr(), len(b["gamma"]), b["kT"], b["seed"])


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


def _assert_bath_state(got, before, b, result, dt, where):
    """draws and coupled bit for bit; reservoir against R_before - fsum(tallies) * dt with R_before the DEVICE's own previous
    value, within 3 eps |T dt| + eps |R|: 2 ulp of T, one rounding of the product, one of the difference."""
    assert (int(got["draws"]), int(got["coupled"])) == (b["draws"], b["coupled"]), where
    if result is None or b["gamma"] is None:
        assert got.tobytes() == before.tobytes(), where
        return
    _, T = result
    want = float(before["reservoir"]) - T * dt
    bound = 3.0 * EPS * abs(T * dt) + EPS * abs(want)
    err = abs(float(got["reservoir"]) - want)
    print(f"{where}: T {T:+.6e}, reservoir error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (where, err, bound)
    b["reservoir"] = np.float64(got["reservoir"])                            # the mirror goes on from the device's value


# ---- 1. one ragged batch ------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 257)
PATTERNS = ("null", "all", "none", "every_third", "last", "short", "null", "negative_and_nan", "row_wins", "row_gamma_zero", "all",
            "every_third", "long")
WANT_COUPLED = (0, 1, 0, 22, 1, 100, 0, 255, 510, 512, 513, 342, 257)


def _gamma_pattern(pattern, n, rng):
    g = rng.uniform(0.05, 0.4, n)
    if pattern == "null":
        return None
    if pattern == "none":
        return np.zeros(n)
    if pattern == "every_third":
        g[np.arange(n) % 3 != 0] = 0.0
    elif pattern == "last":
        g[:-1] = 0.0
    elif pattern == "short":
        g = g[:100]                                                          # bath N shorter than the system's: the tail is uncoupled
    elif pattern == "long":
        g = np.concatenate([g, rng.uniform(0.05, 0.4, 40)])                  # bath N longer than the system's: the excess is idle
    elif pattern == "negative_and_nan":
        g[3], g[n - 2] = -0.25, np.nan
    return g


def test_one_ragged_batch_equals_the_mirror_bit_for_bit():
    rng = np.random.default_rng(20241019)
    B = len(SIZES)
    assert len(PATTERNS) == B == len(WANT_COUPLED) and set(PATTERNS) == {"null", "all", "none", "every_third", "last", "short",
                                                                        "long", "negative_and_nan", "row_wins", "row_gamma_zero"}
    systems, baths = [], []
    for k, (n, pattern) in enumerate(zip(SIZES, PATTERNS)):
        langevin = n // 2 if pattern in ("row_wins", "row_gamma_zero") else -1
        systems.append(_system(n, rng, n_forces=(1, 2, 3, 4)[k % 4], net=(k % 5 != 4), langevin=langevin))
        baths.append(_bath(_gamma_pattern(pattern, n, rng), 3.0e-4 * (1 + k % 3), mirror.item_key(77, k)))
    assert sorted({len(s["forces"]) for s in systems}) == [1, 2, 3, 4] and sum(s["net"] is not None for s in systems) >= 8
    dev = [_to_device(s, b) for s, b in zip(systems, baths)]
    ws = _capi.Workspace(1)
    verlet = _capi.Verlet(ws, [_item(s, d) for s, d in zip(systems, dev)])
    bath = _capi.Bath(verlet, [_bath_item(b, d) for b, d in zip(baths, dev)])
    initial = [_device_bytes(d) for d in dev]
    tags = [_u64(s["pos"][:, 3]).copy() for s in systems]
    masses = [_u64(s["vel"][:, 3]).copy() for s in systems]
    torch.cuda.synchronize()
    verlet.accelerations(_stream())
    for s in systems:
        mirror_accelerations(s)
    assert bath.read(_stream()).tobytes() == bytes(32 * B)

    for step in range(3):                                                    # draws 0, 1, 2
        rows = []
        for k, pattern in enumerate(PATTERNS):
            dt = (0.5, 0.25, 1.0)[k % 3] * (1.0, 0.75, 1.5)[step]            # differs per item and step
            gamma = 0.0 if pattern == "row_gamma_zero" else 0.01 * (k + 1)
            rows.append(_capi.verlet_input_make(dt, gamma, 3.0e-4, rng.uniform(-1.0, 1.0, 3)))
        d_rows = torch.from_numpy(_rows_array(rows)).cuda()
        verlet.step_one(_stream(), d_rows.data_ptr())
        for k, s in enumerate(systems):
            mirror_step_one(s, rows[k])
        before = bath.read(_stream())
        bath.step_two(_stream(), d_rows.data_ptr())
        results = [mirror.mirror_bath_step_two(s, rows[k], baths[k]) for k, s in enumerate(systems)]
        state, got = verlet.read(_stream()), bath.read(_stream())
        for k, (s, d) in enumerate(zip(systems, dev)):
            _assert_equals_mirror(s, d, state[k], ("step two", step, k))
            _assert_bath_state(got[k], before[k], baths[k], results[k], rows[k].dt, (step, k, PATTERNS[k]))
            assert np.array_equal(_u64(d["pos"].cpu().numpy()[:, 3]), tags[k]), k      # pos.w and vel.w keep their bits
            assert np.array_equal(_u64(d["vel"].cpu().numpy()[:, 3]), masses[k]), k
        # every pattern is there and does what it says: counted independently of the mirror
        assert got["coupled"].tolist() == list(WANT_COUPLED), got["coupled"].tolist()
        assert got["draws"].tolist() == [0 if p == "null" else step + 1 for p in PATTERNS]
        assert state["steps"].tolist() == [0] + [step + 1] * (B - 1)
    for k, pattern in enumerate(PATTERNS):
        if SIZES[k] and pattern != "null" and WANT_COUPLED[k]:
            assert float(got[k]["reservoir"]) != 0.0, k
        # the row's bath ran on the one item whose row names a particle AND carries a gamma
        assert (float(state[k]["langevin_reservoir"]) != 0.0) == (pattern == "row_wins"), k
    # the net force carries no bath term: it is the plain sum of the force arrays
    for s, d in zip(systems, dev):
        if s["net"] is not None and s["N"]:
            F = s["forces"][0].copy()
            for f in s["forces"][1:]:
                F = F + f
            assert _same(d["net"].cpu().numpy(), F)
    assert _device_bytes(dev[0]) == initial[0] and got[0].tobytes() == bytes(32)         # N = 0: nothing is touched
    assert got[6].tobytes() == bytes(32)                                                 # d_gamma NULL: no state written
    bath.close()
    verlet.close()
    ws.close()


# ---- 2. placement and repetition ----------------------------------------------------------------------------------------------
def _run_placed(subject, subject_bath, fillers, place, steps=3):
    """the subject system at `place` among copies of the fillers -> the subject's bytes after `steps` steps"""
    systems = [copy.deepcopy(f[0]) for f in fillers]
    baths = [copy.deepcopy(f[1]) for f in fillers]
    systems.insert(place, copy.deepcopy(subject))
    baths.insert(place, copy.deepcopy(subject_bath))
    dev = [_to_device(s, b) for s, b in zip(systems, baths)]
    ws = _capi.Workspace(1)
    verlet = _capi.Verlet(ws, [_item(s, d) for s, d in zip(systems, dev)])
    bath = _capi.Bath(verlet, [_bath_item(b, d) for b, d in zip(baths, dev)])
    torch.cuda.synchronize()
    verlet.accelerations(_stream())
    for step in range(steps):
        rows = [_capi.verlet_input_make(0.5 + 0.25 * step) for _ in systems]
        d_rows = torch.from_numpy(_rows_array(rows)).cuda()
        verlet.step_one(_stream(), d_rows.data_ptr())
        bath.step_two(_stream(), d_rows.data_ptr())
    out = (_device_bytes(dev[place]), verlet.read(_stream())[place].tobytes(), bath.read(_stream())[place].tobytes())
    bath.close()
    verlet.close()
    ws.close()
    return out


def test_a_systems_bytes_do_not_depend_on_its_place_or_on_the_run():
    rng = np.random.default_rng(7)
    subject = _system(513, rng, n_forces=2)
    subject_bath = _bath(rng.uniform(0.05, 0.4, 513), 3.0e-4, 0x1234567890ABCDEF)
    fillers = []
    for k in range(39):
        n = int(rng.choice([1, 64, 300, 513, 700]))
        fillers.append((_system(n, rng), _bath(rng.uniform(0.05, 0.4, n), 5.0e-4, mirror.item_key(3, k))))
    alone = _run_placed(subject, subject_bath, [], 0)
    state = np.frombuffer(alone[2], dtype=_capi.bath_state_dtype())[0]
    assert (int(state["draws"]), int(state["coupled"])) == (3, 513) and float(state["reservoir"]) != 0.0
    assert _run_placed(subject, subject_bath, [], 0) == alone                # run twice
    assert _run_placed(subject, subject_bath, fillers, 0) == alone           # first of 40
    assert _run_placed(subject, subject_bath, fillers, 39) == alone          # last of 40


# ---- 3. items without a bath --------------------------------------------------------------------------------------------------
def test_items_without_a_bath_get_the_bytes_of_the_integrators_step_two():
    rng = np.random.default_rng(8)
    sizes = (1, 65, 513, 1025, 300)
    systems = [_system(n, rng, n_forces=(1, 4, 2, 3, 1)[k], langevin=(0, -1, 512, 7, -1)[k]) for k, n in enumerate(sizes)]
    gammas = (None, np.zeros(65), None, np.full(1025, -1.0), np.full(300, np.nan))      # NULL, or no gamma_j > 0
    baths = [_bath(g, 3.0e-4, mirror.item_key(1, k)) for k, g in enumerate(gammas)]
    sides = []
    for with_bath in (False, True):
        dev = [_to_device(s, b) for s, b in zip(systems, baths)]
        ws = _capi.Workspace(1)
        verlet = _capi.Verlet(ws, [_item(s, d) for s, d in zip(systems, dev)])
        bath = _capi.Bath(verlet, [_bath_item(b, d) for b, d in zip(baths, dev)]) if with_bath else None
        torch.cuda.synchronize()
        verlet.accelerations(_stream())
        for step in range(2):
            rows = [_capi.verlet_input_make(0.5, 0.02, 3.0e-4, (0.3, -0.7, 0.9 - step)) for _ in systems]
            d_rows = torch.from_numpy(_rows_array(rows)).cuda()
            verlet.step_one(_stream(), d_rows.data_ptr())
            if with_bath:
                bath.step_two(_stream(), d_rows.data_ptr())
            else:
                verlet.step_two(_stream(), d_rows.data_ptr())
        sides.append(([_device_bytes(d) for d in dev], verlet.read(_stream()).tobytes()))
        if with_bath:
            got = bath.read(_stream())
            assert got["coupled"].tolist() == [0] * 5 and got["draws"].tolist() == [0, 2, 0, 2, 2]
            assert not got["reservoir"].view(np.uint64).any()
            bath.close()
        verlet.close()
        ws.close()
    assert sides[0] == sides[1]
    state = np.frombuffer(sides[1][1], dtype=_capi.verlet_state_dtype())
    assert state["steps"].tolist() == [2] * 5 and [r != 0.0 for r in state["langevin_reservoir"]] == [True, False, True, True, False]


# ---- 4. replay ------------------------------------------------------------------------------------------------------------------
def _replicas(seeds, rng_seed=42):
    out = []
    for seed in seeds:
        cfg = synthetic.config1(seed=seed)
        n = len(cfg["charge"])
        rng = np.random.default_rng(rng_seed)
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
        v0 = rng.normal(size=(n, 3)) * np.sqrt(3.167e-4 / mass)[:, None]
        out.append({"cfg": cfg, "N": n, "mass": mass, "v0": v0})
    return out


def _build(replicas, gammas_host, kT, seed):
    sysdefs, velocities = [], []
    for r in replicas:
        cfg = r["cfg"]
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        velocities.append(torch.from_numpy(np.concatenate([r["v0"], r["mass"][:, None]], axis=1)).cuda())
    forces = cavitymd.CavityForceBatch(sysdefs, [r["cfg"]["params"] for r in replicas])
    integrator = cavitymd.VerletBatch(forces, velocities, net_forces=True)
    gammas = [None if g is None else torch.from_numpy(g).cuda() for g in gammas_host]
    bath = cavitymd.LangevinBathBatch(integrator, gammas, kT, seed)
    return SimpleNamespace(sysdefs=sysdefs, velocities=velocities, forces=forces, integrator=integrator, bath=bath)


def _snapshot(b):
    torch.cuda.synchronize()
    out = []
    for k, sd in enumerate(b.sysdefs):
        pd = sd.getParticleData()
        out.append((pd.getPositions().cpu().numpy().tobytes(), pd.getImages().cpu().numpy().tobytes(),
                    b.velocities[k].cpu().numpy().tobytes(), b.integrator.accel[k].cpu().numpy().tobytes(),
                    b.integrator.net_forces[k].cpu().numpy().tobytes()))
    return out


def _host_system(b, k, r):
    pd = b.sysdefs[k].getParticleData()
    return {"N": r["N"], "box": tuple(r["cfg"]["box"]), "pos": pd.getPositions().cpu().numpy().copy(),
            "vel": b.velocities[k].cpu().numpy().copy(), "image": pd.getImages().cpu().numpy().copy(), "forces": None,
            "net": b.integrator.net_forces[k].cpu().numpy().copy(), "accel": b.integrator.accel[k].cpu().numpy().copy(), "langevin": -1,
            "steps": 0, "out_of_box": 0, "reservoir": np.float64(0.0)}


def test_captured_step_replays_like_the_eager_one():
    B, REPLAYS, KT, SEED = 3, 200, 3.167e-4, 2024
    replicas = _replicas([11, 12, 13])
    rng = np.random.default_rng(6)
    gammas = [rng.uniform(1e-4, 1e-3, r["N"]) * r["mass"] for r in replicas]    # x = gamma dt / 2 m of order 1e-3
    gammas[1][::2] = 0.0                                                       # a filter: every other particle
    gammas[2] = gammas[2][:300]
    built = [_build(replicas, gammas, KT, SEED) for _ in range(2)]
    rows = np.zeros((REPLAYS, B, 8))
    for r in range(REPLAYS):
        rows[r] = _rows_array([_capi.verlet_input_make(rng.uniform(2.0, 6.0)) for _ in range(B)])
    d_rows = torch.from_numpy(rows).cuda()
    for b in built:
        b.forces.compute()
        b.integrator.prime()
    torch.cuda.synchronize()

    # eager; the first three steps against the mirror, fed with the device's own forces
    e = built[0]
    hosts = [_host_system(e, k, r) for k, r in enumerate(replicas)]
    baths = [_bath(g, KT, mirror.item_key(SEED, k)) for k, g in enumerate(gammas)]
    assert e.bath.keys == [b["seed"] for b in baths]
    for r in range(REPLAYS):
        e.integrator.inputs.copy_(d_rows[r])
        e.integrator.step_one()
        e.forces.compute()
        before = e.bath.state() if r < 3 else None
        e.bath.step_two()
        if r < 3:
            got, state = e.bath.state(), e.integrator.state()
            for k, s in enumerate(hosts):
                row = SimpleNamespace(dt=rows[r, k, 0], langevin_gamma=0.0, langevin_coeff=0.0, uniform=(0.0, 0.0, 0.0), skip=0)
                mirror_step_one(s, row)
                s["forces"] = [e.forces.forces[k].cpu().numpy().copy()]
                result = mirror.mirror_bath_step_two(s, row, baths[k])
                pd = e.sysdefs[k].getParticleData()
                assert _same(pd.getPositions().cpu().numpy(), s["pos"]) and _same(e.velocities[k].cpu().numpy(), s["vel"]), (r, k)
                assert _same(e.integrator.accel[k].cpu().numpy(), s["accel"]), (r, k)
                assert _same(e.integrator.net_forces[k].cpu().numpy(), s["net"]), (r, k)
                assert int(state[k]["steps"]) == s["steps"] == r + 1
                _assert_bath_state(got[k], before[k], baths[k], result, row.dt, ("eager", r, k))
    want = _snapshot(e)
    want_state, want_bath = e.integrator.state(), e.bath.state()

    # captured: the input rows rewritten in stream order before every replay
    c = built[1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.integrator.step_one()
        c.forces.compute()
        c.bath.step_two()
    assert c.bath.state()["draws"].tolist() == [0] * B                         # capturing ran nothing
    for r in range(REPLAYS):
        c.integrator.inputs.copy_(d_rows[r])
        graph.replay()
    assert _snapshot(c) == want
    state, got = c.integrator.state(), c.bath.state()
    assert state.tobytes() == want_state.tobytes() and got.tobytes() == want_bath.tobytes()
    assert got["draws"].tolist() == [REPLAYS] * B == [200] * B and state["steps"].tolist() == [REPLAYS] * B
    assert got["coupled"].tolist() == [501, 250, 300] and np.all(got["reservoir"] != 0.0) and state["out_of_box"].tolist() == [0] * B
    # after a reset the same variates come again: draws restarts at 0
    c.bath.reset()
    c.integrator.inputs.copy_(d_rows[0])
    graph.replay()
    assert c.bath.state()["draws"].tolist() == [1] * B
    for b in built:
        b.bath.close()
        b.integrator.close()
        b.forces.close()


# ---- 5. the bath thermalises free particles -----------------------------------------------------------------------------------
PARAMS = {"omegac": 9.1e-3, "couplstr": 1e-3, "phmass": 1.0}


def test_the_bath_thermalises_free_particles_from_one_graph():
    sizes, total = twin.SIZES, twin.PARTICLES
    assert sizes == (1, 2, 513) and total == 516
    rng = np.random.default_rng(3)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    vel0 = np.zeros((total, 4))
    vel0[:, 3] = twin.MASS
    d_vel = torch.from_numpy(vel0).cuda()                                    # all velocities are row-slices of ONE tensor
    sysdefs = []
    for n in sizes:                                                          # no type 'L' and zero charges: the no-photon path, zero forces
        pd = cavitymd.ParticleData.from_arrays(rng.uniform(-5.0, 5.0, (n, 3)), rng.integers(0, 2, n), np.zeros(n),
                                               np.zeros((n, 3), dtype=np.int32), ["O", "N"], twin.BOX, device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
    velocities = [d_vel[offsets[k]:offsets[k + 1]] for k in range(3)]
    forces = cavitymd.CavityForceBatch(sysdefs, PARAMS)
    integrator = cavitymd.VerletBatch(forces, velocities)
    gammas = [torch.full((n,), twin.GAMMA, dtype=torch.float64, device="cuda") for n in sizes]
    bath = cavitymd.LangevinBathBatch(integrator, gammas, twin.KT, seed=20241019)
    tags0 = [_u64(sd.getParticleData().getPositions().cpu().numpy()[:, 3]).copy() for sd in sysdefs]
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")                 # sums of v_c^2: [after two, after one]

    def tally(slot):
        v = d_vel[:, :3]
        acc[slot] += (v * v).sum()

    forces.compute()                                                         # once: the no-photon path writes zeros
    integrator.prime()
    integrator.set_inputs(twin.DT)                                           # a fixed dt, no row bath
    tally(0)
    tally(1)
    torch.cuda.synchronize()
    assert all(not f.cpu().numpy().view(np.uint64).any() for f in forces.forces)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        integrator.step_one()
        tally(1)
        bath.step_two()
        tally(0)
    for _ in range(twin.BURN_IN):
        graph.replay()
    acc.zero_()
    start = bath.state()["reservoir"].copy()                                 # behind the burn-in replays
    for _ in range(twin.COUNTED):
        graph.replay()
    got, state = bath.state(), integrator.state()
    sums = acc.cpu().numpy()
    gain = got["reservoir"] - start
    ratios = twin.ratios(sums[0], sums[1], 3 * total * twin.COUNTED, float(gain.sum()) / total, twin.COUNTED)
    print(f"\nmeasured / closed form: after step two {ratios[0]:.5f}, after step one {ratios[1]:.5f}; reservoir gain / pre-kick "
          f"growth {ratios[2]:+.6f}; band {twin.BAND} around {twin.EXPECTED}")
    print(f"reservoir ratio by system size: "
          f"{ {n: float(gain[k]) / n / twin.COUNTED / twin.closed_forms()[2] for k, n in enumerate(sizes)} }")
    assert all(band > 0.0 for band in twin.BAND)
    assert twin.EXPECTED == (1.0, 1.0, 0.0)
    assert np.all(np.abs(ratios - np.asarray(twin.EXPECTED)) <= np.asarray(twin.BAND)), (ratios.tolist(), twin.BAND)
    assert got["draws"].tolist() == [twin.BURN_IN + twin.COUNTED] * 3 == [576] * 3 and got["coupled"].tolist() == list(sizes)
    assert state["steps"].tolist() == [576] * 3 and state["out_of_box"].tolist() == [0] * 3
    # every system's own gain is the half-step kinetic energy its n particles lost between the two ends: mean 0, standard
    # deviation sqrt(n) twin.member_sd() however many steps lie between (langevin_twin's (4)); twelve of them, because one or two
    # particles' energies have exponential tails (tests/test_gpu_langevin_batch.py).  A pre-kick tally gains n * 512 steps of
    # closed_forms()[2], 768 n kT / (1 - x) against this bound of 17 sqrt(n) kT / (1 - x).
    bound = 12.0 * twin.member_sd() * np.sqrt(np.asarray(sizes, dtype=np.float64))
    print(f"|gain| by system {np.abs(gain).tolist()}, bounds {bound.tolist()}")
    assert np.all(np.abs(gain) <= bound) and np.all(gain != 0.0) and np.isfinite(got["reservoir"]).all()
    assert not state["langevin_reservoir"].view(np.uint64).any()             # the row's bath never ran
    vel = d_vel.cpu().numpy()
    assert np.all(vel[:, :3] != 0.0) and _same(vel[:, 3], vel0[:, 3])        # masses and type tags keep their bits
    for k, sd in enumerate(sysdefs):
        assert np.array_equal(_u64(sd.getParticleData().getPositions().cpu().numpy()[:, 3]), tags0[k]), k
    bath.close()
    integrator.close()
    forces.close()


# ---- 6. refusals and lifetime -------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime_on_the_device():
    rng = np.random.default_rng(9)
    systems = [_system(n, rng) for n in (65, 300)]
    baths = [_bath(np.full(s["N"], 0.1), 3.0e-4, mirror.item_key(4, k)) for k, s in enumerate(systems)]
    dev = [_to_device(s, b) for s, b in zip(systems, baths)]
    ws = _capi.Workspace(1)
    verlet = _capi.Verlet(ws, [_item(s, d) for s, d in zip(systems, dev)])
    lib = verlet._lib
    items = [_bath_item(b, d) for b, d in zip(baths, dev)]
    # n_items different from the integrator's
    for wrong in (items[:1], items + items[:1]):
        with pytest.raises(_capi.CavmdError) as e:
            _capi.Bath(verlet, wrong)
        assert e.value.status == INV
    bath = _capi.Bath(verlet, items)
    d_rows = torch.from_numpy(_rows_array([_capi.verlet_input_make(0.5) for _ in systems])).cuda()
    torch.cuda.synchronize()
    verlet.accelerations(_stream())
    # while a bath lives the integrator is not destroyed, frees nothing, and still steps afterwards
    assert lib.cavmd_verlet_destroy(verlet.handle) == INV
    verlet.step_one(_stream(), d_rows.data_ptr())
    bath.step_two(_stream(), d_rows.data_ptr())
    assert verlet.read(_stream())["steps"].tolist() == [1, 1] and bath.read(_stream())["draws"].tolist() == [1, 1]
    # the argument checks of the integrator's step two
    with pytest.raises(_capi.CavmdError):
        bath.step_two(_stream(), 0)
    with pytest.raises(_capi.CavmdError):
        bath.step_two(_stream(), d_rows.data_ptr() + 4)
    # set_items and read are refused during a capture of the stream the bath last launched on; the refusal changes nothing
    before = bath.read(_stream()).tobytes()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bath.step_two(_stream(), d_rows.data_ptr())
        with pytest.raises(_capi.CavmdError) as e:
            bath.set_items(0, items[:1])
        assert e.value.status == INV
        with pytest.raises(_capi.CavmdError) as e:
            bath.read(_stream())
        assert e.value.status == INV
        with pytest.raises(_capi.CavmdError) as e:
            verlet.set_items(0, [_item(systems[0], dev[0])])                 # the integrator noted the bath's stream
        assert e.value.status == INV
    torch.cuda.synchronize()
    assert bath.read(_stream()).tobytes() == before                          # capturing ran nothing, the refusals changed nothing
    graph.replay()
    torch.cuda.synchronize()
    assert bath.read(_stream())["draws"].tolist() == [2, 2]
    # set_items: no bath on item 0, a shorter one on item 1; the states are kept and the next step follows the new table
    g_new = torch.full((10,), 0.2, dtype=torch.float64, device="cuda")
    bath.set_items(0, [_capi.bath_item(0, 0, 3.0e-4, 1), _capi.bath_item(g_new.data_ptr(), 10, 3.0e-4, 2)])
    kept = bath.read(_stream())
    assert kept["draws"].tolist() == [2, 2]
    bath.step_two(_stream(), d_rows.data_ptr())
    got = bath.read(_stream())
    assert got["draws"].tolist() == [2, 3] and got["coupled"].tolist() == [int(kept["coupled"][0]), 10]
    assert got[0].tobytes() == kept[0].tobytes()
    # reset zeroes the states, draws included
    bath.reset(_stream())
    assert bath.read(_stream()).tobytes() == bytes(64)
    # destroy order: bath, then integrator, then workspace
    assert lib.cavmd_destroy(ws.handle) == INV
    assert lib.cavmd_verlet_destroy(verlet.handle) == INV
    bath.close()
    assert lib.cavmd_destroy(ws.handle) == INV                               # the integrator still lives
    verlet.close()
    ws.close()


def test_set_gammas_is_followed_by_the_next_step():
    replicas = _replicas([21, 22])
    gammas = [np.full(r["N"], 0.5) for r in replicas]
    b = _build(replicas, gammas, 3.167e-4, 5)
    assert b.bath.keys == [mirror.item_key(5, 0), mirror.item_key(5, 1)]
    b.forces.compute()
    b.integrator.prime()
    b.integrator.set_inputs(2.0)
    b.integrator.step_one()
    b.bath.step_two()
    assert b.bath.state()["coupled"].tolist() == [501, 501]
    every_other = torch.zeros(501, dtype=torch.float64, device="cuda")
    every_other[::2] = 0.5
    b.bath.set_gammas(1, [every_other])
    b.integrator.step_one()
    b.bath.step_two()
    got = b.bath.state()
    assert got["coupled"].tolist() == [501, 251] and got["draws"].tolist() == [2, 2]
    b.bath.set_gammas(0, [None, None])
    b.integrator.step_one()
    b.bath.step_two()
    after = b.bath.state()
    assert after.tobytes() == got.tobytes() and b.integrator.state()["steps"].tolist() == [3, 3]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b.bath.set_gammas(0, [torch.zeros(501, dtype=torch.float64)])
    seeds = cavitymd.LangevinBathBatch(b.integrator, [None, every_other], [1e-4, 2e-4], seeds=[7, 9])
    assert seeds.keys == [7, 9]
    seeds.close()
    seeds.close()                                                            # idempotent
    b.bath.close()
    b.integrator.close()
    with pytest.raises(RuntimeError, match="used after close"):
        cavitymd.LangevinBathBatch(b.integrator, [None, None], 1.0, 3)
    b.forces.close()
