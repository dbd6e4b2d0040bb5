"""cavmd_draw_fill / StepDraw on the device: the step inputs of a batch drawn by ONE kernel, against the numpy restatement of
its contract (tests/draw_mirror.py).  Bit for bit where the contract is IEEE arithmetic (the generator, the uniforms, dt, the
Langevin coefficient, the counters, every fixed-mode column); inside the mirror's derived bound where log, exp or cospi enter
(the normal, the gamma variate, the adaptive c, a ramped tolerance)."""
import ctypes

import numpy as np
import pytest
import torch

import cavitymd
import draw_mirror as mirror
from cavitymd import _capi, synthetic
from gpu_support import same as _same
from gpu_support import stream as _stream

pytestmark = pytest.mark.gpu

INV = _capi.CAVMD_ERR_INVALID_VALUE
SENTINEL = 7.0
DOFS = (0.0, 1.0, 2.0, 3.0, 1293.0)
MODES = ("fixed", "fixed_tau0", "fixed_gamma0", "fixed_dt0", "no_rows_yet", "adaptive", "S_zero", "S_negative", "S_nan", "S_inf",
         "clamp_min", "clamp_max", "ramp", "adaptive_dt0")
ADAPTIVE = MODES.index("no_rows_yet")          # modes from here on read the recorder's series


class Tables:
    """the two input tables, a recorder's series and row counters as a test plants them: plain device tensors"""

    def __init__(self, B, capacity=4):
        self.B, self.capacity = B, capacity
        self.verlet = torch.full((B, 8), SENTINEL, dtype=torch.float64, device="cuda")
        self.bussi = torch.full((B, 8), SENTINEL, dtype=torch.float64, device="cuda")
        self.records = torch.zeros((B, capacity, 16), dtype=torch.float64, device="cuda")
        self.rows = torch.zeros(B, dtype=torch.int64, device="cuda")

    def plant(self, recorded, S):
        """item i has `recorded[i]` rows; its last one carries S[i], every other slot something else"""
        rec = np.full((self.B, self.capacity, 16), 123.0)
        slot = (np.maximum(recorded.astype(np.int64), 1) - 1) % self.capacity
        rec[np.arange(self.B), slot, 14] = S
        self.records.copy_(torch.from_numpy(rec))
        self.rows.copy_(torch.from_numpy(recorded.astype(np.int64)))

    def item(self, k, it, adaptive, verlet=True, bussi=True):
        return _capi.draw_item(self.verlet[k].data_ptr() if verlet else 0, self.bussi[k].data_ptr() if bussi else 0,
                               gamma=it["gamma"][k], kT=it["kT"][k], set_T=it["set_T"][k], tau=it["tau"][k], dof=it["dof"][k],
                               dt=it["dt_initial"][k], records_ptr=self.records[k].data_ptr() if adaptive[k] else 0,
                               rows_ptr=self.rows[k:].data_ptr() if adaptive[k] else 0, capacity=self.capacity if adaptive[k] else 0,
                               tolerance=it["tol_target"][k], tolerance_initial=it["tol_initial"][k],
                               tolerance_time_constant=it["tol_time_constant"][k], dt_min=it["dt_min"][k], dt_max=it["dt_max"][k])


def _state_dict(state):
    return {name: state[name].copy() for name in ("draws", "dt", "elapsed", "tolerance", "exhausted")}


def _plain_items(B, rng, dofs=DOFS):
    """B items of ordinary constants, all in fixed mode"""
    it = dict(gamma=rng.uniform(1e-3, 1e-2, B), kT=rng.uniform(3e-4, 1e-3, B), set_T=rng.uniform(3e-4, 1e-3, B),
              tau=rng.uniform(50.0, 500.0, B), dof=np.array([dofs[k % len(dofs)] for k in range(B)]),
              dt_initial=rng.uniform(2.0, 6.0, B), tol_target=np.zeros(B), tol_initial=np.zeros(B), tol_time_constant=np.zeros(B),
              dt_min=np.zeros(B), dt_max=np.zeros(B))
    return it, np.zeros(B, dtype=bool)


# ---- 1. one ragged table against the mirror -------------------------------------------------------------------------------------
def _ragged_table(B, rng):
    """Items cycle through MODES (i % 14), the dofs (i % 5) and the destinations ((i // 14) % 3: integrator row alone,
    thermostat row alone, both).  -> it, adaptive, mode, per launch (recorded, S)."""
    it, _ = _plain_items(B, rng)
    mode = np.arange(B) % len(MODES)
    adaptive = mode >= ADAPTIVE
    it["tau"][mode == MODES.index("fixed_tau0")] = 0.0
    it["gamma"][mode == MODES.index("fixed_gamma0")] = 0.0
    it["dt_initial"][mode == MODES.index("fixed_dt0")] = 0.0
    it["tau"][(mode == MODES.index("adaptive")) & (np.arange(B) % 3 == 0)] = 0.0          # tau 0 and gamma 0 in adaptive mode too
    it["gamma"][(mode == MODES.index("adaptive")) & (np.arange(B) % 3 == 1)] = 0.0
    it["tol_target"][adaptive] = rng.uniform(1e-3, 2e-3, adaptive.sum())
    it["tol_initial"][adaptive] = it["tol_target"][adaptive] * 0.1
    it["dt_min"][adaptive], it["dt_max"][adaptive] = 0.5, 50.0
    it["tol_time_constant"][mode == MODES.index("ramp")] = 20.0
    last = mode == MODES.index("adaptive_dt0")
    it["dt_min"][last] = it["dt_max"][last] = 0.0
    launches = []
    for launch, rows in enumerate((1, 6, 4)):                      # with capacity 4: slots 0, 1 and 3
        recorded = np.full(B, rows, dtype=np.uint64)
        recorded[mode == MODES.index("no_rows_yet")] = 0
        S = it["tol_target"] / rng.uniform(2.0, 6.0, B) ** 2       # sqrt(tolerance / S) between 2 and 6, inside the clamp
        S[~adaptive] = 1.0
        if launch > 0:                                             # the first launch leaves a dt that is not dt_initial behind
            S[mode == MODES.index("S_zero")] = 0.0 if launch == 1 else -0.0
            S[mode == MODES.index("S_negative")] = -1e-5
            S[mode == MODES.index("S_nan")] = np.nan
            S[mode == MODES.index("S_inf")] = np.inf
        S[mode == MODES.index("clamp_min")] = 1e6
        S[mode == MODES.index("clamp_max")] = 1e-12
        launches.append((recorded, S))
    return it, adaptive, mode, launches


def test_one_ragged_table_equals_the_mirror():
    """600 items, three launches.  The test prints, per launch, the largest error as a share of the mirror's bound, the
    number of items that met each planted case and the gamma draws left out as too close to call.  On an MI355X: at most
    0.09 of the bound for the normal, 0.22 for the gamma variate, 0.08 for the adaptive c; 0 of 702 gamma draws left out."""
    B, SEED = 600, 0x9E3779B97F4A7C15
    rng = np.random.default_rng(31)
    it, adaptive, mode, launches = _ragged_table(B, rng)
    dest = (np.arange(B) // len(MODES)) % 3
    to_verlet, to_bussi = dest != 1, dest != 0
    t = Tables(B)
    ws = _capi.Workspace(1)
    draw = _capi.Draw(ws, SEED, [t.item(k, it, adaptive, to_verlet[k], to_bussi[k]) for k in range(B)])
    assert draw.launch_order == list(range(B))
    st = mirror.new_state(B)
    hit = dict.fromkeys(("verlet_alone", "bussi_alone", "both", "tau0", "gamma0", "fixed", "adaptive", "rows_0", "S_zero", "S_negative",
                         "S_nan", "S_inf", "last_dt_kept", "clamp_min", "clamp_max", "skip", "ramp", "normal", "no_normal", "gamma",
                         "no_gamma", "gamma_small_shape", "gamma_checked", "gamma_left_out"), 0)
    for recorded, S in launches:
        t.plant(recorded, S)
        draw.fill(_stream())
        dev = _state_dict(draw.read(_stream()))
        verlet, bussi = t.verlet.cpu().numpy(), t.bussi.cpu().numpy()
        # the mirror takes the device's ramped tolerance, so that dt and what follows from it are compared bit for bit; the
        # tolerance itself is held to the mirror's own below
        want_v, want_b, new, info = mirror.step(SEED, it, st, adaptive, recorded, S, tolerance=dev["tolerance"])
        # the integrator row: every word bit for bit
        assert _same(verlet[to_verlet], want_v[to_verlet])
        assert (verlet[~to_verlet] == SENTINEL).all()                                       # 2. untouched bytes
        u = verlet[to_verlet][:, 3:6]
        assert (u >= -1.0).all() and (u < 1.0).all()
        # the thermostat row: set_T, skip, reserved and the fixed-mode c bit for bit; the variates and the adaptive c in the bound
        got, want = bussi[to_bussi], want_b[to_bussi]
        assert (bussi[~to_bussi] == SENTINEL).all()
        assert _same(got[:, 3:], want[:, 3:])
        fixed = ~adaptive[to_bussi]
        assert _same(got[fixed, 2], want[fixed, 2])
        assert (np.abs(got[:, 2] - want[:, 2]) <= info["c_bound"][to_bussi]).all()
        assert _same(got[it["tau"][to_bussi] == 0.0, 2], np.zeros(int((it["tau"][to_bussi] == 0.0).sum())))
        print("largest |c - mirror| / bound:", np.max(np.abs(got[~fixed, 2] - want[~fixed, 2]) / info["c_bound"][to_bussi][~fixed].clip(1e-300)))
        nb = info["normal_bound"][to_bussi]
        print("largest |normal - mirror| / bound:", np.max(np.abs(got[:, 0] - want[:, 0])[nb > 0] / nb[nb > 0]))
        assert (np.abs(got[:, 0] - want[:, 0]) <= nb).all()
        assert _same(got[it["dof"][to_bussi] == 0.0, 0], np.zeros(int((it["dof"][to_bussi] == 0.0).sum())))
        check = ~info["gamma_ambiguous"][to_bussi]
        gb = info["gamma_bound"][to_bussi]
        print("largest |gamma - mirror| / bound:", np.max((np.abs(got[:, 1] - want[:, 1]) / gb.clip(1e-300))[check & (gb > 0)]))
        assert (np.abs(got[:, 1] - want[:, 1]) <= gb)[check].all()
        assert _same(got[it["dof"][to_bussi] <= 1.0, 1], np.zeros(int((it["dof"][to_bussi] <= 1.0).sum())))
        # the state
        assert (dev["draws"] == new["draws"]).all() and _same(dev["dt"], new["dt"]) and _same(dev["elapsed"], new["elapsed"])
        assert (dev["exhausted"] == 0).all()
        ramp = adaptive & (it["tol_time_constant"] != 0.0)
        assert _same(dev["tolerance"][~ramp], info["own_tolerance"][~ramp])
        assert (np.abs(dev["tolerance"] - info["own_tolerance"]) <= info["tolerance_bound"]).all()
        assert (dev["tolerance"][ramp] != it["tol_target"][ramp]).all()
        # which planted cases this launch met
        usable = adaptive & (recorded != 0) & (S > 0) & np.isfinite(S)
        kept = adaptive & (recorded != 0) & ~usable
        for name, n in (("verlet_alone", (dest == 0).sum()), ("bussi_alone", (dest == 1).sum()), ("both", (dest == 2).sum()),
                        ("tau0", (it["tau"] == 0).sum()), ("gamma0", (it["gamma"] == 0).sum()), ("fixed", (~adaptive).sum()),
                        ("adaptive", usable.sum()), ("rows_0", (adaptive & (recorded == 0)).sum()),
                        ("S_zero", (kept & (S == 0)).sum()), ("S_negative", (kept & (S < 0)).sum()), ("S_nan", (kept & np.isnan(S)).sum()),
                        ("S_inf", (kept & np.isinf(S)).sum()),
                        ("last_dt_kept", (kept & (new["dt"] == st["dt"]) & (new["dt"] != it["dt_initial"])).sum()),
                        ("clamp_min", (usable & (new["dt"] == it["dt_min"]) & (it["dt_max"] > 0)).sum()),
                        ("clamp_max", (usable & (new["dt"] == it["dt_max"]) & (it["dt_max"] > 0)).sum()),
                        ("skip", (new["dt"] == 0).sum()), ("ramp", ramp.sum()),
                        ("normal", (to_bussi & (it["dof"] != 0)).sum()), ("no_normal", (to_bussi & (it["dof"] == 0)).sum()),
                        ("gamma", (to_bussi & (it["dof"] > 1)).sum()), ("no_gamma", (to_bussi & (it["dof"] <= 1)).sum()),
                        ("gamma_small_shape", (to_bussi & (it["dof"] > 1) & (it["dof"] < 3)).sum()),
                        ("gamma_checked", (to_bussi & (it["dof"] > 1) & ~info["gamma_ambiguous"]).sum()),
                        ("gamma_left_out", (to_bussi & info["gamma_ambiguous"]).sum())):
            hit[name] += int(n)
        st = new
    print("cases met:", hit)
    left_out = hit.pop("gamma_left_out")
    print("gamma draws left out as too close to call:", left_out, "of", hit["gamma"])
    assert left_out * 10000 <= hit["gamma"]
    assert all(n > 0 for n in hit.values()), hit
    assert (st["draws"] == 3).all()
    draw.close()
    ws.close()


def test_the_mirror_leaves_out_at_most_one_draw_in_ten_thousand():
    """On the CPU alone, for the seed of the test above and far more draws than it makes: the share of gamma draws whose
    acceptance is too close to call stays under 1 in 10^4."""
    n = 200000
    draws, item = np.arange(n, dtype=np.uint64) % np.uint64(3), np.arange(n, dtype=np.uint64) // np.uint64(3)
    for dof in (2.0, 3.0, 1293.0):
        g = mirror.gamma(0x9E3779B97F4A7C15, draws, item, np.full(n, (dof - 1.0) / 2.0))
        assert g["ambiguous"].sum() * 10000 <= n, (dof, g["ambiguous"].sum())


# ---- 2. untouched bytes ---------------------------------------------------------------------------------------------------------
def test_set_items_moves_rows_and_leaves_the_rest_alone():
    """(a NULL destination's row is checked in the ragged test)  Items 2 .. 4 are pointed at another pair of tables: a launch
    then writes those rows there and nowhere else; their states are kept."""
    B = 7
    it, adaptive = _plain_items(B, np.random.default_rng(2))
    a, b = Tables(B), Tables(B)
    ws = _capi.Workspace(1)
    draw = _capi.Draw(ws, 5, [a.item(k, it, adaptive) for k in range(B)])
    draw.fill(_stream())
    first = draw.read(_stream())
    assert (a.verlet.cpu().numpy() != SENTINEL).any(axis=1).all() and (a.bussi.cpu().numpy() != SENTINEL).any(axis=1).all()
    a.verlet.fill_(SENTINEL)
    a.bussi.fill_(SENTINEL)
    draw.set_items(2, [b.item(k, it, adaptive) for k in range(2, 5)])
    draw.fill(_stream())
    state = draw.read(_stream())
    moved = np.zeros(B, dtype=bool)
    moved[2:5] = True
    for table_a, table_b in ((a.verlet, b.verlet), (a.bussi, b.bussi)):
        ta, tb = table_a.cpu().numpy(), table_b.cpu().numpy()
        assert (ta[moved] == SENTINEL).all() and (tb[~moved] == SENTINEL).all()
        assert (ta[~moved, 0] != SENTINEL).all() and (tb[moved, 0] != SENTINEL).all()
    assert (first["draws"] == 1).all() and (state["draws"] == 2).all()                      # the states are kept
    want_v, want_b, _, _ = mirror.step(5, it, _state_dict(first), adaptive, np.zeros(B, dtype=np.uint64), np.zeros(B))
    assert _same(b.verlet.cpu().numpy()[moved], want_v[moved]) and _same(a.verlet.cpu().numpy()[~moved], want_v[~moved])
    with pytest.raises(_capi.CavmdError):
        draw.set_items(5, [b.item(k, it, adaptive) for k in range(2, 5)])                  # leaves the table
    draw.close()
    ws.close()


# ---- 3. replay ------------------------------------------------------------------------------------------------------------------
def test_two_hundred_replays_equal_two_hundred_eager_launches():
    B, REPLAYS, SEED = 70, 200, 77
    rng = np.random.default_rng(8)
    it, adaptive = _plain_items(B, rng)
    adaptive[::2] = True                                            # every other item follows a planted series
    it["tol_target"][:] = 1e-3
    it["tol_initial"][:] = 1e-4
    it["tol_time_constant"][::4] = 300.0                            # half of those with a ramp
    it["dt_min"][:], it["dt_max"][:] = 0.5, 50.0
    recorded, S = np.full(B, 3, dtype=np.uint64), 1e-3 / rng.uniform(2.0, 6.0, B) ** 2
    runs = []
    for seed in (SEED, SEED, SEED + 1):
        t = Tables(B)
        t.plant(recorded, S)
        ws = _capi.Workspace(1)
        runs.append((t, ws, _capi.Draw(ws, seed, [t.item(k, it, adaptive) for k in range(B)])))
    torch.cuda.synchronize()

    # eager
    t, _, draw = runs[0]
    want = torch.zeros((REPLAYS, 2, B, 8), dtype=torch.float64, device="cuda")
    for r in range(REPLAYS):
        draw.fill(_stream())
        want[r, 0].copy_(t.verlet)
        want[r, 1].copy_(t.bussi)
    want_state = draw.read(_stream())

    # captured once, replayed: the rows of every replay kept in a device log by copies inside the graph
    t, _, draw = runs[1]
    log = torch.zeros((REPLAYS + 1, 2, B, 8), dtype=torch.float64, device="cuda")   # one row more: the replay after the reset
    at = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        draw.fill(_stream())
        at += 1
        log.index_copy_(0, at, torch.stack([t.verlet, t.bussi]).unsqueeze(0))
    assert draw.read(_stream())["draws"].tolist() == [0] * B       # capturing ran nothing
    for _ in range(REPLAYS):
        graph.replay()
    state = draw.read(_stream())
    assert torch.equal(log[:REPLAYS].view(torch.int64), want.view(torch.int64))
    assert state.tobytes() == want_state.tobytes()
    assert state["draws"].tolist() == [REPLAYS] * B and (state["exhausted"] == 0).all()
    rows = log[:REPLAYS].cpu().numpy()
    assert _same(state["elapsed"], np.add.accumulate(rows[:, 0, :, 0], axis=0)[-1])          # the left-to-right sum of every dt
    # no (item, replay) block of uniforms repeats, within an item or across items
    blocks = rows[:, 0, :, 3:6].reshape(-1, 3)
    assert len(np.unique(blocks, axis=0)) == REPLAYS * B
    assert len(np.unique(blocks.ravel())) == 3 * REPLAYS * B
    assert len(np.unique(rows[:, 1, :, 0][:, it["dof"] != 0.0].ravel())) == REPLAYS * int((it["dof"] != 0.0).sum())
    # the block is a function of (seed, draws, item): an item's first block is the mirror's for ITS index and no other's
    first = mirror.langevin_uniforms(SEED, 0, np.arange(B, dtype=np.uint64))
    assert _same(rows[0, 0, :, 3:6], first) and not (first[1:] == first[:-1]).any()
    # another seed: other blocks
    t, _, other = runs[2]
    other.fill(_stream())
    torch.cuda.synchronize()
    assert not (t.verlet.cpu().numpy()[:, 3:6] == rows[0, 0, :, 3:6]).any()
    # a replay after a reset draws the first block again
    runs[1][2].reset(_stream())
    graph.replay()
    torch.cuda.synchronize()
    assert _same(runs[1][0].verlet.cpu().numpy()[:, 3:6], first)
    for _, ws, d in runs:
        d.close()
        ws.close()


# ---- 4. moments on the device ---------------------------------------------------------------------------------------------------
def test_moments_on_the_device():
    """Mean and variance inside 6 standard errors of the analytic values (the variance of a sample variance is
    (mu4 - sigma^4) / n: 2 / n for the normal, (2 a^2 + 6 a) / n for gamma(a), (1/5 - 1/9) / n for a uniform in [-1, 1))."""
    B, LAUNCHES = 4096, 64
    shapes = (0.5, 1.0, 646.0)
    it, adaptive = _plain_items(B, np.random.default_rng(4), dofs=tuple(2.0 * a + 1.0 for a in shapes))
    t = Tables(B, capacity=1)
    ws = _capi.Workspace(1)
    draw = _capi.Draw(ws, 20240229, [t.item(k, it, adaptive) for k in range(B)])
    log = torch.zeros((LAUNCHES, 2, B, 8), dtype=torch.float64, device="cuda")
    for r in range(LAUNCHES):
        draw.fill(_stream())
        log[r, 0].copy_(t.verlet)
        log[r, 1].copy_(t.bussi)
    state = draw.read(_stream())
    assert (state["exhausted"] == 0).all() and (state["draws"] == LAUNCHES).all()
    rows = log.cpu().numpy()
    u = rows[:, 0, :, 3:6]
    n = u.size
    assert (u >= -1.0).all() and (u < 1.0).all()
    assert abs(u.mean()) < 6.0 * np.sqrt(1.0 / 3.0 / n), u.mean()
    assert abs(u.var() - 1.0 / 3.0) < 6.0 * np.sqrt((1.0 / 5.0 - 1.0 / 9.0) / n), u.var()
    for c in range(3):
        uc = u[:, :, c]
        assert abs(uc.mean()) < 6.0 * np.sqrt(1.0 / 3.0 / uc.size), (c, uc.mean())
        lag = uc[1:] * uc[:-1]                                     # lag-1 across launches, per item: mean 0, variance 1/9
        assert abs(lag.mean()) < 6.0 * (1.0 / 3.0) / np.sqrt(lag.size), (c, lag.mean())
    across = u[:, 1:, :] * u[:, :-1, :]                            # and across neighbouring items of one launch
    assert abs(across.mean()) < 6.0 * (1.0 / 3.0) / np.sqrt(across.size), across.mean()
    z = rows[:, 1, :, 0]
    assert abs(z.mean()) < 6.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 6.0 * np.sqrt(2.0 / z.size), (z.mean(), z.var())
    for k, a in enumerate(shapes):
        g = rows[:, 1, k::3, 1]
        assert (g > 0.0).all()
        assert abs(g.mean() - a) < 6.0 * np.sqrt(a / g.size), (a, g.mean())
        assert abs(g.var() - a) < 6.0 * np.sqrt((2.0 * a * a + 6.0 * a) / g.size), (a, g.var())
    draw.close()
    ws.close()


# ---- 5. the closed loop ---------------------------------------------------------------------------------------------------------
def test_the_adaptive_step_stays_on_the_device():
    """{fill, step_one, compute, step_two, record} captured and replayed: the dt of replay k is sqrt(tolerance / S) of the row
    the recorder wrote before it, taken with numpy's correctly rounded sqrt and /, and never visits the host."""
    REPLAYS = 50
    sizes = (2, 4, 10, 32, 64, 128, 256, 298)                      # N = 3 .. 299 with the photon
    B = len(sizes)
    sysdefs, velocities, params = [], [], []
    for k, n_mol in enumerate(sizes):
        cfg = synthetic.diatomic_box(n_mol, seed=k + 1, box_length=40.0)
        n = len(cfg["charge"])
        rng = np.random.default_rng(100 + k)
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
        v0 = rng.normal(size=(n, 3)) * np.sqrt(3.167e-4 / mass)[:, None]
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        velocities.append(torch.from_numpy(np.concatenate([v0, mass[:, None]], axis=1)).cuda())
        params.append(cfg["params"])
    photon = [n_mol for n_mol in sizes]                            # the photon is the last particle
    forces = cavitymd.CavityForceBatch(sysdefs, params)
    integrator = cavitymd.VerletBatch(forces, velocities, langevin_index=photon, net_forces=True)
    recorder = cavitymd.BatchRecorder(forces, velocities, net_forces=integrator.net_forces, capacity=64)
    forces.compute()
    integrator.prime()
    recorder.record()                                              # row 0: the S the first step's dt comes from
    S0 = recorder.read()["force_mass_sum"][:, 0]
    assert (S0 > 0.0).all()
    tolerance = 16.0 * S0                                          # a first dt of about 4, per system
    draw = cavitymd.StepDraw(2718, integrator, None, recorder, dt=1.0, gamma=1e-3, kT=3.167e-4, tolerance=tolerance, dt_min=0.0,
                             dt_max=1e3)
    assert draw.adaptive and draw.n_systems == B
    log = torch.zeros((REPLAYS, B, 8), dtype=torch.float64, device="cuda")
    at = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        draw.fill()
        at += 1
        log.index_copy_(0, at, integrator.inputs.unsqueeze(0))
        integrator.step_one()
        forces.compute()
        integrator.step_two()
        recorder.record()
    for _ in range(REPLAYS):
        graph.replay()
    series = recorder.read()                                       # read once: rows 0 .. REPLAYS
    state = draw.state()
    rows = log.cpu().numpy()
    S = series["force_mass_sum"]
    assert S.shape == (B, REPLAYS + 1) and (S > 0.0).all() and np.isfinite(S).all()
    want_dt = np.sqrt(tolerance[:, None] / S[:, :REPLAYS]).T        # replay k reads row k
    assert ((want_dt > 0.0) & (want_dt < 1e3)).all()               # the clamp is never met: the rule itself is what is compared
    assert _same(rows[:, :, 0], want_dt)
    assert len(np.unique(rows[:, :, 0])) > REPLAYS * B // 2        # and dt does move, per step and per system
    assert _same(rows[:, :, 2], np.sqrt(((6.0 * 1e-3) * 3.167e-4) / want_dt))
    elapsed = np.zeros(B)
    for k in range(REPLAYS):
        elapsed = elapsed + want_dt[k]
    assert _same(state["elapsed"], elapsed) and _same(state["dt"], want_dt[-1])
    assert state["draws"].tolist() == [REPLAYS] * B and _same(state["tolerance"], tolerance)
    assert integrator.state()["steps"].tolist() == [REPLAYS] * B
    assert (integrator.state()["out_of_box"] == 0).all()
    for owner in (draw, recorder, integrator, forces):
        owner.close()


# ---- 6. refusals and life cycle ------------------------------------------------------------------------------------------------
def test_refusals_and_life_cycle():
    B = 3
    rows = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    draw = cavitymd.StepDraw(1, integrator=rows, dt=2.0)
    with pytest.raises(TypeError, match="callable"):
        cavitymd.StepDraw(1, thermostat=rows, set_T=lambda step: 1.0, tau=1.0, dof=3.0, dt=2.0)
    with pytest.raises(ValueError, match="BatchRecorder"):
        cavitymd.StepDraw(1, integrator=rows, dt=2.0, tolerance=1e-3)
    d = draw.draw
    lib = d._lib
    item = [_capi.draw_item(rows[1].data_ptr(), 0, dt=3.0)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        draw.fill()
        with pytest.raises(_capi.CavmdError) as e:                             # the stream of the last launch is capturing
            d.set_items(1, item)
        assert e.value.status == INV
        with pytest.raises(_capi.CavmdError) as e:
            d.read(_stream())
        assert e.value.status == INV
    d.set_items(1, item)                                                       # outside the capture it goes through,
    graph.replay()                                                             # and the captured launch finds the new item
    state = draw.state()
    assert state["draws"].tolist() == [1] * B and state["dt"].tolist() == [2.0, 3.0, 2.0]
    assert rows.cpu().numpy()[:, 0].tolist() == [2.0, 3.0, 2.0]
    assert d.state_device_ptr() % 8 == 0 and d.state_device_ptr() == d.state_device_ptr()
    # destroying the workspace before its draw object is an error, and harmless
    assert lib.cavmd_destroy(draw.workspace.handle) == INV
    draw.fill()
    assert draw.state()["draws"].tolist() == [2] * B
    # a draw object released inside a capture is destroyed after it, before its workspace
    other = cavitymd.StepDraw(2, integrator=torch.zeros((B, 8), dtype=torch.float64, device="cuda"), dt=2.0)
    assert not _capi._deferred_children and not _capi._deferred
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        draw.fill()
        other.close()
        assert len(_capi._deferred_children) == 1 and len(_capi._deferred) == 1
    graph2.replay()
    assert draw.state()["draws"].tolist() == [3] * B
    _capi.Workspace(1).close()                                                 # outside a capture: the deferred ones go
    assert not _capi._deferred_children and not _capi._deferred
    draw.close()
    draw.close()                                                               # twice
    other.close()
    with pytest.raises(RuntimeError, match="used after close"):
        draw.fill()
