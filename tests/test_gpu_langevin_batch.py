"""The Langevin bath and the device-drawn inputs of ``cavitymd.VerletBatch`` on the GPU, and the examples that use them.  Run with
`-m gpu` on an MI355X.

tests/test_gpu_verlet_batch.py pins the kernels to a mirror of include/cavmd.h with hand-made input rows.  This file is what
that leaves open:
  1. ``draw_inputs`` fills the (B, 8) rows the kernels read: layout, range, cache, generators, the skip word;
  2. a captured ``draw_inputs`` gives fresh variates on every replay, with the moments of U[-1, 1);
  3. the bath IS a thermostat: free particles, stepped from one captured graph, reproduce the three closed forms (two
     temperatures, and a reservoir that gains nothing on average) of
     tests/langevin_twin.py within a band taken from the host twin (tests/test_langevin_twin.py), never from a GPU run;
  4. every file of examples/ runs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
import langevin_twin as twin
from cavitymd import _capi
from gpu_support import bits as _u64
from gpu_support import same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
PARAMS = {"omegac": 9.1e-3, "couplstr": 1e-3, "phmass": 1.0}


def _free_systems(sizes, langevin, seed):
    """Photon-less, uncharged systems: no type 'L' and zero charges, the force batch's no-photon path, which writes zeros.  All
    velocities are row-slices of ONE (sum N, 4) tensor.  Bath particles: at rest, mass twin.MASS.  The others: masses in [1, 4)
    and |v_c| <= 5e-3, so that 576 steps of dt = 4 move them 11.52 at most from |x_c| <= 5 in a box of +-20."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    vel = np.zeros((offsets[-1], 4))
    vel[:, :3] = rng.uniform(-5e-3, 5e-3, (offsets[-1], 3))
    vel[:, 3] = rng.uniform(1.0, 4.0, offsets[-1])
    bath_rows = np.array([offsets[k] + j for k, j in enumerate(langevin) if j >= 0], dtype=np.int64)
    vel[bath_rows] = (0.0, 0.0, 0.0, twin.MASS)
    d_vel = torch.from_numpy(vel).cuda()
    sysdefs = []
    for n in sizes:
        pd = cavitymd.ParticleData.from_arrays(rng.uniform(-5.0, 5.0, (n, 3)), rng.integers(0, 2, n), np.zeros(n),
                                               np.zeros((n, 3), dtype=np.int32), ["O", "N"], twin.BOX, device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
    velocities = [d_vel[offsets[k]:offsets[k + 1]] for k in range(len(sizes))]
    forces = cavitymd.CavityForceBatch(sysdefs, PARAMS)
    integrator = cavitymd.VerletBatch(forces, velocities, langevin_index=list(langevin))
    return {"sysdefs": sysdefs, "vel0": vel, "d_vel": d_vel, "velocities": velocities, "forces": forces, "integrator": integrator,
            "bath_rows": bath_rows, "offsets": offsets}


def _arrays(b, k) -> tuple:
    pd = b["sysdefs"][k].getParticleData()
    return (pd.getPositions().cpu().numpy().tobytes(), pd.getImages().cpu().numpy().tobytes(),
            b["velocities"][k].cpu().numpy().tobytes(), b["integrator"].accel[k].cpu().numpy().tobytes())


def _close(b) -> None:
    b["integrator"].close()
    b["forces"].close()


# ---- 1. draw_inputs, eagerly ------------------------------------------------------------------------------------------------
def _want_constants(dts, gammas, kTs) -> np.ndarray:
    """(B, 3): dt, gamma, coeff as cavmd_verlet_input_make gives them"""
    rows = [_capi.verlet_input_make(dt, g, kT) for dt, g, kT in zip(dts, gammas, kTs)]
    return np.array([[r.dt, r.langevin_gamma, r.langevin_coeff] for r in rows])


def _assert_rows(rows, dts, gammas, kTs):
    assert rows.shape == (len(dts), 8)
    assert _same(rows[:, :3], _want_constants(dts, gammas, kTs))
    u = rows[:, 3:6]
    assert np.isfinite(u).all() and np.all(u >= -1.0) and np.all(u < 1.0)
    assert (_u64(rows[:, 6]) != 0).tolist() == [dt == 0.0 for dt in dts]
    assert not _u64(rows[:, 7]).any()


def test_draw_inputs_fills_the_rows_on_the_device():
    B = 5
    dts = [4.0, 0.0, 2.0, 4.0, 1.0]
    gammas = [0.25, 0.25, 0.0, 0.1, 0.25]
    kTs = [3.167e-4, 3.167e-4, 1e-3, 2e-4, 5e-4]
    b = _free_systems([3, 3, 2, 300, 3], [2, 1, 0, 299, -1], seed=1)    # every system has a particle that moves
    integrator = b["integrator"]
    inputs = lambda: integrator.inputs.cpu().numpy().copy()                  # noqa: E731
    assert _u64(inputs()[:, 6]).all()                                        # before any inputs: every system is skipped

    integrator.draw_inputs(dts, gammas, kTs)
    first = inputs()
    _assert_rows(first, dts, gammas, kTs)
    assert first[2, 2] == 0.0 and first[1, 2] == 0.0 and np.all(first[[0, 3, 4], 2] > 0.0)   # no coefficient without gamma or dt
    integrator.draw_inputs(dts, gammas, kTs)
    second = inputs()
    _assert_rows(second, dts, gammas, kTs)
    assert np.all(second[:, 3:6] != first[:, 3:6])                           # every variate is new
    assert _same(second[:, :3], first[:, :3]) and _same(second[:, 6:], first[:, 6:])

    # another dt: the cached constants must follow (columns 0 and 2), and come back
    other = [2.0, 0.0, 2.0, 8.0, 0.5]
    integrator.draw_inputs(other, gammas, kTs)
    third = inputs()
    _assert_rows(third, other, gammas, kTs)
    changed = [0, 3, 4]
    assert np.all(third[changed, 0] != first[changed, 0]) and np.all(third[changed, 2] != first[changed, 2])
    integrator.draw_inputs(4.0, 0.25, 3.167e-4)                              # one number for all
    _assert_rows(inputs(), [4.0] * B, [0.25] * B, [3.167e-4] * B)
    integrator.draw_inputs(dts, gammas, kTs)
    _assert_rows(inputs(), dts, gammas, kTs)

    # two generators with one seed: identical rows; another seed: other variates
    drawn = []
    for seed in (7, 7, 8):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        integrator.draw_inputs(dts, gammas, kTs, generator=g)
        drawn.append(inputs())
        _assert_rows(drawn[-1], dts, gammas, kTs)
    assert _same(drawn[0], drawn[1])
    assert np.all(drawn[2][:, 3:6] != drawn[0][:, 3:6]) and _same(drawn[2][:, :3], drawn[0][:, :3])

    # a step with these rows: the system with dt == 0 (it has a moving bath particle and gamma != 0) is untouched
    b["d_vel"][torch.from_numpy(b["bath_rows"]).cuda(), :3] = 1e-3           # at rest the tally bd . v would be 0
    b["forces"].compute()
    integrator.prime()
    before = [_arrays(b, k) for k in range(B)]
    state0 = integrator.state()
    assert state0.tobytes() == bytes(32 * B)
    integrator.step_one()
    integrator.step_two()
    state = integrator.state()
    assert _arrays(b, 1) == before[1] and state[1].tobytes() == bytes(32)
    assert state["steps"].tolist() == [1, 0, 1, 1, 1] and state["out_of_box"].tolist() == [0] * B
    assert all(_arrays(b, k) != before[k] for k in (0, 2, 3, 4))
    # the bath ran where there is a bath particle and gamma != 0: systems 0 and 3 (2 has gamma == 0, 4 has no bath particle)
    assert [k for k in range(B) if state["langevin_reservoir"][k] != 0.0] == [0, 3]
    _close(b)


# ---- 2. a captured draw -----------------------------------------------------------------------------------------------------
def test_a_captured_draw_is_fresh_on_every_replay():
    B, REPLAYS = 256, 200
    b = _free_systems([1] * B, [0] * B, seed=2)
    integrator = b["integrator"]
    torch.cuda.manual_seed(20241102)
    integrator.draw_inputs(twin.DT, twin.GAMMA, twin.KT)                     # warm-up outside the capture, as the examples do
    warm = integrator.inputs.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        integrator.draw_inputs(twin.DT, twin.GAMMA, twin.KT)
    kept = torch.empty((REPLAYS, B, 8), dtype=torch.float64, device="cuda")
    for r in range(REPLAYS):
        graph.replay()
        kept[r].copy_(integrator.inputs)                                     # in stream order behind the replay
    torch.cuda.synchronize()
    rows = kept.cpu().numpy()
    warm = warm.cpu().numpy()
    u = rows[:, :, 3:6]
    n = u.size
    assert n == REPLAYS * B * 3
    assert np.isfinite(u).all() and np.all(u >= -1.0) and np.all(u < 1.0)
    blocks = {u[r].tobytes() for r in range(REPLAYS)} | {warm[:, 3:6].tobytes()}
    assert len(blocks) == REPLAYS + 1                                        # no replay repeats another one, or the warm-up
    want = _want_constants([twin.DT] * B, [twin.GAMMA] * B, [twin.KT] * B)
    for r in range(REPLAYS):
        assert _same(rows[r, :, :3], want) and not _u64(rows[r, :, 6:]).any(), r
    # moments of U[-1, 1): mean 0 (variance 1/3), variance 1/3 (u^2 has variance 1/5 - 1/9 = 4/45); six standard deviations
    mean, var = float(u.mean()), float(u.var())
    pairs = u[:-1] * u[1:]                                                   # the same system and component, one replay apart
    lag1 = float(pairs.mean()) / (1.0 / 3.0)                                 # <u u'> / <u^2>: standard deviation 1 / sqrt(pairs)
    print(f"\n{n} variates: mean {mean:+.3e} (bound {6 * np.sqrt(1 / (3 * n)):.3e}), var - 1/3 {var - 1 / 3:+.3e} "
          f"(bound {6 * np.sqrt(4 / (45 * n)):.3e}), lag-1 across replays {lag1:+.3e} (bound {6 / np.sqrt(pairs.size):.3e})")
    assert abs(mean) <= 6.0 * np.sqrt(1.0 / (3.0 * n))
    assert abs(var - 1.0 / 3.0) <= 6.0 * np.sqrt(4.0 / (45.0 * n))
    assert abs(lag1) <= 6.0 / np.sqrt(pairs.size)
    _close(b)


# ---- 3. the bath thermalises a free particle --------------------------------------------------------------------------------
# The acceptance band of the three figures around twin.EXPECTED = (1, 1, 0) comes from the HOST twin: tests/langevin_twin.py, BAND.
BAND = twin.BAND


def test_the_bath_thermalises_free_particles_from_one_graph():
    B = twin.MEMBERS
    sizes = [(1, 3, 300)[k % 3] for k in range(B)]
    langevin = [n - 1 for n in sizes]                                        # 0, 2, 299: first, last, beyond the first 256 lanes
    assert sorted(set(langevin)) == [0, 2, 299] and B == 256
    b = _free_systems(sizes, langevin, seed=3)
    integrator, forces, d_vel = b["integrator"], b["forces"], b["d_vel"]
    bath = torch.from_numpy(b["bath_rows"]).cuda()
    assert len(bath) == B
    tags0 = [_u64(sd.getParticleData().getPositions().cpu().numpy()[:, 3]).copy() for sd in b["sysdefs"]]
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")                 # sums of v_c^2 of the bath rows: [after two, after one]

    def tally(slot):
        v = torch.index_select(d_vel, 0, bath)[:, :3]
        acc[slot] += (v * v).sum()

    torch.cuda.manual_seed(20241103)
    forces.compute()                                                         # once: the no-photon path writes zeros
    integrator.prime()
    integrator.draw_inputs(twin.DT, twin.GAMMA, twin.KT)                     # warm-up of the draw and of the torch kernels
    tally(0)
    tally(1)
    torch.cuda.synchronize()
    assert all(not f.cpu().numpy().view(np.uint64).any() for f in forces.forces[:6])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        integrator.draw_inputs(twin.DT, twin.GAMMA, twin.KT)
        integrator.step_one()
        tally(1)
        integrator.step_two()
        tally(0)
    for _ in range(twin.BURN_IN):
        graph.replay()
    acc.zero_()
    start = integrator.state()["langevin_reservoir"].copy()                  # behind the burn-in replays
    for _ in range(twin.COUNTED):
        graph.replay()
    state = integrator.state()
    sums = acc.cpu().numpy()
    gain = state["langevin_reservoir"] - start
    ratios = twin.ratios(sums[0], sums[1], 3 * B * twin.COUNTED, float(gain.mean()), twin.COUNTED)
    print(f"\nmeasured / closed form: after step two {ratios[0]:.5f}, after step one {ratios[1]:.5f}; reservoir gain / pre-kick "
          f"growth {ratios[2]:+.6f}; band {BAND} around {twin.EXPECTED}")
    by_size = {n: float(gain[[k for k in range(B) if sizes[k] == n]].mean()) / twin.COUNTED / twin.closed_forms()[2]
               for n in (1, 3, 300)}
    print(f"reservoir ratio by system size: {by_size}")
    assert all(band > 0.0 for band in BAND)
    assert twin.EXPECTED == (1.0, 1.0, 0.0)
    assert np.all(np.abs(ratios - np.asarray(twin.EXPECTED)) <= np.asarray(BAND)), (ratios.tolist(), BAND)
    assert state["steps"].tolist() == [twin.BURN_IN + twin.COUNTED] * B == [576] * B
    assert state["out_of_box"].tolist() == [0] * B
    assert np.isfinite(state["langevin_reservoir"]).all() and len(set(state["langevin_reservoir"].tolist())) == B
    # every system's own gain is the half-step kinetic energy its particle lost between the two ends: mean 0, standard deviation
    # twin.member_sd() = 1.4 kT / (1 - x) however many steps lie between (the twin's (4)).  A difference of two chi-square-like
    # energies has exponential tails, P(|gain| > t) of about exp(-t (1 - x) / kT), so the bound for one particle is twelve
    # standard deviations: 256 systems stay inside with probability 1 - 1e-5.  A pre-kick tally gains 512 steps of
    # closed_forms()[2] here, 768 kT / (1 - x) against this bound of 17 kT / (1 - x).
    print(f"largest |gain| of one system {np.abs(gain).max():.3e}, bound {12.0 * twin.member_sd():.3e}")
    assert np.all(np.abs(gain) <= 12.0 * twin.member_sd()) and np.all(gain != 0.0)
    assert 12.0 * twin.member_sd() < 0.03 * twin.COUNTED * twin.closed_forms()[2]
    # nothing but the bath particles' velocities changed among the velocities; masses and type tags keep their bits
    vel = d_vel.cpu().numpy()
    others = np.ones(len(vel), dtype=bool)
    others[b["bath_rows"]] = False
    assert others.sum() == len(vel) - B and _same(vel[others], b["vel0"][others])
    assert np.all(vel[b["bath_rows"], :3] != 0.0) and _same(vel[:, 3], b["vel0"][:, 3])
    for k, sd in enumerate(b["sysdefs"]):
        assert np.array_equal(_u64(sd.getParticleData().getPositions().cpu().numpy()[:, 3]), tags0[k]), k
    _close(b)


# ---- 4. the examples ----------------------------------------------------------------------------------------------------------
EXAMPLES = (("minimal_cavity_force.py", ()), ("batch_step_in_one_graph.py", ("2", "40")), ("batch_md_in_one_graph.py", ("2", "40")),
            ("batch_molecular_md_in_one_graph.py", ("2", "40")), ("batch_coulomb_md_in_one_graph.py", ("2", "40")))


def test_every_example_runs():
    assert sorted(name for name, _ in EXAMPLES) == sorted(f for f in os.listdir(os.path.join(ROOT, "examples")) if f.endswith(".py"))
    for name, args in EXAMPLES:
        try:                                                                 # a fresh child each; the first failure ends the test
            done = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name), *args], cwd=ROOT, stdin=subprocess.DEVNULL,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{name} did not finish in {e.timeout} s:\n{e.stdout}")
        assert done.returncode == 0, f"{name} exited with {done.returncode}:\n{done.stdout}"
        out = done.stdout
        print(f"\n--- {name}\n{out}")
        if name.endswith("_md_in_one_graph.py"):
            assert re.search(r"\b40 MD steps per system\b", out) and re.search(r"\b0 coordinates left outside a box\b", out), out
            drift = re.search(r"worst system (\S+), mean (\S+)", out)
            assert drift is not None, out
            assert all(np.isfinite(float(x.rstrip(","))) for x in drift.groups()), out
        elif name == "batch_step_in_one_graph.py":
            assert "40 thermostat steps per system" in out, out
