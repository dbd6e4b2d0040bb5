"""Charges that change between evaluations are seen by the single-launch kernel.  Run with `-m gpu` on an MI355X.

cavity_persistent_kernel reads the charges with temporal loads (NT_LOAD = 1, csrc/cavmd_persistent_kernel.hpp), so their lines
stay in the L2s and the Infinity Cache from one evaluation to the next.  A charge array that is rewritten in between -- by a
kernel on the evaluation's stream, or by a copy from the host -- must be read as rewritten.

Shapes (small_system_max_n at its default; 256 CUs):
  1025      first size on this path: 5 blocks, the one-hop hand-off
  2049      9 blocks
  4353      17 full tiles of 256 and a ragged one: 18 blocks, the two-level hand-off
  196 609   with reduce_unroll = 1 and persistent_lds_kb = 4: 768 full tiles of 256 on 256 blocks, three per block, two LDS
            slots -- the third tile's charges are read a second time in phase 2, and block 0's ragged tile (one particle) too
each on persistent = 1 and on the default dispatch (the single launch at the first three; two launches at the last, where the
LDS budget does not hold a block's tiles).

Every shape: evaluate; multiply every charge by -0.5 in place on the device, on the evaluation's stream (exact in fp64);
evaluate; overwrite the charges with a third set by a copy from the host; evaluate.  After each evaluation the force array and the
result block are compared bit for bit with persistent = 0 on the same particle data, and with the CPU oracle by the contract of
tests/test_gpu_parity.py (check_parity, P1 to P5).  One evaluation is captured in a graph and replayed across both updates.
The oracle's results of a shape are computed once and shared."""
import numpy as np
import pytest
import torch

from parity_support import check_parity, random_cfg, ref_eval, to_device

pytestmark = pytest.mark.gpu

BLOCK = 256
OVERFLOW = {"reduce_unroll": 1, "persistent_lds_kb": 4}
SHAPES = {1025: {}, 2049: {}, 4353: {}, 196_609: OVERFLOW}
DISPATCHES = {"persistent": {"persistent": 1, "persistent_balanced": 0}, "default": {}}
ONE_LAUNCH, TWO_LAUNCHES = (True, False, False), (True, False, True)   # which of reduction / finalize / map were launched
RESULT_KEYS = ("force", "energies", "dipole", "dipole_lo", "total_dipole", "q", "Dq", "photon_force")

_stages = {}


def stages(ref, oracle_mod, n):
    """the three charge sets of a shape -- as built, times -0.5, a third set -- each with the oracle's result, computed once"""
    if n not in _stages:
        cfg = random_cfg(n, seed=11 * n + 3, photon_at=n - 1, image_range=1)
        third = np.random.default_rng(13 * n + 1).uniform(-2.0, 2.0, n)
        third[n - 1] = 0.0
        made = []
        for charge in (cfg["charge"], cfg["charge"] * -0.5, third):
            cur = dict(cfg, charge=np.ascontiguousarray(charge))
            made.append((cur, ref_eval(ref, oracle_mod, cur)))
        _stages[n] = made
    return _stages[n]


def make_compute(sysdef, cfg, tun, profile=True):
    import cavitymd
    p = cfg["params"]
    comp = cavitymd.CavityForceComputeHIP(sysdef, p["omegac"], p["couplstr"], p["phmass"])
    for k, v in tun.items():
        comp.workspace.set_tunable(k, v)
    if profile:
        comp.workspace.profile_enable(True)
        comp.workspace.profile_read()
    return comp


def read_out(comp):
    res = comp.getResult()
    return {"force": comp.getForceArray().cpu().numpy(), "energies": np.array(comp.getEnergies()),
            "dipole": np.array(res.dipole[:]), "dipole_lo": np.array(res.dipole_lo[:]),
            "total_dipole": np.array(res.total_dipole[:]), "q": np.array(res.q[:]), "Dq": np.array(res.Dq[:]),
            "photon_force": np.array(res.photon_force[:]), "photon_idx": res.photon_idx, "n_L": res.n_photon_typed,
            "n_partials": res.n_partials, "n_particles": res.n_particles}


def evaluate(comp, step):
    """one evaluation, with the launches it made"""
    comp.getForceArray().fill_(float("nan"))  # every entry must be overwritten
    comp.compute(step)
    torch.cuda.synchronize()
    ms, launches = comp.workspace.profile_read()
    assert launches == 1
    out = read_out(comp)
    out["launched"] = tuple(x > 0.0 for x in ms)
    return out


def assert_same_bits(one, two, what):
    for key in RESULT_KEYS:
        a, b = np.ascontiguousarray(one[key]), np.ascontiguousarray(two[key])
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), (what, key)
    for key in ("photon_idx", "n_L", "n_partials", "n_particles"):
        assert one[key] == two[key], (what, key)


def update_charges(pd, stage, made):
    """stage 1: in place on the device, on the current stream; stage 2: a copy from the host"""
    charges = pd.getCharges()
    if stage == 1:
        charges.mul_(-0.5)
    elif stage == 2:
        charges.copy_(torch.from_numpy(made[2][0]["charge"]))
    # what the device now holds is what the oracle was given, to the bit
    assert np.array_equal(charges.cpu().numpy().view(np.int64), made[stage][0]["charge"].view(np.int64))


def expected_launches(n, dispatch):
    return TWO_LAUNCHES if (dispatch == "default" and SHAPES[n]) else ONE_LAUNCH


@pytest.mark.parametrize("dispatch", list(DISPATCHES))
@pytest.mark.parametrize("n", list(SHAPES))
def test_changed_charges_are_seen_by_the_next_evaluation(ref, oracle_mod, n, dispatch):
    made = stages(ref, oracle_mod, n)
    sysdef = to_device(made[0][0])
    pd = sysdef.getParticleData()
    comp = make_compute(sysdef, made[0][0], dict(SHAPES[n], **DISPATCHES[dispatch]))
    two = make_compute(sysdef, made[0][0], dict(SHAPES[n], persistent=0))
    for stage, (cur, refout) in enumerate(made):
        update_charges(pd, stage, made)
        a = evaluate(comp, 2 * stage)
        b = evaluate(two, 2 * stage + 1)
        what = (n, dispatch, stage)
        assert a["launched"] == expected_launches(n, dispatch) and b["launched"] == TWO_LAUNCHES, (what, a["launched"])
        assert a["n_particles"] == n and a["photon_idx"] == n - 1, what
        assert_same_bits(a, b, what)
        check_parity(cur, a, refout)
        check_parity(cur, b, refout)


@pytest.mark.parametrize("n", [4353, 196_609])
def test_replays_of_a_captured_launch_see_changed_charges(ref, oracle_mod, n):
    """One single-launch evaluation captured in a graph; a replay after each charge update, against an eager two-launch
    evaluation of the same particle data bit for bit, and against the oracle."""
    made = stages(ref, oracle_mod, n)
    sysdef = to_device(made[0][0])
    pd = sysdef.getParticleData()
    one = make_compute(sysdef, made[0][0], dict(SHAPES[n], **DISPATCHES["persistent"]), profile=False)  # no events in a capture
    two = make_compute(sysdef, made[0][0], dict(SHAPES[n], persistent=0))
    one.compute(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one.compute(1)
    for stage, (cur, refout) in enumerate(made):
        update_charges(pd, stage, made)
        one.getForceArray().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        a = read_out(one)
        b = evaluate(two, stage)
        assert b["launched"] == TWO_LAUNCHES
        assert_same_bits(a, b, (n, stage))
        check_parity(cur, a, refout)
        check_parity(cur, b, refout)


def test_the_shapes_reach_the_paths_they_name():
    """host arithmetic only: plan_evaluation's rules on 256 CUs"""
    grids = {n: min(256, (n + BLOCK - 1) // BLOCK) for n in SHAPES}          # UNROLL = 1 at all four (N / 512 < 320, or set)
    assert all(n // (2 * BLOCK) < 320 or tun["reduce_unroll"] == 1 for n, tun in SHAPES.items())
    assert grids == {1025: 5, 2049: 9, 4353: 18, 196_609: 256}
    assert grids[1025] <= 16 and grids[2049] <= 16 < grids[4353]             # one hop; two levels
    n = 196_609
    full, slots = n // BLOCK, OVERFLOW["persistent_lds_kb"] * 1024 // (BLOCK * 8)
    assert full == 768 and full // grids[n] == 3 and full % grids[n] == 0 and n - full * BLOCK == 1
    assert slots == 2 < 3                                                    # the third tile is read again in phase 2
