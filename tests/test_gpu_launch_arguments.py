"""The argument blocks of the four kernels an AoS evaluation can launch (csrc/cavmd_persistent_kernel.hpp,
csrc/cavmd_force_kernels.hpp): cavity_persistent_kernel, dipole_partials_aos_kernel, force_map_aos_fused_kernel and
cavity_small_system_kernel take their leading arguments as plain pointers and integers, in the order a block needs them, with
the grid's size G as an argument of its own.  Run with `-m gpu` on an MI355X.

A reordered argument block goes wrong by two arguments of one type changing places, or by G disagreeing with the launch's grid.
So every input of a case differs from every other of its type: Lx != Ly != Lz, omegac, couplstr and phmass away from their
defaults and from each other, images in -1 .. 1, the photon first, in the middle and last, the photon's type id 0 (type table
('L', 'O', 'N')) and 2 (('O', 'N', 'L')), and once per size no type 'L' at all (L_typeid = -1).

Sizes, the smallest that reach each path (small_system_max_n = 0; tile depth by plan_evaluation's own rule, 256 CUs):
  1025      smallest single launch: 5 blocks, the one-hop hand-off, UNROLL = 1, a ragged tile of one particle
  4609      18 full tiles and a ragged one: 19 blocks, the two-level hand-off
  70 001    a grid of 256 (274 tiles of 256), UNROLL = 1, ragged
  170 003   UNROLL = 2 (N / 512 >= 320), the flagship's instantiation, ragged
each with map_nt_store = 0, 1, 2 (the three instantiations of the single-launch kernel and of the fused map).

Every case: single launch (persistent = 1) against two launches (persistent = 0) bit for bit -- all 4 N force entries, the three
energies, the result block -- and both against the CPU oracle with the contract of tests/test_gpu_parity.py (check_parity).
The single-block kernel at N = 1, 2, 501, 1024 against the oracle the same way and against two launches; one evaluation captured
in a graph at 4609 and 170 003 and replayed on positions changed in place (the argument block of a captured launch is frozen,
and the preload reads it on every replay).  The oracle's result of a configuration is computed once and shared."""
import numpy as np
import pytest
import torch

from parity_support import check_parity, random_cfg, ref_eval, to_device

pytestmark = pytest.mark.gpu

BLOCK = 256
SIZES = [1025, 4609, 70_001, 170_003]
SMALL_SIZES = [1, 2, 501, 1024]
STORE_POLICIES = [0, 1, 2]
PARAMS = {"omegac": 0.0173, "couplstr": 2.5e-3, "phmass": 1.7}
BOX = (31.0, 17.5, 23.25)
ONE_LAUNCH, TWO_LAUNCHES = (True, False, False), (True, False, True)   # which of reduction / finalize / map were launched
RESULT_KEYS = ("force", "energies", "dipole", "dipole_lo", "total_dipole", "q", "Dq", "photon_force")

_cases = {}


def unroll_of(n):
    """plan_evaluation's rule on 256 CUs"""
    return 2 if n // (BLOCK * 2) >= 256 * 5 // 4 else 1


def grid_of(n):
    tile = BLOCK * unroll_of(n)
    return min(256, (n + tile - 1) // tile)


def configuration(n, photon, l_first, seed):
    """photon: index of the one L-typed particle, or None for a configuration without the type 'L'"""
    cfg = random_cfg(n, seed=seed, photon_at=n - 1 if photon is None else photon, L=BOX, image_range=1)
    cfg["params"] = dict(PARAMS)
    if photon is None:
        cfg["types"], cfg["L_typeid"] = ["O", "N", "X"], -1
    elif l_first:
        # the type table reordered: 'L' is type 0, the other two move up by one
        cfg["typeid"] = ((cfg["typeid"] + 1) % 3).astype(np.int32)
        cfg["types"], cfg["L_typeid"] = ["L", "O", "N"], 0
        assert cfg["typeid"][photon] == 0 and np.count_nonzero(cfg["typeid"] == 0) == 1
    return cfg


def cases(ref, oracle_mod, n):
    """the configurations of one size with the oracle's result of each, computed once"""
    if n not in _cases:
        places = sorted({0, n // 2, n - 1})
        made = [(f"photon {p}, L_typeid {0 if l_first else 2}", p, configuration(n, p, l_first, seed=7 * n + 2 * p + l_first))
                for p in places for l_first in (False, True)]
        made.append(("no type L", -1, configuration(n, None, False, seed=7 * n + 5)))
        _cases[n] = []
        for name, photon, cfg in made:
            refout = ref_eval(ref, oracle_mod, cfg)
            assert refout["photon_idx"] == photon, (n, name)
            assert len({*cfg["box"]}) == 3 and len({*cfg["params"].values()}) == 3
            if n > 100:
                assert cfg["image"].min() == -1 and cfg["image"].max() == 1
            _cases[n].append((name, cfg, refout))
    return _cases[n]


def make_compute(sysdef, cfg, tun):
    import cavitymd
    p = cfg["params"]
    comp = cavitymd.CavityForceComputeHIP(sysdef, p["omegac"], p["couplstr"], p["phmass"])
    for k, v in tun.items():
        comp.workspace.set_tunable(k, v)
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


def multi_block(persistent, nt_store):
    t = {"small_system_max_n": 0, "persistent": persistent, "map_nt_store": nt_store}
    if persistent:
        t["persistent_balanced"] = 0   # the two-launch path's deal of the tiles: every bit must agree
    return t


@pytest.mark.parametrize("nt_store", STORE_POLICIES)
@pytest.mark.parametrize("n", SIZES)
def test_single_launch_two_launches_and_oracle_agree_on_distinct_arguments(ref, oracle_mod, n, nt_store):
    for step, (name, cfg, refout) in enumerate(cases(ref, oracle_mod, n)):
        sysdef = to_device(cfg)
        one = evaluate(make_compute(sysdef, cfg, multi_block(1, nt_store)), step)
        two = evaluate(make_compute(sysdef, cfg, multi_block(0, nt_store)), step)
        what = (n, nt_store, name)
        assert one["launched"] == ONE_LAUNCH and two["launched"] == TWO_LAUNCHES, (what, one["launched"], two["launched"])
        assert one["n_partials"] == grid_of(n) and one["n_particles"] == n, what   # G as the kernel saw it = the grid
        assert one["force"].shape == (n, 4)
        assert_same_bits(one, two, what)
        assert one["photon_idx"] == refout["photon_idx"], what
        check_parity(cfg, one, refout)
        check_parity(cfg, two, refout)


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_single_block_kernel_against_oracle_and_two_launches(ref, oracle_mod, n):
    for step, (name, cfg, refout) in enumerate(cases(ref, oracle_mod, n)):
        sysdef = to_device(cfg)
        small = evaluate(make_compute(sysdef, cfg, {}), step)
        two = evaluate(make_compute(sysdef, cfg, multi_block(0, -1)), step)
        what = (n, name)
        assert small["launched"] == ONE_LAUNCH and two["launched"] == TWO_LAUNCHES, (what, small["launched"], two["launched"])
        assert small["n_partials"] == 1 and two["n_partials"] == grid_of(n), what
        check_parity(cfg, small, refout)
        check_parity(cfg, two, refout)
        # One block and several fold in different orders, so the dipole may differ in its last bits: each is within 2 ulp
        # of the exactly rounded sum (check_parity), hence within 4 ulp of the other.  What no sum enters is equal to the bit.
        for key in ("photon_idx", "n_L", "n_particles"):
            assert small[key] == two[key], (what, key)
        assert np.array_equal(small["q"], two["q"]), what
        assert np.all(np.abs(small["dipole"] - two["dipole"]) <= 4 * np.spacing(np.abs(two["dipole"])) + 1e-300), what


@pytest.mark.parametrize("n", [4609, 170_003])
def test_replays_of_a_captured_launch_read_its_frozen_arguments(ref, oracle_mod, n):
    """One single-launch evaluation captured in a graph and replayed three times on positions and images changed in place;
    every replay against an eager two-launch evaluation of the same particle data, bit for bit, and against the oracle."""
    from cavitymd import synthetic
    name, cfg, _ = cases(ref, oracle_mod, n)[4]
    assert name == f"photon {n - 1}, L_typeid 2"
    sysdef = to_device(cfg)
    pd = sysdef.getParticleData()
    one = make_compute(sysdef, cfg, multi_block(1, -1))
    two = make_compute(sysdef, cfg, multi_block(0, -1))
    one.workspace.profile_enable(False)   # no events inside a capture
    one.compute(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one.compute(1)
    cur = cfg
    for rep in range(1, 4):
        cur = synthetic.perturb(cur, rep, amplitude=0.5)
        pd.getPositions().copy_(torch.from_numpy(oracle_mod.pack_pos(cur["position"], cur["typeid"])))
        pd.getImages().copy_(torch.from_numpy(cur["image"]))
        one.getForceArray().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        a = read_out(one)
        b = evaluate(two, rep)
        assert b["launched"] == TWO_LAUNCHES
        assert a["n_partials"] == grid_of(n)
        assert_same_bits(a, b, (n, rep))
        refout = ref_eval(ref, oracle_mod, cur)
        assert a["photon_idx"] == n - 1
        check_parity(cur, a, refout)
        check_parity(cur, b, refout)


def test_the_sizes_reach_the_paths_they_name():
    """host arithmetic only"""
    assert [unroll_of(n) for n in SIZES] == [1, 1, 1, 2] and [grid_of(n) for n in SIZES] == [5, 19, 256, 256]
    assert 4609 // BLOCK == 18 and all(n % (BLOCK * unroll_of(n)) for n in SIZES)       # 18 full tiles; every size is ragged
    assert grid_of(1025) <= 16 < grid_of(4609)                                          # one hop; two levels
    assert 170_003 // 512 == 332 and 332 >= 320                                         # plan_evaluation's UNROLL = 2 threshold
