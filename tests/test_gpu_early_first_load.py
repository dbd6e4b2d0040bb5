"""The single-launch kernel's entry (csrc/cavmd_persistent_kernel.hpp): the speculative photon row is fetched with vector loads
ahead of the first tile row (speculative_photon_row, csrc/cavmd_force_kernels.hpp) and nothing waits for it before
scalars_from_total.  Run with `-m gpu` on an MI355X.

Only the order of issue changed, so every case holds the single launch (persistent = 1) against two launches (persistent = 0)
bit for bit -- every force entry, the three energies, the dipole's two words, the all-particle dipole, q, Dq and the photon
force -- and both against the CPU oracle with the contract of tests/test_gpu_parity.py.  The two-launch path reads the same
row in reduce_partials_and_finalize, through the same helper.

Shapes (small_system_max_n = 0, so that these sizes take the multi-block kernels; the grid is min(256, ceil(N / TILE))):
  TILE 256 (reduce_unroll 1)   N = 1025: 4 full tiles, block 4 holds one ragged particle and no full tile;  1280: 5 full
                               tiles, no ragged tile;  1281: 5 full tiles, block 5 holds only the one-particle ragged tile;
                               1300: a ragged tile of 20
  TILE 512 (reduce_unroll 2)   N = 1537, 2048, 2049: the same three;  2100: a ragged tile of 52
  hand-off                     N = 8192: 16 blocks, the largest one-hop grid;  8704: 17 blocks, the smallest two-level grid, no
                               ragged tile;  8705: 18 blocks, the last one with the one-particle ragged tile
Photon: last (the speculation hits), first and middle (the fallback load); last in a one-particle ragged tile = the only
particle of that tile; inside a longer ragged tile without being last.
"""
import numpy as np
import pytest
import torch

from parity_support import check_parity, force_scales, random_cfg, ref_eval, to_device

pytestmark = pytest.mark.gpu

BLOCK = 256
SHAPES = [(1025, 1), (1280, 1), (1281, 1), (1300, 1), (1537, 2), (2048, 2), (2049, 2), (2100, 2), (8192, 2), (8704, 2),
          (8705, 2)]
ONE_LAUNCH, TWO_LAUNCHES = (True, False, False), (True, False, True)   # which of reduction / finalize / map were launched


def tunables(unroll, persistent):
    t = {"small_system_max_n": 0, "reduce_unroll": unroll, "persistent": persistent}
    if persistent:
        t["persistent_balanced"] = 0   # the two-launch path's deal of the tiles: every bit must agree
    return t


def make_compute(sysdef, cfg, tun):
    import cavitymd
    p = cfg["params"]
    comp = cavitymd.CavityForceComputeHIP(sysdef, p["omegac"], p["couplstr"], p["phmass"])
    for k, v in tun.items():
        comp.workspace.set_tunable(k, v)
    return comp


def read_out(comp):
    res = comp.getResult()
    return {"force": comp.getForceArray().cpu().numpy(), "energies": np.array(comp.getEnergies()),
            "dipole": np.array(res.dipole[:]), "dipole_lo": np.array(res.dipole_lo[:]),
            "total_dipole": np.array(res.total_dipole[:]), "q": np.array(res.q[:]), "Dq": np.array(res.Dq[:]),
            "photon_force": np.array(res.photon_force[:]), "photon_idx": res.photon_idx, "n_L": res.n_photon_typed,
            "n_partials": res.n_partials}


def evaluate(cfg, unroll, persistent):
    """one evaluation on a fresh workspace, with the launches it made"""
    comp = make_compute(to_device(cfg), cfg, tunables(unroll, persistent))
    comp.workspace.profile_enable(True)
    comp.workspace.profile_read()
    comp.getForceArray().fill_(float("nan"))  # every entry must be overwritten
    comp.compute(0)
    torch.cuda.synchronize()
    ms, launches = comp.workspace.profile_read()
    out = read_out(comp)
    out["launched"] = tuple(x > 0.0 for x in ms)
    assert launches == 1
    return out


def assert_same_bits(one, two, what):
    for key in ("force", "energies", "dipole", "dipole_lo", "total_dipole", "q", "Dq", "photon_force"):
        a, b = np.ascontiguousarray(one[key]), np.ascontiguousarray(two[key])
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (what, key)
    assert (one["photon_idx"], one["n_L"], one["n_partials"]) == (two["photon_idx"], two["n_L"], two["n_partials"]), what


def one_and_two(cfg, unroll):
    n = len(cfg["charge"])
    one, two = evaluate(cfg, unroll, 1), evaluate(cfg, unroll, 0)
    assert one["launched"] == ONE_LAUNCH and two["launched"] == TWO_LAUNCHES, (n, unroll, one["launched"], two["launched"])
    tile = BLOCK * unroll
    assert one["n_partials"] == min(256, (n + tile - 1) // tile)
    assert_same_bits(one, two, (n, unroll))
    return one, two


def photon_places(n, tile):
    """name -> index; the ragged tile is particles full * tile .. n - 1"""
    full, tail = n // tile, n % tile
    places = {"last": n - 1, "first": 0, "middle": n // 2}
    if tail >= 2:
        places["inside_ragged_tile"] = full * tile + tail // 2
        assert full * tile <= places["inside_ragged_tile"] < n - 1
    return places


@pytest.mark.parametrize("n,unroll", SHAPES)
def test_single_launch_gives_the_bits_of_two_launches_at_every_entry_shape(ref, oracle_mod, n, unroll):
    tile = BLOCK * unroll
    tail = n % tile
    for name, photon in photon_places(n, tile).items():
        cfg = random_cfg(n, seed=11 * n + photon, photon_at=photon)
        one, two = one_and_two(cfg, unroll)
        assert one["photon_idx"] == photon, (n, name)
        refout = ref_eval(ref, oracle_mod, cfg)
        for out in (one, two):
            check_parity(cfg, out, refout)
    if tail == 1:
        # photon last = the only particle of the ragged tile, which is all its block holds
        assert photon_places(n, tile)["last"] == (n // tile) * tile


def test_the_shapes_cover_what_they_claim():
    """host arithmetic only: the grids and tile counts the module's docstring names"""
    def grid(n, tile):
        return min(256, (n + tile - 1) // tile)
    def nfull(n, tile, b):
        full, g = n // tile, grid(n, tile)
        return (full - b + g - 1) // g if full > b else 0
    for n, unroll in SHAPES:
        tile = BLOCK * unroll
        g = grid(n, tile)
        counts = [nfull(n, tile, b) for b in range(g)]
        if n % tile:
            assert counts[-1] == 0 and (n // tile) % g == g - 1      # the last block: the ragged tile and no full tile
        else:
            assert min(counts) == 1                                  # no ragged tile at all
    assert [grid(n, 512) for n in (8192, 8704, 8705)] == [16, 17, 18]
    assert {n % (BLOCK * u) for n, u in SHAPES} >= {0, 1, 20, 52}


@pytest.mark.parametrize("n,unroll", [(1281, 1), (2049, 2), (8705, 2)])
def test_no_L_type_and_two_L_typed_particles(ref, oracle_mod, n, unroll):
    # no type named 'L' at all: the compute passes L_typeid = -1; everything is zero, on both paths
    cfg = random_cfg(n, seed=3 * n, photon_at=n - 1)
    cfg["types"], cfg["L_typeid"] = ["O", "N", "X"], -1
    one, two = one_and_two(cfg, unroll)
    assert one["photon_idx"] == -1 and not one["force"].any() and not one["energies"].any() and not one["dipole"].any()
    refout = ref_eval(ref, oracle_mod, cfg)
    assert refout["photon_idx"] == -1
    check_parity(cfg, one, refout)
    check_parity(cfg, two, refout)
    # two L-typed particles: the first is the photon, the second enters the dipole and gets no force; the photon's charge is
    # fetched late (the lcnt > 1 path of scalars_from_total).  Second one last: the speculative row is NOT the photon's.
    for photon, other in ((n - 1 - 300, n - 1), (0, n // 2), (n // 2, n - 2)):
        cfg = random_cfg(n, seed=3 * n + photon, photon_at=photon)
        cfg["typeid"][other] = 2
        one, two = one_and_two(cfg, unroll)
        assert one["photon_idx"] == photon and one["n_L"] == 2
        refout = ref_eval(ref, oracle_mod, cfg)
        assert refout["photon_idx"] == photon
        S = force_scales(cfg, refout)
        for out in (one, two):
            # the L-sum detour costs one extra rounding: scale-relative bounds, as tests/test_gpu_parity.py::
            # test_several_L_typed_particles
            assert not np.isnan(out["force"]).any()
            assert np.abs(out["dipole"] - refout["dipole"]).max() <= 1e-12 * np.abs(refout["dipole"]).max()
            for k in range(3):
                assert abs(out["energies"][k] - refout["energies"][k]) <= 1e-10 * abs(refout["energies"][k]) + 1e-300
            assert np.all(np.abs(out["force"][:, :3] - refout["force"][:, :3]) <= 1e-10 * S[:, None] + 1e-300)
            assert not out["force"][other].any()


def test_replays_read_the_photon_row_afresh(ref, oracle_mod):
    """A captured single launch replayed three times on positions and images changed in place, the photon's row included: the
    row is read by every launch, never kept across launches.  The two-launch path runs eagerly on the same particle data."""
    from cavitymd import synthetic
    n, unroll = 8705, 2
    cfg = random_cfg(n, seed=77, photon_at=n - 1)
    sysdef = to_device(cfg)
    pd = sysdef.getParticleData()
    one = make_compute(sysdef, cfg, tunables(unroll, 1))
    two = make_compute(sysdef, cfg, tunables(unroll, 0))
    one.compute(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one.compute(1)
    cur, rows = cfg, set()
    for rep in range(1, 4):
        cur = synthetic.perturb(cur, rep, amplitude=0.5)
        rows.add((tuple(cur["position"][-1]), tuple(cur["image"][-1])))
        pd.getPositions().copy_(torch.from_numpy(oracle_mod.pack_pos(cur["position"], cur["typeid"])))
        pd.getImages().copy_(torch.from_numpy(cur["image"]))
        one.getForceArray().fill_(float("nan"))
        two.getForceArray().fill_(float("nan"))
        graph.replay()
        two.compute(rep)
        torch.cuda.synchronize()
        a, b = read_out(one), read_out(two)
        assert_same_bits(a, b, rep)
        refout = ref_eval(ref, oracle_mod, cur)
        assert a["photon_idx"] == n - 1
        check_parity(cur, a, refout)
        check_parity(cur, b, refout)
        q = cur["position"][-1] + cur["image"][-1] * np.asarray(cur["box"])
        assert np.array_equal(a["q"], q)      # this replay's photon row, to the bit
    assert len(rows) == 3                     # the photon moved between replays
