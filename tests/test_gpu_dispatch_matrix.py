"""The dispatch matrix: every force-kernel variant cavmd_compute_hoomd and cavmd_compute_soa can select, walked on purpose.

The two entry points choose among about forty template instantiations by N, the CU count and the tunables.  The other GPU
modules reach them through the automatic rules; this one sets the tunables and derives its sizes from a pure-Python mirror
of the dispatcher's host arithmetic (`dispatch_mirror`), which every evaluation first checks against what can be observed
(cavmd_result.n_partials, and which of the three profile slots a call charged).  A mirror that drifts fails, it never skips.

  part 2  the single-launch kernel under LDS pressure ("persistent_lds_kb"): overflow depth of the fullest block in
          {1, 7, 8, 9, 15, 16, 17, 24, 33} (the batch of 8 and the ping-pong period of 16 with both neighbours, and more
          than two full trips), lds_slots 0 / 1 / several, both unrolls, both partitions, store policies 0 / 1 / 2
  part 3  the AoS matrix at the edges of a reduction tile and of the grid, full product of the tunables
  part 4  the strided layout of cavmd_compute_soa with strides that are not the packed ones
  part 5  one ill-conditioned input (condition number ~1e8) through one case of every path

Bounds are those of tests/test_gpu_parity.py (its docstring is the contract); nothing here is looser.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from cavitymd import _capi
from gpu_support import bits as _bits
from oracle import numpy_mirror as nm
from parity_support import check_parity, force_scales, forces_from_dipole, gpu_eval, ref_eval
from parity_support import random_cfg as _random_cfg

gpu = pytest.mark.gpu

# ---- the dispatcher's constants (cav-hoomd_amd/csrc/cavmd_capi.hip, cavmd_persistent_kernel.hpp) --------------------------------
K_REDUCE_BLOCK = 256
K_REDUCE_UNROLL = 2
K_WAVE = 64
K_PERSIST_MAX_LDS = 156 * 1024
K_PERSIST_SHARED_LDS = 76 * 1024
K_MAX_PERSIST_GRID = 256
K_NT_STORE_MIN_N = 200_000
OVERFLOW_BATCH = 8          # D of the overflow loop; two register sets -> period 16

TUNABLE_DEFAULTS = {"reduce_blocks_per_cu": 1, "map_blocks_per_cu": 2, "map_nt_store": -1, "reduce_nt_load": -1,
                    "fused_finalize": 1, "map_reverse": -1, "small_system_max_n": 1024, "reduce_unroll": -1,
                    "persistent": -1, "persistent_lds_kb": 0, "persistent_balanced": -1}


def _block_nfull(n, tile, grid, balanced):
    """Full tiles of every block (block_range<TILE> of cavmd_persistent_kernel.hpp), as a list over the blocks."""
    if balanced:
        units = (n + K_WAVE - 1) // K_WAVE
        out = []
        for b in range(grid):
            s = (units * b // grid) * K_WAVE
            e = min((units * (b + 1) // grid) * K_WAVE, n)
            out.append(max(e - s, 0) // tile)
        return out
    full_tiles = n // tile
    return [(full_tiles - b + grid - 1) // grid if full_tiles > b else 0 for b in range(grid)]


def dispatch_mirror(n, cus, tunables=None):
    """Host arithmetic of cavmd_compute_hoomd restated: which path, which unroll, which grid, how much LDS, how deep the
    overflow.  `partitions` holds slots / cap_slots / lds_slots and the overflow depth (nfull - resident) of the fullest and
    the emptiest block for the strided (0) and the balanced (1) partition; the top-level copies are those of the partition
    the call would use."""
    t = dict(TUNABLE_DEFAULTS, **(tunables or {}))
    if t["small_system_max_n"] > 0 and n <= t["small_system_max_n"]:
        return {"path": "single_block", "launches": (True, False, False), "n_partials": 1, "unroll": None, "g1": 1}
    unroll = K_REDUCE_UNROLL
    while unroll > 1 and n // (K_REDUCE_BLOCK * unroll) < cus * 5 // 4:
        unroll >>= 1
    if t["reduce_unroll"] in (1, 2):
        unroll = t["reduce_unroll"]
    tile = K_REDUCE_BLOCK * unroll
    g1 = max(1, min((n + tile - 1) // tile, cus * t["reduce_blocks_per_cu"]))
    nt_store = t["map_nt_store"] if t["map_nt_store"] >= 0 else (1 if n >= K_NT_STORE_MIN_N else 0)
    budget = K_PERSIST_MAX_LDS // t["reduce_blocks_per_cu"] - 1024
    if t["persistent_lds_kb"] > 0 and t["persistent_lds_kb"] * 1024 < budget:
        budget = t["persistent_lds_kb"] * 1024
    cap_slots = budget // (tile * 8)
    partitions = {}
    for bal in (0, 1):
        if bal:
            units = (n + K_WAVE - 1) // K_WAVE
            slots = (((units + g1 - 1) // g1) * K_WAVE + tile - 1) // tile
        else:
            slots = ((n + tile - 1) // tile + g1 - 1) // g1
        lds_slots = min(slots, cap_slots)
        depth = [nf - min(nf, lds_slots) for nf in _block_nfull(n, tile, g1, bal)]
        partitions[bal] = {"slots": slots, "cap_slots": cap_slots, "lds_slots": lds_slots, "lds_bytes": lds_slots * tile * 8,
                           "depth_fullest": max(depth), "depth_emptiest": min(depth)}
    balanced = 0 if t["persistent_balanced"] < 0 else int(t["persistent_balanced"] != 0)
    mine = partitions[balanced]
    resident = g1 <= K_MAX_PERSIST_GRID and t["reduce_blocks_per_cu"] <= 4
    single = resident and (t["persistent"] > 0 or (t["persistent"] < 0 and mine["slots"] <= mine["cap_slots"]
                                                   and mine["lds_bytes"] <= K_PERSIST_SHARED_LDS))
    out = {"unroll": unroll, "tile": tile, "g1": g1, "n_partials": g1, "nt_store": nt_store, "balanced": balanced,
           "partitions": partitions}
    out.update(mine)
    if single:
        out.update(path="single_launch", launches=(True, False, False))
    elif t["fused_finalize"]:
        out.update(path="two_launches", launches=(True, False, True))
    else:
        out.update(path="three_launches", launches=(True, True, True))
    return out


def soa_mirror(n, cus, tunables=None):
    """The same for cavmd_compute_soa's strided kernels: no single-block and no single-launch path."""
    t = dict(TUNABLE_DEFAULTS, **(tunables or {}))
    m = dispatch_mirror(n, cus, dict(t, small_system_max_n=0, persistent=0))
    return {"unroll": m["unroll"], "g1": m["g1"], "n_partials": m["g1"],
            "launches": (True, False, True) if t["fused_finalize"] else (True, True, True)}


# ---- one workspace, one set of device buffers, every call observed ---------------------------------------------------------------
PAD = 512  # rows behind N that must stay NaN


class Rig:
    def __init__(self, cap):
        self.cap = cap
        self.ws = _capi.Workspace(cap)
        self.ws.profile_enable(True)
        self.soa_ws = _capi.Workspace(cap)
        self.soa_ws.profile_enable(True)
        self.cus = self.ws.device_info()["compute_units"]
        dev = "cuda"
        self.pos = torch.zeros((cap, 4), dtype=torch.float64, device=dev)
        self.chg = torch.zeros((cap,), dtype=torch.float64, device=dev)
        self.img = torch.zeros((cap, 3), dtype=torch.int32, device=dev)
        self.frc = torch.empty((cap + PAD, 4), dtype=torch.float64, device=dev)
        self.cfg = None
        self._set = {}
        self.ws.profile_read()
        self.soa_ws.profile_read()
        self.cases = 0
        self.largest_n = 0

    def load(self, cfg):
        n = len(cfg["charge"])
        assert n <= self.cap
        pos4 = np.concatenate([cfg["position"], nm_type_tag(cfg["typeid"])[:, None]], axis=1)
        self.pos[:n].copy_(torch.from_numpy(np.ascontiguousarray(pos4)))
        self.chg[:n].copy_(torch.from_numpy(np.ascontiguousarray(cfg["charge"])))
        self.img[:n].copy_(torch.from_numpy(np.ascontiguousarray(cfg["image"])))
        self.cfg, self.n = cfg, n
        p = cfg["params"]
        self.prm = _capi.make_params(p["omegac"], p["couplstr"], p["phmass"])
        return self

    def set_tunables(self, ws, tunables):
        full = dict(TUNABLE_DEFAULTS, **(tunables or {}))
        now = self._set.setdefault(id(ws), {})
        for k, v in full.items():
            if now.get(k) != v:
                ws.set_tunable(k, v)
                now[k] = v
        return full

    def run(self, tunables=None, expect_path=None):
        """One cavmd_compute_hoomd call on the loaded configuration.  Asserts the mirror against the observables first."""
        n, cfg = self.n, self.cfg
        full = self.set_tunables(self.ws, tunables)
        m = dispatch_mirror(n, self.cus, full)
        if expect_path is not None:
            assert m["path"] == expect_path, (m["path"], expect_path, n, tunables)
        self.frc[:n + PAD].fill_(float("nan"))
        self.ws.compute_hoomd(0, n, self.pos.data_ptr(), self.chg.data_ptr(), self.img.data_ptr(), cfg["box"], cfg["L_typeid"],
                              self.prm, self.frc.data_ptr())
        torch.cuda.synchronize()
        res = self.ws.result()
        ms, launches = self.ws.profile_read()
        assert launches == 1
        observed = tuple(x > 0.0 for x in ms)
        assert res.n_partials == m["n_partials"], ("mirror drifted: grid", res.n_partials, m, n, tunables)
        assert observed == m["launches"], ("mirror drifted: launches", ms, m, n, tunables)
        assert res.n_particles == n
        assert bool(torch.isnan(self.frc[n:n + PAD]).all()), "wrote behind N"
        self.cases += 1
        self.largest_n = max(self.largest_n, n)
        return {"force_dev": self.frc[:n].clone(), "energies": np.array(res.energy[:]), "dipole": np.array(res.dipole[:]),
                "dipole_lo": np.array(res.dipole_lo[:]), "total_dipole": np.array(res.total_dipole[:]),
                "photon_idx": res.photon_idx, "n_L": res.n_photon_typed, "mirror": m}


def nm_type_tag(typeid):
    t = np.asarray(typeid, dtype=np.int64) & 0xFFFFFFFF
    return t.astype(np.uint64).view(np.float64)


def host(out):
    """The dict check_parity reads."""
    if "force" not in out:
        out["force"] = out["force_dev"].cpu().numpy()
    return out


def assert_same_bits(a, b, what=""):
    """Forces, dipole high and low words, energies, total dipole and photon index: equal bit patterns (-0.0 != 0.0 here)."""
    assert a["photon_idx"] == b["photon_idx"], what
    for k in ("dipole", "dipole_lo", "energies", "total_dipole"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, a[k], b[k])
    assert torch.equal(a["force_dev"].view(torch.int64), b["force_dev"].view(torch.int64)), (what, "force")


def assert_dipoles_within_one_ulp(a, b, what=""):
    assert np.all(np.abs(a["dipole"] - b["dipole"]) <= np.spacing(np.abs(b["dipole"]))), (what, a["dipole"], b["dipole"])


def check_case(cfg, out, refout):
    """check_parity; with several L-typed particles the bounds test_several_L_typed_particles uses (the L-sum detour costs
    one rounding, so the 2-ulp dipole test does not apply)."""
    out = host(out)
    if refout["photon_idx"] >= 0 and out["n_L"] > 1:
        assert out["photon_idx"] == refout["photon_idx"]
        assert not np.isnan(out["force"]).any()
        assert np.abs(out["dipole"] - refout["dipole"]).max() <= 1e-12 * np.abs(refout["dipole"]).max() + 1e-300
        S = force_scales(cfg, refout)
        assert np.all(np.abs(out["force"][:, :3] - refout["force"][:, :3]) <= 1e-10 * S[:, None] + 1e-300)
        later_L = np.nonzero(cfg["typeid"] == cfg["L_typeid"])[0][1:]
        assert not out["force"][later_L].any()
        return
    check_parity(cfg, out, refout)


_CAP = 4_400_000


@pytest.fixture(scope="module")
def rig():
    r = Rig(_CAP)
    yield r
    print(f"\ndispatch matrix: {r.cases} cavmd_compute_hoomd cases on {r.cus} CUs, largest N = {r.largest_n}")


def _several_L(cfg, extra):
    for i in extra:
        cfg["typeid"][i] = cfg["L_typeid"]
    return cfg


# ---- part 1: the mirror, without a GPU ---------------------------------------------------------------------------------------------
def test_mirror_restates_the_documented_arithmetic():
    """What the dispatcher's comments and the suite state for 256 CUs, reproduced by the mirror: the default paths by N, and
    the one overflow case the suite had (N = 6 000 001: 45-46 tiles per block against 38 slots, so depth 7 or 8 only)."""
    assert dispatch_mirror(501, 256)["path"] == "single_block"
    assert dispatch_mirror(1025, 256)["path"] == "single_launch"
    m = dispatch_mirror(1_000_001, 256)
    assert (m["path"], m["unroll"], m["g1"], m["slots"], m["depth_fullest"]) == ("single_launch", 2, 256, 8, 0)
    assert dispatch_mirror(3_000_017, 256)["path"] == "two_launches"       # beyond half a CU's LDS per block
    assert dispatch_mirror(100_000, 256)["unroll"] == 1 and dispatch_mirror(200_003, 256)["unroll"] == 2
    m = dispatch_mirror(6_000_001, 256, {"persistent": 1, "persistent_balanced": 0})
    assert (m["path"], m["cap_slots"], m["slots"]) == ("single_launch", 38, 46)
    assert (m["depth_fullest"], m["depth_emptiest"]) == (8, 7)
    assert dispatch_mirror(6_000_001, 256, {"persistent": 1, "persistent_balanced": 1})["depth_fullest"] in (7, 8)
    m = dispatch_mirror(200_003, 256, {"fused_finalize": 0, "persistent": 0})
    assert m["path"] == "three_launches" and m["launches"] == (True, True, True)
    assert dispatch_mirror(200_003, 256, {"reduce_blocks_per_cu": 8})["path"] == "two_launches"   # 2048 > 256 blocks
    # one slot is 2 KiB at unroll 1 and 4 KiB at unroll 2: 1 KiB holds none
    for unroll, kb_per_slot in ((1, 2), (2, 4)):
        for slots in (0, 1, 2, 3):
            m = dispatch_mirror(2_000_000, 256, {"persistent": 1, "reduce_unroll": unroll,
                                                 "persistent_lds_kb": max(1, slots * kb_per_slot)})
            assert m["cap_slots"] == slots == m["lds_slots"]
    for cus in (64, 128, 256):
        for unroll in (1, 2):
            for bal in (0, 1):
                for cap in (0, 1, 3):
                    for depth in OVERFLOW_DEPTHS:
                        pressure_size(cus, unroll, bal, cap, depth)   # asserts the depth through the mirror
    for depth, unroll, bal, cap, _ in _pressure_cases():
        assert pressure_size(256, unroll, bal, cap, depth)[0] <= _CAP


@gpu
def test_mirror_of_the_automatic_rules_is_observed(ref, oracle_mod, rig):
    """Every other case sets "persistent" by hand.  Here every tunable is on its default, so the mirror's restatement of the
    automatic rules (single block up to 1024, one launch while a block's charges take at most half a CU's LDS, strided
    partition, unroll by tiles per CU, store policy by N) is what rig.run checks against n_partials and the charged profile
    slots -- at sizes on both sides of each rule for the device at hand."""
    cus = rig.cus
    half_lds_n = (K_PERSIST_SHARED_LDS // (512 * 8)) * 512 * min(cus, K_MAX_PERSIST_GRID)   # largest N of the one-launch default
    seen = set()
    for n in (1024, 1025, cus * 5 // 4 * 512 - 1, cus * 5 // 4 * 512, K_NT_STORE_MIN_N - 1, K_NT_STORE_MIN_N,
              half_lds_n - 7, half_lds_n + 513):
        if n <= 300_000:
            cfg, refout = _cfg_and_ref(ref, oracle_mod, n, n - 1)
        else:   # the observation is the point here; these sizes meet the oracle in tests/test_gpu_parity.py
            cfg, refout = _random_cfg(n, seed=n, photon_at=n - 1), None
        out = rig.load(cfg).run({})
        m = out["mirror"]
        seen.add(m["path"])
        if refout is not None:
            check_case(cfg, out, refout)
        if m["path"] != "single_block":
            # the same call with the automatic choices spelled out: same path, same bits
            spelled = rig.run({"persistent": int(m["path"] == "single_launch"), "persistent_balanced": 0,
                               "reduce_unroll": m["unroll"], "map_nt_store": m["nt_store"]}, expect_path=m["path"])
            assert_same_bits(out, spelled, (n, m["path"]))
    assert seen == {"single_block", "single_launch", "two_launches"}, seen


# ---- part 2: the single-launch kernel under LDS pressure ------------------------------------------------------------------------
OVERFLOW_DEPTHS = (1, 7, 8, 9, 15, 16, 17, 24, 33)
CAP_SLOTS = (0, 1, 3)


def pressure_size(cus, unroll, balanced, cap_slots, depth):
    """N and "persistent_lds_kb" such that, with one block per CU, the fullest block of the single-launch kernel keeps
    `cap_slots` tiles in LDS and re-reads `depth`; other blocks re-read one tile less.  The mirror confirms it."""
    # (one block per CU has to fit the in-launch all-reduce: on a part with more CUs "persistent" = 1 is not honoured at
    # these sizes and there is no overflow to build -- the tests then fail here, they do not skip)
    assert cus <= K_MAX_PERSIST_GRID, cus
    tile = K_REDUCE_BLOCK * unroll
    kb = max(1, cap_slots * tile * 8 // 1024)
    grid = cus
    nfull = cap_slots + depth
    if balanced:
        units = grid * (nfull * tile // K_WAVE) - grid // 2     # half of the blocks one 64-particle unit short of nfull tiles
        n = units * K_WAVE - 5
    else:
        n = (grid * (nfull - 1) + grid // 2 + 1) * tile + 37    # the last round of tiles reaches half of the blocks; ragged tail
    tun = {"persistent": 1, "persistent_balanced": balanced, "reduce_unroll": unroll, "persistent_lds_kb": kb}
    m = dispatch_mirror(n, cus, tun)
    assert m["path"] == "single_launch" and m["g1"] <= grid
    assert (m["lds_slots"], m["depth_fullest"], m["depth_emptiest"]) == (cap_slots, depth, depth - 1), (m, n)
    free = dispatch_mirror(n, cus, dict(tun, persistent_lds_kb=0))
    assert free["depth_fullest"] == 0 and free["lds_slots"] == free["slots"]
    return n, kb


def _pressure_cases():
    """(depth, unroll, balanced, cap_slots, store policy).  N grows as CUs x tile x depth and the oracle is sequential, so every
    depth class runs once with 256-particle tiles and the strided partition (the largest case is about 34 x 256 x CUs
    particles); the other unroll and partition take the classes around the batch of 8 and one beyond the ping-pong period,
    512-particle tiles also the deepest class (what "persistent" = 1 at N = 1e7 runs: the reload of both register sets);
    depth 1 carries every store policy and every budget with both partitions and both unrolls."""
    cases = [(d, 1, 0, CAP_SLOTS[(i + 2) % 3], (i + 2) % 3) for i, d in enumerate(OVERFLOW_DEPTHS)]
    cases += [(d, 1, 1, CAP_SLOTS[i % 3], i % 3) for i, d in enumerate((1, 7, 8, 9, 16))]
    cases += [(1, 2, 0, 3, 1), (9, 2, 0, 1, 2), (17, 2, 0, 0, 0), (33, 2, 0, 0, 1), (1, 2, 1, 1, 0), (8, 2, 1, 0, 2)]
    for unroll in (1, 2):
        for bal in (0, 1):
            for k in (0, 1, 2):
                for case in ((1, unroll, bal, 1, k), (1, unroll, bal, CAP_SLOTS[k], (k + unroll + bal) % 3)):
                    if case not in cases:
                        cases.append(case)
    return cases


def _cfg_and_ref(ref, oracle_mod, n, photon_at, kind="photon"):
    cfg = _random_cfg(n, seed=n * 3 + (photon_at or 0) + 11, photon_at=None if kind == "none" else photon_at)
    if kind == "several_L":
        _several_L(cfg, [i for i in (photon_at + 1, n // 2, n - 1) if photon_at < i < n])
    return cfg, ref_eval(ref, oracle_mod, cfg)


@gpu
@pytest.mark.parametrize("depth,unroll,balanced,cap_slots,nt_store", _pressure_cases())
def test_single_launch_under_lds_pressure(ref, oracle_mod, rig, depth, unroll, balanced, cap_slots, nt_store):
    """Tiles beyond the LDS budget are re-read in batches of 8 through two register sets.  The budget changes where a charge
    is read from, never the arithmetic: same bits as without pressure, and (strided partition) as two launches."""
    n, kb = pressure_size(rig.cus, unroll, balanced, cap_slots, depth)
    cfg, refout = _cfg_and_ref(ref, oracle_mod, n, n - 1 if depth % 2 else n // 3)
    rig.load(cfg)
    tun = {"persistent": 1, "persistent_balanced": balanced, "reduce_unroll": unroll, "map_nt_store": nt_store}
    tight = rig.run(dict(tun, persistent_lds_kb=kb), expect_path="single_launch")
    m = tight["mirror"]
    assert (m["lds_slots"], m["depth_fullest"]) == (cap_slots, depth)
    check_case(cfg, tight, refout)
    free = rig.run(tun, expect_path="single_launch")
    assert free["mirror"]["depth_fullest"] == 0
    assert_same_bits(tight, free, "LDS budget changed bits")
    if not balanced:
        two = rig.run({"persistent": 0, "reduce_unroll": unroll, "map_nt_store": nt_store}, expect_path="two_launches")
        assert_same_bits(tight, two, "single launch (strided) != two launches")


@gpu
@pytest.mark.parametrize("unroll,balanced", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_single_launch_budget_edges(ref, oracle_mod, rig, unroll, balanced):
    """The two sides of `rg.nfull < lds_slots` for the ragged tile: a budget that holds exactly a block's tiles (ragged one
    parked in the last slot) against one slot less (the fullest block's last full tile and the ragged one come from global
    memory), and a budget of no slot at all (0 bytes of dynamic LDS) at a size where every tile is ragged or single."""
    tile = K_REDUCE_BLOCK * unroll
    kb_per_slot = tile * 8 // 1024
    grid = min(rig.cus, K_MAX_PERSIST_GRID)
    for n in (grid * tile * 3 + tile // 2 + 3, grid * tile * 2 + 17 * tile + 1, tile + 9, tile - 9):
        cfg, refout = _cfg_and_ref(ref, oracle_mod, n, n // 2)
        rig.load(cfg)
        tun = {"persistent": 1, "persistent_balanced": balanced, "reduce_unroll": unroll, "small_system_max_n": 0}
        free = rig.run(tun, expect_path="single_launch")
        check_case(cfg, free, refout)
        slots = free["mirror"]["slots"]
        for cap in sorted({slots, slots - 1, 1, 0}):
            if cap < 0:
                continue
            out = rig.run(dict(tun, persistent_lds_kb=max(1, cap * kb_per_slot)), expect_path="single_launch")
            assert out["mirror"]["lds_slots"] == min(cap, slots)
            assert_same_bits(out, free, f"budget of {cap} slots, N={n}")


@gpu
@pytest.mark.parametrize("kind", ["none", "several_L"])
def test_single_launch_slow_map_under_lds_pressure(ref, oracle_mod, rig, kind):
    """No photon, and several L-typed particles: the force map that reads everything from global memory, entered from a
    launch whose LDS budget overflows."""
    for unroll, balanced, cap, depth in ((2, 0, 1, 1), (1, 1, 0, 9)):
        n, kb = pressure_size(rig.cus, unroll, balanced, cap, depth)
        cfg, refout = _cfg_and_ref(ref, oracle_mod, n, 100, kind)
        rig.load(cfg)
        tun = {"persistent": 1, "persistent_balanced": balanced, "reduce_unroll": unroll}
        tight = rig.run(dict(tun, persistent_lds_kb=kb), expect_path="single_launch")
        assert tight["mirror"]["depth_fullest"] == depth
        if kind == "none":
            assert tight["photon_idx"] == -1 == refout["photon_idx"]
            assert not host(tight)["force"].any() and not tight["energies"].any() and not tight["dipole"].any()
        else:
            assert tight["photon_idx"] == 100 and tight["n_L"] == 4
            check_case(cfg, tight, refout)
        assert_same_bits(tight, rig.run(tun, expect_path="single_launch"))
        if not balanced:
            assert_same_bits(tight, rig.run({"persistent": 0, "reduce_unroll": unroll}, expect_path="two_launches"))


# ---- part 3: the rest of the AoS matrix at the tile edges ------------------------------------------------------------------------
def _aos_variants():
    """(bit group, tunables): the full product of the tunables where each applies.  Bit group = (partition, unroll): store
    policy, load policy, tile order and the number of launches do not enter the summation tree.  The three-launch fold is
    finalize_kernel<., 256> -> reduce_partials_and_finalize<., 256>, the very function (same block size, same partials)
    every block of the fused map calls, so three launches share the bits of two: asserted as equality, not as an ulp bound."""
    out = []
    for unroll in (1, 2):
        for nts in (0, 1, 2):
            for bal in (0, 1):
                out.append(((bal, unroll), {"persistent": 1, "persistent_balanced": bal, "reduce_unroll": unroll,
                                            "map_nt_store": nts}))
            for ntl in (0, 1, 2):
                for rev in (0, 1):
                    out.append(((0, unroll), {"persistent": 0, "fused_finalize": 1, "reduce_unroll": unroll, "map_nt_store": nts,
                                              "reduce_nt_load": ntl, "map_reverse": rev}))
                out.append(((0, unroll), {"persistent": 0, "fused_finalize": 0, "reduce_unroll": unroll, "map_nt_store": nts,
                                          "reduce_nt_load": ntl}))
    return out


def _edge_sizes(cus, tile, k_label):
    if k_label == "mid":
        return [K_NT_STORE_MIN_N - 1, K_NT_STORE_MIN_N + 1] if tile == 256 else [K_NT_STORE_MIN_N - 3 * tile, K_NT_STORE_MIN_N + 3 * tile]
    g1 = dispatch_mirror(1 << 22, cus, {"reduce_unroll": tile // K_REDUCE_BLOCK, "small_system_max_n": 0})["g1"]
    k = {"1": 1, "2": 2, "g1": g1, "g1+1": g1 + 1, "2g1+1": 2 * g1 + 1}[k_label]
    return [k * tile - 1, k * tile, k * tile + 1]


@gpu
@pytest.mark.parametrize("k_label", ["1", "2", "g1", "g1+1", "2g1+1", "mid"])
@pytest.mark.parametrize("tile", [256, 512])
def test_aos_matrix_at_tile_and_grid_edges(ref, oracle_mod, rig, tile, k_label):
    """N = k T - 1, k T, k T + 1 around the edges of a reduction tile T and of the grid g1, and either side of the size
    where force stores turn non-temporal; photon first, in the middle and last (its chunk pair is the one special store of
    every map); every variant of the product.  Per bit group one evaluation is checked against the oracle with the full
    contract and every other one must reproduce its bits -- which is check_parity for each of them, it reads nothing else."""
    variants = _aos_variants()
    for n in _edge_sizes(rig.cus, tile, k_label):
        for photon_at in sorted({0, n // 2, n - 1}):
            cfg, refout = _cfg_and_ref(ref, oracle_mod, n, photon_at)
            rig.load(cfg)
            first = {}
            for group, tun in variants:
                out = rig.run(dict(tun, small_system_max_n=0))
                m = out["mirror"]
                assert m["unroll"] == group[1] and m["path"] == ("single_launch" if tun["persistent"] else
                                                                 "two_launches" if tun["fused_finalize"] else "three_launches")
                if tun["map_nt_store"] == 2:
                    assert m["nt_store"] == 2
                if group not in first:
                    check_case(cfg, out, refout)
                    first[group] = out
                else:
                    assert_same_bits(out, first[group], (n, photon_at, tun))
            # across unrolls and partitions: one ulp of each other (2 ulp of the exact sum is part of check_parity)
            groups = list(first)
            for i, a in enumerate(groups):
                for b in groups[i + 1:]:
                    assert_dipoles_within_one_ulp(first[a], first[b], (n, photon_at, a, b))
            if n <= 4096:
                block = rig.run({"small_system_max_n": 8192}, expect_path="single_block")
                check_case(cfg, block, refout)
                assert_dipoles_within_one_ulp(block, first[(0, 1)], (n, photon_at, "single block"))


# ---- part 4: the strided layout beyond packed arrays ----------------------------------------------------------------------------
SENTINEL = 0xA5
ELEM = {"position": 24, "typeid": 4, "image": 12, "charge": 8, "force": 24, "pe": 8}

# layout: array -> (buffer name, byte offset of element 0, byte stride); pe None = potential_energy NULL
LAYOUTS = {
    "packed": {"position": ("p", 0, 24), "typeid": ("t", 0, 4), "image": ("i", 0, 12), "charge": ("c", 0, 8),
               "force": ("f", 0, 24), "pe": ("e", 0, 8)},
    "padded": {"position": ("p", 8, 40), "typeid": ("t", 4, 8), "image": ("i", 12, 24), "charge": ("c", 8, 16),
               "force": ("f", 16, 48), "pe": ("e", 8, 16)},
    # HOOMD's views (32, 32, 12, 8, 32, 32) with one condition of the fast path broken at a time
    "hoomd_base_8_aligned": {"position": ("p", 8, 32), "typeid": ("p", 32, 32), "image": ("i", 0, 12), "charge": ("c", 0, 8),
                             "force": ("f", 8, 32), "pe": ("f", 32, 32)},
    "hoomd_typeid_own_array": {"position": ("p", 0, 32), "typeid": ("t", 0, 32), "image": ("i", 0, 12), "charge": ("c", 0, 8),
                               "force": ("f", 0, 32), "pe": ("f", 24, 32)},
    "hoomd_no_potential_energy": {"position": ("p", 0, 32), "typeid": ("p", 24, 32), "image": ("i", 0, 12),
                                  "charge": ("c", 0, 8), "force": ("f", 0, 32), "pe": None},
    # position and force interleaved in ONE buffer (64-byte rows: x y z tag | Fx Fy Fz pe)
    "interleaved": {"position": ("pf", 0, 64), "typeid": ("pf", 24, 64), "image": ("i", 0, 12), "charge": ("c", 0, 8),
                    "force": ("pf", 32, 64), "pe": ("pf", 56, 64)},
}


def _view(buf, spec, n, dtype, cols):
    _, off, stride = spec
    return np.ndarray((n, cols), dtype=dtype, buffer=buf, offset=off, strides=(stride, np.dtype(dtype).itemsize))


def soa_eval(rig, cfg, layout, tunables=None):
    """cavmd_compute_soa with arbitrary byte strides and base offsets: the six arrays are carved out of larger buffers filled
    with a sentinel byte.  Returns the outputs and checks that no byte outside the addressed force / energy elements moved."""
    lay = LAYOUTS[layout]
    n = len(cfg["charge"])
    sizes = {}
    for name, spec in lay.items():
        if spec is not None:
            b, off, stride = spec
            sizes[b] = max(sizes.get(b, 0), off + (n - 1) * stride + ELEM[name] + 64)
    bufs = {b: np.full(sz, SENTINEL, dtype=np.uint8) for b, sz in sizes.items()}
    _view(bufs[lay["position"][0]], lay["position"], n, np.float64, 3)[:] = cfg["position"]
    _view(bufs[lay["typeid"][0]], lay["typeid"], n, np.int32, 1)[:, 0] = cfg["typeid"]
    _view(bufs[lay["image"][0]], lay["image"], n, np.int32, 3)[:] = cfg["image"]
    _view(bufs[lay["charge"][0]], lay["charge"], n, np.float64, 1)[:, 0] = cfg["charge"]
    dev = {b: torch.from_numpy(a).cuda() for b, a in bufs.items()}
    arg = lambda name: (dev[lay[name][0]].data_ptr() + lay[name][1], lay[name][2])
    full = rig.set_tunables(rig.soa_ws, tunables)
    m = soa_mirror(n, rig.cus, full)
    p = cfg["params"]
    rig.soa_ws.compute_soa(0, n, arg("position"), arg("typeid"), arg("image"), arg("charge"), cfg["box"], cfg["L_typeid"],
                           _capi.make_params(p["omegac"], p["couplstr"], p["phmass"]), arg("force"),
                           arg("pe") if lay["pe"] is not None else None)
    torch.cuda.synchronize()
    res = rig.soa_ws.result()
    ms, _ = rig.soa_ws.profile_read()
    assert res.n_partials == m["n_partials"], ("mirror drifted: grid", res.n_partials, m)
    assert tuple(x > 0.0 for x in ms) == m["launches"], ("mirror drifted: launches", ms, m)
    after = {b: t.cpu().numpy() for b, t in dev.items()}
    force = _view(after[lay["force"][0]], lay["force"], n, np.float64, 3).copy()
    if lay["pe"] is not None:
        pe = _view(after[lay["pe"][0]], lay["pe"], n, np.float64, 1)
        assert not pe.view(np.uint64).any(), "potential energy is not exactly +0.0"
    # every byte that is not an addressed force / energy element is what it was before the call: with the addressed elements
    # put back to the sentinel (the host never wrote them) the buffers must equal what was uploaded
    for name in ("force", "pe"):
        if lay[name] is not None:
            _view(after[lay[name][0]], lay[name], n, np.uint8, ELEM[name])[:] = SENTINEL
    for b in after:
        assert np.array_equal(after[b], bufs[b]), f"{layout}: bytes outside the outputs changed in '{b}'"
    f4 = np.concatenate([force, np.zeros((n, 1))], axis=1)
    return {"force": f4, "energies": np.array(res.energy[:]), "dipole": np.array(res.dipole[:]),
            "dipole_lo": np.array(res.dipole_lo[:]), "total_dipole": np.array(res.total_dipole[:]),
            "photon_idx": res.photon_idx, "n_L": res.n_photon_typed}


def _assert_same_bits_host(a, b, what):
    assert a["photon_idx"] == b["photon_idx"], what
    for k in ("dipole", "dipole_lo", "energies", "total_dipole"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
    assert np.array_equal(_bits(a["force"][:, :3]), _bits(b["force"][:, :3])), (what, "force")


SOA_SIZES = (1, 255, 256, 257, 1025, 70_001, 300_007)


@gpu
@pytest.mark.parametrize("kind", ["photon", "none", "several_L"])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("unroll", [1, 2])
def test_strided_layout_beyond_packed_strides(ref, oracle_mod, rig, unroll, fused, kind):
    """dipole_partials_kernel / finalize_kernel on StridedInput, force_map_strided_fused_kernel and force_map_strided_kernel
    with strides other than the packed ones, and the near misses of the fast path that forwards HOOMD's views to the AoS
    kernels.  Same bits as packed strides and as cavmd_compute_hoomd with the two-launch partition."""
    tun = {"reduce_unroll": unroll, "fused_finalize": fused}
    for n in SOA_SIZES:
        photon_at = {1: 0, 255: 254, 256: 0, 257: 128}.get(n, n - 1 if unroll == 1 else 7)
        cfg = _random_cfg(n, seed=n + 31 * unroll + fused, photon_at=None if kind == "none" else photon_at)
        if kind == "several_L":
            if n < 4:
                continue
            _several_L(cfg, [i for i in (photon_at + 1, n // 2, n - 1) if photon_at < i < n])
        refout = ref_eval(ref, oracle_mod, cfg)
        aos = host(rig.load(cfg).run(dict(tun, persistent=0, persistent_balanced=0, small_system_max_n=0)))
        packed = soa_eval(rig, cfg, "packed", tun)
        _assert_same_bits_host(packed, aos, (n, "packed strides vs cavmd_compute_hoomd"))
        if kind == "none":
            assert packed["photon_idx"] == -1 and not packed["force"].any() and not packed["energies"].any()
        else:
            check_case(cfg, packed, refout)
        for layout in LAYOUTS:
            if layout == "packed":
                continue
            # (the bits of the evaluation just checked against the oracle: check_parity reads nothing else)
            _assert_same_bits_host(soa_eval(rig, cfg, layout, tun), packed, (n, layout))


@gpu
def test_strided_argument_validation():
    """A stride below the element size, a stride that is not a multiple of the element's alignment, a misaligned base: each is
    CAVMD_ERR_INVALID_VALUE and nothing is written."""
    lib = _capi.load()
    n = 300
    ws = _capi.Workspace(n)
    dev = "cuda"
    pos = torch.zeros(n * 8, dtype=torch.float64, device=dev)
    tid = torch.zeros(n * 8, dtype=torch.int32, device=dev)
    img = torch.zeros(n * 8, dtype=torch.int32, device=dev)
    chg = torch.zeros(n * 8, dtype=torch.float64, device=dev)
    frc = torch.full((n * 8,), 7.0, dtype=torch.float64, device=dev)
    pe = torch.full((n * 8,), 7.0, dtype=torch.float64, device=dev)
    prm = _capi.make_params(0.0091, 1e-3, 1.0)
    good = {"position": (pos.data_ptr(), 40), "typeid": (tid.data_ptr(), 8), "image": (img.data_ptr(), 24),
            "charge": (chg.data_ptr(), 16), "force": (frc.data_ptr(), 48), "pe": (pe.data_ptr(), 16)}

    def call(**over):
        a = dict(good, **over)
        flat = []
        for name in ("position", "typeid", "image", "charge"):
            flat += [ctypes.c_void_p(a[name][0]), a[name][1]]
        return lib.cavmd_compute_soa(ws.handle, None, n, *flat, 10.0, 10.0, 10.0, 2, ctypes.byref(prm),
                                     ctypes.c_void_p(a["force"][0]), a["force"][1],
                                     ctypes.c_void_p(a["pe"][0]) if a["pe"] else None, a["pe"][1] if a["pe"] else 0)

    bad = []
    for name, elem, align in (("position", 24, 8), ("typeid", 4, 4), ("image", 12, 4), ("charge", 8, 8), ("force", 24, 8),
                              ("pe", 8, 8)):
        ptr, stride = good[name]
        bad.append({name: (ptr, elem - align)})          # below the element size
        bad.append({name: (ptr, stride + align // 2)})   # not a multiple of the alignment
        bad.append({name: (ptr + align // 2, stride)})   # misaligned base
    for over in bad:
        assert call(**over) == _capi.CAVMD_ERR_INVALID_VALUE, over
    torch.cuda.synchronize()
    assert bool(torch.all(frc == 7.0)) and bool(torch.all(pe == 7.0))
    with pytest.raises(_capi.CavmdError):
        ws.result()                                       # nothing was computed
    assert call() == _capi.CAVMD_OK                       # the same call with every argument in order goes through
    torch.cuda.synchronize()
    assert ws.result().n_particles == n


# ---- part 5: one ill-conditioned input through every path ----------------------------------------------------------------------
def ill_conditioned_cfg(n_pairs, seed=2026, L=(31.0, 17.5, 23.25), target=1e8):
    """Neutral pairs (+c, -c) a short distance apart, far from the origin through images of several hundred box lengths,
    shuffled so that partners land in different lanes, tiles and blocks; photon last.  Per component
    sum |c_i r_i| / |sum c_i r_i| = 2 <c |r|> / <c delta> ~ `target`: every partial sum is ~1e8 times the result."""
    rng = np.random.default_rng(seed)
    box = np.asarray(L)
    pos_a = rng.uniform(-0.45, 0.45, (n_pairs, 3)) * box
    img = (rng.integers(300, 1000, (n_pairs, 3)) * rng.choice([-1, 1], (n_pairs, 3))).astype(np.int32)
    c = rng.uniform(0.1, 1.0, n_pairs)
    dist = np.abs(pos_a + img * box)
    delta0 = 2.0 * (c[:, None] * dist).mean(axis=0) / (c.mean() * target)
    pos_b = pos_a + delta0 * rng.uniform(0.5, 1.5, (n_pairs, 3))
    order = rng.permutation(2 * n_pairs)
    position = np.concatenate([pos_a, pos_b])[order]
    charge = np.concatenate([c, -c])[order]
    image = np.concatenate([img, img])[order]
    typeid = rng.integers(0, 2, 2 * n_pairs).astype(np.int32)
    n = 2 * n_pairs + 1
    cfg = {"name": f"illcond{n}", "seed": seed,
           "position": np.concatenate([position, rng.uniform(-0.5, 0.5, (1, 3)) * box]),
           "typeid": np.concatenate([typeid, [2]]).astype(np.int32), "charge": np.concatenate([charge, [0.0]]),
           "image": np.concatenate([image, rng.integers(-3, 4, (1, 3)).astype(np.int32)]),
           "types": ["O", "N", "L"], "box": tuple(L), "L_typeid": 2,
           "params": {"omegac": 0.0091, "couplstr": 1e-3, "phmass": 1.0}}
    return cfg


ILL_PAIRS = 100_000


def _ill_conditioned_exact(ref, oracle_mod, cfg):
    n = len(cfg["charge"])
    pos4 = oracle_mod.pack_pos(cfg["position"], cfg["typeid"])
    hi, _ = ref.dipole_exact(pos4, cfg["charge"], cfg["image"], cfg["box"], n - 1)
    t = nm.terms(pos4, cfg["charge"], cfg["image"], cfg["box"])[:-1]
    cond = np.abs(t).sum(axis=0) / np.abs(hi)
    return hi, t, cond


def test_ill_conditioned_family_is_what_it_claims(ref, oracle_mod):
    """No GPU: the exactly rounded dipole of the family agrees with an independent exact sum of the same addends, the
    condition number is ~1e8 in every component, and the reference's own sequential sum loses about that many digits."""
    cfg = ill_conditioned_cfg(ILL_PAIRS)
    hi, t, cond = _ill_conditioned_exact(ref, oracle_mod, cfg)
    assert np.array_equal(hi, np.array([math.fsum(t[:, k].tolist()) for k in range(3)]))
    assert np.all(cond >= 3e7) and np.all(cond <= 3e8), cond
    refout = ref_eval(ref, oracle_mod, cfg)
    rel = np.abs(refout["dipole"] - hi) / np.abs(hi)
    assert np.all(rel <= 1e-5) and rel.max() >= 1e-12, rel   # far from the 2 ulp asked of the kernels, by construction
    small = ill_conditioned_cfg(300, seed=5)
    pos4 = oracle_mod.pack_pos(small["position"], small["typeid"])
    # (the addends are rounded products, so the rational sum of the unrounded ones agrees only to the rounding of the terms)
    exact = np.array([float(v) for v in nm.dipole_rational(pos4, small["charge"], small["image"], small["box"], 600)])
    hi_s, t_s, cond_s = _ill_conditioned_exact(ref, oracle_mod, small)
    assert np.all(np.abs(hi_s - exact) <= 2 * np.finfo(float).eps * np.abs(t_s).sum(axis=0))
    assert np.all(cond_s >= 3e7) and np.all(cond_s <= 3e8)


def _check_against_exact(cfg, out, refout, d_exact, what):
    """P4 and P5 of check_parity with the reference's own error term replaced by zero, and the 2-ulp dipole bound; P1 and P3
    compare with the sequential reference sum, which itself loses about eight digits here."""
    assert out["photon_idx"] == refout["photon_idx"] == len(cfg["charge"]) - 1, what
    assert not np.isnan(out["force"]).any(), what
    assert np.all(np.abs(out["dipole"] - d_exact) <= 2 * np.spacing(np.abs(d_exact))), (what, out["dipole"], d_exact)
    S = force_scales(cfg, dict(refout, dipole=d_exact))
    F_exact = forces_from_dipole(cfg, refout, d_exact)
    err = np.abs(out["force"][:, :3] - F_exact[:, :3])
    assert np.all(err <= 1e-14 * S[:, None] + 1e-300), (what, float((err / (S[:, None] + 1e-300)).max()))
    mol = np.ones(len(S), dtype=bool)
    mol[refout["photon_idx"]] = False
    assert np.all(out["force"][mol, 2] == 0.0) and np.all(out["force"][:, 3] == 0.0), what


@gpu
def test_ill_conditioned_input_through_every_path(ref, oracle_mod, rig):
    """A double-double chain of k additions errs by about k^2 eps^2 sum|t|: with k in the hundreds that is below 1e-3 ulp of
    the result at a condition number of 1e8.  A plain fp64 sum, or a merge that dropped a low word, anywhere in a path would
    miss the 2-ulp bound by many orders of magnitude."""
    cfg = ill_conditioned_cfg(ILL_PAIRS)
    n = len(cfg["charge"])
    d_exact, _, cond = _ill_conditioned_exact(ref, oracle_mod, cfg)
    assert np.all(cond >= 3e7) and np.all(cond <= 3e8), cond
    refout = ref_eval(ref, oracle_mod, cfg)
    rig.load(cfg)
    tile_kb = K_REDUCE_BLOCK * 2 * 8 // 1024
    paths = [("single_block", {"small_system_max_n": 1 << 20}),
             ("single_launch", {"persistent": 1, "persistent_balanced": 0, "reduce_unroll": 2}),
             ("single_launch", {"persistent": 1, "persistent_balanced": 1, "reduce_unroll": 2}),
             ("single_launch", {"persistent": 1, "persistent_balanced": 0, "reduce_unroll": 2, "persistent_lds_kb": tile_kb}),
             ("single_launch", {"persistent": 1, "persistent_balanced": 1, "reduce_unroll": 1, "persistent_lds_kb": 1}),
             ("two_launches", {"persistent": 0}),
             ("two_launches", {"persistent": 0, "reduce_unroll": 1, "reduce_blocks_per_cu": 8}),
             ("three_launches", {"persistent": 0, "fused_finalize": 0})]
    for path, tun in paths:
        out = host(rig.run(tun, expect_path=path))
        if "persistent_lds_kb" in tun:
            assert out["mirror"]["depth_fullest"] >= 1, out["mirror"]
        _check_against_exact(cfg, out, refout, d_exact, (path, tun))
    for layout, tun in (("packed", {}), ("padded", {"fused_finalize": 0}), ("interleaved", {"reduce_unroll": 1})):
        _check_against_exact(cfg, soa_eval(rig, cfg, layout, tun), refout, d_exact, (layout, tun))
    # the user-facing object on its defaults, as the sibling module evaluates
    _check_against_exact(cfg, gpu_eval(cfg), refout, d_exact, "defaults")
