"""The rolling tile loop of the dipole reduction (csrc/cavmd_tile_schedule.hpp, accumulate_full_tiles) gives the bits of the
plain loop it replaced.  Run with `-m gpu` on an MI355X.

The yardstick is tests/golden/rolling_tile_loop_parent.json: the result block's doubles and a SHA-256 of the force array's
bytes, recorded for every case below with the commit BEFORE the rolling loop (tests/make_rolling_tile_loop_golden.py wrote it;
that commit's one-launch and two-launch paths agreed bit for bit on every case, which the generator asserts).  Each case is then
also held against the CPU oracle with the contract of tests/test_gpu_parity.py (P1-P5), and the one-launch kernel against the
two-launch path, so the new loop is never compared only with itself.

Shapes: with reduce_unroll = 2 and small_system_max_n = 0 the grid is 256 blocks of 512-particle tiles, so N around k * 131072
(k = 1..3) makes blocks of k - 1 and k full tiles meet: the prologue alone, odd and even trip counts of the two register sets,
blocks with one trip fewer than their neighbours, with and without a ragged tail; N = 1537 has a few blocks of one tile each.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from parity_support import check_parity, force_scales, gpu_eval, ref_eval, to_device
from parity_support import random_cfg

pytestmark = pytest.mark.gpu

BLOCK, UNROLL = 256, 2
TILE = BLOCK * UNROLL
SIZES = [k * 131072 + d for k in (1, 2, 3) for d in (-1, 0, 1, 513)] + [1537]
VARIANTS = ("photon_first", "photon_middle", "photon_last", "planted")
BASE = {"reduce_unroll": 2, "small_system_max_n": 0}
ONE = dict(BASE, persistent=1, persistent_balanced=0)   # the two-launch path's deal of the tiles: every bit must agree
TWO = dict(BASE, persistent=0)
GOLDEN_NAME = "rolling_tile_loop_parent.json"


def planted_indices(n):
    """-> (photon index, the other L-typed indices): rows u = 0 and u = 1 of the first, a middle and the last full tile (hence
    two in one tile, three times), and the last particle of the ragged tail where there is one.  The photon is the FIRST
    L-typed particle (src/CavityForceCompute.cc:122), so it takes row 0 of the first tile."""
    full = n // TILE
    assert full >= 3
    mid, last = full // 2, full - 1
    photon = 5
    extra = [BLOCK + 7, mid * TILE + 100, mid * TILE + BLOCK + 100, last * TILE + 3, last * TILE + TILE - 1]
    if n % TILE:
        extra.append(n - 1)
    assert len(set(extra + [photon])) == len(extra) + 1 and photon < min(extra)
    return photon, extra


def where(i, n):
    """('tile', t, u) for a particle of a full tile, ('tail',) for one of the ragged tail"""
    full = n // TILE
    return ("tile", i // TILE, (i % TILE) // BLOCK) if i < full * TILE else ("tail",)


def make_cfg(n, variant):
    if variant == "planted":
        photon, extra = planted_indices(n)
        cfg = random_cfg(n, seed=7 * n + 3, photon_at=photon)
        cfg["typeid"][:photon] = 0
        cfg["typeid"][extra] = 2
        return cfg
    photon = {"photon_first": 0, "photon_middle": n // 2, "photon_last": n - 1}[variant]
    return random_cfg(n, seed=7 * n + VARIANTS.index(variant), photon_at=photon)


def record(out):
    """what the golden file keeps of one evaluation"""
    r = out["result"]
    doubles = np.array(list(r.dipole) + list(r.q) + list(r.Dq) + list(r.energy) + list(r.photon_force) + list(r.dipole_lo)
                       + list(r.total_dipole), dtype="<f8")
    return {"result_doubles": doubles.tobytes().hex(),
            "result_ints": [int(r.photon_idx), int(r.n_photon_typed), int(r.n_particles), int(r.n_partials)],
            "force_sha256": hashlib.sha256(np.ascontiguousarray(out["force"]).tobytes()).hexdigest()}


def case_key(n, variant, unroll=2):
    return f"N{n}_{variant}_unroll{unroll}"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, GOLDEN_NAME)))["cases"]


def check_against_oracle(cfg, out, refout, extra):
    if not extra:
        check_parity(cfg, out, refout)
        return
    # several L-typed particles: the L-sum detour costs one extra rounding, so scale-relative bounds instead of the 2-ulp
    # dipole test, as tests/test_gpu_parity.py::test_several_L_typed_particles
    assert out["photon_idx"] == refout["photon_idx"] and out["n_L"] == len(extra) + 1
    assert not np.isnan(out["force"]).any()
    assert np.abs(out["dipole"] - refout["dipole"]).max() <= 1e-12 * np.abs(refout["dipole"]).max()
    for k in range(3):
        assert abs(out["energies"][k] - refout["energies"][k]) <= 1e-10 * abs(refout["energies"][k]) + 1e-300
    S = force_scales(cfg, refout)
    assert np.all(np.abs(out["force"][:, :3] - refout["force"][:, :3]) <= 1e-10 * S[:, None] + 1e-300)
    assert not out["force"][extra].any()
    mol = np.ones(len(S), dtype=bool)
    mol[refout["photon_idx"]] = False
    assert np.all(out["force"][mol, 2] == 0.0) and np.all(out["force"][:, 3] == 0.0)


@pytest.mark.parametrize("n", SIZES)
def test_rolling_loop_gives_the_parent_commits_bits(ref, oracle_mod, golden, n):
    full, tail = n // TILE, n % TILE
    seen = {"row0": set(), "row1": set(), "tail": 0, "two_in_one_tile": 0, "photon": set()}
    for variant in VARIANTS:
        cfg = make_cfg(n, variant)
        extra = planted_indices(n)[1] if variant == "planted" else []
        L_idx = np.flatnonzero(cfg["typeid"] == 2)
        assert list(L_idx) == sorted(extra + [int(L_idx[0])])
        # count the planted edges, so that the case cannot pass without them
        per_tile = {}
        for i in L_idx:
            w = where(int(i), n)
            if w[0] == "tail":
                seen["tail"] += 1
            else:
                seen["row%d" % w[2]].add(w[1])
                per_tile[w[1]] = per_tile.get(w[1], 0) + 1
        seen["two_in_one_tile"] += sum(1 for c in per_tile.values() if c >= 2)
        if variant != "planted":
            seen["photon"].add(int(L_idx[0]))
        refout = ref_eval(ref, oracle_mod, cfg)
        one, two = gpu_eval(cfg, ONE), gpu_eval(cfg, TWO)
        assert one["result"].n_partials == two["result"].n_partials == min(256, (n + TILE - 1) // TILE)
        want = golden[case_key(n, variant)]
        assert record(two) == want, (n, variant, "two launches")
        assert record(one) == want, (n, variant, "one launch")
        assert np.array_equal(one["force"].view(np.int64), two["force"].view(np.int64))
        for out in (one, two):
            check_against_oracle(cfg, out, refout, extra)
    mid, last = full // 2, full - 1
    assert {0, mid, last} <= seen["row0"] and {0, mid, last} <= seen["row1"]
    assert seen["two_in_one_tile"] >= 3
    assert seen["photon"] == {0, n // 2, n - 1}
    # photon last: in the ragged tail where there is one (plus the planted tail particle), else in row 1 of the last tile
    assert seen["tail"] >= (2 if tail else 0)


def test_unroll_1_is_untouched(ref, oracle_mod, golden):
    n = 70_001
    cfg = make_cfg(n, "photon_last")
    want = golden[case_key(n, "photon_last", unroll=1)]
    refout = ref_eval(ref, oracle_mod, cfg)
    for tun in (dict(ONE, reduce_unroll=1), dict(TWO, reduce_unroll=1)):
        out = gpu_eval(cfg, tun)
        assert out["result"].n_partials == min(256, (n + BLOCK - 1) // BLOCK)
        assert record(out) == want, tun
        check_parity(cfg, out, refout)


def test_captured_launch_replays_the_same_bits(oracle_mod, golden):
    import cavitymd
    n = 131_073
    cfg = make_cfg(n, "photon_last")
    want = golden[case_key(n, "photon_last")]
    sysdef = to_device(cfg)
    p = cfg["params"]
    comp = cavitymd.CavityForceComputeHIP(sysdef, p["omegac"], p["couplstr"], p["phmass"])
    for k, v in ONE.items():
        comp.workspace.set_tunable(k, v)
    comp.compute(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        comp.compute(1)
    for _ in range(3):
        comp.getForceArray().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        out = {"force": comp.getForceArray().cpu().numpy(), "result": comp.getResult()}
        assert record(out) == want
