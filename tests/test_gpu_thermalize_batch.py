"""The start of a batch on the device (cavmd_thermalize_*, cavitymd.BatchThermalizer).  Run with `-m gpu` on an MI355X.

The contract is the list of expressions in include/cavmd.h; tests/thermalize_mirror.py restates it in element-wise numpy and
derives the bounds used here (log and cospi differ between host and device; everything else is compared bit for bit);
tests/thermalize_cases.py builds the inputs, which tests/test_thermalize_abi.py runs through the mirror alone:
  1. one ragged batch against the mirror, shape by shape, every member variant and planted mass counted;
  2. the momentum: from the device's own velocities of 1 and its own P, bit for bit; P within 2 ulp of math.fsum;
  3. the photon: q = 0 and finite q, g = 0 and g != 0, no photon, a stale result block;
  4. an item's bytes do not depend on its place in a batch; a captured launch replays like eager calls and follows set_items;
  5. the velocities are Maxwell-Boltzmann, and with zero_momentum on no momentum is left."""
import copy
import math

import numpy as np
import pytest
import torch

import cavitymd
import thermalize_cases as cases
import thermalize_mirror as mirror
from cavitymd import _capi
from gpu_support import bits as _u64
from gpu_support import same as _same

pytestmark = pytest.mark.gpu

EPS = mirror.EPS


def _ulps(got, exact) -> float:
    """|got - exact| in units of the spacing of doubles at `exact` (as tests/test_gpu_ledger.py has it)"""
    if got == exact:
        return 0.0
    return abs(got - exact) / float(np.spacing(abs(np.float64(exact))))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _thermalizer(systems, **kw):
    vel = [_cuda(s["vel"]) for s in systems]
    th = cavitymd.BatchThermalizer(vel, [s["kT"] for s in systems], seeds=[s["seed"] for s in systems],
                                   members=[s["members"] for s in systems], **kw)
    return th, vel


# ---- 1. and 2. one ragged batch -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    """the ragged batch run twice on the device: without zero_momentum, then after reset() and set_items with it"""
    systems = cases.ragged()
    th, vel = _thermalizer(systems, zero_momentum=False)
    assert th.thermalizer.launch_order == sorted(range(len(systems)), key=lambda k: -systems[k]["N"])
    th.thermalize()
    state0 = th.state()
    v0 = [v.cpu().numpy() for v in vel]
    th.reset()
    th.update(zero_momentum=True)                                            # cavmd_thermalize_set_items
    th.thermalize()
    state1 = th.state()
    v1 = [v.cpu().numpy() for v in vel]
    th.close()
    th.close()                                                               # twice
    return dict(systems=systems, state0=state0, v0=v0, state1=state1, v1=v1)


def test_one_ragged_batch_equals_the_mirror_shape_by_shape(ragged):
    assert cases.T == _capi.THERMALIZE_TILE and set(cases.VARIANTS) == {"null", "subset", "planted", "empty", "beyond", "subset_planted"}
    assert sorted(cases.SIZES) == sorted({0, 1, 2, 255, 256, 257, cases.T - 1, cases.T, cases.T + 1, 2 * cases.T + 1})
    worst = 0.0
    for k, s in enumerate(ragged["systems"]):
        want = copy.deepcopy(s)
        state = mirror.new_state()
        run = mirror.thermalize(want, state)
        got, st = ragged["v0"][k], ragged["state0"][k]
        where = (k, s["N"], cases.VARIANTS[k])
        if s["N"] == 0:
            assert st.tobytes() == bytes(64), where                          # untouched, its state included
            continue
        assert (int(st["draws"]), int(st["thermalised"]), int(st["skipped"]), int(st["photon"])) \
            == (1, state["thermalised"], state["skipped"], -1), where
        assert not st["momentum"].any(), where
        assert _same(got[:, 3], s["vel"][:, 3]), where                       # the bytes of .w
        written = run["written"]
        untouched = np.setdiff1d(np.arange(s["N"]), written)
        assert _same(got[untouched], s["vel"][untouched]), where
        if len(written):
            err = np.abs(got[written, :3] - want["vel"][written, :3])
            assert np.isfinite(got[written, :3]).all() and (err <= run["bound"][written]).all(), (where, err.max())
            assert not _same(got[written, :3], s["vel"][written, :3]), where
            worst = max(worst, float((err / np.abs(want["vel"][written, :3])).max()))
    print(f"worst |device - mirror| / |v| over the batch: {worst:.3e} (bound {mirror.VELOCITY_REL:.3e})")
    counts = [(int(st["thermalised"]), int(st["skipped"])) for st in ragged["state0"]]
    T = cases.T
    assert counts[:7] + counts[8:] == [(1, 0), (2, 0), (85, 0), (252, 4), (0, 0), (100, 3), (T, 0), (2 * T + 1, 0), (0, 0)]
    assert counts[7][1] == 4 and (T + 1) // 3 - 4 <= counts[7][0] <= (T + 1) // 3


def test_the_momentum_goes_out_bit_for_bit_from_the_devices_own_numbers(ragged):
    worst = 0.0
    for k, s in enumerate(ragged["systems"]):
        v0, v1, st = ragged["v0"][k], ragged["v1"][k], ragged["state1"][k]
        where = (k, s["N"], cases.VARIANTS[k])
        if s["N"] == 0:
            assert st.tobytes() == bytes(64), where
            continue
        first = ragged["state0"][k]
        assert (int(st["draws"]), int(st["thermalised"]), int(st["skipped"])) == (1, int(first["thermalised"]), int(first["skipped"])), where
        written, _ = mirror.member_set(s, -1)
        n = len(written)
        assert n == int(st["thermalised"])
        P = np.array(st["momentum"], dtype=np.float64)
        if n == 0:
            assert not P.any() and _same(v1, v0), where
            continue
        want = v0.copy()
        mirror.remove_momentum(want, written, P)                             # v0 - (P / n) / m, the device's own v0 and P
        assert _same(v1, want), where
        for c in range(3):
            addends = v0[written, 3] * v0[written, c]
            exact = math.fsum(addends.tolist())
            assert math.fsum(np.abs(addends).tolist()) / abs(exact) <= 2.0 ** 40, where   # what the bound presupposes
            worst = max(worst, _ulps(float(P[c]), exact))
            assert _ulps(float(P[c]), exact) <= 2.0, (where, c, P[c], exact)
    print(f"worst P: {worst:.2f} ulp from math.fsum")


# ---- 3. the photon --------------------------------------------------------------------------------------------------------------
def test_the_photon_is_placed_as_the_driver_places_it():
    configs = cases.photon_configs()
    B = len(configs)
    keys = [mirror.item_key(cases.SEED, k) for k in range(B)]
    sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"],
                                                                          cfg["image"], cfg["types"], cfg["box"]))
               for _, cfg, _ in configs]
    cavity = cavitymd.CavityForceBatch(sysdefs, [cfg["params"] for _, cfg, _ in configs])
    vel = [_cuda(v) for _, _, v in configs]
    pos = [sd.getParticleData().getPositions() for sd in sysdefs]
    image = [sd.getParticleData().getImages() for sd in sysdefs]
    pos0 = [p.cpu().numpy().copy() for p in pos]
    image0 = [i.cpu().numpy().copy() for i in image]

    # a stale result block (nothing evaluated yet: n_particles = 0 != N): no photon, every particle thermalised, nothing placed
    th = cavitymd.BatchThermalizer(vel, cases.KT, seeds=keys, cavity=cavity, place_photon=True, finite_q=True, zero_momentum=False)
    th.thermalize()
    st = th.state()
    for k, (name, cfg, v) in enumerate(configs):
        n = len(v)
        assert (int(st[k]["photon"]), int(st[k]["thermalised"]), int(st[k]["skipped"])) == (-1, n, 0), name
        assert _same(pos[k].cpu().numpy(), pos0[k]) and np.array_equal(image[k].cpu().numpy(), image0[k]), name
        item = cases.photon_item(cfg, v, keys[k], np.zeros(3), n_particles=0, place_photon=True, finite_q=True)
        run = mirror.thermalize(item, mirror.new_state())
        assert (np.abs(vel[k].cpu().numpy()[:, :3] - item["vel"][:, :3]) <= run["bound"]).all(), name
    th.close()

    cavity.compute()
    torch.cuda.synchronize()
    results = cavity.results()
    for finite_q in (False, True):
        for k, (_, _, v) in enumerate(configs):
            vel[k].copy_(_cuda(v))
        th = cavitymd.BatchThermalizer(vel, cases.KT, seeds=keys, cavity=cavity, place_photon=True, finite_q=finite_q,
                                       zero_momentum=False)
        before = [p.cpu().numpy().copy() for p in pos]
        th.thermalize()
        st = th.state()
        for k, (name, cfg, v) in enumerate(configs):
            where = (name, finite_q)
            n, r = len(v), results[k]
            has_photon = cases.PHOTON_SYSTEMS[k][3]
            assert int(r.n_particles) == n and (int(r.photon_idx) == n - 1) == has_photon
            item = cases.photon_item(cfg, v, keys[k], np.array(r.dipole[:]), place_photon=True, finite_q=finite_q)
            item["pos"][:, :] = before[k]
            state = mirror.new_state()
            run = mirror.thermalize(item, state)                             # fed the device's own result.dipole
            got_v, got_p, got_i = vel[k].cpu().numpy(), pos[k].cpu().numpy(), image[k].cpu().numpy()
            assert (int(st[k]["photon"]), int(st[k]["thermalised"]), int(st[k]["skipped"]), int(st[k]["draws"])) \
                == (state["photon"], state["thermalised"], 0, 1), where
            assert state["photon"] == (n - 1 if has_photon else -1) and state["thermalised"] == (n - 1 if has_photon else n)
            assert (np.abs(got_v[:, :3] - item["vel"][:, :3]) <= run["bound"]).all() and _same(got_v[:, 3], v[:, 3]), where
            if not has_photon:
                assert run["photon"] is None and _same(got_p, before[k]) and np.array_equal(got_i, image0[k]), where
                continue
            p, placed, L = n - 1, run["photon"], np.asarray(cfg["box"])
            assert not placed["ambiguous"], where
            assert np.array_equal(got_i[p], placed["image"]), (where, got_i[p], placed["image"])
            err = np.abs(got_p[p, :3] - placed["pos"])
            print(f"{name}, finite_q {finite_q}: x {placed['x']}, image {placed['image']}, |device - mirror| {err} (bound {placed['bound']})")
            assert (err <= placed["bound"]).all(), (where, err, placed["bound"])
            assert (got_p[p, :3] >= -L / 2).all() and (got_p[p, :3] < L / 2).all(), where
            assert _u64(got_p[p, 3]) == _u64(before[k][p, 3]), where          # pos.w keeps its bits
            assert _same(got_p[:p], before[k][:p]) and np.array_equal(got_i[:p], image0[k][:p]), where
            if cfg["params"]["couplstr"] == 0.0:                             # no spread, and (-d) * 0 / K is a zero
                assert not got_p[p, :3].any() and not got_i[p].any(), where
            elif finite_q:
                assert got_i[p, :2].any() and got_p[p, 2] != 0.0, where
        th.close()
    cavity.close()


# ---- 4. independence and replay -------------------------------------------------------------------------------------------------
def test_an_items_bytes_do_not_depend_on_its_place_in_the_batch():
    systems = [s for s in cases.ragged() if s["N"] in (1, 2, 255, 257, cases.T + 1, 2 * cases.T + 1)]
    outputs = []
    for order in (list(range(len(systems))), [3, 5, 0, 4, 1, 2]):
        th, vel = _thermalizer([systems[k] for k in order], zero_momentum=True)
        th.thermalize()
        st = th.state()
        outputs.append({k: (vel[place].cpu().numpy().tobytes(), st[place].tobytes()) for place, k in enumerate(order)})
        th.close()
    for k in range(len(systems)):
        assert outputs[0][k] == outputs[1][k], (k, systems[k]["N"])


def test_three_replays_equal_three_eager_calls_and_set_items_is_followed():
    systems = [s for s in cases.ragged() if s["N"] in (2, 257, cases.T + 1)]
    th, vel = _thermalizer(systems, zero_momentum=True)
    kT = [s["kT"] for s in systems]

    def snapshot():
        torch.cuda.synchronize()
        return [v.cpu().numpy().copy() for v in vel]

    eager = []
    for _ in range(3):
        th.thermalize()
        eager.append(snapshot())
    th.update(kT=[4.0 * x for x in kT])
    th.thermalize()
    eager.append(snapshot())
    assert th.state()["draws"].tolist() == [4] * len(systems)

    th.update(kT=kT)
    th.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        th.thermalize()
        with pytest.raises(_capi.CavmdError) as e:                           # the stream of the last launch is capturing
            th.update(kT=kT)
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert th.state()["draws"].tolist() == [0] * len(systems)                # a capture runs nothing
    replayed = []
    for _ in range(3):
        graph.replay()
        replayed.append(snapshot())
    th.update(kT=[4.0 * x for x in kT])                                      # the captured launch finds the new rows
    graph.replay()
    replayed.append(snapshot())
    assert th.state()["draws"].tolist() == [4] * len(systems)
    for r in range(4):
        for k in range(len(systems)):
            assert _same(replayed[r][k], eager[r][k]), (r, k)
    for a in range(4):
        for b in range(a + 1, 4):
            for k, s in enumerate(systems):                                  # (the empty list of N = 257 writes nothing)
                assert _same(replayed[a][k], replayed[b][k]) == (len(mirror.member_set(s, -1)[0]) == 0), (a, b, k)
    # 4 kT doubles sigma exactly, and with it every later operation: the fourth block, at the old kT, times two
    th.update(kT=kT)
    th.reset()
    for _ in range(4):
        th.thermalize()
    old = snapshot()
    for k, s in enumerate(systems):
        written, _ = mirror.member_set(s, -1)
        assert _same(replayed[3][k][written, :3], 2.0 * old[k][written, :3]), k
    # the lifetime rule: cavmd_destroy refuses while the object lives
    assert th._need()._lib.cavmd_destroy(th.workspace.handle) == _capi.CAVMD_ERR_INVALID_VALUE
    th.thermalize()
    assert th.state()["draws"].tolist() == [5] * len(systems)
    th.close()


# ---- 5. Maxwell-Boltzmann ---------------------------------------------------------------------------------------------------------
def test_the_velocities_are_maxwell_boltzmann_and_no_momentum_is_left():
    B, N = cases.STAT_B, cases.STAT_N
    host = np.zeros((B, N, 4))
    host[..., 3] = cases.stat_masses()
    all_vel = _cuda(host)
    vel = [all_vel[k] for k in range(B)]
    th = cavitymd.BatchThermalizer(vel, cases.KT, seed=cases.STAT_SEED, zero_momentum=False)
    assert th.keys == [mirror.item_key(cases.STAT_SEED, k) for k in range(B)]
    th.thermalize()
    assert th.state()["thermalised"].tolist() == [N] * B
    got = all_vel.cpu().numpy()
    assert _same(got[..., 3], host[..., 3])
    print()
    for name, (deviation, bound) in cases.bands(cases.standardised(got, cases.KT)).items():
        print(f"{name}: {deviation:.3e} (bound {bound:.3e})")
        assert deviation <= bound, name
    th.reset()
    th.update(zero_momentum=True)
    th.thermalize()
    st = th.state()
    got = all_vel.cpu().numpy()
    worst = 0.0
    for k in range(B):
        for c in range(3):
            addends = got[k, :, 3] * got[k, :, c]
            left, scale = abs(math.fsum(addends.tolist())), math.fsum(np.abs(addends).tolist())
            worst = max(worst, left / scale)
            assert left <= 8.0 * EPS * scale, (k, c, left, scale)
    assert st["momentum"].all() and st["draws"].tolist() == [1] * B
    print(f"worst |sum m v| / sum |m v| with zero_momentum: {worst:.3e} (bound {8.0 * EPS:.3e})")
    th.close()
