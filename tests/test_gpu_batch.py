"""A batch of independent small systems in ONE launch (cavmd_batch_*, cavitymd.CavityForceBatch) on the GPU.  Run with
`-m gpu` on an MI355X.

Contract checked here: every system's force array and result block are, byte for byte (the sequence number apart), what
cavmd_compute_hoomd gives for that system alone through its single-block kernel; independently of that, parity with the CPU
oracle at the tolerances tests/test_gpu_parity.py states (restated below):
  P1 dipole    |d_gpu - d_ref|_inf <= 1e-10 * |d_ref|_inf, and within 2 ulp of the correctly rounded sum
  P2 energies  each of E_h, E_c, E_d: relative <= 1e-10
  P3 forces    |F_gpu - F_ref| <= 1e-10 * S_i,  S_i = g|c_i|(|q_xy|_inf + (g/K)|d_xy|_inf) for molecules,
               S_L = K|q|_inf + g|d_xy|_inf for the photon
  P4 accuracy  |F_gpu - F_exact| <= |F_ref - F_exact| + 1e-14 * S_i   (exact = correctly rounded dipole)
  P5 structure F.z == 0 and F.w == 0 exactly for molecules, every entry written, no photon -> all zeros
Also: items are independent, the item order does not leak, the per-item result history, graph capture, set_items, a side
stream, the Python classes end to end, and that one evaluation is one kernel dispatch."""
import csv
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi, replicas, synthetic
from parity_support import random_cfg as _random_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
PRM = {"omegac": 0.0091, "couplstr": 1e-3, "phmass": 1.0}
GUARD = 4                                    # guard rows (32 B each) before and after every force array
GUARD_VALUE = -7.25


class Dev:
    """One system's device arrays in HOOMD's layouts, the force array NaN-filled between guard rows."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.n = len(cfg["charge"])
        tag = cavitymd.state.type_tag_as_double(cfg["typeid"])[:, None]
        self.pos = torch.from_numpy(np.concatenate([cfg["position"], tag], axis=1).reshape(self.n, 4)).cuda()
        self.chg = torch.from_numpy(np.ascontiguousarray(cfg["charge"], dtype=np.float64)).cuda()
        self.img = torch.from_numpy(np.ascontiguousarray(cfg["image"], dtype=np.int32).reshape(self.n, 3)).cuda()
        self.store = torch.full((self.n + 2 * GUARD, 4), GUARD_VALUE, dtype=torch.float64, device="cuda")
        self.frc = self.store[GUARD:GUARD + self.n]
        self.frc.fill_(float("nan"))
        p = cfg["params"]
        self.prm = _capi.make_params(p["omegac"], p["couplstr"], p["phmass"])
        self.box = tuple(float(x) for x in cfg["box"])

    def item(self, force=None):
        f = self.frc if force is None else force
        return _capi.batch_item(self.n, self.pos.data_ptr(), self.chg.data_ptr(), self.img.data_ptr(), f.data_ptr(), self.box,
                                self.cfg["L_typeid"], self.prm)

    def guards_intact(self):
        g = self.store.cpu().numpy()
        return bool(np.all(g[:GUARD] == GUARD_VALUE) and np.all(g[GUARD + self.n:] == GUARD_VALUE))

    def alone(self):
        """(force bytes, result block) of cavmd_compute_hoomd on a private workspace, through the single-block kernel."""
        out = torch.full((max(self.n, 1), 4), float("nan"), dtype=torch.float64, device="cuda")
        ws = _capi.Workspace(max(self.n, 1))
        ws.set_tunable("small_system_max_n", max(self.n, 1024))
        ws.compute_hoomd(0, self.n, self.pos.data_ptr(), self.chg.data_ptr(), self.img.data_ptr(), self.box,
                         self.cfg["L_typeid"], self.prm, out.data_ptr())
        torch.cuda.synchronize()
        res = ws.result()
        assert res.n_partials == 1                             # the single-block kernel ran, not another path
        return out[:self.n].cpu().numpy().tobytes(), res


def _block_equal(a, b):
    """two cavmd_result blocks byte-equal except `sequence` (offset 152, 8 bytes)"""
    a, b = bytes(a), bytes(b)
    return a[:152] == b[:152] and a[160:] == b[160:]


def _ragged_systems():
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 501, 1023, 1024, 1025, 4095, 4096, 4097, 20001]
    cfgs = []
    for k, n in enumerate(sizes):
        if n == 0:
            cfgs.append(_random_cfg(0, seed=1))
            continue
        where = [0, n // 2, n - 1, None][k % 4]               # photon first / middle / last / absent
        cfgs.append(_random_cfg(n, seed=n * 7 + k, photon_at=where))
    several = _random_cfg(3000, seed=9, photon_at=100)        # several L-typed particles: only the first is the photon
    for extra in (0, 99, 101, 2500, 2999):
        several["typeid"][extra] = 2
    several["typeid"][0] = 0
    cfgs.append(several)
    cfgs.append(_random_cfg(3000, seed=3, photon_at=1234, photon_charge=7.5))          # a charged photon
    cfgs.append(_random_cfg(4000, seed=21, photon_at=3999, image_range=1 << 20))       # large images
    cfgs.append(_random_cfg(501, seed=77, photon_at=500, L=(40.0, 41.0, 42.0)))        # another box
    return cfgs


# ---- 1. bit equality with the single path -----------------------------------------------------------------------------
def test_ragged_batch_is_bit_equal_to_the_single_path():
    devs = [Dev(c) for c in _ragged_systems()]
    ws = _capi.Workspace(1)
    batch = _capi.Batch(ws, [d.item() for d in devs], history_depth=4)
    assert batch.launch_order == sorted(range(len(devs)), key=lambda i: -devs[i].n)
    batch.compute(0)
    assert batch.last_sequence() == 1
    res = batch.results()
    torch.cuda.synchronize()
    for k, d in enumerate(devs):
        assert d.guards_intact(), (k, d.n)
        got = res[k]
        assert got.sequence == 1 and got.n_particles == d.n
        if d.n == 0:
            assert got.photon_idx == -1 and got.n_photon_typed == 0 and got.n_partials == 0
            blank = _capi.Result()
            blank.photon_idx = -1
            assert _block_equal(got, blank)
            continue
        want_f, want_r = d.alone()
        assert d.frc.cpu().numpy().tobytes() == want_f, (k, d.n)
        assert _block_equal(got, want_r), (k, d.n)
        assert not np.isnan(d.frc.cpu().numpy()).any()


# ---- 2. parity with the oracle ---------------------------------------------------------------------------------------
def _ref_eval(ref, oracle_mod, cfg):
    p = ref.make_params(cfg["params"]["omegac"], cfg["params"]["couplstr"], cfg["params"]["phmass"])
    pos4 = oracle_mod.pack_pos(cfg["position"], cfg["typeid"])
    out = ref.compute(pos4, cfg["charge"], cfg["image"], cfg["box"], cfg["L_typeid"], p)
    out["params"] = p
    if out["photon_idx"] >= 0:
        hi, _ = ref.dipole_exact(pos4, cfg["charge"], cfg["image"], cfg["box"], out["photon_idx"])
        out["dipole_exact"] = hi
    return out


def _force_scales(cfg, refout):
    p = refout["params"]
    g, K = p["couplstr"], p["K"]
    pidx = refout["photon_idx"]
    q = cfg["position"][pidx] + cfg["image"][pidx] * np.asarray(cfg["box"])
    d = refout["dipole"]
    S = g * np.abs(cfg["charge"]) * (np.abs(q[:2]).max() + (g / K) * np.abs(d[:2]).max())
    S[pidx] = K * np.abs(q).max() + g * np.abs(d[:2]).max()
    return S


def _forces_from_dipole(cfg, refout, d):
    p = refout["params"]
    g, K = p["couplstr"], p["K"]
    pidx = refout["photon_idx"]
    q = cfg["position"][pidx] + cfg["image"][pidx] * np.asarray(cfg["box"])
    Dq = np.array([q[0] + (g / K) * d[0], q[1] + (g / K) * d[1]])
    F = np.zeros((len(cfg["charge"]), 4))
    s = (-g) * cfg["charge"]
    F[:, 0] = s * Dq[0]
    F[:, 1] = s * Dq[1]
    F[cfg["typeid"] == cfg["L_typeid"]] = 0.0
    F[pidx, :3] = [-K * q[0] - g * d[0], -K * q[1] - g * d[1], -K * q[2] - g * 0.0]
    return F


def _check_parity(cfg, force, res, refout, tol=1e-10):
    assert res.photon_idx == refout["photon_idx"]
    assert not np.isnan(force).any(), "force entries left unwritten"
    d_ref, d_gpu, d_exact = refout["dipole"], np.array(res.dipole[:]), refout["dipole_exact"]
    assert np.abs(d_gpu - d_ref).max() <= tol * np.abs(d_ref).max() + 1e-300                          # P1
    assert np.all(np.abs(d_gpu - d_exact) <= 2 * np.spacing(np.abs(d_exact)) + 1e-300)
    for k in range(3):                                                                               # P2
        e_ref, e_gpu = refout["energies"][k], res.energy[k]
        assert abs(e_gpu - e_ref) <= tol * abs(e_ref) + 1e-300, ("energy", k, e_gpu, e_ref)
    S = _force_scales(cfg, refout)                                                                   # P3
    diff = np.abs(force[:, :3] - refout["force"][:, :3])
    assert np.all(diff <= tol * S[:, None] + 1e-300), float((diff / (S[:, None] + 1e-300)).max())
    F_exact = _forces_from_dipole(cfg, refout, d_exact)                                              # P4
    err_gpu = np.abs(force[:, :3] - F_exact[:, :3])
    err_ref = np.abs(refout["force"][:, :3] - F_exact[:, :3])
    assert np.all(err_gpu <= err_ref + 1e-14 * S[:, None] + 1e-300)
    mol = np.ones(len(S), dtype=bool)                                                                # P5
    mol[refout["photon_idx"]] = False
    assert np.all(force[mol, 2] == 0.0) and np.all(force[:, 3] == 0.0)


def test_64_config1_seeds_against_the_oracle(ref, oracle_mod):
    cfgs = [synthetic.config1(seed=s) for s in range(1, 65)]
    devs = [Dev(c) for c in cfgs]
    ws = _capi.Workspace(1)
    batch = _capi.Batch(ws, [d.item() for d in devs])
    batch.compute(0)
    res = batch.results()
    torch.cuda.synchronize()
    for k, (cfg, d) in enumerate(zip(cfgs, devs)):
        assert res[k].n_particles == 501 and res[k].photon_idx == 500
        _check_parity(cfg, d.frc.cpu().numpy(), res[k], _ref_eval(ref, oracle_mod, cfg))
        assert d.guards_intact()


# ---- 3. / 4. independence and order -----------------------------------------------------------------------------------
def test_items_are_independent():
    cfgs = [_random_cfg(n, seed=100 + n, photon_at=n - 1) for n in (501, 64, 1500, 501, 257, 5000)]
    devs = [Dev(c) for c in cfgs]
    ws = _capi.Workspace(1)
    batch = _capi.Batch(ws, [d.item() for d in devs])
    batch.compute(0)
    before_r = [bytes(r) for r in batch.results()]
    torch.cuda.synchronize()
    before_f = [d.frc.cpu().numpy().tobytes() for d in devs]
    devs[2].pos[:, :3] += 0.125                                                 # one item's positions change
    batch.compute(0)
    after_r = [bytes(r) for r in batch.results()]
    torch.cuda.synchronize()
    for k, d in enumerate(devs):
        same = _block_equal(before_r[k], after_r[k]) and d.frc.cpu().numpy().tobytes() == before_f[k]
        assert same == (k != 2), k
    # one item without a photon zeroes only itself
    devs[3].pos[500, 3] = 0.0                                                   # type tag 0: no particle of type L left
    batch.compute(0)
    res = batch.results()
    torch.cuda.synchronize()
    for k, d in enumerate(devs):
        f = d.frc.cpu().numpy()
        if k == 3:
            assert res[k].photon_idx == -1 and not f.any() and not any(res[k].energy[:]) and not any(res[k].dipole[:])
        else:
            assert _block_equal(res[k], after_r[k]) and f.tobytes() == (before_f[k] if k != 2 else f.tobytes())
            assert res[k].photon_idx == d.n - 1 and f.any()


def test_item_order_does_not_leak():
    cfgs = [_random_cfg(n, seed=200 + k, photon_at=n // 2) for k, n in enumerate((501, 501, 17, 4097, 1024, 300, 2, 20001, 501))]
    perm = [5, 0, 8, 3, 1, 7, 2, 6, 4]
    out = []
    for order in (list(range(len(cfgs))), perm):
        devs = [Dev(cfgs[i]) for i in order]
        ws = _capi.Workspace(1)
        batch = _capi.Batch(ws, [d.item() for d in devs])
        assert batch.launch_order == sorted(range(len(devs)), key=lambda i: -devs[i].n)
        batch.compute(0)
        res = batch.results()
        torch.cuda.synchronize()
        out.append({order[k]: (bytes(res[k]), devs[k].frc.cpu().numpy().tobytes()) for k in range(len(devs))})
    assert out[0] == out[1]


# ---- 5. history -------------------------------------------------------------------------------------------------------
class Frames:
    """B systems of config 1 whose positions cycle through `count` perturbed frames (device copies, enqueued in order)."""

    def __init__(self, B, count, n_molecular=500):
        self.cfgs = [synthetic.diatomic_box(n_molecular, seed=s + 1, box_length=40.0) for s in range(B)]
        self.devs = [Dev(c) for c in self.cfgs]
        self.pos, self.img = [], []
        cur = list(self.cfgs)
        for f in range(count):
            if f:
                cur = [synthetic.perturb(c, f, amplitude=0.05) for c in cur]
            self.pos.append([torch.from_numpy(c["position"]).cuda() for c in cur])
            self.img.append([torch.from_numpy(c["image"]).cuda() for c in cur])

    def load(self, f):
        f %= len(self.pos)
        for k, d in enumerate(self.devs):
            d.pos[:, :3].copy_(self.pos[f][k])
            d.img.copy_(self.img[f][k])


def test_deferred_reads_equal_synchronous_reads_over_300_steps():
    steps, B = 300, 6
    frames = Frames(B, 8)

    def run(deferred):
        ws = _capi.Workspace(1)
        batch = _capi.Batch(ws, [d.item() for d in frames.devs], history_depth=16)
        rows = []
        for k in range(steps):
            frames.load(k)
            batch.compute(0)
            assert batch.last_sequence() == k + 1
            if not deferred:
                rows.append(np.array([r.energy[:] for r in batch.results()]))
            elif k:
                rows.append(batch.energies_at(k))             # step k - 1, after enqueuing step k
        if deferred:
            rows.append(batch.energies_at(steps))
        return np.stack(rows)

    a, b = run(False), run(True)
    assert a.shape == (steps, B, 3) and a.tobytes() == b.tobytes()
    assert len({a[k].tobytes() for k in range(8)}) == 8         # the energies do change from step to step
    assert not np.array_equal(a[0, 0], a[0, 1])                 # ... and from system to system


def test_ring_bounds():
    frames = Frames(3, 2)
    ws = _capi.Workspace(1)
    for bad in (0, 1, 16385, -1):
        with pytest.raises(_capi.CavmdError) as e:
            _capi.Batch(ws, [d.item() for d in frames.devs], history_depth=bad)
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE, bad
    with pytest.raises(_capi.CavmdError) as e:                 # 16384 x 17 x 256 B > 64 MiB
        _capi.Batch(ws, [frames.devs[0].item()] * 17, history_depth=16384)
    assert e.value.status == _capi.CAVMD_ERR_CAPACITY
    with pytest.raises(_capi.CavmdError) as e:
        _capi.Batch(ws, [], history_depth=4)
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    depth = 4
    batch = _capi.Batch(ws, [d.item() for d in frames.devs], history_depth=depth)
    for call in (batch.results, lambda: batch.results_at(1), lambda: batch.energies_at(1)):
        with pytest.raises(_capi.CavmdError) as e:
            call()
        assert e.value.status == _capi.CAVMD_ERR_NOT_COMPUTED
    assert batch.last_sequence() == 0
    want = []
    for k in range(10):
        frames.load(k)
        batch.compute(0)
        if k < 2:
            want.append(batch.energies_at(k + 1))
    assert batch.last_sequence() == 10
    for s in range(7, 11):                                     # the last `depth` evaluations
        assert batch.energies_at(s).tobytes() == want[(s - 1) % 2].tobytes()
        assert [r.sequence for r in batch.results_at(s)] == [s] * 3
    for s, status in ((6, _capi.CAVMD_ERR_EXPIRED), (1, _capi.CAVMD_ERR_EXPIRED), (11, _capi.CAVMD_ERR_INVALID_VALUE),
                      (0, _capi.CAVMD_ERR_INVALID_VALUE)):
        for call in (batch.results_at, batch.energies_at):
            with pytest.raises(_capi.CavmdError) as e:
                call(s)
            assert e.value.status == status, s
    frames.load(0)
    batch.compute(0)                                           # 11: now 7 is exactly `depth` evaluations back
    with pytest.raises(_capi.CavmdError) as e:
        batch.results_at(7)
    assert e.value.status == _capi.CAVMD_ERR_EXPIRED
    assert [r.sequence for r in batch.results_at(8)] == [8] * 3
    assert bytes(batch.results()) == bytes(batch.results_at(11))


# ---- 6. graph capture -------------------------------------------------------------------------------------------------
def test_captured_batch_replays_on_changing_data():
    B = 5
    frames = Frames(B, 4)
    ws = _capi.Workspace(1)
    eager = _capi.Batch(ws, [d.item() for d in frames.devs])
    want = []
    for f in range(4):
        frames.load(f)
        eager.compute(0)
        res = eager.results()
        torch.cuda.synchronize()
        want.append(([bytes(r) for r in res], [d.frc.cpu().numpy().tobytes() for d in frames.devs]))
    batch = _capi.Batch(ws, [d.item() for d in frames.devs])
    frames.load(0)
    batch.compute(0)
    assert batch.results_at(1)[0].sequence == 1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.compute(torch.cuda.current_stream().cuda_stream)
    for s in range(0, batch.last_sequence() + 2):
        for call in (batch.results_at, batch.energies_at):
            with pytest.raises(_capi.CavmdError) as e:
                call(s)
            assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE, s
    for rep in range(1, 9):
        f = rep % 4
        frames.load(f)
        for d in frames.devs:
            d.frc.fill_(float("nan"))
        graph.replay()
        res = batch.results()                                  # behind a device synchronisation: right on every replay
        for k, d in enumerate(frames.devs):
            assert _block_equal(res[k], want[f][0][k]), (rep, k)
            assert d.frc.cpu().numpy().tobytes() == want[f][1][k], (rep, k)
    frames.load(2)
    batch.compute(0)                                           # eager again: still no history, results still right
    with pytest.raises(_capi.CavmdError) as e:
        batch.energies_at(batch.last_sequence())
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    res = batch.results()
    assert all(_block_equal(res[k], want[2][0][k]) for k in range(B))
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):                                 # set_items is refused while the batch's last stream is being captured
        batch.compute(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(_capi.CavmdError) as e:
            batch.set_items(0, [frames.devs[0].item()])
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    torch.cuda.synchronize()


# ---- 7. set_items, a side stream, the Python classes ------------------------------------------------------------------
def test_set_items_follows_a_box_change_and_a_moved_array():
    cfgs = [_random_cfg(n, seed=300 + n, photon_at=0) for n in (501, 800, 64)]
    devs = [Dev(c) for c in cfgs]
    ws = _capi.Workspace(1)
    batch = _capi.Batch(ws, [d.item() for d in devs])
    batch.compute(0)
    first = [bytes(r) for r in batch.results()]
    # item 1: another box; item 2: grows to 2000 particles in new arrays (the launch order changes with it)
    cfg1 = dict(cfgs[1])
    cfg1["box"] = (33.0, 19.5, 25.25)
    new1 = Dev(cfg1)
    new2 = Dev(_random_cfg(2000, seed=301, photon_at=1999))
    with pytest.raises(_capi.CavmdError) as e:
        batch.set_items(2, [new1.item(), new2.item()])         # a range that leaves the batch
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    bad = new2.item()
    bad.reserved[0] = 1
    with pytest.raises(_capi.CavmdError) as e:
        batch.set_items(1, [new1.item(), bad])                 # one refused row: nothing changes
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    batch.compute(0)
    assert all(_block_equal(a, b) for a, b in zip(first, batch.results()))
    batch.set_items(1, [new1.item(), new2.item()])
    assert batch.launch_order == [2, 1, 0]
    torch.cuda.synchronize()                                   # the uploads above ran on the default stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        batch.compute(side.cuda_stream)                        # a side stream
        res = batch.results()
    side.synchronize()
    for k, d in enumerate((devs[0], new1, new2)):
        want_f, want_r = d.alone()
        assert _block_equal(res[k], want_r) and d.frc.cpu().numpy().tobytes() == want_f, k
        assert d.guards_intact()
    assert not _block_equal(res[1], first[1])                  # the box did matter


def _replica_cfg(rid):
    return synthetic.diatomic_box(500, seed=replicas.replica_seed(rid, 0), finite_q=True, image_range=1,
                                  params=synthetic.default_params(), name=f"config5_style_replica{rid}")


def test_force_batch_and_local_batch_end_to_end(ref, oracle_mod):
    ctx = replicas.ReplicaContext(rank=0, world_size=1, local_rank=0, backend=None, device=torch.device("cuda", 0))
    fb, ids = replicas.local_batch(ctx, range(1, 9), _replica_cfg, history_depth=8)
    assert ids == list(range(1, 9)) and len(fb) == 8
    none, no_ids = replicas.local_batch(replicas.ReplicaContext(3, 4, 3, None, torch.device("cuda", 0)), [1, 2], _replica_cfg)
    assert none is None and no_ids == []
    history = fb.history(depth=8)
    with pytest.raises(ValueError):
        fb.history(depth=9)
    rows = []
    for step in range(5):
        fb.compute(step)
        history.record(step)
        rows += history.drain()
        assert len(history) == 1
    sync = fb.energies()
    rows += history.flush()
    assert [t for t, _ in rows] == list(range(5)) and rows[-1][1].tobytes() == sync.tobytes()
    assert rows[0][1].shape == (8, 3) and fb.energies_at(fb.last_sequence()).tobytes() == sync.tobytes()
    torch.cuda.synchronize()
    for k, rid in enumerate(ids):
        cfg = _replica_cfg(rid)
        res = fb.results()[k]
        _check_parity(cfg, fb.forces[k].cpu().numpy(), res, _ref_eval(ref, oracle_mod, cfg))
        # ... and the very bits of the single-system class
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        p = cfg["params"]
        one = cavitymd.CavityForceComputeHIP(cavitymd.SystemDefinition(pd), p["omegac"], p["couplstr"], p["phmass"])
        one.compute(0)
        assert _block_equal(one.getResult(), res)
        assert torch.equal(one.getForceArray().view(torch.int64), fb.forces[k].view(torch.int64))
    # one parameter set for all, per-item parameters, a box change followed through refresh()
    sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(
        c["position"], c["typeid"], c["charge"], c["image"], c["types"], c["box"], device="cuda")) for c in map(_replica_cfg, (1, 2))]
    fb2 = cavitymd.CavityForceBatch(sysdefs, synthetic.default_params())
    fb2.compute()
    e0 = fb2.energies()
    assert e0.tobytes() == fb.energies_at(fb.last_sequence())[:2].tobytes()
    fb2.setParams(1, 0.0091, 2e-3, 1.0)
    sysdefs[0].getParticleData().setGlobalBox((41.0, 41.0, 41.0))
    fb2.refresh([0])
    fb2.compute()
    e1 = fb2.energies()
    assert not np.array_equal(e1[0], e0[0]) and not np.array_equal(e1[1], e0[1])
    fb2.close()
    fb.close()


def test_pybind_batch_equals_the_ctypes_batch():
    from cavitymd import _cavitymd
    devs = [Dev(_random_cfg(n, seed=400 + n, photon_at=n - 1 if n else None)) for n in (501, 0, 77)]
    ws = _capi.Workspace(1)
    a = _capi.Batch(ws, [d.item() for d in devs])
    a.compute(0)
    want = a.results()
    torch.cuda.synchronize()
    want_f = [d.frc.cpu().numpy().tobytes() for d in devs]
    for d in devs:
        d.frc.fill_(float("nan"))
    p = PRM
    b = _cavitymd.Batch([(d.pos.data_ptr() if d.n else 0, d.chg.data_ptr() if d.n else 0, d.img.data_ptr() if d.n else 0,
                          d.frc.data_ptr() if d.n else 0, d.box[0], d.box[1], d.box[2], p["omegac"], p["couplstr"], p["phmass"],
                          d.n, 2) for d in devs], 8)
    assert len(b) == 3
    b.compute(0)
    got = b.results()
    assert b.lastSequence() == 1 and b.energiesAt(1) == [tuple(r.energy[:]) for r in want]
    torch.cuda.synchronize()
    for k, d in enumerate(devs):
        assert got[k]["dipole"] == tuple(want[k].dipole[:]) and got[k]["photon_idx"] == want[k].photon_idx
        assert d.frc.cpu().numpy().tobytes() == want_f[k]
    assert b.resultsAt(1)[0]["sequence"] == 1 and b.resultsDevicePtr() != 0


# ---- 8. one launch ----------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import torch
from cavitymd import _capi, synthetic
import cavitymd
sysdefs = []
for s in range(1, 9):
    c = synthetic.config1(seed=s)
    sysdefs.append(cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(
        c["position"], c["typeid"], c["charge"], c["image"], c["types"], c["box"], device="cuda")))
fb = cavitymd.CavityForceBatch(sysdefs, synthetic.default_params())
for step in range(100):
    fb.compute(step)
e = fb.energies()
torch.cuda.synchronize()
assert fb.last_sequence() == 100 and e.shape == (8, 3)
print("CHILD-OK")
"""


@pytest.mark.skipif(shutil.which("rocprofv3") is None, reason="rocprofv3 is not installed")
def test_one_evaluation_is_one_dispatch(tmp_path):
    """100 evaluations of an 8-system batch in a fresh child process under a kernel trace: 100 dispatches of
    cavity_batch_kernel, none of cavity_small_system_kernel."""
    child = tmp_path / "batch_child.py"
    child.write_text(CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "cav-hoomd_amd")))
    out = tmp_path / "trace"
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--",
                          sys.executable, str(child)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "CHILD-OK" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    stats = glob.glob(os.path.join(str(out), "**", "*kernel_stats.csv"), recursive=True)
    assert stats, os.listdir(str(out))
    calls = {}
    for path in stats:
        for row in csv.DictReader(open(path)):
            calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    batch_calls = sum(v for k, v in calls.items() if "cavity_batch_kernel" in k)
    single_calls = sum(v for k, v in calls.items() if "cavity_small_system_kernel" in k)
    print(f"\ndispatches: cavity_batch_kernel {batch_calls}, cavity_small_system_kernel {single_calls}")
    assert batch_calls == 100 and single_calls == 0, calls
