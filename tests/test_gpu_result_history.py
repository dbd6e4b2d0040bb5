"""Result history on the GPU (cavmd_result_at / cavmd_energies_at / cavmd_last_sequence, cavitymd.EnergyHistory): every
evaluation publishes into its own slot of a ring in mapped host memory, so a tracker can enqueue step k and read step k - 1
without waiting for step k.  Checked here: the deferred reads return the very bytes the synchronous reads return, on every
launch shape; the ring's bounds; that a read does not wait for a newer (starved) evaluation; that an evaluation that never
published is reported and never replaced by another one's block; graph capture; EnergyHistory end to end."""
import ctypes
import time

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi, synthetic

pytestmark = pytest.mark.gpu

PRM = (0.0091, 1e-3, 1.0)


def _cfg(n, seed, photon_at, L=(31.0, 17.5, 23.25)):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(L)
    tid = rng.integers(0, 2, n).astype(np.int32)
    charge = rng.uniform(-1, 1, n)
    tid[photon_at] = 2
    charge[photon_at] = 0.0
    image = rng.integers(-3, 4, (n, 3)).astype(np.int32)
    return {"name": f"rand{n}", "seed": seed, "position": pos, "typeid": tid, "charge": charge, "image": image,
            "types": ["O", "N", "L"], "box": L, "L_typeid": 2,
            "params": {"omegac": PRM[0], "couplstr": PRM[1], "phmass": PRM[2]}}


class Frames:
    """Device arrays of a pseudo-trajectory (synthetic.perturb steps), in both layouts the C ABI takes."""

    def __init__(self, cfg, count):
        self.n = len(cfg["charge"])
        self.box = cfg["box"]
        self.pos, self.xyz, self.tid, self.img, self.cfgs = [], [], [], [], []
        self.chg = torch.from_numpy(cfg["charge"]).cuda()
        cur = cfg
        for k in range(count):
            if k:
                cur = synthetic.perturb(cur, k, amplitude=0.05)
            self.cfgs.append(cur)
            tag = cavitymd.state.type_tag_as_double(cur["typeid"])[:, None]
            self.pos.append(torch.from_numpy(np.concatenate([cur["position"], tag], axis=1)).cuda())
            self.xyz.append(torch.from_numpy(np.ascontiguousarray(cur["position"])).cuda())
            self.img.append(torch.from_numpy(cur["image"]).cuda())
        self.tid = torch.from_numpy(cfg["typeid"]).cuda()
        self.prm = _capi.make_params(*PRM)

    def __len__(self):
        return len(self.pos)

    def hoomd(self, ws, k, frc):
        f = k % len(self)
        ws.compute_hoomd(0, self.n, self.pos[f].data_ptr(), self.chg.data_ptr(), self.img[f].data_ptr(), self.box, 2,
                         self.prm, frc.data_ptr())

    def soa(self, ws, k, frc):
        """packed (N,3) / (N,) arrays: the strided two-launch route of cavmd_compute_soa"""
        f = k % len(self)
        ws.compute_soa(0, self.n, (self.xyz[f].data_ptr(), 24), (self.tid.data_ptr(), 4), (self.img[f].data_ptr(), 12),
                       (self.chg.data_ptr(), 8), self.box, 2, self.prm, (frc.data_ptr(), 24))


def _fingerprint(frc):
    """bit pattern of a force array folded into one int64 (wrapping sum), enqueued on the same stream as the evaluations"""
    return frc.view(torch.int64).sum()


@pytest.mark.parametrize("n,route,tun", [(501, "hoomd", {}), (60_001, "hoomd", {}), (1_000_001, "hoomd", {}),
                                          (60_001, "hoomd", {"persistent": 0}), (60_001, "soa", {})],
                         ids=["small_system", "single_launch_6e4", "single_launch_1e6", "two_launches", "soa_packed"])
def test_deferred_reads_are_the_bytes_of_synchronous_reads(n, route, tun):
    """1000 steps of a pseudo-trajectory (a cycle of frames at the larger sizes) on one workspace.  Run A reads result() after every step; run B, on a fresh workspace
    and the same inputs, reads result_at(k - 1) after enqueuing step k and flushes at the end.  Every result block, and the
    forces of every step, byte for byte the same."""
    steps = 1000
    frames = Frames(_cfg(n, seed=n + 3, photon_at=n // 2), steps if n <= 1000 else (32 if n <= 60_001 else 8))
    width = 3 if route == "soa" else 4
    frc = torch.empty((n, width), dtype=torch.float64, device="cuda")
    run = getattr(frames, route)

    def workspace():
        ws = _capi.Workspace(n)
        for k, v in tun.items():
            ws.set_tunable(k, v)
        return ws

    ws = workspace()
    blocks_a, prints_a = [], []
    for k in range(steps):
        run(ws, k, frc)
        prints_a.append(_fingerprint(frc))
        blocks_a.append(bytes(ws.result()))
    ws = workspace()
    blocks_b, prints_b = [], []
    for k in range(steps):
        run(ws, k, frc)
        prints_b.append(_fingerprint(frc))
        assert ws.last_sequence() == k + 1
        if k:
            blocks_b.append(bytes(ws.result_at(k)))
    blocks_b.append(bytes(ws.result_at(steps)))
    assert len(blocks_b) == steps
    for k in range(steps):
        assert blocks_a[k] == blocks_b[k], f"step {k}"
        assert _capi.Result.from_buffer_copy(blocks_b[k]).sequence == k + 1
    assert torch.equal(torch.stack(prints_a), torch.stack(prints_b))


def test_ring_bounds_depth_changes_and_empty_systems():
    n = 60_001
    frames = Frames(_cfg(n, seed=5, photon_at=17), 2)
    frc = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    want = []
    ref_ws = _capi.Workspace(n)
    for f in range(2):
        frames.hoomd(ref_ws, f, frc)
        want.append(ref_ws.result())
    ws = _capi.Workspace(n)
    assert ws.get_tunable("result_history") == 64
    with pytest.raises(_capi.CavmdError) as e:
        ws.result_at(1)
    assert e.value.status == _capi.CAVMD_ERR_NOT_COMPUTED
    assert ws.last_sequence() == 0
    for bad in (0, 1, 16385, -1):
        with pytest.raises(_capi.CavmdError) as e:
            ws.set_tunable("result_history", bad)
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    ws.set_tunable("result_history", 4)
    assert ws.get_tunable("result_history") == 4
    for k in range(10):                       # evaluations 1..10, no read in between
        frames.hoomd(ws, k, frc)
    assert ws.last_sequence() == 10
    for s in range(7, 11):
        r = ws.result_at(s)
        assert r.sequence == s
        w = want[(s - 1) % 2]
        assert bytes(r)[:152] == bytes(w)[:152] and bytes(r)[160:] == bytes(w)[160:]
    for s, status in ((6, _capi.CAVMD_ERR_EXPIRED), (1, _capi.CAVMD_ERR_EXPIRED), (11, _capi.CAVMD_ERR_INVALID_VALUE),
                      (0, _capi.CAVMD_ERR_INVALID_VALUE)):
        with pytest.raises(_capi.CavmdError) as e:
            ws.result_at(s)
        assert e.value.status == status, s
        with pytest.raises(_capi.CavmdError) as e:
            ws.energies_at(s)
        assert e.value.status == status, s
    # depth changed while evaluations are queued: the last one's block is carried over, earlier ones expire
    for k in range(10, 20):
        frames.hoomd(ws, k, frc)
    ws.set_tunable("result_history", 32)
    last = want[(20 - 1) % 2]
    e = (ctypes.c_double * 3)(*ws.energies())
    assert bytes(e) == bytes(last.energy)
    r = ws.result()
    assert r.sequence == 20 and bytes(r.dipole) == bytes(last.dipole)
    assert bytes(ws.result_at(20)) == bytes(r)
    for s in (19, 17, 12):
        with pytest.raises(_capi.CavmdError) as ei:
            ws.result_at(s)
        assert ei.value.status == _capi.CAVMD_ERR_EXPIRED
    frames.hoomd(ws, 20, frc)
    assert ws.result_at(21).sequence == 21 and ws.result_at(20).sequence == 20
    # N = 0 consumes no sequence
    ws.compute_hoomd(0, 0, frames.pos[0].data_ptr(), frames.chg.data_ptr(), frames.img[0].data_ptr(), frames.box, 2,
                     frames.prm, frc.data_ptr())
    assert ws.last_sequence() == 21
    assert ws.result_at(21).sequence == 21


def test_a_deferred_read_does_not_wait_for_the_newest_evaluation():
    """Evaluation k starts ~20 ms late (hooks build: one block of the single-launch grid is held back, the others give up
    and leave, the late block completes the evaluation alone).  Reading k - 1 must not wait for it; reading k then returns
    the repaired result, bit for bit the two-launch path's."""
    n = 60_001
    frames = Frames(_cfg(n, seed=41, photon_at=n // 3), 2)
    frc = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    ref_ws = _capi.Workspace(n)
    ref_ws.set_tunable("persistent", 0)
    frames.hoomd(ref_ws, 0, frc)
    want_prev = ref_ws.result()
    frames.hoomd(ref_ws, 1, frc)
    want = ref_ws.result()
    torch.cuda.synchronize()
    want_f = frc.clone()

    ws = _capi.Workspace(n, hooks=True)
    ws.set_tunable("persistent", 1)
    ws.set_tunable("debug_spin_limit", 5000)
    frames.hoomd(ws, 0, frc)                                  # k - 1: runs normally
    ws.set_tunable("debug_late_block", 0)
    ws.set_tunable("debug_late_ticks", 2_000_000)
    frc.fill_(float("nan"))
    frames.hoomd(ws, 1, frc)                                  # k: starved, repaired
    t0 = time.perf_counter()
    prev = ws.result_at(1)
    dt = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    assert dt < 5e-3, dt
    assert busy, "evaluation k had already finished: the test proves nothing"
    for field in ("dipole", "dipole_lo", "total_dipole", "energy", "photon_force", "q"):
        assert bytes(getattr(prev, field)) == bytes(getattr(want_prev, field)), field
    got = ws.result_at(2)
    assert got.sequence == 2
    for field in ("dipole", "dipole_lo", "total_dipole", "energy", "photon_force", "q", "Dq"):
        assert bytes(getattr(got, field)) == bytes(getattr(want, field)), field
    torch.cuda.synchronize()
    assert torch.equal(frc.view(torch.int64), want_f.view(torch.int64))
    assert bytes(ws.result()) == bytes(got)                   # the synchronous read agrees (and consumes the repaired flag)
    assert ws.get_tunable("sync_timeout_seen") == 1


@pytest.mark.parametrize("n,tun", [(501, {}), (60_001, {}), (60_001, {"persistent": 0})],
                         ids=["small_system", "single_launch", "two_launches"])
def test_an_unpublished_evaluation_is_an_error_and_its_neighbours_stay_readable(n, tun):
    frames = Frames(_cfg(n, seed=n + 11, photon_at=n - 1), 3)
    frc = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    ref_ws = _capi.Workspace(n)
    for k, v in tun.items():
        ref_ws.set_tunable(k, v)
    want = []
    for k in range(3):
        frames.hoomd(ref_ws, k, frc)
        want.append(bytes(ref_ws.result()))
    ws = _capi.Workspace(n, hooks=True)
    for k, v in tun.items():
        ws.set_tunable(k, v)
    frames.hoomd(ws, 0, frc)
    ws.set_tunable("debug_skip_publish", 1)                   # evaluation 2 publishes into a block the host never reads
    frames.hoomd(ws, 1, frc)
    ws.set_tunable("debug_skip_publish", 0)
    frames.hoomd(ws, 2, frc)
    with pytest.raises(_capi.CavmdError) as e:
        ws.result_at(2)
    assert e.value.status == 719                              # hipErrorLaunchFailure, never the block of another evaluation
    assert bytes(ws.result_at(1)) == want[0]
    assert bytes(ws.result_at(3)) == want[2]
    with pytest.raises(_capi.CavmdError) as e:
        ws.energies_at(2)
    assert e.value.status == 719


def test_an_evaluation_nobody_could_complete_reports_sync_timeout():
    """One block of the single-launch grid never publishes its record (hooks build): the evaluation fails.  result_at names
    it (CAVMD_ERR_SYNC_TIMEOUT, from the failure word tagged with its sequence) without consuming the workspace's flag: the
    next compute still reports the failure once, as it always has."""
    n = 60_001
    frames = Frames(_cfg(n, seed=77, photon_at=n - 1), 2)
    frc = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    ref_ws = _capi.Workspace(n)
    frames.hoomd(ref_ws, 0, frc)
    want0 = bytes(ref_ws.result())
    frames.hoomd(ref_ws, 1, frc)
    want1 = ref_ws.result()
    ws = _capi.Workspace(n, hooks=True)
    for k, v in (("persistent", 1), ("small_system_max_n", 0), ("debug_spin_limit", 5000)):
        ws.set_tunable(k, v)
    frames.hoomd(ws, 0, frc)
    ws.set_tunable("debug_silent_block", 1)
    frames.hoomd(ws, 1, frc)
    ws.set_tunable("debug_silent_block", -1)
    with pytest.raises(_capi.CavmdError) as e:
        ws.result_at(2)
    assert e.value.status == _capi.CAVMD_ERR_SYNC_TIMEOUT
    with pytest.raises(_capi.CavmdError) as e:
        ws.result_at(2)                                       # asked again: the same answer, never a stale block
    assert e.value.status == _capi.CAVMD_ERR_SYNC_TIMEOUT
    assert bytes(ws.result_at(1)) == want0
    with pytest.raises(_capi.CavmdError) as e:
        frames.hoomd(ws, 1, frc)                              # reported once by the next enqueue, which enqueues nothing
    assert e.value.status == _capi.CAVMD_ERR_SYNC_TIMEOUT
    assert ws.last_sequence() == 2
    frames.hoomd(ws, 1, frc)                                  # two launches from now on
    r = ws.result_at(3)
    assert r.sequence == 3 and bytes(r.dipole) == bytes(want1.dipole) and bytes(r.energy) == bytes(want1.energy)


def test_a_captured_workspace_has_no_history(ref, oracle_mod):
    n = 30_000
    cfg = _cfg(n, seed=12, photon_at=n - 1)
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                           cfg["box"], device="cuda")
    comp = cavitymd.CavityForceComputeHIP(cavitymd.SystemDefinition(pd), *PRM)
    comp.compute(0)
    assert comp.getResultAt(1).sequence == 1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        comp.compute(1)
    for s in range(0, comp.lastSequence() + 2):
        with pytest.raises(_capi.CavmdError) as e:
            comp.getResultAt(s)
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE, s
    rp = ref.make_params(*PRM)
    cur = cfg
    for rep in range(1, 4):
        cur = synthetic.perturb(cur, rep, amplitude=0.5)
        pd.getPositions().copy_(torch.from_numpy(oracle_mod.pack_pos(cur["position"], cur["typeid"])))
        pd.getImages().copy_(torch.from_numpy(cur["image"]))
        graph.replay()
        e = np.array(comp.getEnergies())
        want = ref.compute(oracle_mod.pack_pos(cur["position"], cur["typeid"]), cur["charge"], cur["image"], cur["box"], 2, rp)
        assert np.allclose(e, want["energies"], rtol=1e-10, atol=0)
        with pytest.raises(_capi.CavmdError) as ei:
            comp.getEnergiesAt(comp.lastSequence())
        assert ei.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    comp.compute(5)                                           # eager evaluations after a capture: still no history
    with pytest.raises(_capi.CavmdError) as ei:
        comp.getResultAt(comp.lastSequence())
    assert ei.value.status == _capi.CAVMD_ERR_INVALID_VALUE


def test_energy_history_rows_equal_the_synchronous_getters():
    """cavitymd.EnergyHistory over 200 steps of a CavityForce whose positions change every step: the drained rows are bit for
    bit what the per-step synchronous getters of an identical second run return."""
    steps = 200
    cfg = synthetic.config1(seed=7)
    frames = [cfg]
    for k in range(1, 8):
        frames.append(synthetic.perturb(frames[-1], k, amplitude=0.05))

    def run(deferred):
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        p = cfg["params"]
        force = cavitymd.CavityForce(kvector=[0, 0, 1], couplstr=p["couplstr"], omegac=p["omegac"], phmass=p["phmass"])
        force.attach(cavitymd.SystemDefinition(pd))
        comp = force._force_impl
        pos = [pd.getPositions().clone() for _ in frames]
        img = [pd.getImages().clone() for _ in frames]
        for k, c in enumerate(frames):
            pos[k][:, :3].copy_(torch.from_numpy(c["position"]))
            img[k].copy_(torch.from_numpy(c["image"]))
        history = cavitymd.EnergyHistory(comp)
        rows = []
        for s in range(steps):
            pd.getPositions().copy_(pos[s % len(frames)])
            pd.getImages().copy_(img[s % len(frames)])
            comp.compute(s)
            if deferred:
                history.record(s)
                rows += history.drain()
                assert len(history) == 1
            else:
                rows.append((s,) + tuple(comp.getEnergies()))
        if deferred:
            rows += history.flush()
            assert len(history) == 0 and history.flush() == []
        return rows

    a = run(False)
    b = run(True)
    assert [r[0] for r in b] == list(range(steps))
    assert np.array(a).tobytes() == np.array(b).tobytes()
    assert len({r[1:] for r in a}) > 1                        # the energies do change from step to step
