"""The Bussi thermostat step of a batch of independent small systems in ONE launch (cavmd_bussi_batch_*,
cavitymd.BussiReservoirBatch) on the GPU.  Run with `-m gpu` on an MI355X.

Contract checked here: per item, velocities and state are bit for bit what cavmd_bussi_step_device gives that item alone with
the same inputs; independently of that, the executed reference (tests/golden/bussi_reference_golden.npz) in one launch, bit for
bit; items are independent and their order does not leak; the step replays from a graph behind the force batch and stays
stochastic; the read reports a refusal once; the energy bookkeeping closes; the Python class gives the loggable quantities of
B BussiReservoir objects; one step is one kernel dispatch."""
import csv
import ctypes
import glob
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
from abi_support import bits as _bits
from cavitymd import _capi, synthetic, thermostats
from gpu_support import same_bits_on_device as _same_bits
from gpu_support import same_or_both_nan as _same
from gpu_support import stream as _stream

pytestmark = pytest.mark.gpu

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bussi_reference_golden.npz")
OK, BAD = _capi.CAVMD_OK, _capi.CAVMD_ERR_BAD_PARAMS


def _rows_to_device(rows, dev_rows=None):
    """a list of BussiBatchInput -> a (B, 8) float64 device tensor holding their bytes"""
    arr = (_capi.BussiBatchInput * len(rows))(*rows)
    host = np.frombuffer(bytes(arr), dtype=np.float64).reshape(len(rows), 8).copy()
    t = torch.from_numpy(host).cuda()
    if dev_rows is not None:
        dev_rows.copy_(t)
        return dev_rows
    return t


def _single_read(ws):
    """(status, state) of cavmd_bussi_device_read, the refusal status not raised"""
    st = _capi.BussiDeviceState()
    status = ws._lib.cavmd_bussi_device_read(ws.handle, ctypes.byref(st))
    assert status in (OK, BAD), status
    return status, st


def _velocities(n_rows, rng, at_rest=False):
    v = np.zeros((max(n_rows, 1), 4))
    v[:, 3] = rng.uniform(0.5, 20.0, v.shape[0])
    if not at_rest:
        v[:, :3] = rng.normal(0.0, 1e-3, (v.shape[0], 3))
    return v


class System:
    """One item: a velocity array, an optional member list, its degrees of freedom, kT and tau."""

    def __init__(self, n_rows, rng, members=None, dof=None, at_rest=False, tau=0.5):
        self.host = _velocities(n_rows, rng, at_rest)
        self.members = None if members is None else np.ascontiguousarray(members, dtype=np.uint32)
        self.n = n_rows if members is None else len(self.members)
        self.dof = float((3 * self.n - 3 if self.n >= 2 else 3 * self.n) if dof is None else dof)
        self.tau = tau
        idx = np.arange(n_rows) if members is None else self.members.astype(np.int64)
        ke = 0.5 * float(np.sum(self.host[idx, 3] * (self.host[idx, :3] ** 2).sum(1))) if self.n else 0.0
        self.kT = 2.0 * ke / self.dof if (self.dof > 0 and ke > 0) else 1e-6
        self.vel = torch.from_numpy(self.host.copy()).cuda()           # the batch's array
        self.vel1 = torch.from_numpy(self.host.copy()).cuda()          # the single path's array
        self.mem = None if self.members is None else torch.from_numpy(self.members.view(np.int32).copy()).cuda()
        self.ws = None

    def mem_ptr(self):
        return self.mem.data_ptr() if (self.mem is not None and self.n) else 0

    def item(self, vel=None):
        v = self.vel if vel is None else vel
        return _capi.bussi_batch_item(v.data_ptr() if self.n else 0, self.mem_ptr(), self.n, self.dof)

    def draw(self, rng):
        R = float(rng.standard_normal())
        g = float(rng.gamma((self.dof - 1.0) / 2.0)) if self.dof > 1.0 else 0.0
        return R, g

    def single_step(self, dt, R, g, stream=0):
        if self.ws is None:
            self.ws = _capi.Workspace(max(self.n, 1))
        self.ws.bussi_step_device(stream, self.vel1.data_ptr(), self.mem_ptr() or None, self.n, self.dof, dt, self.kT,
                                  self.tau, R, g)


def _ragged(rng):
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 501, 1023, 1024, 1025, 2049, 4097, 20001, 65536]
    out = [System(n, rng, tau=(0.0 if k % 3 == 0 else 0.05)) for k, n in enumerate(sizes)]          # tau == 0: alpha < 0 for R < 0
    out.append(System(3000, rng, members=rng.permutation(3000)[:700], tau=0.0))                  # unsorted, sparse
    out.append(System(5000, rng, members=np.sort(rng.choice(5000, 1500, replace=False)), tau=0.2))  # sparse, two tiles
    out.append(System(2049, rng, members=rng.permutation(2049), tau=0.1))                         # every particle, shuffled
    out.append(System(64, rng, at_rest=True, dof=3.0))                                            # refused at every step
    out.append(System(100, rng, dof=0.0))                                                         # alpha == 1, counted
    out.append(System(10, rng, dof=1.0, tau=0.0))                                                 # no gamma variate
    return out


# ---- 1. bit equality with the single path -----------------------------------------------------------------------------
def test_ragged_batch_is_bit_equal_to_the_single_path_over_60_steps():
    rng = np.random.default_rng(20240601)
    systems = _ragged(rng)
    B = len(systems)
    ws = _capi.Workspace(1)
    batch = _capi.BussiBatch(ws, [s.item() for s in systems])
    assert batch.launch_order == sorted(range(B), key=lambda i: -systems[i].n)
    dev_rows = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    negative = skipped = refused_reads = 0
    for step in range(60):
        rows = []
        for k, s in enumerate(systems):
            dt = 0.0 if rng.random() < 0.15 else 0.005
            R, g = s.draw(rng)
            rows.append(_capi.bussi_batch_input_make(dt, s.kT, s.tau, R, g))
            skipped += dt == 0.0
            s.single_step(dt, R, g, _stream())
        _rows_to_device(rows, dev_rows)
        batch.step(_stream(), dev_rows.data_ptr())
        states, was_refused = batch.read(raise_refused=False)
        assert batch.last_sequence() == step + 1
        any_single_refused = False
        for k, s in enumerate(systems):
            if s.ws is None:
                continue
            status, want = _single_read(s.ws)
            any_single_refused |= status == BAD
            assert bytes(states[k]) == bytes(want), (step, k, s.n)
            negative += states[k].last_alpha < 0
        assert was_refused == any_single_refused
        refused_reads += was_refused
        for k, s in enumerate(systems):
            assert _same_bits(s.vel, s.vel1), (step, k, s.n)
    assert negative > 50 and skipped > 100 and refused_reads > 30
    st = batch.read(raise_refused=False)[0]
    assert st[0].steps == 0 and st[0].refused == 0 and st[0].last_alpha == 0.0        # the empty item was never counted
    rest = [k for k, s in enumerate(systems) if s.dof == 3.0 and s.n == 64][0]
    assert st[rest].steps == 0 and st[rest].refused > 30 and st[rest].last_alpha == 1.0
    assert np.array_equal(systems[rest].vel.cpu().numpy(), systems[rest].host)
    zero_dof = [k for k, s in enumerate(systems) if s.dof == 0.0 and s.n == 100][0]
    assert st[zero_dof].steps > 40 and st[zero_dof].last_alpha == 1.0 and st[zero_dof].reservoir_translational == 0.0
    batch.close()
    ws.close()


# ---- 2. the executed reference in one launch ------------------------------------------------------------------------------
def _load_golden():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    ic = {name: i for i, name in enumerate(d["in_cols"].tolist())}
    oc = {name: i for i, name in enumerate(d["out_cols"].tolist())}
    return d, ic, oc


class Call:
    def __init__(self, row_in, row_out, ic, oc, name="seq"):
        self.name = name
        for k, i in ic.items():
            setattr(self, k, float(row_in[i]))
        for k, i in oc.items():
            setattr(self, k, float(row_out[i]))
        self.draws = [float(row_in[ic[f"draw{i}"]]) for i in range(4)]
        self.throws = row_out[oc["throws"]] != 0.0

    @property
    def c_agrees(self) -> bool:
        here = math.exp(-self.dt / self.tau) if self.tau != 0.0 else 0.0
        return _bits(here) == _bits(self.c)

    def variates(self):
        """{normal_t, gamma_t} in the order the reference consumed its stream (translational class first; nothing for 0
        degrees of freedom, gamma only for more than one)"""
        if self.dt == 0.0 or self.throws:
            return 0.3, 1.0
        d = list(self.draws)
        R = d.pop(0) if self.dof_t != 0 else 0.0
        g = d.pop(0) if self.dof_t > 1 else 0.0
        return R, g

    def row(self):
        R, g = self.variates()
        return _capi.bussi_batch_input_make(self.dt, self.set_T, self.tau, R, g)


def _exact_velocities(K, n, rng):
    """(n, 4) velocities + masses with 1/2 sum m v.v == K EXACTLY in any summation order: one particle per set bit of 2K
    (m |v|^2 a power of two: v a small integer vector times 2^e, m a power of two); every partial sum is exact.  The other
    particles are at rest (mass 1).  The construction of tests/test_bussi_reference_golden.py."""
    vel = np.zeros((n, 4))
    vel[:, 3] = 1.0
    K2 = 2.0 * K
    if K2 == 0.0:
        return vel
    m, e = math.frexp(K2)
    M, E = int(m * 2.0 ** 53), e - 53
    bits = [i + E for i in range(53) if (M >> i) & 1]
    assert len(bits) <= n
    slots = rng.choice(n, size=len(bits), replace=False)
    patterns = [((1, 0, 0), 0), ((0, 1, 0), 0), ((0, 0, 1), 0), ((1, 1, 0), 1), ((0, 1, 1), 1), ((2, 0, 0), 2), ((2, 0, 2), 3)]
    for p, j in zip(bits, slots):
        comp, log2n = patterns[int(rng.integers(len(patterns)))]
        lo, hi = -((1023 + log2n - p) // 2), (p - log2n + 1074) // 2
        ev = int(np.clip(rng.integers(-6, 7), lo, hi))
        sign = rng.choice([-1.0, 1.0], size=3)
        vel[j, :3] = np.array(comp, dtype=np.float64) * sign * 2.0 ** ev
        vel[j, 3] = 2.0 ** (p - log2n - 2 * ev)
    assert 0.5 * math.fsum(vel[:, 3] * (vel[:, :3] ** 2).sum(1)) == K
    return vel


def _scaled_equal(got, old, alpha):
    want = old.copy()
    if alpha != 1.0:
        with np.errstate(invalid="ignore", over="ignore"):
            want[:, :3] = old[:, :3] * alpha
    return bool(((want.view(np.uint64) == got.view(np.uint64)) | (np.isnan(want) & np.isnan(got))).all())


def test_the_executed_reference_in_one_launch():
    fix, ic, oc = _load_golden()
    cases = [Call(fix["case_in"][i], fix["case_out"][i], ic, oc, str(fix["case_name"][i])) for i in range(fix["case_in"].shape[0])]
    singles = [c for c in cases if c.c_agrees or c.dt == 0.0]
    singles = [c for c in singles if not (c.throws and c.K_t != 0.0)]       # rotational-only throws: not on this path
    assert len(singles) >= 0.99 * len(cases) - 2
    rng = np.random.default_rng(23)
    sizes = [3000 if i % 97 == 5 else 64 for i in range(len(singles))]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    host = np.concatenate([_exact_velocities(c.K_t, n, rng) for c, n in zip(singles, sizes)])
    dvel = torch.from_numpy(host.copy()).cuda()
    ws = _capi.Workspace(1)
    items = [_capi.bussi_batch_item(dvel.data_ptr() + int(offs[k]) * 32, 0, sizes[k], c.dof_t) for k, c in enumerate(singles)]
    batch = _capi.BussiBatch(ws, items)
    rows = _rows_to_device([c.row() for c in singles])
    torch.cuda.synchronize()
    batch.step(_stream(), rows.data_ptr())                                  # ONE launch for ~2000 recorded calls
    states, was_refused = batch.read(raise_refused=False)
    assert was_refused and batch.read(raise_refused=False)[1] is False      # reported once
    torch.cuda.synchronize()
    got = dvel.cpu().numpy()
    n_throw = n_skip = 0
    for k, c in enumerate(singles):
        st = states[k]
        seg, old = got[offs[k]:offs[k + 1]], host[offs[k]:offs[k + 1]]
        if c.dt == 0.0:
            n_skip += 1
            assert bytes(st) == bytes(48) and _scaled_equal(seg, old, 1.0), c.name
        elif c.throws:
            n_throw += 1
            assert st.last_kinetic_energy == 0.0 and st.last_alpha == 1.0 and st.refused == 1 and st.steps == 0
            assert st.reservoir_translational == 0.0 and _scaled_equal(seg, old, 1.0)
        else:
            assert _bits(st.last_kinetic_energy) == _bits(c.K_t), (c.name, st.last_kinetic_energy, c.K_t)
            assert _same(st.last_alpha, c.alpha_t), (c.name, st.last_alpha, c.alpha_t)
            assert _same(st.instantaneous_translational, c.instantaneous_t), c.name
            assert _same(st.reservoir_translational, c.reservoir_t), c.name
            assert st.steps == 1 and st.refused == 0
            assert _scaled_equal(seg, old, c.alpha_t), c.name
    assert n_throw >= 1 and n_skip >= 1
    batch.close()

    # the three 300-step sequences as three items stepped 300 times: every step on a fresh, exact velocity segment (set_items
    # follows it), the counters cumulative
    seqs = [[Call(fix["seq_in"][s, t], fix["seq_out"][s, t], ic, oc) for t in range(fix["seq_in"].shape[1])]
            for s in range(fix["seq_in"].shape[0])]
    seqs = [q for q in seqs if all(c.c_agrees or c.dt == 0.0 or c.throws for c in q)]
    assert len(seqs) == 3 and all(len(q) == 300 for q in seqs)
    S, T, n = len(seqs), 300, 64
    host = np.stack([np.stack([_exact_velocities(c.K_t, n, rng) for c in q]) for q in seqs])       # (S, T, n, 4)
    dvel = torch.from_numpy(host.copy()).cuda()

    def seq_items(t):
        return [_capi.bussi_batch_item(dvel[s, t].data_ptr(), 0, n, seqs[s][t].dof_t) for s in range(S)]

    batch = _capi.BussiBatch(ws, seq_items(0))
    rows = torch.zeros((S, 8), dtype=torch.float64, device="cuda")
    steps, refused = [0] * S, [0] * S
    for t in range(T):
        if t:
            batch.set_items(0, seq_items(t))
        _rows_to_device([seqs[s][t].row() for s in range(S)], rows)
        batch.step(_stream(), rows.data_ptr())
        states, _ = batch.read(raise_refused=False)
        for s in range(S):
            c = seqs[s][t]
            if c.throws:
                assert c.K_t == 0.0
                refused[s] += 1
            elif c.dt != 0.0:
                steps[s] += 1
                assert _bits(states[s].last_kinetic_energy) == _bits(c.K_t) and _same(states[s].last_alpha, c.alpha_t), (s, t)
                assert _same(states[s].instantaneous_translational, c.instantaneous_t), (s, t)
            assert _same(states[s].reservoir_translational, c.reservoir_t), (s, t)
            assert states[s].steps == steps[s] and states[s].refused == refused[s], (s, t)
    torch.cuda.synchronize()
    got = dvel.cpu().numpy()
    for s in range(S):
        for t in range(T):
            c = seqs[s][t]
            alpha = c.alpha_t if (c.dt != 0.0 and not c.throws) else 1.0
            assert _scaled_equal(got[s, t], host[s, t], alpha), (s, t)
    batch.close()
    ws.close()


# ---- 3. independence and order ----------------------------------------------------------------------------------------
def _run(systems, rows_by_step, perm=None):
    """fresh velocity copies stepped through rows_by_step in the item order `perm`; -> (velocity bytes, state bytes) by system"""
    B = len(systems)
    perm = list(range(B)) if perm is None else list(perm)
    vels = [torch.from_numpy(s.host.copy()).cuda() for s in systems]
    ws = _capi.Workspace(1)
    batch = _capi.BussiBatch(ws, [systems[i].item(vels[i]) for i in perm])
    dev_rows = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    for rows in rows_by_step:
        _rows_to_device([rows[i] for i in perm], dev_rows)
        batch.step(_stream(), dev_rows.data_ptr())
    states, _ = batch.read(raise_refused=False)
    torch.cuda.synchronize()
    out_v = [v.cpu().numpy().tobytes() for v in vels]
    out_s = [None] * B
    for pos, i in enumerate(perm):
        out_s[i] = bytes(states[pos])
    batch.close()
    ws.close()
    return out_v, out_s


def test_items_are_independent_and_their_order_does_not_leak():
    rng = np.random.default_rng(5)
    sizes = [501, 64, 2049, 501, 1, 1024, 300, 4097, 501, 0, 65, 1500]
    systems = [System(n, rng, tau=(0.0 if k % 2 else 0.3)) for k, n in enumerate(sizes)]
    B = len(systems)
    rows_by_step = []
    for step in range(5):
        rows_by_step.append([_capi.bussi_batch_input_make(0.005, s.kT, s.tau, *s.draw(rng)) for s in systems])
    base_v, base_s = _run(systems, rows_by_step)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(B)
        v, s = _run(systems, rows_by_step, perm)
        assert v == base_v and s == base_s, seed
    changed = [list(r) for r in rows_by_step]
    victim = 3
    changed[2][victim] = _capi.bussi_batch_input_make(0.005, systems[victim].kT, systems[victim].tau, -1.75, 200.0)
    v, s = _run(systems, changed)
    for k in range(B):
        assert (v[k] == base_v[k] and s[k] == base_s[k]) == (k != victim), k


# ---- 4. graph capture behind the force batch ----------------------------------------------------------------------------
def _force_items(B, n, seed):
    out = []
    for k in range(B):
        cfg = synthetic.config1(seed=seed + k) if n == 501 else synthetic.random_charged_box(n - 1, seed=seed + k)
        N = len(cfg["charge"])
        tag = cavitymd.state.type_tag_as_double(cfg["typeid"])[:, None]
        pos = torch.from_numpy(np.concatenate([cfg["position"], tag], axis=1).reshape(N, 4)).cuda()
        chg = torch.from_numpy(np.ascontiguousarray(cfg["charge"], dtype=np.float64)).cuda()
        img = torch.from_numpy(np.ascontiguousarray(cfg["image"], dtype=np.int32).reshape(N, 3)).cuda()
        frc = torch.full((N, 4), float("nan"), dtype=torch.float64, device="cuda")
        p = cfg["params"]
        prm = _capi.make_params(p["omegac"], p["couplstr"], p["phmass"])
        out.append({"N": N, "pos": pos, "chg": chg, "img": img, "frc": frc, "cfg": cfg, "prm": prm})
    return out


def _fitem(d):
    return _capi.batch_item(d["N"], d["pos"].data_ptr(), d["chg"].data_ptr(), d["img"].data_ptr(), d["frc"].data_ptr(),
                            tuple(float(x) for x in d["cfg"]["box"]), d["cfg"]["L_typeid"], d["prm"])


def test_force_batch_and_thermostat_batch_replay_from_one_graph():
    B, REPLAYS = 6, 50
    rng = np.random.default_rng(77)
    fsys = _force_items(B, 501, seed=40)
    systems = [System(d["N"], rng, tau=(0.0 if k == 1 else 0.1)) for k, d in enumerate(fsys)]
    rows_host = torch.zeros((REPLAYS, B, 8), dtype=torch.float64).pin_memory()
    for r in range(REPLAYS):
        arr = (_capi.BussiBatchInput * B)(*[_capi.bussi_batch_input_make(0.0 if (r == 7 and k == 2) else 0.005, s.kT, s.tau,
                                                                           *s.draw(rng)) for k, s in enumerate(systems)])
        rows_host[r].numpy()[:] = np.frombuffer(bytes(arr), dtype=np.float64).reshape(B, 8)
    ws = _capi.Workspace(1)
    # eager: 50 steps of force batch + thermostat batch on the single-path copies of the velocities
    fb = _capi.Batch(ws, [_fitem(d) for d in fsys])
    tb = _capi.BussiBatch(ws, [s.item(s.vel1) for s in systems])
    rows = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    want_v, want_s = [], []
    for r in range(REPLAYS):
        rows.copy_(rows_host[r], non_blocking=True)
        fb.compute(_stream())
        tb.step(_stream(), rows.data_ptr())
        want_s.append([bytes(x) for x in tb.read(raise_refused=False)[0]])
        torch.cuda.synchronize()
        want_v.append([s.vel1.cpu().numpy().tobytes() for s in systems])
    want_f = [d["frc"].cpu().numpy().tobytes() for d in fsys]
    assert not any(np.isnan(d["frc"].cpu().numpy()).any() for d in fsys)
    tb.close()
    # captured: a linear graph {force batch, thermostat batch} on one stream, the input rows refreshed before every replay
    tb = _capi.BussiBatch(ws, [s.item(s.vel) for s in systems])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fb.compute(_stream())
        tb.step(_stream(), rows.data_ptr())
        with pytest.raises(_capi.CavmdError) as e:                         # set_items is refused while that stream is capturing
            tb.set_items(0, [systems[0].item(systems[0].vel)])
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert tb.last_sequence() == 1
    alphas = []
    for r in range(REPLAYS):
        for d in fsys:
            d["frc"].fill_(float("nan"))
        rows.copy_(rows_host[r], non_blocking=True)                         # asynchronous, on the stream the replay goes to
        graph.replay()
        states = tb.read(raise_refused=False)[0]                            # behind a device synchronisation
        assert [bytes(x) for x in states] == want_s[r], r
        alphas.append(states[0].last_alpha)
        for k, s in enumerate(systems):
            assert s.vel.cpu().numpy().tobytes() == want_v[r][k], (r, k)
            assert fsys[k]["frc"].cpu().numpy().tobytes() == want_f[k], (r, k)
    assert len(set(alphas)) == REPLAYS                                      # still stochastic: a fresh alpha on every replay
    assert tb.read(raise_refused=False)[0][2].steps == REPLAYS - 1          # the row skipped at replay 7 was not counted
    tb.close()
    fb.close()
    ws.close()


# ---- 5. read semantics ------------------------------------------------------------------------------------------------------
def test_read_reset_set_items_and_lifetime():
    rng = np.random.default_rng(9)
    rest = System(64, rng, at_rest=True, dof=3.0)
    live = System(501, rng)
    ws = _capi.Workspace(1)
    batch = _capi.BussiBatch(ws, [rest.item(), live.item()])
    lib = ws._lib
    out = (_capi.BussiDeviceState * 2)()
    assert lib.cavmd_bussi_batch_read(batch.handle, out) == OK and bytes(out) == bytes(96)        # before any step: zeros
    rows = _rows_to_device([_capi.bussi_batch_input_make(0.005, s.kT, s.tau, 0.4, 700.0) for s in (rest, live)])
    for bad_ptr in (0, rows.data_ptr() + 4):
        assert lib.cavmd_bussi_batch_step(batch.handle, None, ctypes.c_void_p(bad_ptr)) == _capi.CAVMD_ERR_INVALID_VALUE
    assert batch.last_sequence() == 0
    batch.step(_stream(), rows.data_ptr())
    out = (_capi.BussiDeviceState * 2)()
    assert lib.cavmd_bussi_batch_read(batch.handle, out) == BAD                                     # reported ...
    assert out[0].refused == 1 and out[0].steps == 0 and out[0].last_alpha == 1.0                  # ... with `out` filled
    assert out[1].refused == 0 and out[1].steps == 1 and out[1].last_kinetic_energy > 0
    assert lib.cavmd_bussi_batch_read(batch.handle, out) == OK and out[0].refused == 1              # ... once
    with pytest.raises(_capi.CavmdError) as e:
        batch.step(_stream(), rows.data_ptr())
        batch.read()
    assert e.value.status == BAD
    # the device states for consumers that stay on the GPU: a stable, aligned device address
    p = batch.state_device_ptr()
    assert p and p % 8 == 0 and batch.state_device_ptr() == p
    # reset: counters to zero, in stream order; the next step counts from there
    batch.reset(_stream())
    assert bytes(batch.read()) == bytes(96)
    batch.step(_stream(), rows.data_ptr())
    st, refused = batch.read(raise_refused=False)
    assert refused and st[0].refused == 1 and st[1].steps == 1
    assert st[1].reservoir_translational == st[1].instantaneous_translational
    # set_items follows a reallocated velocity array; a refused row changes nothing
    moved = live.vel.clone()
    before_old = live.vel.clone()
    bad = live.item(moved)
    bad.reserved[1] = 1
    with pytest.raises(_capi.CavmdError):
        batch.set_items(0, [rest.item(), bad])
    with pytest.raises(_capi.CavmdError):
        batch.set_items(1, [live.item(moved), live.item(moved)])          # leaves the batch
    batch.set_items(1, [live.item(moved)])
    batch.step(_stream(), rows.data_ptr())
    st, _ = batch.read(raise_refused=False)
    torch.cuda.synchronize()
    assert _same_bits(live.vel, before_old)                               # the old array is no longer touched
    assert st[1].steps == 2 and not _same_bits(moved, before_old)         # the counters went on, the new array moved
    want = before_old.cpu().numpy()
    want[:, :3] *= st[1].last_alpha
    assert moved.cpu().numpy().tobytes() == want.tobytes()
    # destroying the workspace before its thermostat batch is an error, and harmless
    assert lib.cavmd_destroy(ws.handle) == _capi.CAVMD_ERR_INVALID_VALUE
    assert ws.device_info()["compute_units"] >= 64                        # the condition of the bit equality, and ws is alive
    batch.step(_stream(), rows.data_ptr())
    assert batch.read(raise_refused=False)[0][1].steps == 3
    batch.close()
    ws.close()
    assert not ws.handle.value


# ---- 6. the bookkeeping closes ------------------------------------------------------------------------------------------
def test_bookkeeping_closes_over_1000_steps():
    """Per item: sum of the instantaneous shares == the cumulative counter == KE_0 - KE_end, at the tolerance
    tests/test_bussi_reservoir.py uses for the same identity on the single path (rel 1e-9, abs 1e-12 KE_0)."""
    rng = np.random.default_rng(31)
    systems = [System(501, rng, tau=0.5) for _ in range(6)] + [System(2049, rng, tau=0.05), System(64, rng, tau=0.0)]
    B = len(systems)

    def ke(s):
        v = s.vel.cpu().numpy()
        return 0.5 * math.fsum(v[:, 3] * (v[:, :3] ** 2).sum(1))

    ke0 = [ke(s) for s in systems]
    ws = _capi.Workspace(1)
    batch = _capi.BussiBatch(ws, [s.item() for s in systems])
    rows = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    total = [0.0] * B
    for step in range(1000):
        _rows_to_device([_capi.bussi_batch_input_make(0.005, s.kT, s.tau, *s.draw(rng)) for s in systems], rows)
        batch.step(_stream(), rows.data_ptr())
        st = batch.read()
        for k in range(B):
            total[k] += st[k].instantaneous_translational
    torch.cuda.synchronize()
    for k, s in enumerate(systems):
        assert st[k].steps == 1000 and st[k].refused == 0
        print(f"item {k}: sum inst {total[k]!r} cumulative {st[k].reservoir_translational!r} KE0-KEend {ke0[k] - ke(s)!r}")
        assert total[k] == pytest.approx(st[k].reservoir_translational, rel=1e-9, abs=1e-12 * ke0[k])
        assert st[k].reservoir_translational == pytest.approx(ke0[k] - ke(s), rel=1e-9, abs=1e-12 * ke0[k])
    batch.close()
    ws.close()


# ---- 7. the Python class --------------------------------------------------------------------------------------------------
QUANTITIES = ("reservoir_energy_translational", "reservoir_energy_rotational", "total_reservoir_energy",
              "instantaneous_reservoir_translational", "instantaneous_reservoir_rotational", "instantaneous_reservoir_total")


def test_reservoir_batch_equals_b_single_reservoirs():
    rng = np.random.default_rng(13)
    systems = [System(501, rng, tau=0.5), System(64, rng, tau=0.0), System(4000, rng, members=rng.permutation(4000)[:1500], tau=0.2),
               System(1025, rng, tau=0.1), System(10, rng, dof=1.0, tau=0.3)]
    B = len(systems)
    kTs = [s.kT for s in systems[:-1]] + [lambda ts: 1e-6 * (1 + ts)]        # one callable of the timestep among numbers
    tb = cavitymd.BussiReservoirBatch(kT=kTs, tau=[s.tau for s in systems])
    assert tb.reservoir_energy_translational.shape == (0,)
    tb.attach([s.vel for s in systems], [s.dof for s in systems], members=[s.members for s in systems])
    assert tb.inputs.shape == (B, 8) and tb.inputs.dtype == torch.float64 and tb.inputs.is_cuda
    tb.step_async()                                                          # before any inputs: every row skips
    assert all(x.steps == 0 for x in tb.device_state())
    singles = []
    for s, kT in zip(systems, kTs):
        th = thermostats.BussiReservoir(kT, s.tau)
        th.attach(s.host.shape[0], members=s.members)
        singles.append(th)
    for ts in range(20):
        dt = 0.0 if ts == 11 else 0.005
        var = np.array([s.draw(rng) for s in systems])
        tb.set_inputs(ts, dt, var)
        tb.step_async()
        for s, th, v in zip(systems, singles, var):
            th.step_async(ts, dt, s.vel1, s.dof, variates=[v[0], v[1], 0.0, 0.0])
        for name in QUANTITIES:
            got = getattr(tb, name)
            want = np.array([getattr(th, name) for th in singles])
            assert got.shape == (B,) and got.tobytes() == want.tobytes(), (ts, name)
        for k, s in enumerate(systems):
            assert _same_bits(s.vel, s.vel1), (ts, k)
    assert [x.steps for x in tb.device_state()] == [19] * B
    tb.reset_reservoir_energy()
    assert not tb.total_reservoir_energy.any() and [x.steps for x in tb.device_state()] == [0] * B
    tb.detach()
    for th in singles:
        th.detach()


def test_draw_inputs_fills_the_rows_on_the_device():
    rng = np.random.default_rng(3)
    systems = [System(501, rng), System(100, rng, dof=0.0), System(10, rng, dof=1.0), System(2, rng, dof=3.0), System(64, rng)]
    dofs = np.array([s.dof for s in systems])
    tb = cavitymd.BussiReservoirBatch(kT=[s.kT for s in systems], tau=0.5)
    tb.attach([s.vel for s in systems], dofs.tolist())
    tb.draw_inputs(0, 0.005)
    a = tb.inputs.cpu().numpy().copy()
    tb.draw_inputs(1, 0.005)
    b = tb.inputs.cpu().numpy().copy()
    for rows in (a, b):
        assert np.isfinite(rows[:, :4]).all()
        assert np.all(rows[dofs <= 1, 1] == 0.0) and np.all(rows[dofs > 1, 1] > 0.0)      # gamma only for more than one
        assert np.all(rows[dofs == 0, 0] == 0.0) and np.all(rows[dofs != 0, 0] != 0.0)    # nothing drawn for none
        assert np.all(rows[:, 2] == math.exp(-0.005 / 0.5)) and np.array_equal(rows[:, 3], [s.kT for s in systems])
        assert not rows[:, 4:].view(np.uint64).any()
    assert np.all(a[dofs != 0, 0] != b[dofs != 0, 0]) and np.all(a[dofs > 1, 1] != b[dofs > 1, 1])
    tb.step_async()
    st = tb.device_state()
    assert [x.steps for x in st] == [1] * len(systems) and st[1].last_alpha == 1.0 and st[0].last_alpha != 1.0
    tb.draw_inputs(2, 0.0)                                                   # dt == 0: every row skips
    assert tb.inputs.cpu().numpy()[:, 4].view(np.uint64).all()
    tb.step_async()
    assert [x.steps for x in tb.device_state()] == [1] * len(systems)
    tb.detach()


# ---- 8. one step is one dispatch ----------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import numpy as np
import torch
import cavitymd
rng = np.random.default_rng(1)
vels = []
for k in range(8):
    v = np.zeros((501, 4)); v[:, 3] = 1.0; v[:, :3] = rng.normal(0, 1e-3, (501, 3))
    vels.append(torch.from_numpy(v).cuda())
tb = cavitymd.BussiReservoirBatch(kT=1e-6, tau=0.5)
tb.attach(vels, 1500.0)
for step in range(100):
    tb.set_inputs(step, 0.005, np.stack([rng.standard_normal(8), rng.gamma(749.5, size=8)], axis=1))
    tb.step_async()
st = tb.device_state()
torch.cuda.synchronize()
assert [x.steps for x in st] == [100] * 8
print("CHILD-OK")
"""


@pytest.mark.skipif(shutil.which("rocprofv3") is None, reason="rocprofv3 is not installed")
def test_one_step_is_one_dispatch(tmp_path):
    """100 steps of an 8-system batch in a fresh child process under a kernel trace: 100 dispatches of bussi_batch_kernel,
    none of the single path's two kernels."""
    child = tmp_path / "bussi_batch_child.py"
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
    batch_calls = sum(v for k, v in calls.items() if "bussi_batch_kernel" in k)
    single_calls = sum(v for k, v in calls.items() if "kinetic_partials_kernel" in k or "bussi_rescale_fused_kernel" in k)
    print(f"\ndispatches: bussi_batch_kernel {batch_calls}, single-path kernels {single_calls}")
    assert batch_calls == 100 and single_calls == 0, calls
