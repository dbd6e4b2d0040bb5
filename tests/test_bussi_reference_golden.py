"""Row f4 against the REFERENCE'S OWN C++, executed: tests/golden/bussi_reference_golden.npz (generator:
tests/golden/make_reference_bussi_golden.py, build container only) holds the inputs and outputs of
BussiReservoirThermostat::getRescalingFactorsOne (src/BussiReservoirThermostat.h:43-98, 177-225) compiled with g++ on an
arithmetic-free HOOMD stand-in (tests/stubs/hoomd_thermostat), with the variates injected: 2000 random single calls, an
edge table and three 300-step sequences with rotational degrees of freedom, the draws each call consumed, and c = exp(-dt/tau).

CPU part: the product's rule (_capi.bussi_rescale_factor), its step with the reservoir counters (_capi.bussi_step), the
oracle restatement (BussiOracle) and the variate slot order of thermostats.draw_variates, all against the executed reference,
bit for bit.  GPU part: the on-device step (cavmd_bussi_step_device) on velocity sets whose kinetic energy is exact in any
summation order, so that the device sees the fixture's K bit for bit: K, alpha, counters and velocities against the reference
with no oracle in between.

Bits are compared only where this machine's exp(-dt/tau) gives the c the reference's build computed (libm may differ);
at least 99 % of the cases must be compared.
"""
import math
import os

import numpy as np
import pytest
import torch

from abi_support import bits as _bits
from cavitymd import _capi, thermostats
from gpu_support import same_or_both_nan as _same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bussi_reference_golden.npz")


def _load():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    ic = {name: i for i, name in enumerate(d["in_cols"].tolist())}
    oc = {name: i for i, name in enumerate(d["out_cols"].tolist())}
    return d, ic, oc


FIX, IC, OC = _load()


class Call:
    """One recorded call: inputs and outputs by column name."""

    def __init__(self, row_in, row_out, name="seq"):
        self.name = name
        for k, i in IC.items():
            setattr(self, k, float(row_in[i]))
        for k, i in OC.items():
            setattr(self, k, float(row_out[i]))
        self.draws = [float(row_in[IC[f"draw{i}"]]) for i in range(4)]
        self.throws = row_out[OC["throws"]] != 0.0
        self.n_draws = int(row_out[OC["n_draws"]])
        self.kinds = [int(row_out[OC[f"kind{i}"]]) for i in range(self.n_draws)]
        self.params = [(float(row_out[OC[f"param0_{i}"]]), float(row_out[OC[f"param1_{i}"]])) for i in range(self.n_draws)]

    @property
    def c_here(self) -> float:
        return math.exp(-self.dt / self.tau) if self.tau != 0.0 else 0.0

    @property
    def c_agrees(self) -> bool:
        return _bits(self.c_here) == _bits(self.c)


CASES = [Call(FIX["case_in"][i], FIX["case_out"][i], str(FIX["case_name"][i])) for i in range(FIX["case_in"].shape[0])]
SEQS = [[Call(FIX["seq_in"][s, t], FIX["seq_out"][s, t]) for t in range(FIX["seq_in"].shape[1])]
        for s in range(FIX["seq_in"].shape[0])]


class InjectedStream:
    """A numpy.random.Generator stand-in that hands out the fixture's injected draws in order and logs what was asked."""

    def __init__(self, draws):
        self.draws = list(draws)
        self.log = []

    def standard_normal(self):
        self.log.append((0, 1.0, 0.0))
        return self.draws.pop(0)

    def gamma(self, shape, scale=1.0):
        self.log.append((1, float(shape), float(scale)))
        return self.draws.pop(0)


def _variates(call):
    rng = InjectedStream(call.draws)
    v = thermostats.draw_variates(rng, call.dof_t, call.dof_r)
    return v, rng.log


def test_fixture_covers_the_issue_cases():
    names = {c.name for c in CASES}
    assert sum(c.name == "random" for c in CASES) >= 2000
    for must in ("dt_zero", "K_t_zero_throws", "K_r_zero_throws", "c_rounds_to_one_tiny_dt", "set_T_zero_tau_zero_R_pos",
                 "K_subnormal", "K_huge", "R_zero_tau_zero", "R_negzero_tau_zero", "R_neg40_tau_zero"):
        assert must in names
    assert len(SEQS) == 3 and all(len(s) == 300 and s[0].dof_r != 0 for s in SEQS)
    rnd = [c for c in CASES if c.name == "random"]
    assert {c.dof_t for c in rnd} == {0.0, 1.0, 2.0, 3.0, 297.0, 2999997.0}
    assert {c.tau == 0.0 for c in rnd} == {True, False} and sum(c.alpha_t < 0 for c in rnd) > 50
    # the reference's own consumption: nothing for a class with 0 degrees of freedom, gamma only for more than one, the
    # translational class first -- the claim of draw_variates and include/cavmd.h, now a recorded fact
    for c in CASES + [s for seq in SEQS for s in seq]:
        if c.throws or c.dt == 0.0:
            assert c.n_draws == 0
            continue
        want = []
        for dof in (c.dof_t, c.dof_r):
            if dof != 0:
                want.append(0)
                if dof > 1:
                    want.append(1)
        assert c.kinds == want, c.name
    # edges recorded as documented
    by = {c.name: c for c in CASES}
    assert by["K_t_zero_throws"].throws and by["K_r_zero_throws"].throws and not by["K_t_zero_dof_zero"].throws
    assert _bits(by["set_T_zero_tau_zero_R_pos"].alpha_t) == _bits(-0.0)            # 0/0 in the sign term: the - branch
    assert by["R_zero_tau_zero"].alpha_t > 0 and by["R_negzero_tau_zero"].alpha_t > 0  # sign_term == 0: the + branch
    assert by["c_rounds_to_one_tiny_dt"].c == 1.0 and by["c_rounds_to_one_tiny_dt"].alpha_t == 1.0
    assert by["K_subnormal"].K_t < 2.2250738585072014e-308 and by["K_huge"].K_t > 1e300


def _compared(results):
    n_cmp, n_all = sum(results), len(results)
    assert n_cmp >= 0.99 * n_all, f"only {n_cmp} of {n_all} cases compared: this machine's exp differs from the fixture's"
    return n_cmp


def test_draw_variates_consumes_like_the_reference():
    """thermostats.draw_variates fed the fixture's stream asks for the same distributions, with the same parameters, in the
    same order as the reference, and puts each draw into the slot the reference used it for."""
    for c in CASES + [s for seq in SEQS for s in seq]:
        if c.throws or c.dt == 0.0:
            continue
        v, log = _variates(c)
        assert [k for k, _, _ in log] == c.kinds, c.name
        for (kind, p0, p1), (q0, q1) in zip(log, c.params):
            assert (p0, p1) == (q0, q1), c.name                                     # normal(sigma 1, mu 0), gamma((Nf-1)/2, 1)
        consumed = c.draws[:c.n_draws]
        slots = [i for i, dof in enumerate((c.dof_t, c.dof_t, c.dof_r, c.dof_r)) if dof != 0 and (i % 2 == 0 or dof > 1)]
        assert [v[i] for i in slots] == consumed, c.name
        assert all(v[i] == 0.0 for i in range(4) if i not in slots)


def test_rescale_factor_is_the_executed_reference_bit_for_bit(capi):
    ok = []
    for c in CASES + [s for seq in SEQS for s in seq]:
        if c.throws or c.dt == 0.0:
            continue
        ok.append(c.c_agrees)
        if not ok[-1]:
            continue
        v, _ = _variates(c)
        at = _capi.bussi_rescale_factor(c.K_t, c.dof_t, c.dt, c.set_T, c.tau, v[0], v[1])
        ar = _capi.bussi_rescale_factor(c.K_r, c.dof_r, c.dt, c.set_T, c.tau, v[2], v[3])
        assert _same(at, c.alpha_t) and _same(ar, c.alpha_r), (c.name, at, c.alpha_t, ar, c.alpha_r)
    _compared(ok)


def _counters(st):
    return (st.reservoir_translational, st.reservoir_rotational, st.instantaneous_translational, st.instantaneous_rotational)


def _want_counters(c):
    return (c.reservoir_t, c.reservoir_r, c.instantaneous_t, c.instantaneous_r)


def test_step_is_the_executed_reference_bit_for_bit(capi):
    """_capi.bussi_step: factors and all four counters, single calls on a fresh state and the sequences step by step; where
    the reference throws, CAVMD_ERR_BAD_PARAMS and the counters untouched."""
    ok = []
    for c in CASES:
        st = _capi.BussiReservoirState()
        if c.throws:
            st.reservoir_translational, st.reservoir_rotational = 1.25, -2.5      # must survive the refused call
            st.instantaneous_translational, st.instantaneous_rotational = 0.5, 0.75
            with pytest.raises(_capi.CavmdError) as e:
                _capi.bussi_step(st, c.K_t, c.dof_t, c.K_r, c.dof_r, c.dt, c.set_T, c.tau, [0.1, 1.0, 0.1, 1.0])
            assert e.value.status == _capi.CAVMD_ERR_BAD_PARAMS
            assert _counters(st) == (1.25, -2.5, 0.5, 0.75)
            continue
        ok.append(c.c_agrees or c.dt == 0.0)
        if not ok[-1]:
            continue
        v, _ = _variates(c) if c.dt != 0.0 else ([9.0, 9.0, 9.0, 9.0], None)
        f = _capi.bussi_step(st, c.K_t, c.dof_t, c.K_r, c.dof_r, c.dt, c.set_T, c.tau, v)
        assert _same(f[0], c.alpha_t) and _same(f[1], c.alpha_r), c.name
        assert all(_same(a, b) for a, b in zip(_counters(st), _want_counters(c))), (c.name, _counters(st), _want_counters(c))
    for seq in SEQS:
        if not all(c.c_agrees or c.dt == 0.0 or c.throws for c in seq):
            ok.append(False)
            continue
        ok.append(True)
        st = _capi.BussiReservoirState()
        for t, c in enumerate(seq):
            if c.throws:
                with pytest.raises(_capi.CavmdError):
                    _capi.bussi_step(st, c.K_t, c.dof_t, c.K_r, c.dof_r, c.dt, c.set_T, c.tau, [0.1, 1.0, 0.1, 1.0])
            else:
                v, _ = _variates(c) if c.dt != 0.0 else ([9.0, 9.0, 9.0, 9.0], None)
                f = _capi.bussi_step(st, c.K_t, c.dof_t, c.K_r, c.dof_r, c.dt, c.set_T, c.tau, v)
                assert _same(f[0], c.alpha_t) and _same(f[1], c.alpha_r), t
            assert all(_same(a, b) for a, b in zip(_counters(st), _want_counters(c))), t
    assert any(c.throws for seq in SEQS for c in seq) and any(c.dt == 0.0 for seq in SEQS for c in seq)
    _compared(ok)


def test_oracle_is_the_executed_reference_bit_for_bit(oracle_mod):
    """BussiOracle (oracle/bussi_ref.c), until now pinned by reading alone, against the same fixture."""
    bussi = oracle_mod.BussiOracle()
    ok = []
    for run in [[c] for c in CASES] + SEQS:
        state = np.zeros(4)
        for c in run:
            if c.throws:
                before = state.copy()
                with pytest.raises(RuntimeError):
                    bussi.step(state, c.K_t, c.dof_t, c.K_r, c.dof_r, c.dt, c.set_T, c.tau, [0.1, 1.0, 0.1, 1.0])
                assert np.array_equal(state, before)
            else:
                ok.append(c.c_agrees or c.dt == 0.0)
                if not ok[-1]:
                    break
                v, _ = _variates(c) if c.dt != 0.0 else ([9.0, 9.0, 9.0, 9.0], None)
                f = bussi.step(state, c.K_t, c.dof_t, c.K_r, c.dof_r, c.dt, c.set_T, c.tau, v)
                assert _same(f[0], c.alpha_t) and _same(f[1], c.alpha_r), c.name
            assert all(_same(a, b) for a, b in zip(state, _want_counters(c))), c.name
    _compared(ok)


# ---- GPU: the on-device step against the executed reference ---------------------------------------------------------------
def _exact_velocities(K, n, rng):
    """(n, 4) velocities + masses with 1/2 sum m v.v == K EXACTLY, in any summation order: one particle per set bit of 2K
    (a power of two m * |v|^2 with v a small integer vector times 2^e, |v|^2 in {1, 2, 4, 8} x 4^e, m a power of two); all
    terms lie within the 53 bits of 2K, so every partial sum is exact.  The other particles are at rest (mass 1)."""
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
        lo, hi = -((1023 + log2n - p) // 2), (p - log2n + 1074) // 2           # mass exponent within [-1074, 1023]
        ev = int(np.clip(rng.integers(-6, 7), lo, hi))
        sign = rng.choice([-1.0, 1.0], size=3)
        vel[j, :3] = np.array(comp, dtype=np.float64) * sign * 2.0 ** ev
        vel[j, 3] = 2.0 ** (p - log2n - 2 * ev)
    assert 0.5 * math.fsum(vel[:, 3] * (vel[:, :3] ** 2).sum(1)) == K                # exactly representable, checked by fsum
    return vel


def test_exact_velocity_sets_hit_every_fixture_K():
    rng = np.random.default_rng(3)
    for c in CASES[::7] + [c for c in CASES if c.name != "random"]:
        v = _exact_velocities(c.K_t, 64, rng)
        terms = v[:, 3] * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])  # the kernel's expression
        assert 0.5 * math.fsum(terms) == c.K_t and 0.5 * float(np.sum(terms[::-1])) == c.K_t


@pytest.mark.gpu
def test_device_step_is_the_executed_reference():
    """Every fixture case the on-device step can reach (translational class; the rotational one stays on the host path):
    last_kinetic_energy == the fixture's K, last_alpha == the fixture's alpha, the counters == the fixture's, velocities ==
    old * alpha, all bit for bit.  Single calls on a reset state; the three sequences cumulatively on one workspace."""
    rng = np.random.default_rng(17)
    runs = []   # (list of calls, cumulative)
    singles = [c for c in CASES if c.c_agrees or c.dt == 0.0]
    singles = [c for c in singles if not (c.throws and c.K_t != 0.0)]       # rotational-only throws: not on this path
    runs += [([c], False) for c in singles]
    runs += [(seq, True) for seq in SEQS if all(c.c_agrees or c.dt == 0.0 or c.throws for c in seq)]
    assert len(singles) >= 0.99 * len(CASES) - 2 and len(runs) - len(singles) == 3
    # one segment of velocities per call; every 97th call spans several tiles (and blocks of the first launch)
    calls = [c for run, _ in runs for c in run]
    sizes = [3000 if i % 97 == 5 else 64 for i in range(len(calls))]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    host = np.concatenate([_exact_velocities(c.K_t, n, rng) for c, n in zip(calls, sizes)])
    dvel = torch.from_numpy(host.copy()).cuda()
    torch.cuda.synchronize()
    ws = _capi.Workspace(max(sizes))
    stream = torch.cuda.current_stream().cuda_stream
    alphas = np.ones(len(calls))
    k = 0
    n_refused = 0
    for run, cumulative in runs:
        ws.bussi_device_reset(stream)
        steps = 0
        for c in run:
            v, _ = _variates(c) if (c.dt != 0.0 and not c.throws) else ([0.3, 1.0, 0.0, 0.0], None)
            ptr = dvel.data_ptr() + int(offs[k]) * 32
            ws.bussi_step_device(stream, ptr, None, sizes[k], c.dof_t, c.dt, c.set_T, c.tau, v[0], v[1])
            if c.throws:
                with pytest.raises(_capi.CavmdError) as e:
                    ws.bussi_device_read()
                assert e.value.status == _capi.CAVMD_ERR_BAD_PARAMS
                n_refused += 1
            st = ws.bussi_device_read()
            if c.dt != 0.0 and not c.throws:
                steps += 1
                alphas[k] = c.alpha_t
                assert _bits(st.last_kinetic_energy) == _bits(c.K_t), (c.name, st.last_kinetic_energy, c.K_t)
                assert _same(st.last_alpha, c.alpha_t), (c.name, st.last_alpha, c.alpha_t)
                assert _same(st.instantaneous_translational, c.instantaneous_t), c.name
            elif c.throws:
                assert st.last_kinetic_energy == 0.0 and st.last_alpha == 1.0
            # the reference's instantaneous counter keeps the previous step's value when it throws; the device's refused step
            # zeroes it (nothing was exchanged) -- the cumulative counter is what both leave untouched
            assert _same(st.reservoir_translational, c.reservoir_t), (c.name, st.reservoir_translational, c.reservoir_t)
            assert st.steps == steps and (not cumulative or st.refused == sum(x.throws for x in run[:run.index(c) + 1]))
            k += 1
    assert n_refused >= 2
    torch.cuda.synchronize()
    got = dvel.cpu().numpy()
    for i in range(len(calls)):
        seg, old = got[offs[i]:offs[i + 1]], host[offs[i]:offs[i + 1]]
        want = old.copy()
        if alphas[i] != 1.0:
            with np.errstate(invalid="ignore"):                              # alpha = inf: 0 * inf = NaN, as on the device
                want[:, :3] = old[:, :3] * alphas[i]
        same = (want.view(np.uint64) == seg.view(np.uint64)) | (np.isnan(want) & np.isnan(seg))
        assert same.all(), (calls[i].name, i)
    ws.close()
