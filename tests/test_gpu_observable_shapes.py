"""The density-field and sum |F|/m kernels beyond one tile per wave (cavmd_observable_kernels.hpp).

Every size is derived from the CU count of the device at hand through `mirror`, a restatement of cavmd_density_field's
host arithmetic; every density call of this module first asserts that mirror against the read-only tunables
`rho_last_mapping` and `rho_last_blocks`.  A case that is meant to reach a second or third trip of a tile loop, or a
given depth of the fold, asserts from the mirror that it does: on a device that cannot meet a case's purpose the case
fails, it does not skip.

Yardsticks.  `exact_rho`: the phases k.r = (x kx + y ky) + z kz without FMA (the kernels' association),
cos / sin of them (`_terms`), summed in 80-bit np.longdouble -- at N = 850 003 that sum equals math.fsum of the same terms
to the last bit, so it stands for oracle.observables.density_field_exact at a fraction of the cost.  Bound 1e-13 * N per
component (tests/test_gpu_observables.py).  The reference expression: np.sum of cos / sin of np.dot(position, k), what
oracle.observables.density_field spells; bound 1e-12 * N.  The size sweep evaluates both for ONE array of positions and
reads the sums of its prefixes (every N of the sweep is a prefix of that array), which is what keeps this module
faster than tests/test_gpu_parity.py; the prefix form is held against the oracle's own functions at the smallest size.
Huge-argument cases are compared with the exact, same-association yardstick only: the reference expression goes
through a BLAS dot and differs from it by ulp(k.r) per huge term.

Which wave the last tile lands on: tile t belongs to wave t mod GW, and the wave of the last tile makes
floor(t / GW) + 1 = ceil(tiles / GW) trips, as many as wave 0.  The N of about 3.3 x 64 W therefore has ragged trip
counts (busiest 4, idlest 3) with its partial last tile on a wave other than wave 0, in the middle of a block."""
import ctypes
import os
import threading
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from cavitymd import _capi
from oracle import observables as obs

pytestmark = pytest.mark.gpu

kWave = 64
KC_OF = {0: 64, 1: 25, 2: 10, 3: 5}         # wavevectors per blockIdx.y
NW_OF = {0: 16, 1: 4, 2: 4, 3: 4}           # waves per block: 1024 threads lane = wavevector, 256 lane = particle
FOLD_BATCH = 16 * 8                          # density_fold_kernel: 16 waves x 8 loads in flight per trip
MAPPINGS = (0, 1, 2, 3)

Plan = namedtuple("Plan", "mapping kc nw gx gy tiles gw trips_max trips_min fold_trips last_tile_wave")

_POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
STATS = {"density_calls": 0, "force_mass_calls": 0, "largest_n": 0, "max_trips": {m: 0 for m in MAPPINGS},
         "max_fold_blocks": 0, "max_fold_trips": 0, "mixed_path_max_err_over_n": 0.0}


def mirror(n, n_k, setting, num_cu):
    """cavmd_density_field's host arithmetic: mapping, KC, grid, trips of the tile loop and of the fold loop."""
    n_chunks = (n_k + kWave - 1) // kWave
    tiles = (n + kWave - 1) // kWave
    mapping = setting if setting >= 0 else (3 if n_k * 4 < n_chunks * kWave * 3 else 0)
    nw, kc = NW_OF[mapping], KC_OF[mapping]
    cap = 4 * num_cu if mapping else num_cu
    gx = max(1, min((tiles + nw - 1) // nw, cap))
    gy = (n_k + kc - 1) // kc
    gw = gx * nw
    trips_max = (tiles + gw - 1) // gw           # wave 0
    trips_min = tiles // gw                      # wave gw - 1
    fold_trips = (gx + FOLD_BATCH - 1) // FOLD_BATCH
    return Plan(mapping, kc, nw, gx, gy, tiles, gw, trips_max, trips_min, fold_trips, (tiles - 1) % gw if tiles else 0)


def wave_capacity(num_cu):
    """W: waves of the capped grid, per mapping."""
    return {m: mirror(1 << 30, 50, m, num_cu).gw for m in MAPPINGS}


# ---- yardsticks -------------------------------------------------------------------------------------------------------
def _phases(pos, kv):
    return (pos[:, 0] * kv[0] + pos[:, 1] * kv[1]) + pos[:, 2] * kv[2]


def _terms_into(kr, c, s):
    """cos and sin of every phase: torch's CPU kernels (Sleef, <= 1 ulp over the whole range, 5 ms for 865 000 values where
    numpy's take 80 ms); within 1.2e-16 of numpy's per term, and held against the oracle's numpy forms in the sweep"""
    t, tc, ts = torch.from_numpy(kr), torch.from_numpy(c), torch.from_numpy(s)
    step = 16384          # below torch's parallel grain: the callers already run one wavevector per thread
    for lo in range(0, t.numel(), step):
        torch.cos(t[lo:lo + step], out=tc[lo:lo + step])
        torch.sin(t[lo:lo + step], out=ts[lo:lo + step])


def _terms(kr):
    kr = np.ascontiguousarray(kr, dtype=np.float64)
    c, s = np.empty_like(kr), np.empty_like(kr)
    _terms_into(kr, c, s)
    return c, s


_LOCAL = threading.local()


def _scratch(n):
    """three arrays of n doubles per worker thread, kept: a fresh allocation of this size costs more than the arithmetic"""
    if getattr(_LOCAL, "n", -1) < n:
        _LOCAL.buf, _LOCAL.n = np.empty((3, n)), n
    return _LOCAL.buf[0, :n], _LOCAL.buf[1, :n], _LOCAL.buf[2, :n]


def _phase_terms(pos_t, kv):
    """phases (x kx + y ky) + z kz of the (3, N) array pos_t and their cos / sin, in this thread's scratch"""
    a, c, s = _scratch(pos_t.shape[1])
    np.multiply(pos_t[0], kv[0], out=a)
    np.multiply(pos_t[1], kv[1], out=c)
    a += c
    np.multiply(pos_t[2], kv[2], out=c)
    a += c
    _terms_into(a, c, s)
    return a, c, s


def _exact_sums(pos, k):
    """per wavevector the two sums in np.longdouble, shape (n_k, 2)"""
    pos_t = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).T)

    def one(kv):
        _, c, s = _phase_terms(pos_t, kv)
        return c.sum(dtype=np.longdouble), s.sum(dtype=np.longdouble)
    return np.array(list(_POOL.map(one, np.asarray(k, dtype=np.float64))), dtype=np.longdouble).reshape(len(k), 2)


def _to_complex(sums):
    return sums[:, 0].astype(np.float64) + 1j * sums[:, 1].astype(np.float64)


def exact_rho(pos, k):
    return _to_complex(_exact_sums(pos, k))


class ExactBase:
    """The exact sums of one configuration; a variant that differs in a few particles is base - old terms + new terms,
    all in np.longdouble (a NaN term makes the sum NaN, as a direct evaluation would)."""

    def __init__(self, pos, k):
        self.pos, self.k = pos, np.asarray(k, dtype=np.float64)
        self.sums = _exact_sums(pos, self.k)

    def permuted(self, order):
        other = object.__new__(ExactBase)
        other.pos, other.k, other.sums = self.pos, self.k[order], self.sums[order]
        return other

    def with_changes(self, idx, new_rows):
        idx = np.asarray(idx)
        new_rows = np.asarray(new_rows, dtype=np.float64).reshape(len(idx), 3)
        sums = self.sums.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for i, kv in enumerate(self.k):
                co, so = _terms(_phases(self.pos[idx], kv))
                cn, sn = _terms(_phases(new_rows, kv))
                sums[i, 0] += cn.sum(dtype=np.longdouble) - co.sum(dtype=np.longdouble)
                sums[i, 1] += sn.sum(dtype=np.longdouble) - so.sum(dtype=np.longdouble)
        pos = self.pos.copy()
        pos[idx] = new_rows
        return pos, _to_complex(sums)


def prefix_yardsticks(pos, k, sizes):
    """{N: (exact, reference expression)} for prefixes pos[:N] of one array: the terms are evaluated once for the whole
    array; the exact sums accumulate segment by segment in np.longdouble, the reference expression's np.sum runs over
    each prefix of cos / sin of np.dot(position, k)."""
    sizes = sorted(set(sizes))
    assert sizes[-1] <= len(pos)
    pos_t = np.ascontiguousarray(pos.T)                  # (3, N): unit-stride columns
    cols = pos_t.T                                       # the same (N, 3) values, column-major, for np.dot

    def one(kv):
        a, c, s = _phase_terms(pos_t, kv)
        ex, rf = [], []
        acc_c = acc_s = np.longdouble(0)
        lo = 0
        for n in sizes:
            acc_c = acc_c + c[lo:n].sum(dtype=np.longdouble)
            acc_s = acc_s + s[lo:n].sum(dtype=np.longdouble)
            lo = n
            ex.append(complex(float(acc_c), float(acc_s)))
        np.dot(cols, kv, out=a)
        _terms_into(a, c, s)
        for n in sizes:
            rf.append(complex(np.sum(c[:n]), np.sum(s[:n])))
        return ex, rf
    rows = list(_POOL.map(one, np.asarray(k, dtype=np.float64)))
    return {n: (np.array([r[0][j] for r in rows]), np.array([r[1][j] for r in rows])) for j, n in enumerate(sizes)}


def _cmax(a, b):
    """largest difference per component; NaN anywhere counts as infinite"""
    d = np.concatenate([np.abs(a.real - b.real), np.abs(a.imag - b.imag)])
    return float("inf") if np.isnan(d).any() else float(d.max(initial=0.0))


# ---- device side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def num_cu():
    return _capi.Workspace(1).device_info()["compute_units"]


def to_device(pos, stride):
    """(N, stride / 8) doubles on the device; whatever the kernels must not read (HOOMD's .w, padding) is NaN"""
    host = np.full((len(pos), stride // 8), np.nan)
    host[:, :3] = pos
    return torch.from_numpy(host).cuda()


def density(ws, dev, n, stride, setting, n_k, num_cu, stream=0, offset_rows=0):
    """one cavmd_density_field call, its mirror assertion, its result"""
    ws.set_tunable("rho_lane_particle", setting)
    ws.density_field(stream, n, dev.data_ptr() + offset_rows * stride, stride)
    plan = mirror(n, n_k, setting, num_cu)
    assert ws.get_tunable("rho_last_mapping") == plan.mapping, (n, n_k, setting)
    assert ws.get_tunable("rho_last_blocks") == plan.gx, (n, n_k, setting)
    STATS["density_calls"] += 1
    STATS["largest_n"] = max(STATS["largest_n"], n)
    STATS["max_trips"][plan.mapping] = max(STATS["max_trips"][plan.mapping], plan.trips_max)
    STATS["max_fold_blocks"] = max(STATS["max_fold_blocks"], plan.gx)
    STATS["max_fold_trips"] = max(STATS["max_fold_trips"], plan.fold_trips)
    got = ws.density_field_read()
    assert got.shape == (n_k,)
    return got, plan


def all_mappings(ws, dev, n, stride, n_k, num_cu, exact, bound=1e-13, want_nan=None, record_mixed=False):
    """every mapping against the exact yardstick, and the four against each other within twice the bound"""
    out = {}
    worst = 0.0
    for m in MAPPINGS:
        got, plan = density(ws, dev, n, stride, m, n_k, num_cu)
        if want_nan is not None:
            assert np.all(np.isnan(got.real[want_nan]) & np.isnan(got.imag[want_nan])), (m, n)
            keep = ~want_nan
            err = _cmax(got[keep], exact[keep])
        else:
            err = _cmax(got, exact)
        print(f"N={n} n_k={n_k} stride={stride} mapping={m} grid=({plan.gx},{plan.gy}) trips={plan.trips_min}..{plan.trips_max} "
              f"err/N={err / n:.3e}")
        assert err <= bound * n, (m, n, err / n)
        worst = max(worst, err)
        out[m] = got
    if want_nan is None:
        for a in MAPPINGS:
            for b in MAPPINGS[a + 1:]:
                assert _cmax(out[a], out[b]) <= 2 * bound * n, (a, b, n)
    if record_mixed:
        STATS["mixed_path_max_err_over_n"] = max(STATS["mixed_path_max_err_over_n"], worst / n)
    return out


# ---- the sizes of the sweep, from the mirror ------------------------------------------------------------------------------
FOLD_DEPTHS = (1, 2, 15, 16, 17, 127, 128, 129)


def sweep_sizes(num_cu):
    """{N: purpose}: grid edges around 64 W, two and three-to-four trips, fold depths per block shape"""
    sizes = {}
    for w in sorted(set(wave_capacity(num_cu).values())):
        full = kWave * w
        for n in (full - 1, full, full + 1, full + 64, full + 65, 2 * full + 1):
            sizes[n] = "edge"
        ragged = int(3.3 * full) // kWave * kWave + 37
        sizes[ragged] = "ragged"
    for nw in sorted(set(NW_OF.values())):
        for gb in FOLD_DEPTHS:
            sizes.setdefault(gb * kWave * nw - 5, "fold")
    return sizes


KSETS = {"fib50": lambda: obs.fibonacci_sphere(50),
         # 67 = 2 * 25 + 17 = 6 * 10 + 7 = 13 * 5 + 2: a partial last KC-chunk for every KC, several chunks in y for every mapping,
         # and chunks that straddle wavevector 64 of the [chunk-of-64][block][2][64] partial layout (50..66, 60..66, 60..64)
         "fib67x1.7": lambda: obs.fibonacci_sphere(67) * 1.7}


@pytest.fixture(scope="module")
def base_positions(num_cu):
    n_max = max(sweep_sizes(num_cu))
    return np.random.default_rng(20261016).uniform(-20.0, 20.0, (n_max, 3))


@pytest.fixture(scope="module")
def device_positions(base_positions):
    return {stride: to_device(base_positions, stride) for stride in (24, 32, 64)}


def test_mirror_and_case_tables_reach_what_they_are_for(num_cu):
    """Pure arithmetic on the CU count: the sweep reaches >= 3 trips of the tile loop in every mapping, both sides of
    every grid edge, every fold depth, and the capped fold; the chosen wavevector counts have the chunk geometry claimed."""
    caps = wave_capacity(num_cu)
    sizes = sweep_sizes(num_cu)
    for m in MAPPINGS:
        full = kWave * caps[m]
        assert mirror(full, 50, m, num_cu).trips_max == 1 and mirror(full + 1, 50, m, num_cu).trips_max == 2
        assert mirror(full - 1, 50, m, num_cu).gx == mirror(full, 50, m, num_cu).gx == (4 * num_cu if m else num_cu)
        assert mirror(full + 64, 50, m, num_cu).tiles == caps[m] + 1 and mirror(full + 65, 50, m, num_cu).tiles == caps[m] + 2
        assert mirror(2 * full + 1, 50, m, num_cu).trips_max == 3 and mirror(2 * full + 1, 50, m, num_cu).trips_min == 2
        assert max(mirror(n, 50, m, num_cu).trips_max for n in sizes) >= 3
        ragged = [n for n, why in sizes.items() if why == "ragged" and mirror(n, 50, m, num_cu).trips_max >= 4]
        assert ragged, m
        p = mirror(ragged[0], 50, m, num_cu)
        assert p.trips_max == p.trips_min + 1 and 0 < p.last_tile_wave < p.gw - 1
        assert ragged[0] % kWave not in (0, 1, 63)
        reached = {mirror(n, 50, m, num_cu).gx for n in sizes}
        assert set(FOLD_DEPTHS) <= reached and (4 * num_cu if m else num_cu) in reached, (m, sorted(reached))
        assert {mirror(n, 50, m, num_cu).fold_trips for n in sizes} >= {1, 2}
    assert max(mirror(n, 50, 1, num_cu).fold_trips for n in sizes) >= 3      # lane = particle at the cap: > 256 blocks
    # the automatic rule decides differently for the two wavevector sets
    assert mirror(1000, 50, -1, num_cu).mapping == 0 and mirror(1000, 67, -1, num_cu).mapping == 3
    for kc in (25, 10, 5):
        assert 67 % kc and (67 + kc - 1) // kc > 1 and kWave % kc        # wavevector 64 is not the first of its chunk
    for n_k, want in ((48, 0), (49, 0), (50, 0), (64, 0), (65, 3), (95, 3), (96, 0), (128, 0), (129, 3)):
        assert mirror(10, n_k, -1, num_cu).mapping == want, n_k


@pytest.mark.parametrize("kname", sorted(KSETS))
def test_size_sweep_every_mapping(kname, num_cu, base_positions, device_positions):
    k = KSETS[kname]()
    n_k = len(k)
    sizes = sweep_sizes(num_cu)
    yard = prefix_yardsticks(base_positions, k, sizes)
    smallest = min(sizes)
    # the prefix form of both yardsticks against the oracle's own functions
    assert _cmax(yard[smallest][0], obs.density_field_exact(base_positions[:smallest], k)) <= 1e-15 * smallest
    assert _cmax(yard[smallest][1], obs.density_field(base_positions[:smallest], k)) <= 1e-14 * smallest
    ws = _capi.Workspace(1)
    assert ws.get_tunable("rho_last_mapping") == -1 and ws.get_tunable("rho_last_blocks") == -1
    for name in ("rho_last_mapping", "rho_last_blocks"):
        with pytest.raises(_capi.CavmdError) as e:
            ws.set_tunable(name, 0)
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    ws.set_wavevectors(k)
    assert ws.get_tunable("rho_last_mapping") == -1
    side = torch.cuda.Stream()
    padded = {n for n, why in sizes.items() if why == "ragged"} | {n for n in sizes if n % 1024 == 1019 and n < 20000}
    padded |= {kWave * w + 1 for w in wave_capacity(num_cu).values()}
    for n in sorted(sizes):
        exact, want = yard[n]
        res = all_mappings(ws, device_positions[24], n, 24, n_k, num_cu, exact)
        for m in MAPPINGS:
            assert _cmax(res[m], want) <= 1e-12 * n, (m, n)
            # bit-identical on repeat and on a side stream
            assert np.array_equal(density(ws, device_positions[24], n, 24, m, n_k, num_cu)[0], res[m]), (m, n)
            torch.cuda.synchronize()
            assert np.array_equal(density(ws, device_positions[24], n, 24, m, n_k, num_cu, stream=side.cuda_stream)[0], res[m])
            # other strides: the same particles in the same order -> the same bits; the NaN in .w / the padding is never read
            for stride in (32, 64) if n in padded else (32,):
                assert np.array_equal(density(ws, device_positions[stride], n, stride, m, n_k, num_cu)[0], res[m]), (m, n, stride)
        auto, plan = density(ws, device_positions[24], n, 24, -1, n_k, num_cu)
        assert plan.mapping == (0 if n_k == 50 else 3)
        assert np.array_equal(auto, res[plan.mapping])


# ---- path mixing within one call ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mix(num_cu, base_positions):
    """An all-fast configuration of W + 2 tiles: tile W is a full tile reached on the second trip (wave 0), tile W + 1 the
    partial last tile (37 particles, second trip of wave 1)."""
    caps = set(wave_capacity(num_cu).values())
    assert len(caps) == 1, "the four mappings cap at different wave counts: give each its own mixing configuration"
    w = caps.pop()
    n = kWave * w + kWave + 37
    for m in MAPPINGS:
        p = mirror(n, 7, m, num_cu)
        assert p.trips_max == 2 and p.tiles == w + 2 and p.gw == w
    return {"w": w, "n": n, "pos": base_positions[:n].copy(), "second": kWave * w, "partial": kWave * w + kWave}


def _run_variant(base, idx, rows, num_cu, want_nan_from_exact=False, ws=None):
    pos, exact = base.with_changes(idx, rows)
    ws = ws or _capi.Workspace(1)
    ws.set_wavevectors(base.k)
    dev = to_device(pos, 32)
    nan = (np.isnan(exact.real) | np.isnan(exact.imag)) if want_nan_from_exact else None
    return all_mappings(ws, dev, len(pos), 32, len(base.k), num_cu, exact, want_nan=nan, record_mixed=not want_nan_from_exact), dev


def test_one_huge_particle_anywhere(mix, num_cu):
    """|k.r| ~ 1e12 for one particle: (int)n of the fast path saturates there, so a tile that wrongly stays fast is wrong in
    the first digit.  Planted at the lanes where the 64-lane maximum / __any has to carry it, and on the second trip."""
    base = ExactBase(mix["pos"], obs.fibonacci_sphere(7))
    n, second, partial = mix["n"], mix["second"], mix["partial"]
    huge = np.array([1.3e12, -0.7e12, 2.1e12])
    spots = {"index 0": 0, "index 63": 63, "index 64": 64, "second trip, lane 0": second, "second trip, lane 63": second + 63,
             "partial tile, inside": partial + 10, "last particle": n - 1}
    assert partial + 10 < n - 1 and (n - 1) // kWave == partial // kWave
    for label, i in spots.items():
        print(label)
        _run_variant(base, [i], [huge * (1 + 0.01 * (i % 7))], num_cu)
    idx = sorted(spots.values())
    _run_variant(base, idx, [huge * (1 + 0.01 * j) for j in range(len(idx))], num_cu)


def test_value_at_the_gate_of_the_fast_path(mix, num_cu):
    """ksum * m one part in 1e9 below and above 1e8 for the largest wavevector.  Value checks only: the fast path's
    reduction is still exact there, so either choice gives a correct number."""
    k = np.vstack([obs.fibonacci_sphere(6), [[0.3, -0.4, 1.2]]])
    ksum = (0.3 + 0.4) + 1.2
    assert all((abs(v[0]) + abs(v[1])) + abs(v[2]) < ksum for v in k[:6])
    below, above = 1e8 / ksum * (1 - 1e-9), 1e8 / ksum * (1 + 1e-9)
    assert ksum * below < 1e8 and not ksum * above < 1e8
    base = ExactBase(mix["pos"], k)
    for m_coord in (below, above):
        for i in (mix["second"] + 21, mix["partial"] + 3):
            _run_variant(base, [i], [[3.0, -m_coord, 1.5]], num_cu)


def test_deciding_pair_meets_only_through_the_full_wave_maximum(mix, num_cu):
    """Lane = wavevector forms ksum * m per lane from its own wavevector and the wave-wide maximum coordinate.  One
    wavevector of |k| = 1e3 among 63 of |k| = 1e-3, one particle with a coordinate of 2e9: only that pair (2e12) is above
    1e8; every other product is below 4e6.  A maximum that is one step short of 64 lanes leaves the tile on the fast path."""
    small = obs.fibonacci_sphere(64) * 1e-3
    big = np.array([0.6, -0.5, 0.62]) * 1e3
    k0 = small.copy()
    k0[0] = big
    base0 = ExactBase(mix["pos"], k0)
    assert 2e9 * 1.73e-3 < 1e7 and 20.0 * 1.72e3 < 1e8
    for lane_particle, lane_k in ((5, 53), (53, 5), (5, 9), (37, 18)):
        # halves and 16-lane rows: (0, 0) vs (1, 3); swapped; same row; (1, 2) vs (0, 1)
        order = np.arange(64)
        order[[0, lane_k]] = order[[lane_k, 0]]
        base = base0.permuted(order)
        assert np.array_equal(base.k[lane_k], big)
        print(f"particle lane {lane_particle}, wavevector lane {lane_k}")
        _run_variant(base, [mix["second"] + lane_particle], [[-7.0, 2.0e9, 11.0]], num_cu)
        _run_variant(base, [lane_particle], [[2.0e9, 3.0, -1.0]], num_cu)


def test_fast_and_slow_chunks_of_one_tile(mix, num_cu):
    """|k| from 1e-3 to 1e1 and one of 1e6 against one particle at |r| ~ 1e6: products 1e3 .. 1e7 (fast) and 1e12 (slow).
    The large wavevector has index 67: second 64-chunk of lane = wavevector (the first stays fast), and in lane =
    particle the chunks 50..69 / 60..69 / 65..69, never first of its chunk, each behind an all-fast chunk."""
    rng = np.random.default_rng(5)
    k = obs.fibonacci_sphere(70) * 10.0 ** rng.uniform(-3, 1, 70)[:, None]
    k[67] = np.array([0.55, 0.6, -0.58]) * 1e6
    for kc in (25, 10, 5):
        assert 67 % kc != 0 and 67 // kc > 0
    assert 1.74e1 * 1.1e6 < 1e8 and 1.73e6 * 20.0 < 1e8
    base = ExactBase(mix["pos"], k)
    for i in (mix["second"] + 5, 130, mix["partial"] + 20):
        _run_variant(base, [i], [[1.1e6, 0.9e6, -0.7e6]], num_cu)     # k[67] . r = 1.55e12


def test_non_finite_input_and_recovery(mix, num_cu):
    """One NaN, one +Inf, one 1e301 (above the kernels' 1e300 finiteness guard), in a full tile and in the partial last
    tile.  NaN where the yardstick is NaN, in every mapping; the next clean call equals a fresh workspace's bit for bit."""
    k = obs.fibonacci_sphere(7)
    base = ExactBase(mix["pos"], k)
    clean_dev = to_device(mix["pos"], 32)
    fresh = _capi.Workspace(1)
    fresh.set_wavevectors(k)
    clean = {m: density(fresh, clean_dev, mix["n"], 32, m, 7, num_cu)[0] for m in MAPPINGS}
    for bad in (np.nan, np.inf, 1e301):
        for i in (mix["second"] + 7, mix["n"] - 3):
            row = mix["pos"][i].copy()
            row[0] = bad
            _, exact = base.with_changes([i], [row])
            n_nan = int((np.isnan(exact.real) | np.isnan(exact.imag)).sum())
            assert n_nan == (0 if bad == 1e301 else 7), (bad, n_nan)
            ws = _capi.Workspace(1)
            _run_variant(base, [i], [row], num_cu, want_nan_from_exact=True, ws=ws)
            for m in MAPPINGS:
                assert np.array_equal(density(ws, clean_dev, mix["n"], 32, m, 7, num_cu)[0], clean[m]), (bad, i, m)


# ---- wavevector-set geometry and workspace re-use --------------------------------------------------------------------------
NK_LIST = (1, 4, 5, 6, 9, 10, 11, 24, 25, 26, 49, 51, 63, 64, 65, 66, 70, 128, 129, 130)


def test_wavevector_counts_and_workspace_reuse(num_cu):
    rng = np.random.default_rng(11)
    pos = rng.uniform(-20.0, 20.0, (1000, 3))
    dev = to_device(pos, 24)
    kall = rng.normal(size=(130, 3))
    ws = _capi.Workspace(1)
    for n_k in NK_LIST:
        k = kall[:n_k] if n_k != 1 else np.array([[0.3, -0.4, 1.2]])
        ws.set_wavevectors(k)
        for n in (65, 1000):
            res = all_mappings(ws, dev, n, 24, n_k, num_cu, exact_rho(pos[:n], k))
            auto, plan = density(ws, dev, n, 24, -1, n_k, num_cu)
            assert np.array_equal(auto, res[plan.mapping])

    def fresh(n_k, m):
        w2 = _capi.Workspace(1)
        w2.set_wavevectors(kall[:n_k])
        return density(w2, dev, 1000, 24, m, n_k, num_cu)[0]
    want = {(n_k, m): fresh(n_k, m) for n_k in (130, 7, 65) for m in MAPPINGS}
    ws = _capi.Workspace(1)
    for n_k in (130, 7, 65, 130):
        ws.set_wavevectors(kall[:n_k])
        with pytest.raises(_capi.CavmdError) as e:                      # nothing computed for THIS set yet
            ws.density_field_read()
        assert e.value.status == _capi.CAVMD_ERR_NOT_COMPUTED
        for m in MAPPINGS:
            assert np.array_equal(density(ws, dev, 1000, 24, m, n_k, num_cu)[0], want[(n_k, m)]), (n_k, m)
    lib = _capi.load()
    one = np.zeros(3)
    for bad in (0, (1 << 20) + 1):
        assert lib.cavmd_set_wavevectors(ws.handle, bad, ctypes.c_void_p(one.ctypes.data)) == _capi.CAVMD_ERR_INVALID_VALUE
    # a refused set leaves the stored one in place
    assert np.array_equal(density(ws, dev, 1000, 24, 2, 130, num_cu)[0], want[(130, 2)])


# ---- input validation -----------------------------------------------------------------------------------------------------
def test_density_field_refuses_bad_arguments_and_goes_on(num_cu):
    rng = np.random.default_rng(13)
    pos = rng.uniform(-20.0, 20.0, (777, 3))
    dev = to_device(pos, 32)
    k = obs.fibonacci_sphere(50)
    exact = exact_rho(pos, k)
    ws = _capi.Workspace(1)
    ws.set_wavevectors(k)
    first, _ = density(ws, dev, 777, 32, 1, 50, num_cu)
    refusals = (("stride 16", dict(stride=16), _capi.CAVMD_ERR_INVALID_VALUE),
                ("stride 28", dict(stride=28), _capi.CAVMD_ERR_INVALID_VALUE),
                ("base + 4", dict(ptr=dev.data_ptr() + 4), _capi.CAVMD_ERR_INVALID_VALUE),
                ("null", dict(ptr=0), _capi.CAVMD_ERR_INVALID_VALUE),
                ("N = 2^31", dict(n=1 << 31), _capi.CAVMD_ERR_CAPACITY))     # refused before any launch
    for label, change, status in refusals:
        with pytest.raises(_capi.CavmdError) as e:
            ws.density_field(0, change.get("n", 777), change.get("ptr", dev.data_ptr()), change.get("stride", 32))
        assert e.value.status == status, label
        assert ws.get_tunable("rho_last_mapping") == 1                      # a refused call records nothing
        res = all_mappings(ws, dev, 777, 32, 50, num_cu, exact)
        assert np.array_equal(res[1], first), label
        ws.set_tunable("rho_lane_particle", 1)
        ws.density_field(0, 777, dev.data_ptr(), 32)


# ---- sum |F| / m -----------------------------------------------------------------------------------------------------------
def force_mass_sizes(num_cu):
    edge = num_cu * 1024            # the grid stops growing here: one block per CU, 1024 particles per block and trip
    return (1023, 1024, 1025, edge - 1, edge, edge + 1, 4 * edge + 1, 10_000_019)


def _fm_blocks_and_trips(n, num_cu):
    tiles = (n + 1023) // 1024
    g = max(1, min(tiles, num_cu))
    return g, (tiles + g - 1) // g, tiles // g


def test_force_mass_sum_sweep(num_cu):
    """Sizes on both sides of the grid's cap, four trips and ~1e7.  Yardsticks: oracle.observables.force_mass_sum_exact's
    terms summed in np.longdouble over prefixes (rel 1e-15), and the reference expression np.sum(norm / mass) (rel 1e-12)
    -- the oracle's own per-row loop up to N = 1025, its vectorised form sqrt((fx^2 + fy^2) + fz^2) above (the loop costs
    2 us per particle), held against the loop where both run."""
    sizes = force_mass_sizes(num_cu)
    edge = num_cu * 1024
    assert _fm_blocks_and_trips(edge, num_cu) == (num_cu, 1, 1) and _fm_blocks_and_trips(edge + 1, num_cu) == (num_cu, 2, 1)
    assert _fm_blocks_and_trips(edge - 1, num_cu)[0] == num_cu and _fm_blocks_and_trips(4 * edge + 1, num_cu)[1] == 5
    assert _fm_blocks_and_trips(sizes[-1], num_cu)[1] >= 30
    rng = np.random.default_rng(17)
    n_max = max(sizes)
    f = np.empty((n_max, 4))
    v = np.empty((n_max, 4))
    f[:, :3] = rng.uniform(-1.0, 1.0, (n_max, 3))
    f[:, 3] = 7.0
    v[:, :3] = 0.25
    v[:, 3] = rng.uniform(0.5, 50.0, n_max)
    f[5::1000, :3] = 0.0                                   # rows with F = 0 contribute nothing
    term = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]) / v[:, 3]
    assert not term[5::1000].any()
    fg, vg = torch.from_numpy(f).cuda(), torch.from_numpy(v).cuda()
    dirty_f, dirty_v = fg.clone(), vg.clone()
    dirty_f[:, 3] = float("nan")                            # what the kernel must ignore: F.w, vx, vy, vz
    dirty_v[:, :3] = float("nan")
    ws = _capi.Workspace(1)
    acc, lo = np.longdouble(0), 0
    for n in sorted(sizes):
        acc = acc + term[lo:n].sum(dtype=np.longdouble)
        lo = n
        exact = float(acc)
        got = ws.force_mass_sum(0, n, fg.data_ptr(), vg.data_ptr())
        STATS["force_mass_calls"] += 3
        STATS["largest_n"] = max(STATS["largest_n"], n)
        want = float(np.sum(term[:n]))
        print(f"force-mass N={n} blocks,trips={_fm_blocks_and_trips(n, num_cu)} rel err={abs(got - exact) / exact:.2e}")
        if n <= 1025:
            assert abs(exact - obs.force_mass_sum_exact(f[:n, :3], v[:n, 3])) <= 2.3e-16 * exact
            loop = obs.force_mass_sum(f[:n, :3], v[:n, 3])
            assert abs(want - loop) <= 1e-14 * loop
            assert abs(got - loop) <= 1e-12 * loop
        assert abs(got - exact) <= 1e-15 * exact, n
        assert abs(got - want) <= 1e-12 * want, n
        assert ws.force_mass_sum(0, n, fg.data_ptr(), vg.data_ptr()) == got                    # bit-identical on repeat
        assert ws.force_mass_sum(0, n, dirty_f.data_ptr(), dirty_v.data_ptr()) == got          # reads nothing it must ignore
    # only rows with F = 0: exactly 0
    z = torch.zeros((3000, 4), dtype=torch.float64, device="cuda")
    z[:, 3] = float("nan")
    assert ws.force_mass_sum(0, 3000, z.data_ptr(), vg.data_ptr()) == 0.0
    STATS["force_mass_calls"] += 1


def test_force_mass_sum_and_kinetic_energy_share_their_scratch(num_cu):
    """Both reductions use d_fm_part, one ticket counter and fm_sequence: alternating them on one workspace, at sizes that
    give different grids, must give each the value it has alone."""
    rng = np.random.default_rng(19)
    edge = num_cu * 1024
    n_big, n_small = edge + 1025, 3 * 1024 + 1
    f = rng.normal(size=(n_big, 4))
    v = rng.normal(size=(n_big, 4))
    v[:, 3] = rng.uniform(0.5, 50.0, n_big)
    fg, vg = torch.from_numpy(f).cuda(), torch.from_numpy(v).cuda()

    def alone(what, n):
        w = _capi.Workspace(1)
        return w.force_mass_sum(0, n, fg.data_ptr(), vg.data_ptr()) if what == "fm" else w.kinetic_energy(0, vg.data_ptr(), None, n)
    want = {(what, n): alone(what, n) for what in ("fm", "ke") for n in (n_big, n_small)}
    for n in (n_big, n_small):
        ke = 0.5 * float((v[:n, 3] * ((v[:n, 0] ** 2 + v[:n, 1] ** 2) + v[:n, 2] ** 2)).sum(dtype=np.longdouble))
        assert abs(want[("ke", n)] - ke) <= 1e-15 * ke
        fm = obs.force_mass_sum_exact(f[:n, :3], v[:n, 3]) if n == n_small else None
        assert fm is None or abs(want[("fm", n)] - fm) <= 1e-15 * fm
    ws = _capi.Workspace(1)
    for what, n in (("fm", n_big), ("ke", n_small), ("fm", n_small), ("ke", n_big), ("ke", n_big), ("fm", n_big), ("fm", n_small),
                    ("ke", n_small)) * 2:
        got = ws.force_mass_sum(0, n, fg.data_ptr(), vg.data_ptr()) if what == "fm" else ws.kinetic_energy(0, vg.data_ptr(), None, n)
        STATS["force_mass_calls"] += what == "fm"
        assert got == want[(what, n)], (what, n)


def test_zz_what_the_module_reached(num_cu):
    """Runs last: the counters of the calls made above.  The trip counts and the fold depth the whole module reaches are
    asserted here from what was run (and from the case tables alone in the first test)."""
    print("observable shapes:", {**STATS, "max_trips": dict(STATS["max_trips"])}, "CUs", num_cu)
    if STATS["density_calls"] > 1000:                       # the whole module ran, not a selection of it
        assert min(STATS["max_trips"].values()) >= 3
        assert STATS["max_fold_blocks"] == 4 * num_cu
