"""The energy ledger (cavmd_ledger_*, cavitymd.BatchEnergyLedger) on the GPU: one launch appends one 192-byte row per system --
every term of the conserved energy -- to a time series in device memory, also when that launch is replayed from a graph.

Asserted (include/cavmd.h), per item and recorded row:
  potential[t]                     within 2 ulp of math.fsum of the .w column (the bound the header states for this project's
                                   fixed-order compensated sums), for columns with sum |w| / |sum w| <= 2^40, which is asserted too
  kinetic_group, kinetic_cavity    the bits of a BatchRecorder's kinetic_energy and cavity_kinetic over the same arrays
  cavity, reservoir, time          the bytes of cavmd_batch_results_read and of the tensors the pointers name
  every derived column             the numpy float64 evaluation of its listed expression on the row's own columns, bit for bit
One ragged batch is recorded once and shared by the tests that only read it."""
import math

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi, synthetic
from gpu_support import same as _same
from gpu_support import stream as _stream

pytestmark = pytest.mark.gpu
KB = cavitymd.PhysicalConstants.KB_HARTREE_PER_K
L_TYPEID = 1
BOX = (40.0, 41.0, 42.0)
INV = _capi.CAVMD_ERR_INVALID_VALUE
DERIVED = ("cavity_potential", "potential_total", "kinetic_total", "system_total", "reservoir_total", "universe_total", "temperature")
HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=8.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=8.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=8.0)}


def _expect_status(status, call, *args):
    with pytest.raises(_capi.CavmdError) as e:
        call(*args)
    assert e.value.status == status, (call, args, e.value.status)


def _ulps(got, exact) -> float:
    """|got - exact| in units of the spacing of doubles at `exact`"""
    if got == exact:
        return 0.0
    return abs(got - exact) / float(np.spacing(abs(np.float64(exact))))


def _planted(n, rng):
    """pairs a_j, -a_j + v_j with a_j in 2^30 [1, 2) and v_j in [0.5, 1.5), shuffled: sum |w| / |sum w| is about 2^31.6"""
    pairs = n // 2
    a = 2.0 ** 30 * rng.uniform(1.0, 2.0, pairs)
    v = rng.uniform(0.5, 1.5, pairs)
    w = np.concatenate([a, -a + v, rng.uniform(0.5, 1.5, n - 2 * pairs)])
    return rng.permutation(w)


class Sys:
    """One system of a ragged batch: HOOMD-layout device arrays, a photon at a chosen place (or none), a member list, up to
    four force arrays with an energy share in .w"""

    def __init__(self, N, photon, members, n_terms, rng, planted=None):
        self.N, self.n_terms = N, n_terms
        typeid = np.zeros(N, dtype=np.int32)
        if photon is not None and N:
            typeid[{"first": 0, "middle": N // 2, "last": N - 1}[photon]] = L_TYPEID
        self.photon = int(np.flatnonzero(typeid == L_TYPEID)[0]) if (typeid == L_TYPEID).any() else -1
        pos = np.zeros((N, 4))
        pos[:, :3] = rng.uniform(-0.5, 0.5, (N, 3)) * np.array(BOX)
        pos[:, 3] = cavitymd.state.type_tag_as_double(typeid)
        chg = rng.uniform(-1.0, 1.0, N)
        if self.photon >= 0:
            chg[self.photon] = 0.0
            pos[self.photon, :3] = rng.uniform(0.5, 2.0, 3)                      # a finite q: three cavity energies that are not 0
        vel = rng.normal(0.0, 1e-3, (N, 4))
        vel[:, 3] = rng.uniform(0.5, 30.0, N)
        self.pos = torch.from_numpy(pos).cuda()
        self.chg = torch.from_numpy(chg).cuda()
        self.img = torch.from_numpy(rng.integers(-2, 3, (N, 3)).astype(np.int32)).cuda()
        self.frc = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        self.vel = torch.from_numpy(vel).cuda()
        if members == "all" or N == 0:
            self.members, self.n_members = None, N
        elif members == "sorted":
            idx = np.flatnonzero(typeid != L_TYPEID)
            self.members, self.n_members = torch.from_numpy(idx.astype(np.int32)).cuda(), len(idx)
        else:   # unsorted and sparse: a shuffled third of the particles
            idx = rng.permutation(N)[:max(N // 3, 1)]
            self.members, self.n_members = torch.from_numpy(idx.astype(np.int32)).cuda(), len(idx)
        self.w = []                                                              # host copies of the .w columns
        self.terms = []
        for t in range(n_terms):
            f = rng.normal(0.0, 1.0, (N, 4))
            f[:, 3] = _planted(N, rng) if planted == t else rng.uniform(-1.0, 0.25, N) * 10.0 ** rng.integers(-3, 4)
            self.w.append(f[:, 3].copy())
            self.terms.append(torch.from_numpy(f).cuda())
        self.params = _capi.make_params(0.0091, 1e-3, 1.0)

    def force_item(self):
        ptr = (lambda t: t.data_ptr()) if self.N else (lambda t: 0)
        return _capi.batch_item(self.N, ptr(self.pos), ptr(self.chg), ptr(self.img), ptr(self.frc), BOX, L_TYPEID, self.params)

    def recorder_item(self, result_ptr):
        return _capi.recorder_item(result_ptr, self.vel.data_ptr() if self.N else 0, 0,
                                   self.members.data_ptr() if (self.members is not None and self.n_members) else 0, 0, self.n_members)

    def ledger_item(self, result_ptr, reservoir_ptrs=(), time_ptr=0, dof=0.0, add_cavity_kinetic=0):
        return _capi.ledger_item(result_ptr, self.vel.data_ptr() if self.N else 0,
                                 self.members.data_ptr() if (self.members is not None and self.n_members) else 0, self.n_members,
                                 self.N, [t.data_ptr() for t in self.terms] if self.N else [], reservoir_ptrs, time_ptr, dof,
                                 add_cavity_kinetic)


#        N      photon    members   terms reservoirs dof     add  planted  result  time
SPEC = ((0,     None,     "all",    0,    0,         0.0,    0,   None,    True,   False),
        (1,     "first",  "all",    1,    1,         3.0,    1,   None,    True,   True),
        (255,   "middle", "sorted", 2,    3,         762.0,  1,   None,    True,   True),
        (256,   "last",   "sparse", 4,    4,         255.0,  0,   None,    True,   False),
        (257,   "first",  "all",    1,    0,         0.0,    1,   None,    True,   True),
        (1023,  "middle", "sorted", 2,    1,         3066.0, 1,   None,    True,   True),
        (1024,  "last",   "sparse", 4,    3,         1023.0, 0,   0,       True,   False),
        (1025,  "first",  "all",    1,    4,         9216.0, 1,   0,       True,   True),
        (2049,  "middle", "sorted", 2,    1,         6144.0, 0,   1,       True,   True),
        (65536, "last",   "sparse", 4,    3,         1.0e5,  1,   None,    True,   True),
        (501,   None,     "all",    2,    1,         1503.0, 1,   None,    False,  True))   # photon-less, d_result NULL
COLUMNS = ("N", "photon", "members", "n_terms", "n_reservoirs", "dof", "add", "planted", "result", "time")


class Ragged:
    """The ragged batch of SPEC with its force batch, a ledger and a recorder over the same arrays, recorded twice"""

    def __init__(self, capacity=8):
        rng = np.random.default_rng(2025)
        self.spec = [dict(zip(COLUMNS, row)) for row in SPEC]
        self.systems = [Sys(c["N"], c["photon"], c["members"], c["n_terms"], rng, c["planted"]) for c in self.spec]
        B = self.B = len(self.systems)
        self.reservoir_host = rng.normal(0.0, 1.0, (B, 4)) * 10.0 ** rng.integers(-6, 3, (B, 4))
        self.reservoir_host[3, 1] = -0.0
        self.time_host = rng.uniform(0.0, 1e4, B)
        self.reservoirs = torch.from_numpy(self.reservoir_host).cuda()
        self.times = torch.from_numpy(self.time_host).cuda()
        self.ws = _capi.Workspace(1)
        self.fb = _capi.Batch(self.ws, [s.force_item() for s in self.systems])
        res = self.fb.results_device_ptr()
        self.ledger = _capi.Ledger(self.ws, [self.item(k) for k in range(B)], capacity, 1, KB)
        self.recorder = _capi.Recorder(self.ws, [s.recorder_item(res + 192 * k) for k, s in enumerate(self.systems)], capacity, 1, KB)
        self.fb.compute(_stream())
        self.ledger.record(_stream())
        self.ledger.record(_stream())
        self.recorder.record(_stream())
        torch.cuda.synchronize()
        self.results = self.fb.results()
        self.rows = self.ledger.read(_stream(), 0, B, 0, 2)
        self.records = self.recorder.read(_stream(), 0, B, 0, 1)[:, 0]

    def item(self, k):
        c, s = self.spec[k], self.systems[k]
        return s.ledger_item(self.fb.results_device_ptr() + 192 * k if c["result"] else 0,
                             [self.reservoirs.data_ptr() + 8 * (4 * k + r) for r in range(c["n_reservoirs"])],
                             self.times.data_ptr() + 8 * k if c["time"] else 0, c["dof"], c["add"])

    def close(self):
        self.recorder.close()
        self.ledger.close()
        self.fb.close()
        self.ws.close()


@pytest.fixture(scope="module")
def ragged():
    r = Ragged()
    yield r
    r.close()


def _derived(row, dof, add, kB=KB):
    """the listed expressions in numpy float64 scalars, one rounding per operation, from the row's own columns"""
    p, c, r = (np.asarray(row[name], dtype=np.float64) for name in ("potential", "cavity", "reservoir"))
    kg, kc = np.float64(row["kinetic_group"]), np.float64(row["kinetic_cavity"])
    with np.errstate(invalid="ignore", over="ignore"):
        out = {"cavity_potential": (c[0] + c[1]) + c[2]}
        out["potential_total"] = (((p[0] + p[1]) + p[2]) + p[3]) + out["cavity_potential"]
        out["kinetic_total"] = kg + kc if add else kg
        out["system_total"] = out["kinetic_total"] + out["potential_total"]
        out["reservoir_total"] = ((r[0] + r[1]) + r[2]) + r[3]
        out["universe_total"] = out["system_total"] + out["reservoir_total"]
        out["temperature"] = np.float64(0.0) if dof == 0 else (np.float64(2.0) * kg) / (np.float64(dof) * np.float64(kB))
    return out


def _assert_derived(row, dof, add, where):
    for name, want in _derived(row, dof, add).items():
        got = np.float64(row[name])
        assert _same(got, want) or (np.isnan(got) and np.isnan(want)), (where, name, got, want)


# ---- 1. potential terms ------------------------------------------------------------------------------------------------------
def test_potential_terms_are_within_2_ulp_of_the_exact_sums(ragged):
    assert ragged.ledger.launch_order == sorted(range(ragged.B), key=lambda i: -max(ragged.systems[i].N, ragged.systems[i].n_members))
    planted = 0
    for k, (c, s) in enumerate(zip(ragged.spec, ragged.systems)):
        for t in range(4):
            got = float(ragged.rows[k, 0]["potential"][t])
            if t >= s.n_terms or s.N == 0:
                assert _same(got, 0.0), (k, t, got)                               # absent terms are +0
                continue
            w = s.w[t]
            exact = math.fsum(w)
            ratio = math.fsum(np.abs(w)) / abs(exact)
            assert ratio <= 2.0 ** 40, (k, t, ratio)                             # what the bound presupposes
            plain = _ulps(float(np.cumsum(w)[-1]), exact)
            print(f"item {k} (N = {s.N}) term {t}: sum|w|/|sum w| = 2^{math.log2(ratio):.1f}, ledger {_ulps(got, exact):.2f} ulp, "
                  f"np.cumsum {plain:.3g} ulp")
            assert _ulps(got, exact) <= 2.0, (k, t, got, exact)
            if c["planted"] == t:
                planted += 1
                assert ratio > 2.0 ** 30 and plain > 2.0, (k, t, ratio, plain)   # a plain sum cannot pass here
    assert planted == 3 and sorted(s.N for c, s in zip(ragged.spec, ragged.systems) if c["planted"] is not None) == [1024, 1025, 2049]
    # the same call repeated gives the same bits
    for name in ragged.rows.dtype.names:
        if name != "call":
            assert ragged.rows[:, 0][name].tobytes() == ragged.rows[:, 1][name].tobytes(), name
    assert list(ragged.rows[:, 0]["call"]) == [1] * ragged.B and list(ragged.rows[:, 1]["call"]) == [2] * ragged.B


# ---- 2. kinetic columns --------------------------------------------------------------------------------------------------------
def test_kinetic_columns_have_the_recorders_bits(ragged):
    for k, s in enumerate(ragged.systems):
        row, rec = ragged.rows[k, 0], ragged.records[k]
        assert _same(row["kinetic_group"], rec["kinetic_energy"]), (k, row["kinetic_group"], rec["kinetic_energy"])
        assert _same(row["kinetic_cavity"], rec["cavity_kinetic"]), (k, row["kinetic_cavity"], rec["cavity_kinetic"])
        assert (row["kinetic_group"] > 0) == (s.n_members > 0) and (row["kinetic_cavity"] > 0) == (s.photon >= 0)
        assert ragged.results[k].photon_idx == s.photon


# ---- 3. copied columns ---------------------------------------------------------------------------------------------------------
def test_copied_columns_are_the_bytes_they_point_at(ragged):
    for k, (c, s) in enumerate(zip(ragged.spec, ragged.systems)):
        row = ragged.rows[k, 0]
        want = np.array(ragged.results[k].energy[:]) if c["result"] else np.zeros(3)
        assert _same(row["cavity"], want), (k, row["cavity"], want)
        assert (s.photon >= 0) == bool(row["cavity"][0] != 0.0), k              # a photon at a finite q has a harmonic energy
        assert int(row["n_terms"]) == (s.n_terms if s.N else 0) and int(row["n_reservoirs"]) == c["n_reservoirs"], k
        for r in range(4):
            assert _same(row["reservoir"][r], ragged.reservoir_host[k, r] if r < c["n_reservoirs"] else 0.0), (k, r)
        assert _same(row["time"], ragged.time_host[k] if c["time"] else 0.0), k
        assert _same(row["reserved"], 0.0)
    assert np.signbit(ragged.rows[3, 0]["reservoir"][1])                           # the bytes, a -0.0 included


# ---- 4. derived columns ----------------------------------------------------------------------------------------------------------
def test_derived_columns_are_their_listed_expressions(ragged):
    for k, c in enumerate(ragged.spec):
        _assert_derived(ragged.rows[k, 0], c["dof"], c["add"], k)
    dofs, adds = [c["dof"] for c in ragged.spec], [c["add"] for c in ragged.spec]
    assert 0.0 in dofs and any(d > 0 for d in dofs) and 0 in adds and 1 in adds
    rows = ragged.rows[:, 0]
    for k, c in enumerate(ragged.spec):
        if c["N"] > 1:
            assert (rows[k]["temperature"] > 0) == (c["dof"] > 0), k
        if c["photon"] is not None:
            assert (rows[k]["kinetic_total"] != rows[k]["kinetic_group"]) == bool(c["add"]), k
    # the expression the reference itself uses for its temperature column is this one with dof = 9 n: the same number up to
    # the roundings of the two expressions (four operations each, 2^-53 apiece)
    row = rows[7]
    assert ragged.spec[7]["dof"] == 9.0 * 1024
    reference = (2.0 / 3.0) * float(row["kinetic_group"]) / (3.0 * 1024 * KB)
    assert float(row["temperature"]) == pytest.approx(reference, rel=8 * 2.0 ** -53)


# ---- 5. independence -------------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_term_stays_in_its_item():
    ragged = Ragged()
    k, t, j = 6, 2, 700
    ragged.systems[k].terms[t][j, 3] = float("nan")
    ragged.ledger.record(_stream())
    got = ragged.ledger.read(_stream(), 0, ragged.B, 2, 1)[:, 0]
    first = ragged.rows[:, 0]
    poisoned = {"potential", "potential_total", "system_total", "universe_total"}
    for i in range(ragged.B):
        for name in got.dtype.names:
            if name == "call" or (i == k and name in poisoned):
                continue
            assert got[i][name].tobytes() == first[i][name].tobytes(), (i, name)
    assert np.isnan(got[k]["potential"][t]) and all(np.isnan(got[k][name]) for name in poisoned - {"potential"})
    others = [x for x in range(4) if x != t]
    assert got[k]["potential"][others].tobytes() == first[k]["potential"][others].tobytes()
    _assert_derived(got[k], ragged.spec[k]["dof"], ragged.spec[k]["add"], "the item with the NaN")
    ragged.close()


# ---- 6. period and ring ----------------------------------------------------------------------------------------------------------
def test_period_and_ring_follow_the_recorders_rules():
    rng = np.random.default_rng(4)
    systems = [Sys(300, "first", "sorted", 2, rng), Sys(1500, None, "sparse", 1, rng)]
    B = len(systems)
    ws = _capi.Workspace(1)
    fb = _capi.Batch(ws, [s.force_item() for s in systems])
    res = fb.results_device_ptr()
    clock = torch.zeros(B, dtype=torch.float64, device="cuda")
    led = _capi.Ledger(ws, [s.ledger_item(res + 192 * k, (), clock.data_ptr() + 8 * k, 3.0, 1) for k, s in enumerate(systems)], 4, 3, KB)
    rec = _capi.Recorder(ws, [s.recorder_item(res + 192 * k) for k, s in enumerate(systems)], 4, 3, KB)
    _expect_status(_capi.CAVMD_ERR_NOT_COMPUTED, led.read, _stream(), 0, B, 0, 1)
    assert ws._lib.cavmd_destroy(ws.handle) == INV                              # refused while the ledger lives
    fb.compute(_stream())
    for call in range(1, 15):
        clock.fill_(float(call))                                                 # in stream order: what the call reads
        led.record(_stream())
        rec.record(_stream())
    assert list(led.rows(_stream())) == list(rec.rows(_stream())) == [4] * B     # calls 3, 6, 9, 12
    got, want = led.read(_stream(), 0, B, 0, 4), rec.read(_stream(), 0, B, 0, 4)
    for k in range(B):
        assert list(got[k]["call"]) == list(want[k]["call"]) == [3, 6, 9, 12]
        assert list(got[k]["time"]) == [3.0, 6.0, 9.0, 12.0]                     # row j sits in slot j and was written by that call
    _expect_status(INV, led.read, _stream(), 0, B, 4, 1)
    # the fifteenth call writes row 4 into slot 0: row 0 has been overwritten
    clock.fill_(15.0)
    led.record(_stream())
    rec.record(_stream())
    assert list(led.rows(_stream())) == list(rec.rows(_stream())) == [5] * B
    for first, count in ((0, 1), (0, 5), (0, 4)):
        _expect_status(_capi.CAVMD_ERR_EXPIRED, led.read, _stream(), 0, B, first, count)
        _expect_status(_capi.CAVMD_ERR_EXPIRED, rec.read, _stream(), 0, B, first, count)
    for first, count in ((5, 1), (4, 2), (1, 0)):
        _expect_status(INV, led.read, _stream(), 0, B, first, count)
    for first_item, n_items in ((B, 1), (0, B + 1), (0, 0)):
        _expect_status(INV, led.read, _stream(), first_item, n_items, 4, 1)
    ring = led.read(_stream(), 0, B, 1, 4)                                       # slots 1, 2, 3, then 0: two runs of the ring
    for k in range(B):
        assert list(ring[k]["call"]) == list(rec.read(_stream(), 0, B, 1, 4)[k]["call"]) == [6, 9, 12, 15]
        assert list(ring[k]["time"]) == [6.0, 9.0, 12.0, 15.0]
        assert ring[k, :3].tobytes() == got[k, 1:].tobytes()
    assert led.read(_stream(), 1, 1, 4, 1)[0, 0].tobytes() == ring[1, 3].tobytes()
    series_ptr, rows_ptr = led.device_ptr()
    assert series_ptr and rows_ptr and series_ptr % 16 == 0
    # reset: counters to zero, the next row is row 0 written by call 3
    led.reset(_stream())
    assert list(led.rows(_stream())) == [0] * B
    _expect_status(_capi.CAVMD_ERR_NOT_COMPUTED, led.read, _stream(), 0, B, 0, 1)
    for call in range(1, 4):
        led.record(_stream())
    assert list(led.rows(_stream())) == [1] * B and list(led.read(_stream(), 0, B, 0, 1)[:, 0]["call"]) == [3] * B
    led.close()
    rec.close()
    fb.close()
    ws.close()


# ---- 7. set_items ----------------------------------------------------------------------------------------------------------------
def test_set_items_takes_effect_on_the_next_call_and_keeps_the_series():
    rng = np.random.default_rng(6)
    systems = [Sys(501, "last", "all", 2, rng), Sys(300, "first", "sorted", 1, rng), Sys(1500, None, "sparse", 4, rng)]
    other = Sys(777, "middle", "sparse", 3, rng)
    B = len(systems)
    ws = _capi.Workspace(1)
    fb = _capi.Batch(ws, [s.force_item() for s in systems + [other]])
    res = fb.results_device_ptr()
    reservoirs = torch.from_numpy(rng.normal(size=B + 1)).cuda()
    item = lambda s, k: s.ledger_item(res + 192 * k, [reservoirs.data_ptr() + 8 * k], 0, 3.0 * s.n_members, 1)   # noqa: E731
    led = _capi.Ledger(ws, [item(s, k) for k, s in enumerate(systems)], 16, 1, KB)
    alone = _capi.Ledger(ws, [item(other, B)], 16, 1, KB)                        # what `other` gives as an item of its own
    fb.compute(_stream())
    led.record(_stream())
    led.record(_stream())
    alone.record(_stream())
    before = led.read(_stream(), 0, B, 0, 2)
    # a call refused at its second item changes nothing: not the table, not the order, not the series
    bad = item(systems[2], 2)
    bad.dof = -1.0
    _expect_status(INV, led.set_items, 0, [item(other, B), bad])
    too_large = item(systems[2], 2)
    too_large.N = _capi.BATCH_MAX_ITEM_N + 1
    _expect_status(_capi.CAVMD_ERR_CAPACITY, led.set_items, 1, [item(other, B), too_large])
    _expect_status(INV, led.set_items, B, [item(other, B)])
    led.record(_stream())
    third = led.read(_stream(), 0, B, 2, 1)[:, 0]
    for name in third.dtype.names:
        if name != "call":
            assert third[name].tobytes() == before[:, 1][name].tobytes(), name
    assert led.sizes == [501, 300, 1500]
    # the item in the middle replaced (another N, other pointers): the next call records it; counters and series are kept
    led.set_items(1, [item(other, B)])
    assert led.sizes == [501, 777, 1500] and led.launch_order == [2, 1, 0]
    assert list(led.rows(_stream())) == [3] * B and led.read(_stream(), 0, B, 0, 2).tobytes() == before.tobytes()
    led.record(_stream())
    assert list(led.rows(_stream())) == [4] * B
    fourth, want = led.read(_stream(), 0, B, 3, 1)[:, 0], alone.read(_stream(), 0, 1, 0, 1)[0, 0]
    assert list(fourth["call"]) == [4] * B
    for name in fourth.dtype.names:
        if name != "call":
            assert fourth[1][name].tobytes() == want[name].tobytes(), name
            assert fourth[[0, 2]][name].tobytes() == third[[0, 2]][name].tobytes(), name
    assert int(fourth[1]["n_terms"]) == 3 and fourth[1]["kinetic_group"] != third[1]["kinetic_group"]
    alone.close()
    led.close()
    fb.close()
    ws.close()


# ---- 8. replay -------------------------------------------------------------------------------------------------------------------
def _replica_run(captured: bool, B: int, steps: int):
    """B replicas of N = 501: cavity force + ledger + thermostat batch per step with hand-set thermostat inputs, positions moved
    in place between the steps; eager, or as replays of one captured graph.  Same seeds and initial state either way."""
    rng = np.random.default_rng(5)
    sysdefs, velocities = [], []
    for k in range(B):
        cfg = synthetic.config1(seed=k + 1)
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        v = np.ones((pd.getN(), 4))
        v[:, :3] = rng.normal(0.0, 1e-3, (pd.getN(), 3))
        velocities.append(torch.from_numpy(v).cuda())
    moves = [torch.from_numpy(rng.normal(0.0, 1e-3, (steps, 501, 3))).cuda() for _ in range(B)]
    shares = [torch.from_numpy(rng.normal(0.0, 1e-3, (501, 4))).cuda() for _ in range(B)]
    variates = np.stack([rng.standard_normal((steps, B)), rng.gamma(749.5, size=(steps, B))], axis=2)
    forces = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    thermostat = cavitymd.BussiReservoirBatch(kT=1e-6, tau=0.5)
    thermostat.attach(velocities, translational_dof=3.0 * 501 - 3.0)
    ledger = cavitymd.BatchEnergyLedger(forces, velocities, terms=[("share", shares)], reservoirs=[("bussi", thermostat)], capacity=64)
    positions = [s.getParticleData().getPositions() for s in sysdefs]

    def advance(r):
        for k in range(B):
            positions[k][:, :3].add_(moves[k][r])                               # in place, on the stream the step goes to
        thermostat.set_inputs(r, 0.005, variates[r])

    torch.cuda.synchronize()
    if captured:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            forces.compute(0)
            ledger.record()
            thermostat.step_async()
        assert list(ledger.rows()) == [0] * B                                    # a capture runs nothing
        for r in range(steps):
            advance(r)
            graph.replay()
            if r == steps // 2:                                                  # a read between replays disturbs nothing
                assert list(ledger.rows()) == [r + 1] * B
    else:
        for r in range(steps):
            advance(r)
            forces.compute(0)
            ledger.record()
            thermostat.step_async()
    rows = ledger.rows()
    series = ledger.read()
    final = thermostat.reservoir_energy_translational
    ledger.close()
    thermostat.detach()
    forces.close()
    return rows, series, final


def test_a_replayed_graph_appends_the_rows_of_the_eager_steps():
    B, REPLAYS = 3, 50
    rows_e, eager, final_e = _replica_run(False, B, REPLAYS)
    rows_g, replayed, final_g = _replica_run(True, B, REPLAYS)
    assert list(rows_e) == [REPLAYS] * B and list(rows_g) == [REPLAYS] * B
    assert eager.shape == replayed.shape == (B, REPLAYS)
    assert replayed.tobytes() == eager.tobytes() and final_e.tobytes() == final_g.tobytes()
    for k in range(B):
        assert list(replayed[k]["call"]) == list(range(1, REPLAYS + 1))
        # the kernel reads the thermostat's state when it runs: the reservoir before this step's thermostat launch
        assert len(set(replayed[k]["reservoir"][:, 0])) == REPLAYS and replayed[k]["reservoir"][0, 0] == 0.0
        assert replayed[k]["bussi"].tobytes() == replayed[k]["reservoir"][:, 0].tobytes()
        assert replayed[k]["share"].tobytes() == replayed[k]["potential"][:, 0].tobytes()
        assert list(replayed[k]["n_terms"]) == [1] * REPLAYS and list(replayed[k]["n_reservoirs"]) == [1] * REPLAYS
        for name in ("kinetic_group", "kinetic_cavity", "universe_total"):
            assert len(set(replayed[k][name])) == REPLAYS, name
        assert len({c.tobytes() for c in replayed[k]["cavity"]}) == REPLAYS
        # the default group: everything but the photon, with the photon's kinetic energy added to the total
        assert np.all(replayed[k]["kinetic_total"] == replayed[k]["kinetic_group"] + replayed[k]["kinetic_cavity"])
        for j in (0, REPLAYS - 1):
            _assert_derived(replayed[k, j], 3.0 * 500, 1, (k, j))


# ---- 9. refusals on a capturing stream ----------------------------------------------------------------------------------------------
def test_a_capturing_stream_is_refused_as_the_recorders_is():
    rng = np.random.default_rng(8)
    s = Sys(501, "last", "all", 1, rng)
    ws = _capi.Workspace(1)
    fb = _capi.Batch(ws, [s.force_item()])
    res = fb.results_device_ptr()
    led = _capi.Ledger(ws, [s.ledger_item(res, (), 0, 3.0, 1)], 8, 1, KB)
    rec = _capi.Recorder(ws, [s.recorder_item(res)], 8, 1, KB)
    fb.compute(_stream())
    led.record(_stream())
    rec.record(_stream())
    first = led.read(_stream(), 0, 1, 0, 1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = _stream()
        led.record(stream)
        rec.record(stream)
        for obj, item in ((led, s.ledger_item(res, (), 0, 3.0, 1)), (rec, s.recorder_item(res))):
            _expect_status(INV, obj.rows, stream)
            _expect_status(INV, obj.read, stream, 0, 1, 0, 1)
            _expect_status(INV, obj.set_items, 0, [item])
    torch.cuda.synchronize()
    assert list(led.rows(_stream())) == [1]                                      # capturing ran nothing, the refusals changed nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert list(led.rows(_stream())) == list(rec.rows(_stream())) == [3]
    got = led.read(_stream(), 0, 1, 0, 3)
    assert list(got[0]["call"]) == [1, 2, 3]
    for name in got.dtype.names:
        if name != "call":
            assert got[0][name].tobytes() == np.repeat(first[0][name], 3, axis=0).tobytes(), name
    led.close()
    rec.close()
    fb.close()
    ws.close()


# ---- 10. the full step -----------------------------------------------------------------------------------------------------------
def test_forty_full_steps_with_both_baths_row_by_row():
    """B = 2 systems of 27 diatomics and the photon, 40 eager steps of the full step of examples/batch_coulomb_md_in_one_graph.py
    (cavity force, bonds and Lennard-Jones, Ewald Coulomb, the Langevin bath on the photon, the Bussi thermostat on the
    molecules): after every step the ledger's row is the host's view of the state the kernel saw.  This test holds the row's
    terms; that their sum, universe_total, is CONSERVED under these baths is asserted by tests/test_gpu_conserved_energy.py,
    against a band measured on the host twin of this step (tests/thermostatted_twin.py), so no excursion is printed here."""
    B, STEPS, kT, dt = 2, 40, 3.167e-4, 5.0
    rng = np.random.default_rng(0)
    sysdefs, velocities, bonds, bond_typeid = [], [], [], []
    for k in range(B):
        cfg = synthetic.diatomic_lattice(3, 8.0, seed=k + 1)                     # N = 55, box 24 bohr
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
        v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(kT / mass)[:, None]
        velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
        b, t = synthetic.diatomic_bonds(cfg)
        bonds.append(b)
        bond_typeid.append(t)
    N = sysdefs[0].getParticleData().getN()
    photon = int(np.flatnonzero(cfg["typeid"] == 2)[0])
    molecules = [np.flatnonzero(cfg["typeid"] != 2)] * B
    cavity = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    molecular = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, harmonic=HARMONIC, lj=LJ)
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=8.0, accuracy=1e-5)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(molecular.forces, coulomb.forces)],
                                      langevin_index=photon)
    recorder = cavitymd.BatchRecorder(cavity, velocities, members=molecules, capacity=STEPS)
    thermostat = cavitymd.BussiReservoirBatch(kT=kT, tau=1000.0)
    thermostat.attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
    ticks = torch.zeros((B, 8), dtype=torch.float64, device="cuda")              # a clock of its own: it draws into a spare table
    clock = cavitymd.StepDraw(11, integrator=ticks, dt=dt)
    ledger = cavitymd.BatchEnergyLedger(cavity, velocities, terms=[("molecular", molecular), ("coulomb", coulomb)],
                                        reservoirs=[("bussi", thermostat), ("langevin", integrator)], clock=clock, capacity=STEPS)
    assert ledger.term_names == ("molecular", "coulomb") and ledger.reservoir_names == ("bussi", "langevin")
    assert ledger.ledger.sizes == [N] * B and N == 55
    cavity.compute()
    molecular.compute()
    coulomb.compute()
    integrator.prime()
    seen = []
    for step in range(STEPS):
        clock.fill()
        integrator.draw_inputs(dt, gamma=1e-3, kT=kT)
        integrator.step_one()
        cavity.compute()
        molecular.compute()
        coulomb.compute()
        integrator.step_two()
        recorder.record()
        ledger.record()
        # the host's view at that point: before the thermostat's launch of this step
        state = integrator.state()
        seen.append(dict(w=[[f[:, 3].cpu().numpy() for f in batch.forces] for batch in (molecular, coulomb)],
                         bussi=np.array([s.reservoir_translational for s in thermostat.device_state()]) if step else np.zeros(B),
                         langevin=state["langevin_reservoir"].copy(), cavity=cavity.energies(), elapsed=clock.state()["elapsed"].copy()))
        thermostat.draw_inputs(0, dt)
        thermostat.step_async()
    series, records = ledger.read(), recorder.read()
    assert series.shape == (B, STEPS) and list(ledger.rows()) == [STEPS] * B
    worst = 0.0
    for k in range(B):
        assert list(series[k]["call"]) == list(range(1, STEPS + 1))
        for j, view in enumerate(seen):
            row = series[k, j]
            for t in range(2):
                exact = math.fsum(view["w"][t][k])
                assert math.fsum(np.abs(view["w"][t][k])) / abs(exact) <= 2.0 ** 40
                worst = max(worst, _ulps(float(row["potential"][t]), exact))
                assert _ulps(float(row["potential"][t]), exact) <= 2.0, (k, j, t, row["potential"][t], exact)
            assert _same(row["potential"][2:], np.zeros(2)) and int(row["n_terms"]) == 2 and int(row["n_reservoirs"]) == 2
            assert _same(row["reservoir"], [view["bussi"][k], view["langevin"][k], 0.0, 0.0]), (k, j)
            assert _same(row["cavity"], view["cavity"][k]) and _same(row["time"], view["elapsed"][k]), (k, j)
            assert _same(row["kinetic_group"], records[k, j]["kinetic_energy"]), (k, j)
            assert _same(row["kinetic_cavity"], records[k, j]["cavity_kinetic"]), (k, j)
            _assert_derived(row, 3.0 * (N - 1), 1, (k, j))
        assert _same(series[k]["molecular"], series[k]["potential"][:, 0]) and _same(series[k]["langevin"], series[k]["reservoir"][:, 1])
        assert np.all(np.diff(series[k]["time"]) == dt) and series[k]["time"][-1] > 0                 # the clock's dt is fixed
        # the columns are alive
        for name in ("molecular", "coulomb", "kinetic_group", "kinetic_cavity", "langevin", "universe_total"):
            assert len(set(series[k][name])) == STEPS, name
        assert len(set(series[k]["bussi"])) == STEPS and series[k]["bussi"][0] == 0.0
    print(f"worst potential term: {worst:.2f} ulp from math.fsum")
    for obj in (ledger, clock, recorder, integrator, coulomb, molecular, cavity):
        obj.close()
    thermostat.detach()
