"""What is specific to the bath object (cavmd_bath_*) on a machine WITHOUT a GPU (tests/test_batch_objects_abi.py runs the shared
checks a to i on its row of tests/batch_objects.py; none is skipped: the one difference, a create from an integrator instead
of a workspace, is a first argument that is refused when it is NULL either way): the header's prose, the further null-argument
cases, a bath's deferred destroy before its integrator's, every refusal of its item check, the mirror's variates
(tests/bath_mirror.py) against the known answers of Philox in the header, the derived per-item keys, and the host twin
(tests/bath_twin.py) inside its band over 24 seeds and outside it with a frozen step counter or a pre-kick tally."""
import ctypes

import numpy as np
import pytest
import torch

import batch_objects as checks
import bath_mirror as mirror
import bath_twin as twin
import draw_mirror
from abi_support import HEADER
from abi_support import good_bath as _good

byref, vp = ctypes.byref, ctypes.c_void_p


ROW = checks.ROWS["bath"]


# ---- what this object adds to the checks every batch object gets (tests/batch_objects.py a to i) ------------------------------
def test_header_declares_the_eight_entry_points_and_the_contract():
    checks.header_declares_exactly_the_entry_points(ROW)
    text = open(HEADER).read()
    for words in ("0x80000000 + b", "coeff_j = sqrt(((6 * gamma_j) * kT) / dt)", "tally_j = (bd_x * v'_x + bd_y * v'_y) + bd_z * v'_z",
                  "reservoir = reservoir - T * dt", "examples/05_advanced_run.py:649-666", "not HOOMD's RandomGenerator",
                  "after it the same variates come again", "exactly the bytes"):
        assert words in text, words
    assert "Out of scope: Langevin on more than one particle" not in text


def test_the_version_is_still_2(capi):
    checks.the_version_is_still_2(capi)                                    # not a check on a row: it stays with each object


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)
    lib = capi.load()
    it = _good(capi)
    for bad in (None, vp(0x1004)):                     # the integrator's argument checks: a null or misaligned input table
        assert lib.cavmd_bath_step_two(None, None, bad) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_bath_create(None, 0, byref(it), byref(vp())) == capi.CAVMD_ERR_INVALID_VALUE


def test_launch_order_is_a_stable_descending_sort(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)
    assert capi.Bath._size(_good(capi, N=77)) == 77


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
    import cavitymd
    doc = cavitymd.bath_batch.__doc__
    step = doc[doc.index("with torch.cuda.graph(graph):"):]
    order = [step.index(call) for call in ("draw.fill()", "integrator.step_one()", "forces.compute()", "bath.step_two()",
                                          "recorder.record()")]
    assert order == sorted(order)                        # the captured step, in its launch order
    assert "0x9E3779B97F4A7C15" in doc and "not HOOMD's RandomGenerator" in doc

    class Closed:                                        # what a closed VerletBatch answers
        n_systems = 1

        def _need(self):
            raise RuntimeError("VerletBatch used after close()")

    with pytest.raises(RuntimeError, match="used after close"):
        cavitymd.LangevinBathBatch(Closed(), [None], 1.0, 3)


def test_deferred_destroy_takes_a_bath_before_its_integrator(capi, monkeypatch):
    """whichever of the two was closed first during the capture"""
    from types import SimpleNamespace
    for bath_first in (True, False):
        order = []
        lib = SimpleNamespace(cavmd_destroy=lambda h: order.append("ws") or 0, cavmd_bath_destroy=lambda h: order.append("bath") or 0,
                              cavmd_verlet_destroy=lambda h: order.append("verlet") or 0)
        ws = object.__new__(capi.Workspace)
        ws._lib, ws._h = lib, vp(0x10)
        v = object.__new__(capi.Verlet)
        v._lib, v._h, v._ws = lib, vp(0x20), ws
        b = object.__new__(capi.Bath)
        b._lib, b._h, b._ws, b._verlet = lib, vp(0x30), ws, v
        monkeypatch.setattr(capi, "_capturing", lambda: True)
        for h in ((b, v) if bath_first else (v, b)):
            h.close()
        ws.close()
        assert order == []
        monkeypatch.setattr(capi, "_capturing", lambda: False)
        capi._destroy_deferred()
        assert order == ["bath", "verlet", "ws"], (bath_first, order)
        assert not capi._deferred and not capi._deferred_children and not capi._deferred_baths


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    chk = capi.bath_item_check
    assert lib.cavmd_bath_item_check(None) == INV
    assert chk(_good(capi)) == 0
    # no bath on this item: NULL with N == 0; either without the other is refused
    assert chk(_good(capi, gamma_ptr=0, N=0)) == 0
    assert chk(_good(capi, gamma_ptr=0)) == INV and chk(_good(capi, N=0)) == INV
    # misalignment: 8 bytes
    for off, status in ((4, INV), (1, INV), (2, INV), (8, 0)):
        assert chk(_good(capi, gamma_ptr=0x10000 + off)) == status, off
    # kT: finite and >= 0; 0 is legal
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert chk(_good(capi, kT=bad)) == INV, bad
    assert chk(_good(capi, kT=0.0)) == 0 and chk(_good(capi, kT=1e300)) == 0
    # any seed is a key
    for seed in (0, 1, 2 ** 64 - 1):
        assert chk(_good(capi, seed=seed)) == 0
    # the cap
    assert chk(_good(capi, N=capi.BATCH_MAX_ITEM_N)) == 0 and chk(_good(capi, N=capi.BATCH_MAX_ITEM_N + 1)) == CAP
    # reserved words
    it = _good(capi)
    it.reserved0 = 1
    assert chk(it) == INV
    for k in range(4):
        it = _good(capi)
        it.reserved[k] = 1 << (15 * k)
        assert chk(it) == INV, k
    # precedence: reserved words and pointers before the capacity
    it = _good(capi, N=capi.BATCH_MAX_ITEM_N + 1)
    it.reserved[0] = 1
    assert chk(it) == INV
    assert chk(_good(capi, N=capi.BATCH_MAX_ITEM_N + 1, kT=-1.0)) == INV


# ---- the generator ----------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                  "d16cfe09 94fdcceb 5001e420 24126ea1"))


def test_the_mirrors_variates_against_the_known_answers_of_philox():
    text = " ".join(open(HEADER).read().replace("*", " ").split())          # a known answer may run over a comment's line end
    for counter, key, want in KNOWN_ANSWERS:
        assert want in text
        # block() puts the words where the contract says: key = (seed low, seed high), counter = (draws low, draws high, j,
        # 0x80000000 + b); the known counters' fourth words are reached with b = word - 0x80000000 mod 2^32
        seed, draws = key[0] | (key[1] << 32), counter[0] | (counter[1] << 32)
        got = mirror.block(seed, draws, np.array([counter[2]]), (counter[3] - mirror.PURPOSE) % 2 ** 32)[0]
        assert " ".join("%08x" % int(w) for w in got) == want, (counter, key)
    # the variates of a particle are those words' doubles: u_x, u_y from block 0, u_z from block 1, each 2 * (k * 2^-53) - 1
    seed, draws, j = 0x299f31d0a4093822, 7, np.array([0, 1, 512, 65535])
    u = mirror.variates(seed, draws, j)
    for n, jj in enumerate(j):
        w0 = draw_mirror.philox(np.array([7, 0, jj, 0x80000000], dtype=np.uint64), np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
        w1 = draw_mirror.philox(np.array([7, 0, jj, 0x80000001], dtype=np.uint64), np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
        k = [(int(a) << 21) | (int(b) >> 11) for a, b in ((w0[0], w0[1]), (w0[2], w0[3]), (w1[0], w1[1]))]
        assert u[n].tolist() == [2.0 * (kk * 2.0 ** -53) - 1.0 for kk in k], jj
    # in [-1, 1), new with every step, particle and key; the moments of U[-1, 1) within six standard errors
    many = np.concatenate([mirror.variates(11, d, np.arange(2000)) for d in range(20)])
    n = many.size
    assert (many >= -1.0).all() and (many < 1.0).all() and len(np.unique(many)) == n
    assert abs(many.mean()) < 6.0 * np.sqrt(1.0 / 3.0 / n) and abs(many.var() - 1.0 / 3.0) < 6.0 * np.sqrt(4.0 / 45.0 / n)
    assert (mirror.variates(11, 0, np.arange(8)) != mirror.variates(12, 0, np.arange(8))).all()
    # apart from cavmd_draw's counters under an equal key: its purposes are all below 48
    assert mirror.PURPOSE > draw_mirror.PURPOSE_GAMMA_TRY + 2 * draw_mirror.GAMMA_TRIES == 48


def test_the_derived_keys_are_distinct_for_65536_items(capi):
    assert mirror.KEY_STRIDE == capi.BATH_KEY_STRIDE == 0x9E3779B97F4A7C15 and capi.BATCH_MAX_ITEMS == 65536
    for seed in (0, 1, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15):
        keys = [capi.bath_item_key(seed, i) for i in range(65536)]
        assert len(set(keys)) == 65536 and all(0 <= k < 2 ** 64 for k in keys)
        assert keys[:3] == [mirror.item_key(seed, i) for i in range(3)] and seed not in keys
    assert capi.bath_item_key(5, 0) == 5 + 0x9E3779B97F4A7C15 and capi.bath_item_key(2 ** 64 - 1, 0) == 0x9E3779B97F4A7C14


def test_the_mirror_leaves_what_the_contract_leaves(capi):
    """no bath: the integrator's mirror, byte for byte; a NaN, a negative or a zero gamma, the tail beyond bath N and the row's
    Langevin particle are not coupled"""
    import copy
    from types import SimpleNamespace

    import verlet_mirror
    rng = np.random.default_rng(5)
    n = 9
    vel = rng.normal(size=(n, 4))
    vel[:, 3] = rng.uniform(1.0, 4.0, n)
    s = {"N": n, "vel": vel, "forces": [rng.normal(size=(n, 4)), rng.normal(size=(n, 4))], "net": np.zeros((n, 4)),
         "accel": np.zeros((n, 3)), "langevin": 2, "steps": 0, "reservoir": 0.0}
    row = SimpleNamespace(dt=2.0, langevin_gamma=0.5, langevin_coeff=0.3, uniform=(0.1, -0.2, 0.3), skip=0)
    for gamma in (None, np.zeros(n), np.array([np.nan, -1.0, 3.0])):         # particle 2 is the row's
        a, b = copy.deepcopy(s), copy.deepcopy(s)
        bath = {"gamma": gamma, "kT": 1e-3, "seed": 1, "draws": 0, "coupled": 0, "reservoir": 0.0}
        verlet_mirror.mirror_step_two(a, row)
        mirror.mirror_bath_step_two(b, row, bath)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("vel", "net", "accel", "reservoir")) and b["steps"] == 1
        assert bath["coupled"] == 0 and bath["reservoir"] == 0.0 and bath["draws"] == (0 if gamma is None else 1)
    gamma = np.array([0.2, np.nan, 3.0, -1.0, 0.0, 0.4, 0.4])                # 0 and 5, 6 are coupled; 7, 8 lie beyond bath N
    bath = {"gamma": gamma, "kT": 1e-3, "seed": 1, "draws": 0, "coupled": 0, "reservoir": 0.0}
    assert mirror.coupled_particles(s, row, bath).tolist() == [0, 5, 6]
    row.langevin_gamma = 0.0                                                 # without a row gamma the group's bath applies to 2
    assert mirror.coupled_particles(s, row, bath).tolist() == [0, 2, 5, 6]
    tallies, T = mirror.mirror_bath_step_two(s, row, bath)
    assert len(tallies) == 4 and bath["coupled"] == 4 and bath["draws"] == 1 and bath["reservoir"] == 0.0 - np.float64(T) * 2.0


# ---- the twin -----------------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(24))
NAMES = ("m <v^2> / kT after step two", "m <v^2> (1 - x) / kT after step one", "reservoir gain / pre-kick growth")
EXPECTED = np.asarray(twin.EXPECTED)


@pytest.fixture(scope="module")
def runs() -> np.ndarray:
    return np.array([twin.run(seed) for seed in SEEDS])                      # (24, 3)


def test_the_twin_is_a_thermostat_inside_its_band(runs):
    assert twin.SIZES == (1, 2, 513) and twin.PARTICLES == 516 and (twin.BURN_IN, twin.COUNTED) == (64, 512)
    std = runs.std(axis=0, ddof=1)
    band = 6.0 * std
    print()
    for name, mean, sd, b, worst in zip(NAMES, runs.mean(axis=0), std, band, np.abs(runs - EXPECTED).max(axis=0)):
        print(f"{name}: mean {mean:.6f}, std across {len(SEEDS)} seeds {sd:.6f}, band 6 std = {b:.6f}, "
              f"worst seed {worst:.6f} from the expected")
    # the literals are this run's figures rounded (the third to six decimals); they come from this host run, never from a GPU run
    assert tuple(EXPECTED) == (1.0, 1.0, 0.0)
    assert len(twin.BAND) == 3 and np.all(np.abs(np.asarray(twin.BAND) - band) <= np.asarray(twin.BAND_DIGITS)), (twin.BAND, band.tolist())
    assert np.all(np.asarray(twin.BAND) < 0.03)
    assert np.all(np.abs(runs - EXPECTED) <= np.asarray(twin.BAND)), runs.tolist()     # every seed inside the band
    assert np.all(np.abs(runs.mean(axis=0) - EXPECTED) <= 3.0 * std / np.sqrt(len(SEEDS)))   # and the mean within 3 standard errors
    # the reservoir's spread is the derived one (langevin_twin, (4)): per particle member_sd(), whatever the number of steps
    derived = twin.member_sd() / np.sqrt(twin.PARTICLES) / twin.COUNTED / twin.closed_forms()[2]
    print(f"reservoir figure: std across the seeds {std[2]:.3e}, derived {derived:.3e}")
    assert 0.55 * derived <= std[2] <= 1.45 * derived


def test_a_frozen_step_counter_leaves_the_band():
    for seed in SEEDS[:2]:
        r = twin.run(seed, mistake="frozen_step_counter")
        print(f"frozen step counter, seed {seed}: figures {r.round(4).tolist()}")
        # both temperatures leave the band; the reservoir cannot show it under either tally: at the terminal velocity bd = 0
        assert np.all(np.abs(r[:2] - 1.0) > np.asarray(twin.BAND[:2])), (seed, r)
        assert r[0] > 3.0 and r[1] > 2.0 and abs(r[2]) < 1e-9


def test_a_pre_kick_tally_leaves_the_band():
    for seed in SEEDS[:2]:
        r = twin.run(seed, mistake="tally_with_pre_kick_velocity")
        print(f"pre-kick tally, seed {seed}: figures {r.round(4).tolist()}")
        assert np.all(np.abs(r[:2] - 1.0) <= np.asarray(twin.BAND[:2])) and abs(r[2] - EXPECTED[2]) > twin.BAND[2], (seed, r)
        assert abs(r[2] - 1.0) <= 0.0081                                     # the old contract's closed form, to its old band
