"""What is specific to the draw object (cavmd_draw_*) on a machine WITHOUT a GPU (tests/test_batch_objects_abi.py runs the shared
checks a to i on its row of tests/batch_objects.py): the header's prose, every refusal of its item check, the known answers of its generator through the numpy mirror
(tests/draw_mirror.py), the mirror's fixed-mode rows against the library's two row makers byte for byte, and the mirror's
moments and try counts."""
import ctypes

import numpy as np
import pytest
import torch

import batch_objects as checks
import draw_mirror as mirror
from abi_support import HEADER
from abi_support import bits as _bits
from abi_support import good_draw as _good

ROW = checks.ROWS["draw"]


# ---- what this object adds to the checks every batch object gets (tests/batch_objects.py a to i) ------------------------------
def test_header_declares_the_eight_entry_points_and_the_contract():
    checks.header_declares_exactly_the_entry_points(ROW)
    text = open(HEADER).read()
    for words in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "6627e8d5 e169c58d bc57ac4c 9b00dbd8",
                  "cospi", "Marsaglia and Tsang", "src/cavitymd/simulation.py:57-92"):
        assert words in text, words


def test_the_version_is_still_2(capi):
    checks.the_version_is_still_2(capi)                                    # not a check on a row: it stays with each object


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_workspace_hence_no_draw_object(capi):
    with pytest.raises(capi.CavmdError) as e:
        capi.Draw(capi.Workspace(1), 7, [_good(capi)])
    assert e.value.status == capi.CAVMD_ERR_NO_DEVICE


def test_launch_order_is_item_order(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)     # the handle's rule, as for every object
    h = object.__new__(capi.Draw)
    h.sizes = [capi.Draw._size(_good(capi, dof=d)) for d in (3.0, 1293.0, 0.0, 2.0)]   # and its key is the same for all items
    assert h.sizes == [0, 0, 0, 0] and h.launch_order == [0, 1, 2, 3]


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
    import cavitymd
    with pytest.raises(ValueError, match="an integrator, a thermostat or both"):
        cavitymd.StepDraw(1)
    assert "callable raises" in cavitymd.step_draw.__doc__


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    chk = capi.draw_item_check
    assert lib.cavmd_draw_item_check(None) == INV
    assert chk(_good(capi)) == 0
    # either destination alone, not neither
    assert chk(_good(capi, verlet_row_ptr=0)) == 0 and chk(_good(capi, bussi_row_ptr=0)) == 0
    assert chk(_good(capi, verlet_row_ptr=0, bussi_row_ptr=0)) == INV
    # fixed mode: no records; the row counter and the capacity are then not looked at
    assert chk(_good(capi, records_ptr=0)) == 0 and chk(_good(capi, records_ptr=0, rows_ptr=0, capacity=0)) == 0
    # records without a counter, or with capacity 0
    assert chk(_good(capi, rows_ptr=0)) == INV and chk(_good(capi, capacity=0)) == INV
    # misalignment: 8 bytes for every pointer
    for field in ("d_verlet_row", "d_bussi_row", "d_records", "d_rows"):
        for off, status in ((4, INV), (1, INV), (8, 0)):
            it = _good(capi)
            setattr(it, field, getattr(it, field) + off)
            assert chk(it) == status, (field, off)
    # non-finite or negative constants; 0 is legal for each
    doubles = ("langevin_gamma", "langevin_kT", "bussi_set_T", "bussi_tau", "bussi_dof", "dt_initial", "tolerance_target",
               "tolerance_initial", "tolerance_time_constant", "dt_min", "dt_max")
    assert [name for name, ctype in capi.DrawItem._fields_ if ctype is ctypes.c_double] == list(doubles)
    for field in doubles:
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
            it = _good(capi)
            setattr(it, field, bad)
            assert chk(it) == INV, (field, bad)
        it = _good(capi, dt_min=0.0)
        if field != "dt_max":
            setattr(it, field, 0.0)
            assert chk(it) == 0, field
    # the clamp
    assert chk(_good(capi, dt_min=2.0, dt_max=1.0)) == INV and chk(_good(capi, dt_min=2.0, dt_max=2.0)) == 0
    assert chk(_good(capi, dt_min=0.0, dt_max=0.0)) == 0
    # reserved words
    for k in range(4):
        it = _good(capi)
        it.reserved[k] = 1 << (15 * k)
        assert chk(it) == INV, k
    # precedence, as the other objects have it: reserved words before pointers before values (all one status here)
    it = _good(capi, dt_min=2.0, dt_max=1.0)
    it.reserved[0] = 1
    assert chk(it) == INV


# ---- the generator ----------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                  "d16cfe09 94fdcceb 5001e420 24126ea1"))


def test_known_answers_of_philox_through_the_mirror():
    for counter, key, want in KNOWN_ANSWERS:
        got = mirror.philox(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert " ".join("%08x" % int(w) for w in got) == want, (counter, key)
    # block() puts seed and draws where the contract says: key = (seed low, seed high), counter = (draws low, high, item, purpose)
    seed, draws = 0x299f31d0a4093822, 0x85a308d3243f6a88
    got = mirror.block(seed, draws, 0x13198a2e, 0x03707344)
    assert " ".join("%08x" % int(w) for w in got) == KNOWN_ANSWERS[2][2]
    # vectorised over items as over single counters
    many = mirror.block(seed, np.array([draws, 0], dtype=np.uint64), np.array([0x13198a2e, 5], dtype=np.uint64), 0x03707344)
    assert (many[0] == got).all() and (many[1] == mirror.block(seed, 0, 5, 0x03707344)).all() and (many[1] != got).any()


def test_words_to_doubles_are_exact():
    top = np.uint64(0xffffffff)
    zero = np.uint64(0)
    assert mirror.unit(zero, zero) == 0.0 and mirror.unit(top, top) == 1.0 - 2.0 ** -53
    assert mirror.log_arg(zero, zero) == 2.0 ** -53 and mirror.log_arg(top, top) == 1.0
    assert mirror.unit(np.uint64(0x80000000), zero) == 0.5 and mirror.unit(zero, np.uint64(0x7ff)) == 0.0   # 11 low bits dropped
    assert mirror.unit(zero, np.uint64(0x800)) == 2.0 ** -53
    u = mirror.langevin_uniforms(11, np.arange(2000, dtype=np.uint64), 3)
    assert u.shape == (2000, 3) and (u >= -1.0).all() and (u < 1.0).all()
    assert (2.0 * mirror.unit(zero, zero) - 1.0, 2.0 * mirror.unit(top, top) - 1.0) == (-1.0, 1.0 - 2.0 ** -52)
    t = np.arange(0, 2049) / 1024.0
    assert np.abs(mirror.cospi(t) - np.cos(np.pi * t)).max() < 1e-15 and mirror.cospi(0.5) == 0.0 and mirror.cospi(1.5) == 0.0
    assert (mirror.cospi(np.array([0.0, 1.0, 2.0])) == [1.0, -1.0, 1.0]).all()


def test_the_bound_is_derived_from_the_function_accuracy(capi):
    assert mirror.EPS == 2.0 ** -52 and mirror.DELTA == 2 * mirror.FUNCTION_ULP * mirror.EPS and mirror.FUNCTION_ULP == 4
    assert mirror.NORMAL_REL == 16 * mirror.EPS and mirror.C_REL == mirror.DELTA
    assert "None of this is fitted" in mirror.__doc__


# ---- the fixed-mode rows ----------------------------------------------------------------------------------------------------
def test_fixed_mode_rows_equal_the_two_row_makers_byte_for_byte(capi):
    rng = np.random.default_rng(23)
    cases = [(5.0, 0.01, 3.167e-4, 9.5e-4, 100.0), (0.0, 0.01, 1.0, 1.0, 1.0), (5.0, 0.0, 1.0, 1.0, 0.0), (1e-300, 1e-3, 1e-3, 0.0, 1e-300),
             (41.341, 2.5e-5, 9.5e-4, 9.5e-4, 4134.1)]
    cases += [tuple(float(x) for x in 10.0 ** rng.uniform(-6, 3, 5)) for _ in range(300)]
    dt, gamma, kT, set_T, tau = (np.array(col) for col in zip(*cases))
    B = len(cases)
    it = dict(gamma=gamma, kT=kT, set_T=set_T, tau=tau, dof=np.full(B, 3.0), dt_initial=dt, tol_target=np.zeros(B),
              tol_initial=np.zeros(B), tol_time_constant=np.zeros(B), dt_min=np.zeros(B), dt_max=np.zeros(B))
    verlet, bussi, state, _ = mirror.step(5, it, mirror.new_state(B), np.zeros(B, dtype=bool), np.zeros(B, dtype=np.uint64),
                                          np.zeros(B))
    for k in range(B):
        v = capi.verlet_input_make(dt[k], gamma[k], kT[k], verlet[k, 3:6])
        b = capi.bussi_batch_input_make(dt[k], set_T[k], tau[k], bussi[k, 0], bussi[k, 1])
        assert bytes(v) == verlet[k].tobytes(), (k, cases[k])
        assert bytes(b) == bussi[k].tobytes(), (k, cases[k])
    assert (state["dt"] == dt).all() and (state["elapsed"] == dt).all() and (state["draws"] == 1).all()
    assert verlet[1, 6:7].view(np.uint64)[0] == 1 and bussi[1, 4:5].view(np.uint64)[0] == 1 and _bits(verlet[0, 6]) == 0


# ---- the mirror's samplers --------------------------------------------------------------------------------------------------
N_DRAWS = 100000
SHAPES = (0.5, 1.0, 1.5, 646.0)


@pytest.fixture(scope="module")
def gamma_draws():
    draws, item = np.arange(N_DRAWS, dtype=np.uint64) // np.uint64(1000), np.arange(N_DRAWS, dtype=np.uint64) % np.uint64(1000)
    return {a: mirror.gamma(2024, draws, item, np.full(N_DRAWS, a)) for a in SHAPES}


def test_moments_of_the_mirror(gamma_draws):
    """Mean and variance inside 6 standard errors of the analytic values: gamma(a) has mean a, variance a and fourth central
    moment 3 a^2 + 6 a, so the sample variance has variance (mu4 - a^2) / n = (2 a^2 + 6 a) / n."""
    for a, g in gamma_draws.items():
        v = g["value"]
        assert (v > 0.0).all() and not g["exhausted"].any()
        assert abs(v.mean() - a) < 6.0 * np.sqrt(a / N_DRAWS), (a, v.mean())
        assert abs(v.var() - a) < 6.0 * np.sqrt((2.0 * a * a + 6.0 * a) / N_DRAWS), (a, v.var())
        assert (g["bound"] >= 0.0).all() and (g["bound"] <= 1e-11 * v).all(), a     # the bound stays a rounding-error bound
    draws, item = np.arange(N_DRAWS, dtype=np.uint64) // np.uint64(1000), np.arange(N_DRAWS, dtype=np.uint64) % np.uint64(1000)
    n = mirror.normal(2024, draws, item, mirror.PURPOSE_NORMAL)
    assert abs(n.mean()) < 6.0 / np.sqrt(N_DRAWS) and abs(n.var() - 1.0) < 6.0 * np.sqrt(2.0 / N_DRAWS)
    u = mirror.langevin_uniforms(2024, draws, item)
    assert np.abs(u.mean(axis=0)).max() < 6.0 * np.sqrt(1.0 / 3.0 / N_DRAWS)
    assert np.abs(u.var(axis=0) - 1.0 / 3.0).max() < 6.0 * np.sqrt((1.0 / 5.0 - 1.0 / 9.0) / N_DRAWS)


def test_try_counts_of_the_mirror(gamma_draws):
    """No draw of the 4 x 10^5 needs more than 8 of the 16 tries, and at most 1 in 10^4 is too close to call."""
    for a, g in gamma_draws.items():
        assert g["tries"].max() <= 8, (a, g["tries"].max())
        assert g["ambiguous"].sum() <= N_DRAWS // 10000, (a, g["ambiguous"].sum())
    assert gamma_draws[646.0]["tries"].mean() < gamma_draws[1.0]["tries"].mean() < 1.1      # acceptance rises with the shape


def test_the_dt_rule_of_the_mirror():
    """Every branch of item 5 on hand-made numbers."""
    B = 8
    it = dict(gamma=np.full(B, 0.5), kT=np.full(B, 2.0), set_T=np.full(B, 2.0), tau=np.full(B, 4.0), dof=np.full(B, 3.0),
              dt_initial=np.full(B, 3.0), tol_target=np.full(B, 4.0), tol_initial=np.full(B, 1.0), tol_time_constant=np.zeros(B),
              dt_min=np.full(B, 0.5), dt_max=np.full(B, 8.0))
    st = mirror.new_state(B)
    st["draws"][:], st["dt"][:] = 2, 7.0
    adaptive = np.array([0, 1, 1, 1, 1, 1, 1, 1], dtype=bool)
    recorded = np.array([5, 0, 5, 5, 5, 5, 5, 5], dtype=np.uint64)
    S = np.array([1.0, 1.0, 1.0, 0.0, np.nan, np.inf, 1e-9, 1e9])
    ts = mirror.time_step(it, st, adaptive, recorded, S)
    assert list(ts["dt"]) == [3.0, 3.0, 2.0, 7.0, 7.0, 7.0, 8.0, 0.5]
    assert ts["coeff"][2] == np.sqrt(6.0 * 0.5 * 2.0 / 2.0) and ts["c"][2] == np.exp(-2.0 / 4.0) and ts["tolerance"][0] == 0.0
    st["draws"][:] = 0
    assert list(mirror.time_step(it, st, adaptive, recorded, S)["dt"][3:6]) == [3.0, 3.0, 3.0]      # no last dt yet: dt_initial
    it["tol_time_constant"][:] = 10.0
    st["elapsed"][:] = 10.0
    ts = mirror.time_step(it, st, adaptive, recorded, S)
    assert ts["tolerance"][2] == 4.0 - 3.0 * np.exp(-1.0) and ts["tolerance_bound"][2] < 1e-14 and ts["tolerance_bound"][0] == 0.0
