"""The two parts of the Ewald sum and the kick (cavmd_mts_*) on a machine WITHOUT a GPU: the header declares the three names
and the two constants, a C99 program sees them, every library exports them and _capi binds them, null handles are refused (the
refusals that need a live handle are tests/test_gpu_coulomb_parts.py's and tests/test_gpu_verlet_kick.py's: without a device
there is no workspace, hence no batch) -- and the numpy restatement of the parts (tests/coulomb_parts_mirror.py) against
tests/coulomb_mirror.py, and the impulse scheme on the host twin of the dimers (tests/mts_twin.py) against second order."""
import ctypes
import math
import re

import numpy as np
import pytest

import abi_support as abi
import coulomb_mirror as mirror
import coulomb_parts_mirror as parts
import device_start_cases as cases
import device_start_twin as twin
from coulomb_ragged import KAPPA, R_CUT, ragged_system

NAMES = ["cavmd_mts_verlet_kick", "cavmd_mts_coulomb_set_long_forces", "cavmd_mts_coulomb_compute_parts"]
SYSTEMS = ((1, 2), (2, 1), (17, 65), (63, 300), (64, 63), (65, 0), (501, 200), (130, 1000))


# ---- the names -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_names_the_constants_and_the_grouping():
    assert abi.declared("cavmd_mts_") == sorted(NAMES)
    text = abi.header_text()
    at = [text.index("%s(" % n) for n in NAMES]
    assert at == sorted(at)                                                        # the kick with the integrator, the parts behind
    assert text.index("cavmd_verlet_step_two(") < at[0] < text.index("cavmd_verlet_read(")     # the reciprocal methods
    assert text.index("cavmd_ewald_get_reciprocal(") < at[1] < text.index("cavmd_trajectory_item_check(")
    assert re.search(r"#define\s+CAVMD_COULOMB_PART_SHORT\s+1u\b", text) and re.search(r"#define\s+CAVMD_COULOMB_PART_LONG\s+2u\b", text)
    raw = " ".join(open(abi.HEADER).read().replace("*", " ").split())
    for words in ("NOT an exclusion partner and has rsq < r_cut^2 (strict)", "no self and no background term",
                  "the erf term of the at most four exclusion partners (no cut-off)", "Q accumulated over all j on the way",
                  "p = p + (2 q_i) r", "stores {Q, 0} behind the structure factors", "NOT bit-comparable with cavmd_coulomb_compute",
                  "never touches a long array", "h = weight dt; minv = 1.0 / m; v_c = v_c + (f_c minv) h",
                  "vel.w, d_accel, d_net_force, the state and its `steps` keep their bytes",
                  "under the adaptive rule it is unsupported", "unmatched opening kick"):
        assert words in raw, words


def test_a_c99_program_sees_the_constants_and_the_null_refusals(capi, tmp_path):
    out = abi.run_c99("mts_abi_check", capi, tmp_path)
    assert "MTS-ABI-OK" in out
    assert "CAVMD_COULOMB_PART_SHORT 1\n" in out and "CAVMD_COULOMB_PART_LONG 2\n" in out
    assert (capi.COULOMB_PART_SHORT, capi.COULOMB_PART_LONG) == (1, 2)
    assert capi.COULOMB_PARTS == {"short": 1, "long": 2, "both": 3}


def test_libraries_export_them_and_capi_binds_them(capi):
    paths = [capi.LIB_PATH, capi.HOOKS_LIB_PATH] + [capi.split_variant_path(name) for name in capi.SPLIT_VARIANTS]
    for path in paths:
        assert {s for s in abi.exported(path) if s.startswith("cavmd_mts_")} == set(NAMES), path
    assert set(NAMES) <= set(capi.EXPORTED_SYMBOLS)
    for lib in (capi.load(), capi.load_hooks_build()):
        for n in NAMES:
            assert getattr(lib, n).restype is ctypes.c_int
        assert len(lib.cavmd_mts_verlet_kick.argtypes) == 5 and lib.cavmd_mts_verlet_kick.argtypes[4] is ctypes.c_double
        assert len(lib.cavmd_mts_coulomb_set_long_forces.argtypes) == 3 and len(lib.cavmd_mts_coulomb_compute_parts.argtypes) == 3
    blob = open(capi.LIB_PATH, "rb").read()
    for kernel in (b"coulomb_short_kernel", b"coulomb_long_kernel", b"ewald_long_factored_kernel", b"verlet_kick_kernel"):
        assert kernel in blob, kernel
    assert callable(capi.Coulomb.set_long_forces) and callable(capi.Coulomb.compute_parts) and callable(capi.Verlet.kick)
    import cavitymd
    assert callable(cavitymd.VerletBatch.kick) and callable(cavitymd.VerletBatch.kick_table)
    assert isinstance(cavitymd.CoulombForceBatch.forces_long, property)


def test_null_handles_are_refused(capi):
    INV = capi.CAVMD_ERR_INVALID_VALUE
    for lib in (capi.load(), capi.load_hooks_build()):
        two = (ctypes.c_void_p * 2)(0x10000, 0x20000)
        assert lib.cavmd_mts_coulomb_set_long_forces(None, 2, two) == INV
        assert lib.cavmd_mts_coulomb_set_long_forces(None, 0, None) == INV
        for p in (0, 1, 2, 3, 4, 0xFFFFFFFF):
            assert lib.cavmd_mts_coulomb_compute_parts(None, None, p) == INV
        for weight in (0.5, math.nan, math.inf):
            assert lib.cavmd_mts_verlet_kick(None, None, ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), weight) == INV


# ---- the mirror of the parts -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def systems():
    rng = np.random.default_rng(20261018)
    return [ragged_system(k, n, K, rng) for k, (n, K) in enumerate(SYSTEMS)]


@pytest.mark.parametrize("method", ["direct", "factored"])
def test_short_plus_long_is_the_ewald_sum_within_the_two_bounds(systems, method):
    """Held to b_short + b_long alone, not to coulomb_mirror's bound on top: the three are different orders of the same terms."""
    worst = 0.0
    for k, s in enumerate(systems):
        args = (s["x"], s["q"], s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"])
        whole = mirror.forces(*args)[0]
        Fs, bs = parts.short(*args)
        Fl, bl = parts.long(*args, method=method)
        assert Fs.shape == Fl.shape == whole.shape and np.isfinite(Fs).all() and np.isfinite(Fl).all()
        assert (bs >= 0).all() and (bl >= 0).all()
        err, allowed = np.abs((Fs + Fl) - whole), bs + bl
        ratio = float((err[allowed > 0] / allowed[allowed > 0]).max()) if (allowed > 0).any() else 0.0
        worst = max(worst, ratio)
        print(f"\nitem {k}: N = {s['N']}, K = {s['K']}, largest |short + long - whole| / (b_short + b_long) = {ratio:.4f}")
        assert (err <= allowed).all(), (k, ratio)
        if method == "direct":
            # the absolute terms are split, none is counted twice: the two bounds sum to at most the whole bound
            assert (allowed <= mirror.forces(*args)[1] * (1.0 + 1e-12)).all(), k
        if s["N"] > 17:
            assert Fs[:, :3].any() and Fl[:, :3].any()                               # neither part is the whole in disguise
    print(f"\nlargest ratio ({method}): {worst:.4f}")


def test_short_is_the_sum_without_k_vectors_and_exclusions_less_self_and_background(systems):
    for k, s in enumerate(systems):
        whole, bound = mirror.forces(s["x"], s["q"], s["box"], KAPPA, R_CUT, 0.0, ())
        Fs, bs = parts.short(s["x"], s["q"], s["box"], KAPPA, R_CUT, 0.0, ())
        assert (Fs[:, :3] == whole[:, :3]).all(), k                                  # the same terms in the same arithmetic
        w = whole[:, 3] - parts.self_and_background(s["q"], s["box"], KAPPA)
        assert (np.abs(Fs[:, 3] - w) <= bs[:, 3] + bound[:, 3]).all(), k
        # ... and with the exclusions, the excluded pairs are what is missing: long carries their erf terms instead
        Fx = parts.short(s["x"], s["q"], s["box"], KAPPA, R_CUT, 0.0, s["ex"])[0]
        if len(s["ex"]) and s["N"] > 17:
            assert (Fx != Fs).any(), k
        if s["N"] > 17:
            assert (Fs[17] == 0.0).all() and (parts.long(s["x"], s["q"], s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"])[0][17] == 0.0).all()


# ---- the impulse scheme on the host twin ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dimers(capi):
    import mts_twin
    return mts_twin.Dimers("direct")


def _drift_ratio(dimers, n, weight=None):
    import mts_twin
    DT, STEPS = cases.DRIFT_DT, cases.DRIFT_STEPS
    drift = {dt: twin.drift(mts_twin.system_total(dimers.run_mts(dt, steps, n, weight)))
             for dt, steps in ((DT, STEPS), (0.5 * DT, 2 * STEPS))}
    ratio = drift[DT] / drift[0.5 * DT]
    print(f"\nn = {n}, weight = {0.5 * n if weight is None else weight}: drift over {STEPS} steps at dt = {DT}: {drift[DT]:.4e}; at dt / 2: "
          f"{drift[0.5 * DT]:.4e}; ratio {ratio:.4f}")
    return drift, ratio


@pytest.mark.parametrize("n", [1, 2, 4])
def test_the_impulse_scheme_conserves_energy_to_second_order_on_the_host(dimers, n):
    """The band tests/test_device_start_twin.py and tests/test_ewald_reciprocal_abi.py hold their NVE twins to: 200 steps at
    dt = 10 against 400 at dt = 5.  Rehearsed: ratio 3.9998 (n = 1, drift 1.5256e-4 at dt, the plain twin's), 3.9999 (n = 2),
    3.8956 (n = 4, drift 1.4936e-4)."""
    drift, ratio = _drift_ratio(dimers, n)
    assert 3.5 <= ratio <= 4.5, (drift, ratio)


def test_a_kick_of_weight_one_half_instead_of_n_halves_leaves_the_band(dimers):
    """A planted mistake: with n = 4 and kicks of weight 1 / 2 the long force acts a quarter as long as it should, the energy
    is no longer conserved and halving dt does not help (rehearsed: drift 2.4e-3 at either dt, ratio 1.02)."""
    drift, ratio = _drift_ratio(dimers, 4, weight=0.5)
    assert not 3.5 <= ratio <= 4.5, (drift, ratio)
