"""The reciprocal-space method of the Coulomb batch (cavmd_ewald_*) on a machine WITHOUT a GPU: the header declares the three
names and the two constants, every library exports them and _capi binds them, cavmd_ewald_order answers without a device, null
arguments are refused -- and the numpy restatement of the factored method (tests/coulomb_factored_mirror.py), which the GPU
tests compare the kernels with, against the direct mirror (within the sum of the two derived bounds) and against physics (the
Madelung constant of rock salt, and the energy of an NVE run of the host integrator, tests/ewald_factored_twin.py, conserved to
second order: the CPU twin of the GPU test's run)."""
import ctypes
import re

import numpy as np

import abi_support as abi
import coulomb_factored_mirror as factored
import coulomb_mirror as mirror
from coulomb_ragged import KAPPA, R_CUT, ragged_system

NAMES = ["cavmd_ewald_order", "cavmd_ewald_set_reciprocal", "cavmd_ewald_get_reciprocal"]
MADELUNG = 1.7475645946331822


# ---- the names -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_names_the_constants_and_the_multiplication_order():
    assert abi.declared("cavmd_ewald_") == sorted(NAMES)
    text = abi.header_text()
    at = [text.index("%s(" % n) for n in NAMES]
    assert at == sorted(at) and text.index("cavmd_coulomb_structure_device_ptr(") < at[0] < text.index("cavmd_trajectory_item_check(")
    assert re.search(r"#define\s+CAVMD_EWALD_RECIPROCAL_DIRECT\s+0\b", text) and re.search(r"#define\s+CAVMD_EWALD_RECIPROCAL_FACTORED\s+1\b", text)
    raw = " ".join(open(abi.HEADER).read().replace("*", " ").split())
    for words in ("phi_c = k1_c x_c with k1_c = (2 pi 1) / L_c", "ONE device sincos per particle and axis", "E_c(0) = (1, 0)",
                  "E_c(m) = E_c(m - 1) E_c(1)", "E_c(-m) = conj E_c(m)", "P(mx, my, zs) = (E_x(mx) E_y(my)) E_z(zs)",
                  "P(mx, my, mz + 1) = P(mx, my, mz) E_z(1)", "(a.re b.re - a.im b.im, a.re b.im + a.im b.re)",
                  "max(mx - 1, 0) + max(|my| - 1, 0) + max(|zs| - 1, 0) + 2 + (mz - zs)", "NOT bit-comparable",
                  "keeps the kernels it was captured with", "never an out-of-bounds access"):
        assert words in raw, words


def test_libraries_export_them_and_capi_binds_them(capi):
    paths = [capi.LIB_PATH, capi.HOOKS_LIB_PATH] + [capi.split_variant_path(name) for name in capi.SPLIT_VARIANTS]
    for path in paths:
        assert {s for s in abi.exported(path) if s.startswith("cavmd_ewald_")} == set(NAMES), path
    assert [n for n in capi._PROTOTYPES if n.startswith("cavmd_ewald_")] == NAMES                # the header's order
    assert set(NAMES) <= set(capi.EXPORTED_SYMBOLS)
    for lib in (capi.load(), capi.load_hooks_build()):
        for n in NAMES:
            assert getattr(lib, n).restype is ctypes.c_int
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"ewald_structure_factored_kernel" in blob and b"ewald_force_factored_kernel" in blob
    assert capi.EWALD_RECIPROCAL == {"direct": 0, "factored": 1}
    assert callable(capi.Coulomb.set_reciprocal) and isinstance(capi.Coulomb.reciprocal, property)
    import cavitymd
    assert callable(cavitymd.CoulombForceBatch.set_reciprocal) and isinstance(cavitymd.CoulombForceBatch.reciprocal, property)


def test_order_answers_without_a_device_and_the_limit_follows_from_the_lds(capi):
    text = abi.header_text()
    define = {name: int(re.search(r"#define\s+CAVMD_EWALD_%s\s+(\d+)\b" % name, text).group(1)) for name in ("TILE", "SEGMENT", "MAX_M")}
    for lib in (capi.load(), capi.load_hooks_build()):
        tile, seg, max_m, rows, seg_rows = capi.ewald_order(lib)
        assert (tile, seg, max_m) == (define["TILE"], define["SEGMENT"], define["MAX_M"])
        assert max_m >= 16 and seg == factored.SEGMENT
        assert rows >= 1 and 256 % rows == 0 and seg_rows >= 1 and 256 % seg_rows == 0 and tile % (256 // seg_rows) == 0
        # the LDS arithmetic of the header: the largest M whose tile of tables fits 64 KiB, and launch 2's tables as well
        assert tile * (3 * (max_m + 1) * 16 + 8) <= 65536 < tile * (3 * (max_m + 2) * 16 + 8)
        assert rows * 3 * (max_m + 1) * 16 <= 65536
        assert lib.cavmd_ewald_order(None, None, None, None, None) == 0
        only = ctypes.c_int(-1)
        assert lib.cavmd_ewald_order(None, None, ctypes.byref(only), None, None) == 0 and only.value == max_m
    # the split variants answer the same: the factored kernels do not depend on the direct kernels' splits
    for name in capi.SPLIT_VARIANTS:
        assert capi.ewald_order(capi.load_split_variant(name)) == capi.ewald_order()


def test_null_handles_and_null_outputs_are_refused(capi):
    INV = capi.CAVMD_ERR_INVALID_VALUE
    for lib in (capi.load(), capi.load_hooks_build()):
        method = ctypes.c_int(7)
        assert lib.cavmd_ewald_set_reciprocal(None, capi.EWALD_RECIPROCAL_DIRECT) == INV
        assert lib.cavmd_ewald_set_reciprocal(None, capi.EWALD_RECIPROCAL_FACTORED) == INV
        assert lib.cavmd_ewald_set_reciprocal(None, 2) == INV
        assert lib.cavmd_ewald_get_reciprocal(None, ctypes.byref(method)) == INV and method.value == 7
        assert lib.cavmd_ewald_get_reciprocal(None, None) == INV


# ---- the factored mirror -----------------------------------------------------------------------------------------------------
def test_segments_cut_every_row_from_its_first_vector():
    m = mirror.k_vectors((8.0, 10.0, 30.0), 2.6)[0]
    start = factored.segments(m)
    assert len(m) > 300 and start[0] == 0
    longest = 0
    for k in range(len(m)):
        s = start[k]
        assert 0 <= k - s < factored.SEGMENT and (m[k, :2] == m[s, :2]).all() and m[k, 2] - m[s, 2] == k - s
        if s == k and k:
            prev_row = tuple(m[k - 1, :2]) == tuple(m[k, :2]) and m[k - 1, 2] + 1 == m[k, 2]
            assert not prev_row or k - start[k - 1] == factored.SEGMENT            # a new segment inside a row: the last one was full
        longest = max(longest, k - s + 1)
    assert longest == factored.SEGMENT                                            # rows of 2 * 12 + 1 vectors: full segments occur


def test_factored_mirror_agrees_with_the_direct_mirror_within_the_sum_of_the_bounds():
    """The bound holds for the reference arithmetic alone, before any kernel is held to it: the ragged systems of the GPU test."""
    rng = np.random.default_rng(20261018)
    worst = 0.0
    for k, (n, K) in enumerate(((1, 2), (2, 1), (17, 65), (63, 300), (64, 63), (65, 0), (501, 200), (130, 1000))):
        s = ragged_system(k, n, K, rng)
        direct = mirror.forces(s["x"], s["q"], s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"])
        F, bound = factored.forces(s["x"], s["q"], s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"], direct=direct)
        assert F.shape == direct[0].shape and np.isfinite(F).all() and (bound >= 0).all()
        err, allowed = np.abs(F - direct[0]), bound + direct[1]
        ratio = float((err[allowed > 0] / allowed[allowed > 0]).max()) if (allowed > 0).any() else 0.0
        worst = max(worst, ratio)
        print(f"\nitem {k}: N = {n}, K = {K}, largest |factored - direct| / (sum of the bounds) = {ratio:.4f}")
        assert (err <= allowed).all(), (k, n, K, ratio)
        if K == 0:
            assert (F == direct[0]).all()                                         # no reciprocal part: the same arithmetic
        elif n >= 17:
            assert (F != direct[0]).any()                                         # and not the same evaluation in disguise
    print(f"\nlargest ratio: {worst:.4f}")


def test_phases_lie_on_the_unit_circle_and_follow_the_exact_angle():
    rng = np.random.default_rng(7)
    box = (8.0, 10.0, 30.0)
    x = rng.uniform(-0.5, 0.5, (50, 3)) * np.array(box)
    x[0] = (-4.0, -5.0, -15.0)                                                    # x = -L / 2 exactly
    m, k, _ = mirror.k_vectors(box, 2.6)
    c, s = factored.phases(x, box, m)
    theta = np.asarray([[float(np.dot(np.longdouble(kk), np.longdouble(xx))) for kk in k] for xx in x])
    # G is counted against the exact m_c k1_c x_c; the direct k_c = (2 pi m_c) / L_c rounds differently, by at most eps |theta|
    G = factored.phase_term(x, box, m) + float(np.abs(theta).max())
    assert np.abs(c - np.cos(theta)).max() <= mirror.EPS * G and np.abs(s - np.sin(theta)).max() <= mirror.EPS * G
    assert np.abs(c * c + s * s - 1.0).max() <= mirror.EPS * G


def test_factored_mirror_gives_the_madelung_constant_of_rock_salt():
    g = np.arange(4)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    x = ijk.astype(np.float64) - 2.0
    q = np.where(ijk.sum(axis=1) % 2 == 0, 1.0, -1.0)
    F, bound = factored.forces(x, q, (4.0, 4.0, 4.0), 2.0, 2.0, 18.209)
    madelung = -2.0 * F[:, 3].sum() / 64
    print(f"\nMadelung constant from the factored mirror: {madelung!r}, off by {madelung - MADELUNG:.3e}")
    assert abs(madelung - MADELUNG) <= 2e-7
    assert np.abs(F[:, :3]).max() < 1e-12
    assert (bound >= 0).all() and bound[:, 3].max() < 1e-10


def test_cpu_twin_with_the_factored_forces_conserves_energy_to_second_order(capi):
    """The NVE run of tests/test_gpu_ewald_reciprocal.py on the host (tests/ewald_factored_twin.py: the 12 charged dimers and the
    photon from that test's own start, the host integrator of tests/device_start_twin.py with the factored mirror's Ewald
    forces): 200 steps at dt = 10 against 400 at dt = 5, the band tests/test_device_start_twin.py holds the direct twin to.
    Beside it the same run with the direct mirror: the two differ by rounding per step, so their energies stay together far
    below the integrator's own drift (1e-3 of it leaves thirteen orders of magnitude over one rounding)."""
    import device_start_cases as cases
    import device_start_twin as twin
    import ewald_factored_twin
    d = ewald_factored_twin.Dimers("factored")
    runs = {dt: twin.system_total(d.run_thermal(dt, steps))
            for dt, steps in ((cases.DRIFT_DT, cases.DRIFT_STEPS), (0.5 * cases.DRIFT_DT, 2 * cases.DRIFT_STEPS))}
    drift = {dt: twin.drift(H) for dt, H in runs.items()}
    ratio = drift[cases.DRIFT_DT] / drift[0.5 * cases.DRIFT_DT]
    direct = twin.system_total(ewald_factored_twin.Dimers("direct").run_thermal(cases.DRIFT_DT, cases.DRIFT_STEPS))
    apart = float(np.abs(direct - runs[cases.DRIFT_DT]).max())
    print(f"\nfactored twin: drift over {cases.DRIFT_STEPS} steps at dt = {cases.DRIFT_DT}: {drift[cases.DRIFT_DT]:.4e}; at dt / 2: "
          f"{drift[0.5 * cases.DRIFT_DT]:.4e}; ratio {ratio:.4f}; largest |H_factored - H_direct|: {apart:.3e}")
    assert 3.5 <= ratio <= 4.5, (drift, ratio)
    assert runs[cases.DRIFT_DT][0] == runs[0.5 * cases.DRIFT_DT][0]               # one start
    assert apart <= 1e-3 * drift[cases.DRIFT_DT], (apart, drift)
