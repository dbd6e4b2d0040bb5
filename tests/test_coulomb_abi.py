"""What is specific to the Coulomb force batch (cavmd_coulomb_*) on a machine WITHOUT a GPU: the limits and the origin of the
expressions the header states, the order the library answers, every refusal of the item check, the k-vector count against the
mirror's enumeration, the parameter formula -- and the mirror itself (tests/coulomb_mirror.py), which the GPU tests compare
the kernels with, against physics: the Madelung constant of rock salt, independence of the splitting parameter kappa with and
without a net charge, and F = -dE/dx.  Header, exports, layouts, null arguments, launch order, Python surface and deferred
destroy are the shared checks of tests/batch_objects.py, called here with this object's row."""
import ctypes
import re

import numpy as np
import pytest
import torch

import batch_objects as checks
import coulomb_mirror as mirror
from abi_support import COULOMB_BOX as BOX
from abi_support import HEADER, header_text
from abi_support import good_coulomb as _good

MADELUNG = 1.7475645946331822
ROW = checks.ROWS["coulomb"]


# ---- 1. header and limits ---------------------------------------------------------------------------------------------
def test_header_declares_the_nine_entry_points_and_keeps_the_version():
    checks.header_declares_exactly_the_entry_points(ROW)
    raw, text = open(HEADER).read(), header_text()
    assert re.search(r"#define\s+CAVMD_COULOMB_MAX_ITEM_N\s+2048\b", text) and re.search(r"#define\s+CAVMD_COULOMB_MAX_K\s+4096\b", text)
    section = raw[raw.index("Ewald Coulomb forces of a batch"):]
    assert "[HOOMD upstream, not in checkout]" in section and "NOT pinned" in section and "discretisation error" in section
    molecular = raw[raw.index("harmonic bonds and Lennard-Jones pairs of a batch"):raw.index("Ewald Coulomb forces of a batch")]
    assert "out of scope" not in molecular and "cavmd_coulomb_" in molecular


def test_libraries_export_them_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)
    rows, split, k_rows, k_split = capi.coulomb_order()
    assert split in (1, 4, 16, 64) and rows * split == 256 and k_split in (1, 4, 16, 64) and k_rows * k_split == 256


def test_c_layout_equals_the_ctypes_one(capi, tmp_path):
    """... and tests/c_abi/coulomb_abi_check.c prints the header's limits and what cavmd_coulomb_order answers a C caller"""
    stdout = checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)
    limits = tuple(int(x) for x in re.search(r"limits (\d+) (\d+) (\d+) (\d+) (\d+)", stdout).groups())
    assert limits[:3] == (capi.COULOMB_MAX_ITEM_N, capi.COULOMB_MAX_K, capi.COULOMB_MAX_EXCLUSIONS) == (2048, 4096, 4)
    order = tuple(int(x) for x in re.search(r"order (\d+) (\d+) (\d+) (\d+)", stdout).groups())
    assert order == capi.coulomb_order() and limits[3:] == (order[1], order[3])


# ---- 2. refusals and counts ---------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    chk = capi.coulomb_item_check
    assert lib.cavmd_coulomb_item_check(None) == INV
    assert chk(_good(capi)) == 0 and chk(_good(capi, 4)) == 0 and chk(_good(capi, 2048)) == 0
    assert chk(capi.coulomb_item(0, 0, 0, 0, (0.0, 0.0, 0.0), 0.0, 0.0, 0.0)) == 0   # an empty item may leave everything out
    assert chk(_good(capi, 2049)) == CAP and chk(_good(capi, 2**32 - 1)) == CAP
    # null and misaligned pointers
    for field, misaligned in (("d_pos", 8), ("d_force", 8), ("d_charge", 4)):
        it = _good(capi)
        setattr(it, field, None)
        assert chk(it) == INV, field
        for off, status in ((misaligned, INV), (1, INV), (16, 0)):
            it = _good(capi)
            setattr(it, field, getattr(it, field) + off)
            assert chk(it) == status, (field, off)
    it = _good(capi)
    it.d_charge += 8                                                             # charges need 8-byte alignment only
    assert chk(it) == 0
    it = _good(capi)
    it.h_exclusions = None
    assert chk(it) == INV
    it = _good(capi)
    it.h_exclusions += 2
    assert chk(it) == INV
    # the box and the real-space cut-off: r_cut^2 <= (min(L) / 2)^2
    assert chk(_good(capi, box=(8.0, 9.0, 10.0), r_cut=4.0)) == 0                # r_cut = L / 2 exactly
    for box in ((np.nextafter(8.0, 0.0), 9.0, 10.0), (9.0, 7.0, 10.0), (9.0, 9.0, 1.0), (0.0, 9.0, 9.0), (-8.0, 9.0, 9.0),
                (np.nan, 9.0, 9.0), (np.inf, 9.0, 9.0)):
        assert chk(_good(capi, box=box)) == INV, box
    # kappa: finite and positive; r_cut and k_cut: finite and not negative
    for bad in (0.0, -0.5, np.nan, np.inf, -np.inf):
        assert chk(_good(capi, kappa=bad)) == INV, bad
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        assert chk(_good(capi, r_cut=bad)) == INV and chk(_good(capi, k_cut=bad)) == INV, bad
    assert chk(_good(capi, r_cut=0.0)) == 0 and chk(_good(capi, k_cut=0.0)) == 0
    assert chk(_good(capi, k_cut=1e300)) == CAP and chk(_good(capi, k_cut=1e9)) == CAP     # answered at once, not enumerated
    # the exclusion list
    for ex, status in ((((0, 1),), 0), (((0, 501),), INV), (((501, 0),), INV), (((7, 7),), INV),
                       (((0, 1), (0, 2), (0, 3), (4, 0)), 0), (((0, 1), (0, 2), (0, 3), (4, 0), (0, 5)), INV),
                       (((0, 1), (2, 1), (3, 1), (1, 4), (5, 1)), INV), (((2**32 - 1, 0),), INV)):
        assert chk(_good(capi, exclusions=ex)) == status, ex
    assert chk(_good(capi, 1, exclusions=())) == 0 and chk(_good(capi, 1, exclusions=((0, 0),))) == INV
    assert chk(capi.coulomb_item(0, 0, 0, 0, (1.0, 1.0, 1.0), 1.0, 0.0, 0.0, np.array([[0, 1]]))) == INV
    it = capi.coulomb_item(501, 0x10000, 0x30000, 0x20000, BOX, 0.9, 4.0, 3.0, np.array([[0, 1, 77], [2, 3, 5]]))
    assert chk(it) == 0 and it.n_exclusions == 2                                # a bond list as it is: the type is ignored
    it = _good(capi)
    it.reserved = 1 << 40
    assert chk(it) == INV


def test_k_count_equals_the_mirror_enumeration(capi):
    CAP = capi.CAVMD_ERR_CAPACITY
    # k2 does not change with the signs of my and mz, so the counts a k_cut reaches come in shells: the box is stretched by
    # a fraction of a per cent until a shell ends after exactly K vectors (mirror.box_and_k_cut_for)
    for K in (0, 1, 2, 63, 64, 65, 300, 4096):
        box, k_cut = mirror.box_and_k_cut_for(BOX, K)
        assert capi.coulomb_k_count(_good(capi, box=box, k_cut=k_cut)) == K == len(mirror.k_vectors(box, k_cut)[2]), K
    # one vector beyond 4096
    box, k_cut = mirror.box_and_k_cut_for(BOX, 4097)
    assert len(mirror.k_vectors(box, k_cut)[2]) == 4097
    assert capi.coulomb_item_check(_good(capi, box=box, k_cut=k_cut)) == CAP
    with pytest.raises(capi.CavmdError) as e:
        capi.coulomb_k_count(_good(capi, box=box, k_cut=k_cut))
    assert e.value.status == CAP
    # the first vector is the longest box length's: k = 2 pi / 10 along z, kept when k2 == k_cut^2 exactly
    k1 = (mirror.TWO_PI * 1.0) / 10.0
    assert capi.coulomb_k_count(_good(capi, k_cut=np.sqrt(k1 * k1))) in (0, 1)
    assert capi.coulomb_k_count(_good(capi, k_cut=np.nextafter(k1, 1.0))) == 1 and capi.coulomb_k_count(_good(capi, k_cut=0.99 * k1)) == 0
    # rock salt's parameters, and an empty item
    assert capi.coulomb_k_count(_good(capi, 64, (), (4.0, 4.0, 4.0), 2.0, 2.0, 18.209)) == 3309 == len(mirror.k_vectors((4.0,) * 3, 18.209)[2])
    assert capi.coulomb_k_count(capi.coulomb_item(0, 0, 0, 0, (0.0, 0.0, 0.0), 0.0, 0.0, 0.0)) == 0
    m, k, k2 = mirror.k_vectors(BOX, 3.0)
    assert (m[:, 0] >= 0).all() and not ((m[:, 0] == 0) & (m[:, 1] < 0)).any() and (k2 > 0).all()
    assert [tuple(v) for v in m] == sorted(tuple(v) for v in m)                  # mx, then my, then mz ascending


def test_parameters_follow_the_formula(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    for r_cut, accuracy in ((4.0, 1e-6), (12.0, 1e-5), (2.0, 1e-12), (15.0, 0.5)):
        kappa, k_cut = capi.coulomb_parameters(r_cut, accuracy)
        s = np.sqrt(-np.log(accuracy))
        assert np.isclose(kappa, s / r_cut, rtol=1e-15) and np.isclose(k_cut, 2.0 * (s / r_cut) * s, rtol=1e-15)
    kappa, k_cut = ctypes.c_double(), ctypes.c_double()
    for bad in ((0.0, 1e-6), (-1.0, 1e-6), (np.nan, 1e-6), (np.inf, 1e-6), (4.0, 0.0), (4.0, 1.0), (4.0, -1e-6), (4.0, np.nan)):
        assert lib.cavmd_coulomb_parameters(*bad, ctypes.byref(kappa), ctypes.byref(k_cut)) == INV, bad
    assert lib.cavmd_coulomb_parameters(4.0, 1e-6, None, ctypes.byref(k_cut)) == INV


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)
    assert capi.load().cavmd_coulomb_order(None, None, None, None) == 0


# ---- 3. the Python surface ------------------------------------------------------------------------------------------------
def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    import cavitymd
    from cavitymd import synthetic
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
    cfg = synthetic.diatomic_lattice(2, 8.0, seed=3)
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"], cfg["box"],
                                           device="cpu")
    assert isinstance(pd.getCharges(), torch.Tensor)


# ---- 4. the mirror against physics ------------------------------------------------------------------------------------------
def test_mirror_gives_the_madelung_constant_of_rock_salt():
    g = np.arange(4)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    x = ijk.astype(np.float64) - 2.0
    q = np.where(ijk.sum(axis=1) % 2 == 0, 1.0, -1.0)
    F, bound = mirror.forces(x, q, (4.0, 4.0, 4.0), 2.0, 2.0, 18.209)
    assert len(mirror.k_vectors((4.0, 4.0, 4.0), 18.209)[2]) == 3309
    madelung = -2.0 * F[:, 3].sum() / 64
    print(f"\nMadelung constant from the mirror: {madelung!r}, off by {madelung - MADELUNG:.3e}")
    assert abs(madelung - MADELUNG) <= 2e-7
    assert np.abs(F[:, :3]).max() < 1e-12
    assert (bound >= 0).all() and bound[:, 3].max() < 1e-10


def _random_system(shifted):
    rng = np.random.default_rng(40)
    box = (8.0, 10.0, 12.0)
    x = rng.uniform(-0.5, 0.5, (40, 3)) * np.array(box)
    q = rng.uniform(-1.0, 1.0, 40)
    if shifted:
        q -= q.mean()
    return x, q, box


def test_mirror_is_independent_of_kappa_for_a_neutral_system():
    x, q, box = _random_system(True)
    Fa, _ = mirror.forces(x, q, box, 0.8, 4.0, 6.5)
    Fb, _ = mirror.forces(x, q, box, 0.9, 4.0, 7.3)
    dF, dE = np.abs(Fa[:, :3] - Fb[:, :3]).max(), abs(Fa[:, 3].sum() - Fb[:, 3].sum())
    print(f"\nneutral: force difference {dF:.3e} (scale {np.abs(Fa[:, :3]).max():.3f}), energy difference {dE:.3e}")
    assert dF <= 1e-5 and dE <= 1e-6
    assert np.abs(Fa[:, :3].sum(axis=0)).max() < 1e-13 and np.abs(Fb[:, :3].sum(axis=0)).max() < 1e-13


def test_mirror_is_independent_of_kappa_with_a_net_charge():
    """the neutralising background: without it the energy would move with kappa by pi Q^2 (1 / kappa_a^2 - 1 / kappa_b^2) / 2V"""
    x, q, box = _random_system(False)
    Q = q.sum()
    assert abs(Q) > 0.5
    Ea, Eb = mirror.energy(x, q, box, 0.8, 4.0, 6.5), mirror.energy(x, q, box, 0.9, 4.0, 7.3)
    background = np.pi * Q * Q / (2.0 * np.prod(box)) * (1.0 / 0.8 ** 2 - 1.0 / 0.9 ** 2)
    print(f"\ncharged (Q = {Q:.3f}): energy difference {abs(Ea - Eb):.3e}; the background term's share {background:.3e}")
    assert abs(Ea - Eb) <= 1e-6 and abs(background) > 1e-4


def test_mirror_force_is_minus_the_energy_gradient():
    x, q, box = _random_system(True)
    x[7] = x[3] + np.array([0.3, 0.0, 0.0])                                       # an excluded partner at r = 0.3
    ex = [(3, 7), (10, 11)]
    args = (q, box, 0.8, 4.0, 6.5, ex)
    F, _ = mirror.forces(x, *args)
    h = 1e-5
    for i in (3, 7, 20):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += h
            xm[i, c] -= h
            grad = (mirror.energy(xp, *args) - mirror.energy(xm, *args)) / (2 * h)
            # central differences: h^2 |E'''| / 6 (E''' ~ 6 q^2 / r^4 < 1e3 at r = 0.3: 2e-8) plus eps |E| / h rounding (1e-10)
            assert abs(F[i, c] + grad) <= 1e-7 * max(1.0, abs(F[i, c])), (i, c, F[i, c], -grad)
