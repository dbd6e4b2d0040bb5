"""What is specific to the molecular force batch (cavmd_molecular_*) on a machine WITHOUT a GPU: the limits and the origin of the
expressions the header states, the order the library answers, every refusal of the two validations, the pair maker against the
numpy mirror bit for bit -- and the mirror itself (tests/molecular_mirror.py), which the GPU tests compare the kernel with,
against the closed-form answers.  Header, exports, layouts, null arguments, launch order, Python surface and deferred destroy
are the shared checks of tests/batch_objects.py, called here with this object's row."""
import ctypes
import re

import numpy as np
import torch

import batch_objects as checks
import molecular_mirror as mirror
from abi_support import HEADER, header_text
from abi_support import bits as _bits
from abi_support import good_molecular as _good
from abi_support import molecular_params as _params

ROW = checks.ROWS["molecular"]


# ---- 1. header and limits ---------------------------------------------------------------------------------------------
def test_header_declares_the_eight_entry_points_and_keeps_the_version():
    checks.header_declares_exactly_the_entry_points(ROW)
    raw = open(HEADER).read()
    assert re.search(r"#define\s+CAVMD_MOLECULAR_MAX_ITEM_N\s+2048\b", header_text())
    section = raw[raw.index("harmonic bonds and Lennard-Jones pairs of a batch"):]
    assert "[HOOMD upstream, not in checkout]" in section and "NOT pinned" in section


def test_libraries_export_them_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)
    rows, split = capi.molecular_order()
    assert split in (1, 4, 16) and rows * split == 256


def test_c_layouts_equal_the_ctypes_ones(capi, tmp_path):
    """... and tests/c_abi/molecular_abi_check.c prints the header's limits and what cavmd_molecular_order answers a C caller"""
    stdout = checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)
    limits = tuple(int(x) for x in re.search(r"limits (\d+) (\d+) (\d+) (\d+) (\d+)", stdout).groups())
    assert limits[:4] == (capi.MOLECULAR_MAX_ITEM_N, 8, 8, capi.MOLECULAR_MAX_BONDS) == (2048, 8, 8, 4)
    assert tuple(int(x) for x in re.search(r"order (\d+) (\d+)", stdout).groups()) == capi.molecular_order()
    assert limits[4] == capi.molecular_order()[1]


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------
def test_params_check_refusals(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    chk = capi.molecular_params_check
    assert lib.cavmd_molecular_params_check(None) == INV
    assert chk(_params(capi)) == 0 and chk(capi.MolecularParams()) == 0
    for field, value in (("n_types", 9), ("n_bond_types", 9), ("reserved", 1)):
        p = _params(capi)
        setattr(p, field, value)
        assert chk(p) == INV, field
    p = _params(capi)
    p.n_types = p.n_bond_types = 8                                           # the unused entries are zeros: legal
    assert chk(p) == 0
    for name in ("lj1", "lj2", "lj1_12", "lj2_6", "rcutsq", "eshift"):
        for bad in (np.nan, np.inf, -np.inf) + (() if name == "eshift" else (-1.0,)):
            p = _params(capi)
            setattr(p.pair[0][1], name, bad)
            setattr(p.pair[1][0], name, bad)
            assert chk(p) == INV, (name, bad)
    p = _params(capi)
    p.pair[0][1].eshift = p.pair[1][0].eshift = -1.0                         # an energy shift may have either sign
    assert chk(p) == 0
    p = _params(capi)
    p.pair[1][0].lj1 = np.nextafter(p.pair[0][1].lj1, np.inf)                # asymmetric by one ulp
    assert chk(p) == INV
    p = _params(capi)
    p.pair[2][2].reserved[1] = 1
    assert chk(p) == INV
    p.n_types = 2                                                            # ... but entries not in use are not looked at
    assert chk(p) == 0
    for field in ("K", "r0"):
        for bad in (np.nan, np.inf, -1.0):
            p = _params(capi)
            setattr(p.bond[1], field, bad)
            assert chk(p) == INV, (field, bad)
            p.n_bond_types = 1
            assert chk(p) == 0


def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    prm = _params(capi)
    chk = lambda it, p=prm: capi.molecular_item_check(p, it)
    assert lib.cavmd_molecular_item_check(ctypes.byref(prm), None) == INV
    assert lib.cavmd_molecular_item_check(None, ctypes.byref(_good(capi))) == INV
    bad_params = _params(capi)
    bad_params.reserved = 1
    assert chk(_good(capi), bad_params) == INV
    assert chk(_good(capi)) == 0 and chk(_good(capi, 4)) == 0 and chk(_good(capi, 2048)) == 0
    assert chk(capi.molecular_item(0, 0, 0, (0.0, 0.0, 0.0))) == 0           # an empty item may leave everything out
    assert chk(_good(capi, 2049)) == CAP and chk(_good(capi, 2**32 - 1)) == CAP
    # null and misaligned pointers
    for field in ("d_pos", "d_force"):
        it = _good(capi)
        setattr(it, field, None)
        assert chk(it) == INV, field
        for off, status in ((8, INV), (1, INV), (16, 0)):
            it = _good(capi)
            setattr(it, field, getattr(it, field) + off)
            assert chk(it) == status, (field, off)
    it = _good(capi)
    it.h_bonds = None
    assert chk(it) == INV
    it = _good(capi)
    it.h_bonds += 2
    assert chk(it) == INV
    # the box: every cut-off in use must fit min(L) / 2
    assert chk(_good(capi, box=(6.0, 9.0, 10.0))) == 0                       # r_cut = 3 = L / 2 exactly
    for box in ((np.nextafter(6.0, 0.0), 9.0, 10.0), (9.0, 5.0, 10.0), (9.0, 9.0, 1.0), (0.0, 9.0, 9.0), (-8.0, 9.0, 9.0),
                (np.nan, 9.0, 9.0), (np.inf, 9.0, 9.0)):
        assert chk(_good(capi, box=box)) == INV, box
    short = _params(capi)
    short.n_types = 1                                                        # pair (1, 1) is no longer in use, (0, 0) still is
    assert chk(_good(capi, box=(5.0, 9.0, 10.0)), short) == INV
    # the bond list
    for bonds, status in ((((0, 1, 0),), 0), (((0, 501, 0),), INV), (((501, 0, 0),), INV), (((7, 7, 0),), INV), (((0, 1, 2),), INV),
                          (((0, 1, 1),), 0), (((0, 1, 0), (0, 2, 0), (0, 3, 0), (4, 0, 1)), 0),
                          (((0, 1, 0), (0, 2, 0), (0, 3, 0), (4, 0, 1), (0, 5, 0)), INV),
                          (((0, 1, 0), (2, 1, 0), (3, 1, 0), (1, 4, 1), (5, 1, 0)), INV), (((2**32 - 1, 0, 0),), INV)):
        assert chk(_good(capi, bonds=bonds)) == status, bonds
    assert chk(_good(capi, 1, bonds=())) == 0 and chk(_good(capi, 1, bonds=((0, 0, 0),))) == INV
    assert chk(capi.molecular_item(0, 0, 0, (1.0, 1.0, 1.0), np.array([[0, 1, 0]]))) == INV
    it = _good(capi)
    it.reserved = 1 << 40
    assert chk(it) == INV


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)
    assert capi.load().cavmd_molecular_order(None, None) == 0


# ---- 3. the pair maker --------------------------------------------------------------------------------------------------
def test_pair_make_equals_the_mirror_bit_for_bit(capi):
    rng = np.random.default_rng(23)
    cases = [(0.00016685201, 6.230426584, 15.0), (0.000083426, 5.48277488, 15.0), (0.00025027802, 4.9832074319, 15.0),
             (0.0, 1.0, 0.0), (1.0, 1.0, 3.0), (1.0, 1.0, 0.0)]
    cases += [tuple(float(v) for v in (10.0 ** rng.uniform(-6, 1), 10.0 ** rng.uniform(-1, 1), 10.0 ** rng.uniform(-1, 1.5)))
              for _ in range(200)]
    names = ("lj1", "lj2", "lj1_12", "lj2_6", "rcutsq", "eshift")
    for epsilon, sigma, r_cut in cases:
        for shift in (True, False):
            got = capi.molecular_pair_make(epsilon, sigma, r_cut, shift)
            want = mirror.pair_constants(epsilon, sigma, r_cut, shift)
            assert [_bits(getattr(got, n)) for n in names] == [_bits(w) for w in want], (epsilon, sigma, r_cut, shift)
            assert list(got.reserved) == [0, 0]
            if not shift or r_cut == 0.0:
                assert _bits(got.eshift) == _bits(0.0)
    lib = capi.load()
    out = capi.MolecularPair()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_molecular_pair_make(1.0, 1.0, 3.0, 1, None) == INV
    for bad in ((-1.0, 1.0, 3.0), (1.0, -1.0, 3.0), (1.0, 1.0, -3.0), (np.nan, 1.0, 3.0), (1.0, np.inf, 3.0), (1.0, 1.0, np.nan),
                (1.0, 1e60, 3.0)):
        assert lib.cavmd_molecular_pair_make(*bad, 1, ctypes.byref(out)) == INV, bad
    tab = mirror.tables(_params(capi))
    assert tab["n_types"] == 3 and tab["n_bond_types"] == 2 and tab["rcutsq"][0, 1] == tab["rcutsq"][1, 0] == 9.0
    assert tab["rcutsq"][2, 0] == 0.0 and tab["K"][1] == 1.4                  # unlisted pairs stay switched off


# ---- 4. the Python surface, and the lattice its CPU systems are made of ------------------------------------------------------
def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
    import cavitymd
    from cavitymd import synthetic
    cfg = synthetic.diatomic_lattice(2, 8.0, seed=3)
    bonds, bond_typeid = synthetic.diatomic_bonds(cfg)
    assert len(cfg["charge"]) == 17 and bonds.tolist() == [[2 * m, 2 * m + 1] for m in range(8)]
    assert bond_typeid.tolist() == cfg["typeid"][0:16:2].tolist() and set(bond_typeid.tolist()) == {0, 1}
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"], cfg["box"],
                                           device="cpu")
    assert isinstance(pd.getPositions(), torch.Tensor)


def test_lattice_has_no_overlaps_and_its_molecules_are_at_their_bond_lengths():
    from cavitymd import synthetic
    cfg = synthetic.diatomic_lattice(4, 8.0, seed=1)
    x, L = cfg["position"][:-1], np.asarray(cfg["box"])
    assert len(cfg["charge"]) == 129 and cfg["typeid"][-1] == 2 and L.tolist() == [32.0] * 3 and not cfg["image"].any()
    d = x[:, None, :] - x[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d ** 2).sum(axis=2))
    bonds, bond_typeid = synthetic.diatomic_bonds(cfg)
    lengths = r[bonds[:, 0], bonds[:, 1]]
    assert np.allclose(lengths, np.where(bond_typeid == 0, synthetic.BOND_OO, synthetic.BOND_NN), rtol=1e-12)
    r[bonds[:, 0], bonds[:, 1]] = r[bonds[:, 1], bonds[:, 0]] = np.inf
    np.fill_diagonal(r, np.inf)
    assert r.min() >= 8.0 - synthetic.BOND_OO


# ---- 5. the mirror's own known answers -----------------------------------------------------------------------------------
def _lj_only(capi, epsilon, sigma, r_cut):
    return mirror.tables(capi.molecular_params(1, {}, {(0, 0): (epsilon, sigma, r_cut)}))


def test_mirror_two_particles_at_sigma_and_at_the_minimum(capi):
    S = capi.molecular_order()[1]
    epsilon, sigma = 0.25, 1.5
    tab = _lj_only(capi, epsilon, sigma, 4.0)
    F = mirror.forces(np.array([[-0.75, 0.0, 0.0], [0.75, 0.0, 0.0]]), [0, 0], (16.0, 16.0, 16.0), tab, [], S)
    assert np.allclose(F[:, 0], [-24 * epsilon / sigma, 24 * epsilon / sigma], rtol=1e-14) and not F[:, 1:3].any()
    assert np.isclose(F[:, 3].sum(), -tab["eshift"][0, 0], rtol=1e-13) and F[0, 3] == F[1, 3]
    r_min = 2.0 ** (1.0 / 6.0) * sigma
    F = mirror.forces(np.array([[0.0, 0.0, 0.0], [0.0, r_min, 0.0]]), [0, 0], (16.0, 16.0, 16.0), tab, [], S)
    assert np.abs(F[:, :3]).max() <= 1e-13 * 24 * epsilon / sigma             # the two terms of 24 eps / sigma cancel to rounding
    assert np.isclose(F[:, 3].sum(), -epsilon - tab["eshift"][0, 0], rtol=1e-13)


def test_mirror_one_stretched_bond(capi):
    S = capi.molecular_order()[1]
    K, r0, delta = 0.73204, 2.281655158, 0.125
    tab = mirror.tables(capi.molecular_params(1, {0: (K, r0)}, {}))
    x = np.array([[1.0, 2.0, 3.0], [1.0 + r0 + delta, 2.0, 3.0]])
    F = mirror.forces(x, [0, 0], (20.0, 20.0, 20.0), tab, [(0, 1, 0)], S)
    assert np.allclose(F[:, 0], [K * delta, -K * delta], rtol=1e-12) and not F[:, 1:3].any()
    assert np.allclose(F[:, 3], [0.25 * K * delta ** 2] * 2, rtol=1e-12) and F[0, 3] == F[1, 3]
    # across the periodic boundary the same bond gives the same answer
    x = np.array([[9.5, 0.0, 0.0], [9.5 + r0 + delta - 20.0, 0.0, 0.0]])
    trace = {}
    G = mirror.forces(x, [0, 0], (20.0, 20.0, 20.0), tab, [(0, 1, 0)], S, trace)
    assert np.allclose(G, F, rtol=1e-12) and trace["bond_across_boundary"] == 2


def test_mirror_pair_forces_are_antisymmetric_bit_for_bit(capi):
    """f_ij = -f_ji exactly, away from d = +-L/2 (where the two directions pick different images): each particle of a pair in
    an otherwise empty box carries exactly that one term."""
    S = capi.molecular_order()[1]
    tab = _lj_only(capi, 0.3, 1.1, 5.0)
    rng = np.random.default_rng(5)
    met = 0
    for _ in range(200):
        x = rng.uniform(-6.0, 6.0, (2, 3))
        F = mirror.forces(x, [0, 0], (12.0, 12.0, 12.0), tab, [], S)
        met += bool(F[0, :3].any())
        # equal as values: bit for bit wherever a term was added (a pair beyond the cut-off leaves +0 on both sides)
        assert np.array_equal(F[0, :3], -F[1, :3]) and not np.isnan(F).any() and F[0, 3] == F[1, 3]
    assert met >= 20
