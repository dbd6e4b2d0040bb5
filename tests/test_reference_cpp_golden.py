"""The CPU oracle against the reference's own compiled class, executed.  No GPU; runs on every machine and never skips.

tests/golden/cavity_reference_cpp_golden.npz holds inputs and the numbers the reference's CavityForceCompute (its .cc and
.h, unmodified, on the stand-in headers of tests/stubs/hoomd_force_reference) wrote for them; the generator next to it says
how.  Here oracle/cavity_ref.c -- the restatement every parity statement of the suite goes through -- must reproduce those
numbers BIT FOR BIT at -O2 and at -O3, as compiled by the compiler of the machine the test runs on.  So must the numpy
mirror's sequential mode (the bound tests/test_oracle_golden.py holds it to against the C oracle is equality).  What is NOT
pinned by this: the stand-in's vec3 operators and dot are written from memory of HOOMD-blue's header, unverified.
"""
import ctypes
import math

import numpy as np
import pytest

from oracle import numpy_mirror as nm
from oracle import reference_run
from reference_cpp_cases import NON_FINITE, SENTINEL, bits, load, same_bits

CASES, GENERATED_BY = load()
NAMES = [c["name"] for c in CASES]
EPS = np.finfo(float).eps


def _case(name):
    return CASES[NAMES.index(name)]


def _terms(c):
    """The addends c_i * (p_i + img_i * L) of the dipole, every operation rounded once, in index order; photon left in."""
    r = c["position"] + c["image"].astype(np.float64) * np.asarray(c["box"])[None, :]
    return c["charge"][:, None] * r


def _sequential(t):
    d = [0.0, 0.0, 0.0]
    for row in t.tolist():
        d[0] += row[0]
        d[1] += row[1]
        d[2] += row[2]
    return np.array(d)


def test_fixture_layout():
    assert "CavityForceCompute.cc" in GENERATED_BY and "-O2 -ffp-contract=off" in GENERATED_BY
    assert len(CASES) == 37 and len(set(NAMES)) == 37
    sizes = {len(c["charge"]) for c in CASES}
    assert {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1025, 2049} <= sizes
    for c in CASES:
        n = len(c["charge"])
        assert c["position"].shape == (n, 3) and c["image"].shape == (n, 3) and c["want"]["force"].shape == (n, 4)
        finite = np.isfinite(c["position"]).all()
        assert finite == (c["name"] not in NON_FINITE)
        # the reference wrote every entry: nothing of the driver's pre-fill is left
        assert not (c["want"]["force"] == SENTINEL).any(), c["name"]
        # photon index: the first particle whose tag's LOW word is the type id of 'L'
        hits = np.nonzero(c["typeid"] == c["L_typeid"])[0]
        assert c["want"]["photon_idx"] == (int(hits[0]) if hits.size else -1), c["name"]
    assert {c["L_typeid"] for c in CASES} == {0, 1, 2}
    assert _case("garbage_tag_high_words")["tag_high"].any() and not _case("size_257")["tag_high"].any()
    assert len(np.nonzero(_case("three_L")["typeid"] == 2)[0]) == 3
    assert _case("charged_photon")["charge"][128] == 7.5 and not _case("zero_charges")["charge"].any()
    assert np.abs(_case("images_1e5")["image"]).max() == 300_000 and not _case("images_zero")["image"].any()
    assert _case("phmass_1p7")["params"]["phmass"] == 1.7 and len(set(_case("cubic_box")["box"])) == 1
    assert len(set(_case("size_2049")["box"])) == 3


@pytest.mark.parametrize("opt", ["O2", "O3"])
def test_oracle_reproduces_the_executed_reference_bit_for_bit(oracle_mod, opt):
    ref = oracle_mod.RefOracle(opt)
    for c in CASES:
        want, finite = c["want"], c["name"] not in NON_FINITE
        p = ref.make_params(c["params"]["omegac"], c["params"]["couplstr"], c["params"]["phmass"])
        assert same_bits(p["K"], want["K"]), (c["name"], "K")
        pos4 = reference_run.pos4_of(c)
        out = ref.compute(pos4, c["charge"], c["image"], c["box"], c["L_typeid"], p)
        assert out["photon_idx"] == want["photon_idx"], c["name"]
        assert same_bits(out["force"], want["force"], finite), (c["name"], "force")
        assert same_bits(out["energies"], want["energies"], finite), (c["name"], "energies", out["energies"], want["energies"])
        # the dipole as computeDipoleMoment returns it for that index (with -1 it skips nobody): the oracle's own function
        n = len(c["charge"])
        r = np.ascontiguousarray(ref.unwrap(pos4, c["image"], c["box"]))
        chg = np.ascontiguousarray(c["charge"], dtype=np.float64)
        d = np.zeros(3)
        ref.lib.cavref_dipole(r.ctypes.data, chg.ctypes.data, n, ctypes.c_int(want["photon_idx"]), d.ctypes.data)
        assert same_bits(d, want["dipole"], finite), (c["name"], "dipole", d, want["dipole"])
        if want["photon_idx"] >= 0:
            assert same_bits(out["dipole"], want["dipole"], finite), (c["name"], "dipole of compute()")
        else:
            assert not bits(out["force"]).any() and not bits(out["energies"]).any(), c["name"]


def test_numpy_mirror_sequential_agrees_bit_for_bit():
    for c in CASES:
        want, finite = c["want"], c["name"] not in NON_FINITE
        p = dict(c["params"], K=want["K"])
        with np.errstate(invalid="ignore"):                            # 0.625 * NaN and 0 * Inf of the two non-finite cases
            m = nm.compute(reference_run.pos4_of(c), c["charge"], c["image"], c["box"], c["L_typeid"], p, "sequential")
        assert m["photon_idx"] == want["photon_idx"], c["name"]
        assert same_bits(m["force"], want["force"], finite), (c["name"], "force")
        assert same_bits(m["energies"], want["energies"], finite), (c["name"], "energies")
        if want["photon_idx"] >= 0:
            assert same_bits(m["dipole"], want["dipole"], finite), (c["name"], "dipole")


def test_numpy_mirror_fsum_dipole_within_the_a_priori_bound():
    """|sequential - exactly rounded| <= N eps sum|c_i r_i| (the classical bound test_oracle_golden.py uses)."""
    checked = 0
    for c in CASES:
        want = c["want"]
        if c["name"] in NON_FINITE or want["photon_idx"] < 0:
            continue
        p = dict(c["params"], K=want["K"])
        m = nm.compute(reference_run.pos4_of(c), c["charge"], c["image"], c["box"], c["L_typeid"], p, "fsum")
        t = np.abs(_terms(c))
        t[want["photon_idx"]] = 0.0
        bound = len(c["charge"]) * EPS * t.sum(axis=0)
        assert np.all(np.abs(m["dipole"] - want["dipole"]) <= bound), (c["name"], m["dipole"], want["dipole"], bound)
        checked += 1
    assert checked == 33        # 37 cases less two non-finite ones and two without a photon


# ---- the comparison has teeth, shown on the fixture itself --------------------------------------------------------------
def test_bit_equality_sees_the_summation_order():
    """The same addends summed by numpy's pairwise tree: some recorded dipole with N >= 257 differs in at least one bit, while
    the index-order loop reproduces every one of them."""
    differs = []
    for c in CASES:
        want = c["want"]
        if c["name"] in NON_FINITE or want["photon_idx"] < 0 or len(c["charge"]) < 257:
            continue
        t = np.delete(_terms(c), want["photon_idx"], axis=0)
        assert same_bits(_sequential(t), want["dipole"]), c["name"]
        # (numpy's tree applies to a contiguous 1-d array; a sum down the rows of an (N, 3) array runs in index order)
        pairwise = np.array([np.ascontiguousarray(t[:, k]).sum() for k in range(3)])
        if not same_bits(pairwise, want["dipole"]):
            differs.append(c["name"])
    assert differs, "a pairwise sum reproduced every recorded dipole: bit equality would not notice another order"


def test_bit_equality_sees_the_skip_rule():
    """Three L-typed particles: the reference's CPU class leaves out the FIRST one only (by index), the two others enter the
    dipole with their charges and get exactly zero force.  Leaving out by type gives another dipole."""
    c = _case("three_L")
    want = c["want"]
    t = _terms(c)
    L = np.nonzero(c["typeid"] == c["L_typeid"])[0]
    assert list(L) == [5, 100, 256] and want["photon_idx"] == 5 and np.all(c["charge"][L[1:]] != 0.0)
    assert same_bits(_sequential(np.delete(t, 5, axis=0)), want["dipole"])
    by_type = _sequential(np.delete(t, L, axis=0))
    assert not np.array_equal(by_type[:2], want["dipole"][:2])
    assert not bits(want["force"][L[1:]]).any()                       # all four entries +0.0: memset, never stored again
    assert want["force"][5, :3].all()


def test_recorded_zeros_carry_their_sign():
    for c in CASES:
        f, pidx = c["want"]["force"], c["want"]["photon_idx"]
        assert not bits(f[:, 3]).any(), c["name"]                      # .w: +0.0 everywhere
        mol = np.ones(len(f), dtype=bool)
        if pidx >= 0:
            mol[pidx] = False
        assert not bits(f[mol, 2]).any(), c["name"]                    # molecular z: +0.0
        if pidx < 0:
            assert not bits(f).any() and not bits(c["want"]["energies"]).any(), c["name"]
    # all charges zero: (-g * 0) * Dq = (-0.0) * Dq, whose sign is that of -Dq; d = 0 and Dq = q_xy + (g/K) * 0 = q_xy
    c = _case("zero_charges")
    f, pidx = c["want"]["force"], c["want"]["photon_idx"]
    assert not bits(c["want"]["dipole"]).any()
    q = c["position"][pidx] + c["image"][pidx].astype(np.float64) * np.asarray(c["box"])
    mol = np.arange(len(f)) != pidx
    assert q[0] != 0.0 and q[1] != 0.0 and not f[mol].any()
    for k in (0, 1):
        assert np.all(np.signbit(f[mol, k]) == (q[k] > 0.0)), k
    assert math.copysign(1.0, c["want"]["energies"][1]) == 1.0 and c["want"]["energies"][0] > 0.0
    # photon at the origin: q = +0.0, so E_h = +0.0 and the photon's z force is -K * 0 - g * 0 = -0.0
    c = _case("photon_at_origin")
    pidx = c["want"]["photon_idx"]
    assert bits(c["want"]["energies"][0]) == 0 and bits(c["want"]["energies"][1]) == 0
    assert bits(c["want"]["force"][pidx, 2]) == bits(-0.0)
