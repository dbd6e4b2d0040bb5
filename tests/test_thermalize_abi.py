"""What is specific to the thermalize object (cavmd_thermalize_*, cavitymd.BatchThermalizer) on a machine WITHOUT a GPU
(tests/test_batch_objects_abi.py runs the shared checks a to i on its row of tests/batch_objects.py; none is skipped): the
header's prose, the split variants' exports, the tile constant, every refusal of its item check, the mirror's counters
(tests/thermalize_mirror.py) against the known answers of Philox in the header, the mirror's photon expressions against the
driver's own numpy lines bit for bit, and the inputs of tests/test_gpu_thermalize_batch.py (tests/thermalize_cases.py) run
through the mirror alone: inside the statistical bands, and without one ambiguous wrap."""
import ctypes

import numpy as np
import pytest
import torch

import batch_objects as checks
import draw_mirror
import thermalize_cases as cases
import thermalize_mirror as mirror
from abi_support import HEADER, exported
from abi_support import good_thermalize as _good

byref, vp = ctypes.byref, ctypes.c_void_p


ROW = checks.ROWS["thermalize"]


# ---- what this object adds to the checks every batch object gets (tests/batch_objects.py a to i) ------------------------------
def test_header_declares_the_eight_entry_points_and_the_contract():
    checks.header_declares_exactly_the_entry_points(ROW)
    text = open(HEADER).read()
    for words in ("0xC0000000 + c", "0xC0000008 + c", "sigma = sqrt(kT / m)", "v_c = v_c - (P_c / (double)thermalised) / m",
                  "x_c = FINITE_Q ? ((-d_c) * g) / K : 0", "i_c = floor((x_c + L_c / 2) / L_c)", "pos_c = x_c - i_c * L_c",
                  "examples/05_advanced_run.py:710-750", ":455-494", "FROM KNOWLEDGE",
                  "this is NOT checked", "after it the same variates come again", "#define CAVMD_THERMALIZE_TILE 512u"):
        assert words in text, words
    assert "parity with it is pinned by nothing" in " ".join(text.replace("*", " ").split())
    # the new prefix is no prefix of another object's, nor another's of it
    for obj in checks.OBJECTS:
        assert obj is ROW or not ((obj.prefix + "_").startswith(ROW.prefix + "_") or (ROW.prefix + "_").startswith(obj.prefix + "_")), \
            obj.prefix


def test_libraries_export_the_entry_points_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)
    for name in sorted(capi.SPLIT_VARIANTS):                                 # and so does every split variant
        mine = {s for s in exported(capi.split_variant_path(name)) if s.startswith(ROW.prefix + "_")}
        assert mine == {ROW.prefix + "_" + e for e in ROW.entry_points}, name


def test_the_version_is_still_2(capi):
    checks.the_version_is_still_2(capi)                                    # not a check on a row: it stays with each object


def test_c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)
    assert mirror.TILE == capi.THERMALIZE_TILE == cases.T == 512


def test_null_arguments_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)
    assert capi.load().cavmd_thermalize_create(None, 0, byref(_good(capi)), byref(vp())) == capi.CAVMD_ERR_INVALID_VALUE


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_workspace_hence_no_thermalize_object(capi):
    with pytest.raises(capi.CavmdError) as e:
        capi.Thermalize(capi.Workspace(1), [_good(capi)])
    assert e.value.status == capi.CAVMD_ERR_NO_DEVICE


def test_launch_order_is_a_stable_descending_sort(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)
    assert capi.Thermalize._size(_good(capi, N=77)) == 77


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
    import cavitymd
    doc = cavitymd.thermalize_batch.__doc__
    order = [doc.index(call) for call in ("cavity.compute()   ", "thermalizer.thermalize()", "cavity.compute(); molecular.compute()",
                                          "integrator.prime()")]
    assert order == sorted(order)                        # the order of a start
    assert "0x9E3779B97F4A7C15" in doc and "not HOOMD's RandomGenerator" in doc and "pinned by nothing" in doc
    assert [capi.bath_item_key(5, i) for i in range(4)] == [mirror.item_key(5, i) for i in range(4)]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    ZERO, PLACE, FQ, PV = (capi.THERMALIZE_ZERO_MOMENTUM, capi.THERMALIZE_PLACE_PHOTON, capi.THERMALIZE_FINITE_Q,
                           capi.THERMALIZE_PHOTON_VELOCITY)
    chk = capi.thermalize_item_check
    assert lib.cavmd_thermalize_item_check(None) == INV
    assert chk(_good(capi)) == 0
    assert chk(capi.ThermalizeItem()) == 0                                   # N == 0 with nothing behind it: untouched
    # d_vel is required; the default set needs no list, an empty list is a pointer with n_members 0
    assert chk(_good(capi, vel_ptr=0)) == INV and chk(_good(capi, vel_ptr=0, N=0)) == 0
    assert chk(_good(capi, members_ptr=0, n_members=0)) == 0 and chk(_good(capi, n_members=0)) == 0
    assert chk(_good(capi, members_ptr=0)) == INV
    # misalignment: 16 bytes for the Scalar4 arrays, 4 for the index and image arrays, 8 for the result block
    for field, offsets in (("d_vel", ((8, INV), (4, INV), (1, INV), (16, 0))), ("d_pos", ((8, INV), (4, INV), (16, 0))),
                           ("d_members", ((1, INV), (2, INV), (4, 0))), ("d_image", ((1, INV), (2, INV), (4, 0))),
                           ("d_result", ((4, INV), (1, INV), (8, 0)))):
        for off, status in offsets:
            it = _good(capi)
            setattr(it, field, getattr(it, field) + off)
            assert chk(it) == status, (field, off)
    # kT, the box and the params: finite and >= 0
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert chk(_good(capi, kT=bad)) == INV, bad
        for c in range(3):
            box = [40.0, 41.0, 42.0]
            box[c] = bad
            assert chk(_good(capi, box_L=box)) == INV, (c, bad)
        for name in ("omegac", "couplstr", "K", "phmass"):
            it = _good(capi)
            setattr(it.params, name, bad)
            assert chk(it) == INV, (name, bad)
    assert chk(_good(capi, kT=0.0)) == 0 and chk(_good(capi, kT=1e300)) == 0
    assert chk(_good(capi, params=capi.make_params(0.0091, 0.0, 1.0))) == 0  # g = 0: no spread, no displacement
    # the placement divides by every edge and by K; without it a box of 0 and K = 0 are nobody's business
    assert chk(_good(capi, box_L=(40.0, 0.0, 42.0))) == INV and chk(_good(capi, params=capi.make_params(0.0, 1e-3, 1.0))) == INV
    assert chk(_good(capi, flags=ZERO | PV, box_L=(0.0, 0.0, 0.0), params=capi.Params())) == 0
    # the displaced start needs the dipole; the placement needs the photon's row, its image and the result block
    assert chk(_good(capi, flags=FQ, result_ptr=0)) == INV and chk(_good(capi, flags=FQ)) == 0
    for missing in ("pos_ptr", "image_ptr", "result_ptr"):
        assert chk(_good(capi, flags=PLACE, **{missing: 0})) == INV, missing
        assert chk(_good(capi, flags=ZERO | PV, **{missing: 0})) == 0, missing
    assert chk(_good(capi, flags=PLACE)) == 0 and chk(_good(capi, flags=0)) == 0
    # any seed is a key; an unknown flag is refused
    for seed in (0, 1, 2 ** 64 - 1):
        assert chk(_good(capi, seed=seed)) == 0
    for bit in (16, 1 << 31):
        assert chk(_good(capi, flags=ZERO | bit)) == INV, bit
    # the cap, on N and on the list
    assert chk(_good(capi, N=capi.BATCH_MAX_ITEM_N, n_members=capi.BATCH_MAX_ITEM_N)) == 0
    assert chk(_good(capi, N=capi.BATCH_MAX_ITEM_N + 1)) == CAP and chk(_good(capi, n_members=capi.BATCH_MAX_ITEM_N + 1)) == CAP
    # reserved words
    it = _good(capi)
    it.reserved0 = 1
    assert chk(it) == INV
    for k in range(4):
        it = _good(capi)
        it.reserved[k] = 1 << (15 * k)
        assert chk(it) == INV, k
    # precedence, as the bath has it: reserved words, pointers and values before the capacity
    it = _good(capi, N=capi.BATCH_MAX_ITEM_N + 1)
    it.reserved[0] = 1
    assert chk(it) == INV
    assert chk(_good(capi, N=capi.BATCH_MAX_ITEM_N + 1, kT=-1.0)) == INV


# ---- the generator ----------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                  "d16cfe09 94fdcceb 5001e420 24126ea1"))


def test_the_mirrors_counters_against_the_known_answers_of_philox():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for counter, key, want in KNOWN_ANSWERS:
        assert want in text
        # block() puts the words where the contract says: key = (seed low, seed high), counter = (draws low, draws high, j,
        # purpose); the known counters' fourth words are reached with the velocity purposes' c = word - 0xC0000000 mod 2^32
        seed, draws = key[0] | (key[1] << 32), counter[0] | (counter[1] << 32)
        c = (counter[3] - mirror.PURPOSE_VELOCITY) % 2 ** 32
        got = mirror.block(seed, draws, np.array([counter[2]]), (mirror.PURPOSE_VELOCITY + c) % 2 ** 32)[0]
        assert " ".join("%08x" % int(w) for w in got) == want, (counter, key)
    # a normal is one block: u1 from w0,w1 as an argument of log, u2 from w2,w3
    seed, draws, j = 0x299f31d0a4093822, 7, np.array([0, 1, 512, 65535])
    n = mirror.normals(seed, draws, j, mirror.PURPOSE_VELOCITY)
    p = mirror.normals(seed, draws, j, mirror.PURPOSE_POSITION)
    for row, jj in enumerate(j):
        for c in range(3):
            for got, purpose in ((n, 0xC0000000 + c), (p, 0xC0000008 + c)):
                w = draw_mirror.philox(np.array([7, 0, jj, purpose], dtype=np.uint64), np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
                want = np.sqrt(-2.0 * np.log(draw_mirror.log_arg(w[0], w[1]))) * draw_mirror.cospi(2.0 * draw_mirror.unit(w[2], w[3]))
                assert got[row, c] == want, (jj, c, purpose)
    # apart from cavmd_draw's purposes (all below 48) and from the bath's two
    import bath_mirror
    assert draw_mirror.PURPOSE_GAMMA_TRY + 2 * draw_mirror.GAMMA_TRIES == 48 < bath_mirror.PURPOSE + 1 < mirror.PURPOSE_VELOCITY
    assert mirror.PURPOSE_VELOCITY + 2 < mirror.PURPOSE_POSITION and mirror.VELOCITY_REL == draw_mirror.NORMAL_REL + draw_mirror.EPS


# ---- the photon's expressions against the driver's ---------------------------------------------------------------------------------
def _driver_photon(dipmom, couplstr, omegac, kT, finite_q, normal, box):
    """examples/05_advanced_run.py:464-494 transcribed; np.random.normal(loc, scale, size=3) is loc + scale * n, with n handed in"""
    if finite_q:                                                              # :464
        newpos = -dipmom * couplstr / omegac**2                               # :466
        newpos[-1] = 0.0                                                      # :467
        if couplstr != 0.0:                                                   # :469
            sigma = np.sqrt(kT / omegac**2)                                   # :470
            newpos = newpos + sigma * normal                                  # :471
    else:
        newpos = np.array([0.0, 0.0, 0.0])                                    # :477
        if couplstr != 0.0:                                                   # :479
            sigma = np.sqrt(kT / omegac**2)                                   # :480
            newpos = newpos + sigma * normal                                  # :481

    def wrap_position(x, L):                                                  # :487
        image_flags = np.floor((x + L/2) / L)                                 # :489
        wrapped_position = x - image_flags * L                                # :491
        return wrapped_position, image_flags.astype(int)                      # :492
    return wrap_position(newpos, np.array(box))                               # :494


def test_the_mirrors_photon_expressions_equal_the_drivers_bit_for_bit(capi):
    rng = np.random.default_rng(17)
    omegac = 2000.0 / 219474.63
    nonzero_images = zero_spread = 0
    for trial in range(1000):
        g = 0.0 if trial % 5 == 0 else float(10.0 ** rng.uniform(-4, -2))
        finite_q = trial % 2 == 0
        box = rng.uniform(8.0, 50.0, 3) if trial % 3 else rng.uniform(0.5, 2.0, 3)      # small boxes force images
        dipole = rng.normal(0.0, 30.0, 3)
        kT = float(rng.uniform(1e-4, 2e-3))
        K = capi.make_params(omegac, g, 1.0).K
        assert K == omegac**2                                                 # phmass = 1: the driver's denominator, bit for bit
        item = dict(N=9, kT=kT, seed=trial, L=box, K=K, g=g, result=dict(dipole=dipole), **cases.flags(place_photon=True, finite_q=finite_q))
        got = mirror.place(item, 8, draws=3)
        n = mirror.normals(trial, 3, [8], mirror.PURPOSE_POSITION)[0]
        want_pos, want_image = _driver_photon(dipole.copy(), g, omegac, kT, finite_q, n, box)
        assert got["pos"].tobytes() == want_pos.tobytes() and got["image"].tolist() == want_image.tolist(), trial
        assert (got["pos"] >= -box / 2).all() and (got["pos"] < box / 2).all()
        nonzero_images += bool(got["image"].any())
        zero_spread += g == 0.0
        if g == 0.0 and not finite_q:
            assert not got["pos"].any() and not got["image"].any() and not got["bound"].any()
    assert nonzero_images > 300 and zero_spread == 200, (nonzero_images, zero_spread)


# ---- the GPU test's inputs through the mirror alone ------------------------------------------------------------------------------
def test_the_mirror_counts_what_the_contract_counts():
    systems = cases.ragged()
    want = {"null": lambda n: (n, 0), "subset": lambda n: (n // 3, 0), "planted": lambda n: (n - cases.PLANTED, cases.PLANTED),
            "empty": lambda n: (0, 0), "beyond": lambda n: (100, cases.BEYOND)}
    for s, variant in zip(systems, cases.VARIANTS):
        before = s["vel"].copy()
        state = mirror.new_state()
        run = mirror.thermalize(s, state)
        if s["N"] == 0:
            assert run is None and repr(state) == repr(mirror.new_state())    # untouched, its state included
            continue
        assert state["draws"] == 1 and state["photon"] == -1 and not state["momentum"].any()
        if variant in want:
            assert (state["thermalised"], state["skipped"]) == want[variant](s["N"]), (variant, s["N"])
        else:                                                                 # subset_planted: the four bad masses are in the list
            assert state["skipped"] == cases.PLANTED and state["thermalised"] == len(s["members"]) - cases.PLANTED
        untouched = np.setdiff1d(np.arange(s["N"]), run["written"])
        assert s["vel"][untouched].tobytes() == before[untouched].tobytes() and s["vel"][:, 3].tobytes() == before[:, 3].tobytes()
        assert np.isfinite(s["vel"][run["written"]]).all() and not run["bound"][untouched].any()
    # the momentum goes out of the thermalised rows, and of them alone
    s = cases.ragged()[7]
    s["zero_momentum"] = True
    state = mirror.new_state()
    run = mirror.thermalize(s, state)
    w = run["written"]
    left = (s["vel"][w, 3][:, None] * s["vel"][w, :3]).sum(axis=0)
    assert state["momentum"].all() and (np.abs(left) <= 8.0 * mirror.EPS * np.abs(run["addends"]).sum(axis=0)).all()


def test_the_mirror_alone_is_inside_the_bands_of_the_gpu_test():
    m = cases.stat_masses()
    vel = np.zeros((cases.STAT_B, cases.STAT_N, 4))
    vel[..., 3] = m
    for k in range(cases.STAT_B):
        item = dict(N=cases.STAT_N, vel=vel[k], members=None, kT=cases.KT, seed=mirror.item_key(cases.STAT_SEED, k), result=None,
                    **cases.flags())
        mirror.thermalize(item, mirror.new_state())
    print()
    for name, (deviation, bound) in cases.bands(cases.standardised(vel, cases.KT)).items():
        print(f"{name}: {deviation:.3e} (bound {bound:.3e})")
        assert deviation <= bound, name


def test_no_photon_case_of_the_gpu_test_is_ambiguous(capi):
    """the cap is zero excluded cases: every placement the GPU test makes stays farther than 1e-9 from a change of image"""
    assert mirror.WRAP_MARGIN == 1e-9
    placed = 0
    for k, (name, cfg, vel) in enumerate(cases.photon_configs()):
        for finite_q in (False, True):
            item = cases.photon_item(cfg, vel, mirror.item_key(cases.SEED, k), cases.host_dipole(cfg), place_photon=True, finite_q=finite_q)
            p = mirror.photon_of(item)
            assert (p >= 0) == cases.PHOTON_SYSTEMS[k][3] and (p < 0 or p == item["N"] - 1)
            if p < 0:
                continue
            got = mirror.place(item, p, draws=0)
            assert not got["ambiguous"], (name, finite_q, got["x"])
            placed += 1
            if finite_q and item["g"] != 0.0:
                assert got["image"][:2].any(), (name, got["image"])            # the displaced start leaves the box
    assert placed == 6
