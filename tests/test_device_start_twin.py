"""A batch started on the device and taken through its first steps, rehearsed on the host (no GPU): tests/device_start_twin.py
composes the contract's numpy mirrors in the documented order of a start, on the very inputs tests/device_start_cases.py
gives tests/test_gpu_device_start.py.  Four things are pinned before a kernel is asked for them:
  1. the fifth system of the finite-q test carries the photon over both signs of the image and beyond one box; and the
     rounding bounds derived in device_start_cases hold for the mirrors, with the liveness factor at q = 0;
  2. the two lattices of the documented start are what the GPU test says they are;
  3. the three means of the first ledger row over 256 systems are inside their analytic six-sigma bands for the mirror alone
     (if they were not, the band or the formula would be wrong, not the seed);
  4. the twin's drift of system_total over 200 steps at dt and 400 at dt / 2 has a ratio in [3.5, 4.5]: the time steps the GPU
     test uses; and the ledger with its Coulomb term left out does not."""
import numpy as np
import pytest

import device_start_cases as cases
import device_start_twin as twin
import thermalize_cases
import thermalize_mirror as mirror
from gpu_support import same as _same


# ---- 1. the displaced equilibrium ----------------------------------------------------------------------------------------------------
def test_the_fifth_system_carries_the_photon_over_both_signs_and_two_boxes(capi):
    configs = cases.placed_configs()
    assert [name for name, _, _ in configs] == [row[0] for row in cases.PLACED_SYSTEMS]
    assert [len(cfg["typeid"]) for _, cfg, _ in configs] == [41, 42, 64, 514, 97]
    assert cases.IMAGES_SYSTEM[2] > max(row[2] for row in thermalize_cases.PHOTON_SYSTEMS)
    images = []
    for (name, cfg, _), (_, _, g, has_photon) in zip(configs, cases.PLACED_SYSTEMS):
        if has_photon and g != 0.0:
            x, i = cases.equilibrium(cfg)
            print(f"{name}: x {x}, image {i}")
            images.append(i)
    assert cases.images_cover_both_signs_and_two_boxes(images)
    assert cases.images_cover_both_signs_and_two_boxes(images[-1:])               # the fifth system alone does


def _placed_on_the_host(cfg, vel, key, finite_q):
    """{cavity force, thermalize at kT = 0, cavity force} -> (first evaluation, item, second evaluation)"""
    first = twin.cavity(cfg, cfg["position"], np.asarray(cfg["image"]))
    item = thermalize_cases.photon_item(cfg, vel, key, first["dipole"], place_photon=True, finite_q=finite_q)
    item["kT"] = 0.0
    mirror.thermalize(item, mirror.new_state())
    return first, item, twin.cavity(cfg, item["pos"], item["image"])


def test_the_bounds_of_the_finite_q_test_hold_for_the_mirrors(capi):
    worst = dict(photon=0.0, molecular=0.0, energy=0.0)
    live = dict(photon=np.inf, molecular=np.inf)
    for k, ((name, cfg, vel), (_, _, g, has_photon)) in enumerate(zip(cases.placed_configs(), cases.PLACED_SYSTEMS)):
        key = mirror.item_key(cases.PLACED_SEED, k)
        first, item, after = _placed_on_the_host(cfg, vel, key, True)
        assert not item["vel"][:-1 if has_photon else None, :3].any(), name       # kT = 0: every thermalised velocity is +-0
        if not has_photon:
            assert _same(item["pos"][:, :3], cfg["position"]) and not after["force"].any(), name
            continue
        assert _same(after["dipole"], first["dipole"]), name                      # the photon is not part of d
        K = cases.spring_constant(cfg["params"])
        q, d, F, E = after["q"], after["dipole"], after["force"], after["energies"]
        assert F[-1, 2] == 0.0 and q[2] == 0.0, name
        if g == 0.0:
            assert not F.any() and not E.any() and not q.any() and not item["image"][-1].any(), name
            continue
        bound_p = cases.photon_force_bound(K, g, q, d)
        bound_m = cases.molecular_force_bound(g, cfg["charge"][:-1], q)
        assert (np.abs(F[-1, :2]) <= bound_p).all(), (name, F[-1], bound_p)
        assert (np.abs(F[:-1, :2]) <= bound_m).all() and not F[:-1, 2:].any(), name
        assert abs((E[0] + E[1]) + E[2]) <= cases.energy_bound(E[2]), (name, E)
        worst["photon"] = max(worst["photon"], float((np.abs(F[-1, :2]) / bound_p).max()))
        worst["molecular"] = max(worst["molecular"], float((np.abs(F[:-1, :2]) / bound_m).max()))
        worst["energy"] = max(worst["energy"], abs((E[0] + E[1]) + E[2]) / cases.energy_bound(E[2]))
        # liveness: the same system placed at q = 0 is far from the force's zero
        _, item0, at0 = _placed_on_the_host(cfg, vel, key, False)
        assert not item0["pos"][-1, :3].any() and not item0["image"][-1].any(), name
        live["photon"] = min(live["photon"], float((np.abs(at0["force"][-1, :2]) / bound_p).min()))
        live["molecular"] = min(live["molecular"], float((np.abs(at0["force"][:-1, :2]) / bound_m).min()))
    print(f"\nworst |F| / bound on the host: photon {worst['photon']:.3f}, molecules {worst['molecular']:.3f}, "
          f"|E_h + E_c + E_d| / bound {worst['energy']:.3f}; at q = 0 the least |F| / bound: photon {live['photon']:.3e}, "
          f"molecules {live['molecular']:.3e}")
    assert min(live.values()) >= cases.LIVENESS


# ---- 2. the documented start ---------------------------------------------------------------------------------------------------------
def test_the_lattices_of_the_documented_start(capi):
    cfgs, bonds, bond_typeid = cases.start_lattices()
    assert [len(c["charge"]) for c in cfgs] == [55, 17] and [len(b) for b in bonds] == [27, 8]
    assert all(not c["image"][:-1].any() for c in cfgs)
    # the displaced equilibrium lies outside either box, by more than the thermal spread sqrt(kT / K) can bring back: the
    # thermalizer has to write image flags that are not 0, and the integrator has to continue from them
    from water_systems import KT
    for c in cfgs:
        x, i = cases.equilibrium(c)
        spread = np.sqrt(KT / cases.spring_constant(c["params"]))
        print(f"N = {len(c['charge'])}: equilibrium {x}, image {i}, spread {spread:.3f}")
        assert (np.abs(x) - 0.5 * np.asarray(c["box"]) > 3.0 * spread).any() and i.any()


# ---- 3. the first ledger row -----------------------------------------------------------------------------------------------------------
def test_the_mirror_alone_is_inside_the_bands_of_the_first_ledger_row(capi):
    configs = cases.ledger_configs()
    assert len(configs) == cases.LEDGER_B == 256 and all(len(v) == 41 for _, v in configs)
    rows = [twin.first_row(cfg, vel, mirror.item_key(cases.LEDGER_SEED, k), cases.LEDGER_KT) for k, (cfg, vel) in enumerate(configs)]
    expected = cases.ledger_expectations(np.array([vel[:-1, 3] for _, vel in configs]))
    n = cases.LEDGER_N
    assert expected["kinetic_group"][0] > 1.5 * (n - 1) * cases.LEDGER_KT          # unequal masses leave more than n - 1 hold
    print()
    for name, (mean, band) in expected.items():
        got = float(np.mean([r[name] for r in rows]))
        print(f"{name}: mean over {len(rows)} systems {got:.6e}, expected {mean:.6e}, |difference| {abs(got - mean):.3e} (band {band:.3e})")
        assert abs(got - mean) <= band, name
    print(f"kinetic_group for n - 1 degrees of freedom would be {1.5 * (n - 1) * cases.LEDGER_KT:.6e}")


# ---- 4. the conserved column -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dimer_runs(capi):
    d = twin.Dimers()
    assert len(d.bonds) == 12 and len(d.cfg["charge"]) == 25
    return {dt: d.run(dt, steps) for dt, steps in ((cases.DRIFT_DT, cases.DRIFT_STEPS), (0.5 * cases.DRIFT_DT, 2 * cases.DRIFT_STEPS))}


def test_the_twins_system_total_is_conserved_to_second_order(dimer_runs):
    drift = {dt: twin.drift(twin.system_total(rows)) for dt, rows in dimer_runs.items()}
    ratio = drift[cases.DRIFT_DT] / drift[0.5 * cases.DRIFT_DT]
    print(f"\ntwin: drift of system_total over {cases.DRIFT_STEPS} steps at dt = {cases.DRIFT_DT}: {drift[cases.DRIFT_DT]:.4e}; "
          f"at dt / 2: {drift[0.5 * cases.DRIFT_DT]:.4e}; ratio {ratio:.4f}")
    assert 3.5 <= ratio <= 4.5, (drift, ratio)
    # both runs start from the same state: the start does not depend on dt
    assert dimer_runs[cases.DRIFT_DT][0].tobytes() == dimer_runs[0.5 * cases.DRIFT_DT][0].tobytes()


def test_a_ledger_without_its_coulomb_term_is_not_conserved(dimer_runs):
    drift = {dt: twin.drift(twin.system_total(rows, coulomb=False)) for dt, rows in dimer_runs.items()}
    ratio = drift[cases.DRIFT_DT] / drift[0.5 * cases.DRIFT_DT]
    print(f"\ntwin without the Coulomb term: drifts {drift}, ratio {ratio:.4f}")
    assert not 3.0 <= ratio <= 5.0, (drift, ratio)
