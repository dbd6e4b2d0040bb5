"""The numpy twin of M cells in one shared cavity (tests/shared_cavity_twin.py) proves itself on a machine WITHOUT a GPU, before
tests/test_gpu_shared_cavity.py holds the captured step to it: velocity Verlet conserves the cavity-summed energy to second order,
the planted mistake "every cell feels its own dipole only" does not, one cell alone is conserved as well, and the members of a
cavity exchange energy (no member is conserved on its own)."""
import numpy as np
import pytest

import shared_cavity_twin as twin


@pytest.fixture(scope="module")
def measured():
    return {seed: twin.measure(seed) for seed in twin.SEEDS}


def test_the_literals_are_this_twins_figures(measured):
    for seed, got in measured.items():
        print(f"\nseed {seed}: excursion {got[0]:.4e} at dt = 10, {got[1]:.4e} at dt = 20, {got[2]:.4e} with the planted mistake")
        assert np.allclose(got, twin.MEASURED[seed], rtol=2e-3, atol=0.0), (seed, got)
    assert np.allclose(twin.measure(0, cells=1), twin.MEASURED_ALONE, rtol=2e-3, atol=0.0)


def test_the_energy_is_conserved_to_second_order(measured):
    for seed, (fine, coarse, _) in measured.items():
        assert 3.5 <= coarse / fine <= 4.5, (seed, coarse / fine)
    fine, coarse = twin.measure(0, cells=1)
    assert 3.5 <= coarse / fine <= 4.5, coarse / fine


def test_the_planted_mistake_is_at_least_100_times_worse_on_every_seed(measured):
    for seed, (fine, _, wrong) in measured.items():
        assert wrong >= 100.0 * fine, (seed, wrong / fine)


def test_the_forces_are_the_gradient_of_the_energy():
    cells = twin.start(0)
    F, U = twin.forces(cells)
    rng = np.random.default_rng(7)
    for _ in range(12):
        c = int(rng.integers(len(cells)))
        i, k = int(rng.integers(len(cells[c]["charge"]))), int(rng.integers(3))
        h = 1e-5
        x0 = cells[c]["position"][i, k]
        cells[c]["position"][i, k] = x0 + h
        up = twin.forces(cells)[1]
        cells[c]["position"][i, k] = x0 - h
        down = twin.forces(cells)[1]
        cells[c]["position"][i, k] = x0
        assert abs(-(up - down) / (2 * h) - F[c][i, k]) <= 1e-6 * max(abs(F[c][i, k]), 1e-4), (c, i, k)
    wrong = twin.forces(cells, mistake="own_dipole")[0]
    assert any(not np.allclose(wrong[c], F[c], rtol=1e-9, atol=0.0) for c in range(len(cells)))
