"""The Langevin bath of include/cavmd.h as a thermostat, on the host (no GPU): tests/langevin_twin.py drives the contract's
numpy mirror with a free particle and compares with the three closed forms derived there.  Three things are pinned:
  (a) the contract's expressions reproduce the closed forms: over 24 seeds each ratio averages 1 within 3 standard errors;
  (b) the mistakes tests/test_gpu_langevin_batch.py exists for -- variates in [0, 1), the same variates every step, the tally
      taken with the post-kick velocity -- each move a ratio out of the acceptance band used on the GPU;
  (c) that band is 6 standard deviations of THIS twin across the seeds (same members, steps and parameters as the GPU run),
      and the literals next to the GPU assertions are these figures."""
import numpy as np
import pytest

import langevin_twin as twin

SEEDS = tuple(range(24))
NAMES = ("m <v^2> / kT after step two", "m <v^2> (1 - x) / kT after step one", "reservoir growth / closed form")


@pytest.fixture(scope="module")
def runs() -> np.ndarray:
    return np.array([twin.run(seed) for seed in SEEDS])                      # (24, 3)


@pytest.fixture(scope="module")
def measured_band(runs) -> np.ndarray:
    std = runs.std(axis=0, ddof=1)
    band = 6.0 * std
    print()
    for name, mean, sd, b, worst in zip(NAMES, runs.mean(axis=0), std, band, np.abs(runs - 1.0).max(axis=0)):
        print(f"{name}: mean {mean:.5f}, std across {len(SEEDS)} seeds {sd:.5f}, band 6 std = {b:.5f}, "
              f"worst seed {worst:.5f} from 1")
    return band


def test_the_closed_forms_are_what_the_rehearsal_uses():
    assert twin.x_of() == 0.25
    full, half, rate = twin.closed_forms()
    assert full == 3.167e-4 / 2.0 and half == 3.167e-4 / 1.5
    assert rate == pytest.approx(3 * 0.25 * 3.167e-4 * 4.0 / 1.5, rel=1e-15)
    # the twin's coefficient is the library's (host arithmetic), so the twin and the kernel are driven alike
    from cavitymd import _capi
    row = _capi.verlet_input_make(twin.DT, twin.GAMMA, twin.KT)
    assert row.langevin_coeff == pytest.approx(np.sqrt(6.0 * twin.GAMMA * twin.KT / twin.DT), rel=4e-16)


def test_the_contract_is_a_thermostat(runs, measured_band):
    assert runs.shape == (len(SEEDS), 3) and len(SEEDS) >= 24
    mean = runs.mean(axis=0)
    stderr = runs.std(axis=0, ddof=1) / np.sqrt(len(SEEDS))
    for name, m, e in zip(NAMES, mean, stderr):
        print(f"{name}: |mean - 1| = {abs(m - 1.0):.2e}, 3 standard errors = {3 * e:.2e}")
    assert np.all(np.abs(mean - 1.0) <= 3.0 * stderr), (mean, stderr)


def test_the_band_next_to_the_gpu_assertions_is_six_sigma_of_this_twin(measured_band):
    # the literals are these figures rounded to four decimals; they come from this host run, never from a GPU run
    assert len(twin.BAND) == 3
    assert np.all(np.abs(np.asarray(twin.BAND) - measured_band) <= 0.5e-4), (twin.BAND, measured_band.tolist())
    assert np.all(np.asarray(twin.BAND) < 0.03)                                    # a band this tight is what (b) relies on


@pytest.mark.parametrize("mistake", twin.MISTAKES)
def test_a_planted_mistake_leaves_the_band(mistake):
    for seed in SEEDS[:4]:
        r = twin.run(seed, mistake=mistake)
        print(f"{mistake}, seed {seed}: ratios {r.round(4).tolist()}")
        assert np.any(np.abs(r - 1.0) > np.asarray(twin.BAND)), (mistake, seed, r)
