"""The Langevin bath of include/cavmd.h as a thermostat, on the host (no GPU): tests/langevin_twin.py drives the contract's
numpy mirror with a free particle and compares with the three closed forms derived there.  Three things are pinned:
  (a) the contract's expressions reproduce the closed forms: over 24 seeds each figure averages its expected value (1, 1 and
      0) within 3 standard errors, and the reservoir's spread is the derived one;
  (b) the mistakes tests/test_gpu_langevin_batch.py exists for -- variates in [0, 1), the same variates every step, the tally
      taken with the pre-kick velocity -- each move a figure out of the acceptance band used on the GPU;
  (c) that band is 6 standard deviations of THIS twin across the seeds (same members, steps and parameters as the GPU run),
      and the literals next to the GPU assertions are these figures."""
import numpy as np
import pytest

import langevin_twin as twin

SEEDS = tuple(range(24))
NAMES = ("m <v^2> / kT after step two", "m <v^2> (1 - x) / kT after step one", "reservoir gain / pre-kick growth")
EXPECTED = np.asarray(twin.EXPECTED)


@pytest.fixture(scope="module")
def runs() -> np.ndarray:
    return np.array([twin.run(seed) for seed in SEEDS])                      # (24, 3)


@pytest.fixture(scope="module")
def measured_band(runs) -> np.ndarray:
    std = runs.std(axis=0, ddof=1)
    band = 6.0 * std
    print()
    for name, mean, sd, b, worst in zip(NAMES, runs.mean(axis=0), std, band, np.abs(runs - EXPECTED).max(axis=0)):
        print(f"{name}: mean {mean:.6f}, std across {len(SEEDS)} seeds {sd:.6f}, band 6 std = {b:.6f}, "
              f"worst seed {worst:.6f} from the expected")
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
        print(f"{name}: mean = {m:.6f}, 3 standard errors = {3 * e:.2e}")
    assert tuple(EXPECTED) == (1.0, 1.0, 0.0)
    assert np.all(np.abs(mean - EXPECTED) <= 3.0 * stderr), (mean, stderr)


def test_the_reservoirs_spread_is_the_derived_one(runs):
    # (4) of the twin: one particle's gain has the standard deviation member_sd() whatever the number of steps; a seed's figure
    # is the mean of MEMBERS of them per step and unit.  24 seeds estimate a standard deviation to 1 / sqrt(2 * 23) = 15 %:
    # three of those either way.  The pre-kick tally's figure, 1, lies hundreds of these away.
    derived = twin.member_sd() / np.sqrt(twin.MEMBERS) / twin.COUNTED / twin.closed_forms()[2]
    measured = runs[:, 2].std(ddof=1)
    print(f"reservoir figure: std across the seeds {measured:.3e}, derived {derived:.3e}")
    assert 0.55 * derived <= measured <= 1.45 * derived
    assert twin.BAND[2] < 50.0 * derived < 0.01


def test_the_band_next_to_the_gpu_assertions_is_six_sigma_of_this_twin(measured_band):
    # the literals are these figures rounded (the third to six decimals); they come from this host run, never from a GPU run
    assert len(twin.BAND) == 3
    assert np.all(np.abs(np.asarray(twin.BAND) - measured_band) <= np.asarray(twin.BAND_DIGITS)), (twin.BAND, measured_band.tolist())
    assert np.all(np.asarray(twin.BAND) < 0.03)                                    # a band this tight is what (b) relies on


@pytest.mark.parametrize("mistake", twin.MISTAKES)
def test_a_planted_mistake_leaves_the_band(mistake):
    for seed in SEEDS[:4]:
        r = twin.run(seed, mistake=mistake)
        print(f"{mistake}, seed {seed}: figures {r.round(4).tolist()}")
        assert np.any(np.abs(r - EXPECTED) > np.asarray(twin.BAND)), (mistake, seed, r)
        if mistake == "tally_with_pre_kick_velocity":                        # the old contract's closed form, to its old band
            assert np.all(np.abs(r[:2] - 1.0) <= np.asarray(twin.BAND[:2])) and abs(r[2] - 1.0) <= 0.0080, r
