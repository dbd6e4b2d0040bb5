"""The ledger's conserved column under a bath, rehearsed on the host (no GPU): tests/thermostatted_twin.py steps 12 charged dimers
and the photon through the contract's numpy mirrors with a thermostat on and takes the ledger's row where cavmd_ledger_record
takes it.  What is pinned:
  (a) the diagnosis: with the tally taken BEFORE the kick, universe_total gains the closed form 3 gamma kT dt / (m (1 - x)) per
      step and coupled particle, within the statistical margin of 8 seeds;
  (b) the contract: with the tally taken AFTER the kick the worst excursion of universe_total stays inside the band, 3 times the
      largest excursion of this twin over 8 seeds, and the literals tests/test_gpu_conserved_energy.py asserts are these figures;
  (c) the band separates: on every seed the pre-kick excursion is at least 3 bands, and every planted mistake leaves the band;
  (d) the check is alive: system_total itself moves by at least 10 bands, so the reservoirs are what close the balance."""
import numpy as np
import pytest

import thermostatted_twin as twin


@pytest.fixture(scope="module", params=twin.CONFIGURATIONS)
def runs(request):
    return request.param, [twin.run(seed, request.param) for seed in twin.SEEDS]


def test_the_parameters_are_the_rehearsed_ones():
    assert twin.TALLY_VELOCITY == "after" and len(twin.SEEDS) >= 8 and twin.STEPS == 200
    assert (twin.SEPARATION, twin.LIVENESS) == (3.0, 10.0)
    masses = twin.dimers().mass
    assert len(masses) == 25 and masses[-1] == 1.0
    for name in twin.CONFIGURATIONS:
        assert twin.BAND[name] == 3.0 * twin.MEASURED[name][0] > 0.0
    # x = gamma dt / (2 m) < 1 for every coupled particle, and the closed-form drift alone exceeds the band by the factor
    assert 0.0 < twin.ROW_GAMMA * twin.DT["row_bussi"] / 2.0 < 1.0 and 0.0 < twin.GROUP_RATE * twin.DT["group"] / 2.0 < 1.0
    assert twin.pre_kick_drift("row_bussi") >= twin.SEPARATION * twin.BAND["row_bussi"]
    assert twin.pre_kick_drift("group", masses[:-1]) >= twin.SEPARATION * twin.BAND["group"]


def test_the_pre_kick_tally_drifts_by_the_closed_form(runs):
    name, series = runs
    gain = np.array([np.diff(twin.universe_total(s, "pre_kick_tally")[[0, -1]])[0] for s in series])
    closed = twin.pre_kick_drift(name, twin.dimers().mass[:-1])
    stderr = gain.std(ddof=1) / np.sqrt(len(gain))
    print(f"\n{name}: last row - first row under the pre-kick tally: mean {gain.mean():+.4e}, standard error {stderr:.2e}, "
          f"closed form {closed:+.4e}")
    assert abs(gain.mean() - closed) <= 3.0 * stderr, (gain.tolist(), closed)
    assert np.all(np.abs(gain - closed) <= 0.15 * closed)                     # and every single seed shows it


def test_the_post_kick_tally_stays_inside_the_band_measured_here(runs):
    name, series = runs
    assert twin.TALLY_VELOCITY == "after"
    post = np.array([twin.excursion(twin.universe_total(s)) for s in series])
    pre = np.array([twin.excursion(twin.universe_total(s, "pre_kick_tally")) for s in series])
    live = np.array([twin.excursion(s["system_total"]) for s in series])
    band = twin.BAND[name]
    print(f"\n{name}: excursion of universe_total, tally after the kick: {post.tolist()}\n  before the kick: {pre.tolist()}\n"
          f"  system_total: {live.tolist()}\n  band {band:.4e}")
    # the literals are this run's figures to five digits; they come from this host run, never from a GPU run
    measured = np.array([post.max(), pre.min(), live.min()])
    assert np.all(np.abs(measured - np.asarray(twin.MEASURED[name])) <= 1e-4 * measured), (measured.tolist(), twin.MEASURED[name])
    assert np.all(post <= band)
    assert np.all(pre >= twin.SEPARATION * band), (pre.tolist(), band)        # a condition on the parameters, not a measurement
    assert np.all(live >= twin.LIVENESS * band), (live.tolist(), band)


def test_every_planted_mistake_leaves_the_band_on_every_seed(runs):
    name, series = runs
    assert "pre_kick_tally" in twin.MISTAKES[name] and "reservoir_with_the_wrong_sign" in twin.MISTAKES[name]
    assert any(m.endswith("_left_out") for m in twin.MISTAKES[name])
    assert ("bussi_read_after_this_steps_rescale" in twin.MISTAKES[name]) == (name == "row_bussi")
    for mistake in twin.MISTAKES[name]:
        worst = [twin.excursion(twin.universe_total(s, mistake)) for s in series]
        print(f"{name}, {mistake}: {worst}")
        assert min(worst) > twin.BAND[name], (name, mistake, worst)


def test_the_switch_selects_the_reservoir_and_nothing_else():
    a, b = twin.run(0, "row_bussi", "after", steps=12), twin.run(0, "row_bussi", "before", steps=12)
    assert a["langevin"].tobytes() == b["langevin_other"].tobytes() and a["langevin_other"].tobytes() == b["langevin"].tobytes()
    assert a["langevin"].tobytes() != a["langevin_other"].tobytes()
    for column in ("system_total", "bussi", "bussi_after"):
        assert a[column].tobytes() == b[column].tobytes(), column
    # the row holds the Bussi reservoir as the PREVIOUS step left it
    assert a["bussi"][0] == 0.0 and a["bussi"][1:].tobytes() == a["bussi_after"][:-1].tobytes() and np.all(a["bussi_after"] != 0.0)
