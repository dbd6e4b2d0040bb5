"""The thermostatted MD step of a batch on the host, and the ledger's conserved column under it: 12 charged dimers and the photon
(tests/device_start_twin.Dimers, N = 25) stepped with a bath on, a ledger row taken after every step.  What
tests/test_thermostatted_twin.py checks without a GPU, and where the band of tests/test_gpu_conserved_energy.py comes from.

Nothing is restated here.  The forces and the start are device_start_twin's, step one is verlet_mirror.mirror_step_one, step two
is verlet_mirror.mirror_step_two (the photon's row bath, rows from cavmd_verlet_input_make) or bath_mirror.mirror_bath_step_two
(a bath on the molecules, the contract's Philox variates), the Bussi step is cavmd_bussi_step on the host; only the order of the
calls and the ledger's sums (plain numpy) are this file's.  The order is that of the step of tests/checkpoint_runs.Run: the row
is taken after step two and BEFORE this step's Bussi launch, so it holds the Bussi reservoir as the previous step left it.

Two configurations, 200 steps of dt = 10 each:
  "row_bussi"   the photon under the integrator's row bath (gamma = 1e-2, m = 1, kT), the molecules under the Bussi step at
                8 kT with tau = 100.  Everything starts at kT: the molecules are HEATED, so that system_total rises by many bands
                while the photon stays at its own bath's temperature.
  "group"       a LangevinBathBatch on the 24 molecular particles with gamma_j = GROUP_RATE * m_j at kT, no Bussi step, no row
                bath; started at 16 kT, so that system_total falls by many bands.
In both the reservoirs are what close the balance (LIVENESS).

The tally velocity is a parameter (TALLY_VELOCITY is what the contract says).  The state does not depend on it, only the Langevin
reservoir does, so every run carries BOTH reservoirs: the selected one in "langevin", the other in "langevin_other", from a second
call of the same mirror on a copy of the step's state.

Why the tally is taken AFTER the kick.  The bath force bd of a step acts through two half-kicks with the same stored
acceleration: v' = h + a dt / 2 in this step's step two and h' = v' + a dt / 2 in the next step's step one.  Its work on the
kinetic energy is bd . (h + v') dt / 4 + bd . (v' + h') dt / 4 = bd . v' dt exactly, since h + h' = 2 v'.  So -tally dt with v'
is the energy the bath took, step by step and not only on average, and universe_total is conserved to the integrator's own
error.  What is left in a row is that the row is taken between the two half-kicks: it already holds the whole tally but only the
first half of the work, a zero-mean offset of about bd . v' dt / 2 per coupled particle that does not accumulate.  With the
velocity h from BEFORE the kick the reservoir misses bd . (v' - h) dt, the noise's heating, and universe_total drifts by
pre_kick_drift() -- what the contract said until this was found.

How the constants below were measured (host, numpy; never a GPU run), from the repository's root:
    PYTHONPATH=.:cav-hoomd_amd python tests/thermostatted_twin.py
prints, per configuration, the worst excursion of universe_total of every seed under every planted mistake, with the tally after
and before the kick, the last row minus the first under the pre-kick tally, and the excursion of system_total."""
import numpy as np

import bath_mirror
import device_start_twin as base
import thermalize_mirror
from verlet_mirror import mirror_accelerations, mirror_step_one, mirror_step_two
from water_systems import KT

TALLY_VELOCITY = "after"                   # the contract; "before" is the planted mistake
CONFIGURATIONS = ("row_bussi", "group")
DT, STEPS = {"row_bussi": 10.0, "group": 10.0}, 200
SEEDS = tuple(range(8))
START_KT = {"row_bussi": KT, "group": 16.0 * KT}
ROW_GAMMA = 1e-2                           # the photon's row bath; m = 1, x = gamma dt / 2 m = 0.05
BUSSI_TAU, BUSSI_KT = 100.0, 8.0 * KT      # the molecules are HEATED: the photon stays at its bath's temperature
GROUP_RATE = 7e-4                          # gamma_j = GROUP_RATE * m_j: x = GROUP_RATE * dt / 2 = 3.5e-3 for every molecule
GROUP_SEED = 77
# The planted mistakes of each configuration.  Without a Bussi step there is no Bussi reservoir to misread or to drop.  With the
# row bath the reservoir that is dropped is the Bussi one: the photon's own holds a few kT of ONE particle, which is the size of
# the row's zero-mean offset and so of the band; what its tally must get right shows in "pre_kick_tally", which accumulates.
MISTAKES = {"row_bussi": ("reservoir_with_the_wrong_sign", "bussi_reservoir_left_out", "bussi_read_after_this_steps_rescale",
                          "pre_kick_tally"),
            "group": ("reservoir_with_the_wrong_sign", "langevin_reservoir_left_out", "pre_kick_tally")}

# Measured by the command above, seeds 0..7 (rows 1..200: 199 steps between the first row and the last).
# MEASURED[configuration] = (largest excursion of universe_total with the tally after the kick over the 8 seeds,
#                            smallest excursion with the tally before the kick over the 8 seeds,
#                            smallest excursion of system_total over the 8 seeds)
# tests/test_thermostatted_twin.py fails if these literals are not that run's figures.  The same run, pre-kick tally, last row
# minus first: row_bussi mean +1.9818e-02, standard deviation 6.5e-04 over the seeds, closed form 1.9902e-02; group mean
# +3.1577e-02, standard deviation 6.0e-04, closed form 3.1875e-02.
MEASURED = {"row_bussi": (6.1797e-04, 1.9000e-02, 1.0488e-01), "group": (2.3403e-03, 3.0662e-02, 1.0082e-01)}
# The band of the conserved column: 3 times the largest excursion the twin shows.  Measured on the twin, never on a device.
BAND = {name: 3.0 * m[0] for name, m in MEASURED.items()}
SEPARATION, LIVENESS = 3.0, 10.0           # the pre-kick excursion is >= 3 bands on every seed; system_total moves by >= 10 bands


def pre_kick_drift(configuration, masses=None, steps=STEPS - 1, kT=KT) -> float:
    """What universe_total gains in `steps` steps under the pre-kick tally, at the bath's temperature.  The two tallies differ by
    bd . (v' - v) dt = bd . (F + bd) dt^2 / (2 m) per step, whose mean is <bd^2> dt^2 / (2 m) = 3 gamma kT dt / m +
    3 gamma^2 <v^2> dt^2 / (2 m) with <v^2> = kT / (m (1 - x)) per component (tests/langevin_twin.py), x = gamma dt / (2 m):
    3 gamma kT dt / (m (1 - x)) per step and coupled particle, 3 gamma kT t / m for small x whatever dt."""
    dt = DT[configuration]
    rate = ROW_GAMMA / 1.0 if configuration == "row_bussi" else GROUP_RATE * np.ones_like(masses)   # gamma_j / m_j
    return float(np.sum(3.0 * rate * kT * dt * steps / (1.0 - 0.5 * rate * dt)))


_DIMERS = []


def dimers():
    if not _DIMERS:
        _DIMERS.append(base.Dimers())
    return _DIMERS[0]


def run(seed, configuration, tally_velocity=TALLY_VELOCITY, steps=STEPS) -> dict:
    """One start at START_KT and `steps` thermostatted steps -> the columns of the ledger's row after every step, each (steps,):
    system_total, bussi (as the previous step left it), bussi_after (after this step's rescale: a planted mistake reads it),
    langevin (the tally velocity selected), langevin_other (the other one)."""
    assert configuration in CONFIGURATIONS and tally_velocity in ("after", "before")
    other = "before" if tally_velocity == "after" else "after"
    dt = DT[configuration]
    d = dimers()
    cfg, mass = d.cfg, d.mass
    n = len(cfg["charge"])
    photon = int(np.flatnonzero(np.asarray(cfg["typeid"]) == cfg["L_typeid"])[0])
    molecules = np.delete(np.arange(n), photon)
    rng = np.random.default_rng(seed)
    vel = np.concatenate([np.zeros((n, 3)), mass[:, None]], axis=1)
    item = base.start(cfg, vel, thermalize_mirror.item_key(1000 + seed, 0), START_KT[configuration])
    with_row = configuration == "row_bussi"
    s = {"N": n, "box": cfg["box"], "pos": item["pos"], "vel": item["vel"], "image": item["image"], "net": None,
         "langevin": photon if with_row else -1, "steps": 0, "out_of_box": 0, "reservoir": np.float64(0.0)}
    bath = None
    if not with_row:
        gamma = GROUP_RATE * mass
        gamma[photon] = 0.0
        bath = {"gamma": gamma, "kT": KT, "seed": bath_mirror.item_key(GROUP_SEED + seed, 0), "draws": 0, "coupled": 0,
                "reservoir": np.float64(0.0)}
    from cavitymd import _capi
    bussi = _capi.BussiReservoirState()
    dof = 3.0 * len(molecules) - 3.0
    other_reservoir = np.float64(0.0)
    s["forces"], U = d.forces(s)
    mirror_accelerations(s)
    out = {name: np.zeros(steps) for name in ("system_total", "bussi", "bussi_after", "langevin", "langevin_other")}
    for step in range(steps):
        if with_row:
            row = d.verlet_input_make(dt, ROW_GAMMA, KT, 2.0 * rng.random(3) - 1.0)
        else:
            row = d.verlet_input_make(dt)
        mirror_step_one(s, row)
        s["forces"], U = d.forces(s)
        # the other tally, from the same state: a copy of what step two writes, the same mirror, the other switch
        twin_s = dict(s, vel=s["vel"].copy(), reservoir=other_reservoir)
        if with_row:
            mirror_step_two(twin_s, row, tally_velocity=other)
            mirror_step_two(s, row, tally_velocity=tally_velocity)
            other_reservoir = twin_s["reservoir"]
            langevin = s["reservoir"]
        else:
            twin_bath = dict(bath, reservoir=other_reservoir)
            bath_mirror.mirror_bath_step_two(twin_s, row, twin_bath, tally_velocity=other)
            bath_mirror.mirror_bath_step_two(s, row, bath, tally_velocity=tally_velocity)
            other_reservoir = twin_bath["reservoir"]
            langevin = bath["reservoir"]
            assert bath["coupled"] == len(molecules)
        assert np.array_equal(twin_s["vel"], s["vel"])                      # the state does not depend on the tally
        # the ledger's row: after step two, before this step's Bussi launch
        ke = 0.5 * (mass * (s["vel"][:, :3] ** 2).sum(axis=1))
        out["system_total"][step] = float(ke.sum()) + ((U[0] + U[1]) + U[2])
        out["bussi"][step] = bussi.reservoir_translational
        out["langevin"][step] = langevin
        out["langevin_other"][step] = other_reservoir
        if with_row:
            K = float(ke[molecules].sum())
            alpha, _ = _capi.bussi_step(bussi, K, dof, 0.0, 0.0, dt, BUSSI_KT, BUSSI_TAU,
                                        (rng.standard_normal(), rng.standard_gamma(0.5 * (dof - 1.0)), 0.0, 0.0))
            s["vel"][molecules, :3] = s["vel"][molecules, :3] * alpha
        out["bussi_after"][step] = bussi.reservoir_translational
    assert s["out_of_box"] == 0 and s["steps"] == steps
    return out


def universe_total(series, mistake=None) -> np.ndarray:
    """system_total + reservoir_total of every row, as include/cavmd.h defines the column; or with one planted mistake"""
    assert mistake is None or any(mistake in m for m in MISTAKES.values())
    bussi = series["bussi_after" if mistake == "bussi_read_after_this_steps_rescale" else "bussi"]
    langevin = series["langevin_other" if mistake == "pre_kick_tally" else "langevin"]
    if mistake == "langevin_reservoir_left_out":
        langevin = np.zeros_like(langevin)
    elif mistake == "bussi_reservoir_left_out":
        bussi = np.zeros_like(bussi)
    reservoir_total = bussi + langevin
    if mistake == "reservoir_with_the_wrong_sign":
        reservoir_total = -reservoir_total
    return series["system_total"] + reservoir_total


def excursion(column) -> float:
    """max |column - column[0]|"""
    return float(np.abs(column - column[0]).max())


if __name__ == "__main__":
    for name in CONFIGURATIONS:
        runs = [run(seed, name, "after") for seed in SEEDS]
        post = [excursion(universe_total(r)) for r in runs]
        pre = [excursion(universe_total(r, "pre_kick_tally")) for r in runs]
        gain = [float(np.diff(universe_total(r, "pre_kick_tally")[[0, -1]])[0]) for r in runs]
        live = [excursion(r["system_total"]) for r in runs]
        for mistake in MISTAKES[name][:-1]:
            print(f"{name}: {mistake} {' '.join(f'{excursion(universe_total(r, mistake)):.3e}' for r in runs)}")
        print(f"{name}: tally after the kick  {' '.join(f'{x:.3e}' for x in post)}  (largest {max(post):.4e})")
        print(f"{name}: tally before the kick {' '.join(f'{x:.3e}' for x in pre)}  (smallest {min(pre):.4e})")
        print(f"{name}: pre-kick last - first {' '.join(f'{x:+.3e}' for x in gain)}  (mean {np.mean(gain):+.4e}, "
              f"std {np.std(gain, ddof=1):.2e}, closed form {pre_kick_drift(name, dimers().mass[:-1]):.4e})")
        print(f"{name}: system_total          {' '.join(f'{x:.3e}' for x in live)}  (smallest {min(live):.4e})")
