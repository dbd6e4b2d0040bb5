"""examples/trajectory/batch_trajectory_in_one_graph.py run to an END TIME: B replicas of the reference's model under an adaptive
dt drawn on the device, one captured graph per step, replayed until every replica's own clock has reached t_end -- what the
reference's driver does with --runtime (ElapsedTimeTracker, src/cavitymd/analysis.py:1230-1259), --energy-output-period-ps
(EnergyTracker, analysis.py:692-701), --fkt-output-period-ps / --fkt-ref-interval (analysis.py:366-378) and
--gsd-output-period-ps.  Replicas under an adaptive dt reach t_end after different
numbers of steps; one that has reached it rests (its rows carry `skip`: nothing of it moves, it writes no further energy row
or frame) while the others finish, so all replicas cover the same time span and the host reads the device once per chunk of
replays, not B clocks per step.

    python examples/run_clock/batch_run_to_end_time.py [B] [t_end in atomic units of time] [output period]"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cavitymd  # noqa: E402
from cavitymd import synthetic  # noqa: E402

# examples/05_advanced_run.py:568-582 of the reference
HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}      # 'O-O', 'N-N'
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=15.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=15.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=15.0)}                       # pairs with 'L': not listed


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    t_end = float(sys.argv[2]) if len(sys.argv) > 2 else 2000.0
    period = float(sys.argv[3]) if len(sys.argv) > 3 else t_end / 20.0
    assert torch.cuda.is_available(), "this example needs a GPU; the package has no CPU fallback"
    kT, dt, dt_min, dt_max = 3.167e-4, 5.0, 0.5, 10.0                      # 100 K in hartree; atomic units of time
    rng = np.random.default_rng(0)
    sysdefs, velocities, bonds, bond_typeid = [], [], [], []
    for k in range(B):
        cfg = synthetic.diatomic_lattice(6, 8.0, seed=k + 1)               # 216 molecules + the photon: N = 433, box 48 bohr
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
        v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(kT / mass)[:, None]
        velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
        b, t = synthetic.diatomic_bonds(cfg)
        bonds.append(b)
        bond_typeid.append(t)
    photon = int(np.flatnonzero(cfg["typeid"] == 2)[0])
    molecules = [np.flatnonzero(cfg["typeid"] != 2)] * B
    cavity = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    molecular = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, harmonic=HARMONIC, lj=LJ)
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=15.0, accuracy=1e-5)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(molecular.forces, coulomb.forces)],
                                      langevin_index=photon, net_forces=True)
    recorder = cavitymd.BatchRecorder(cavity, velocities, net_forces=integrator.net_forces, capacity=16)   # the dt rule reads its last row
    thermostat = cavitymd.BussiReservoirBatch(kT=kT, tau=1000.0)
    thermostat.attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
    draw = cavitymd.StepDraw(2024, integrator, thermostat, recorder, dt=dt, gamma=1e-3, kT=kT, tolerance=1e-3, dt_min=dt_min,
                             dt_max=dt_max)
    rows_expected = int(t_end / period) + 2
    ledger = cavitymd.BatchEnergyLedger(cavity, velocities, terms=[("molecular", molecular), ("coulomb", coulomb)],
                                        reservoirs=[("bussi", thermostat), ("langevin", integrator)], clock=draw,
                                        capacity=rows_expected)
    trajectory = cavitymd.BatchTrajectoryRecorder(cavity, velocities, capacity=rows_expected, time_interval=period, clock=draw)
    positions = [sd.getParticleData().getPositions() for sd in sysdefs]
    fields = cavitymd.BatchFieldRecorder(positions, kmag=1.0, capacity=rows_expected, reference_interval=0)
    # the run clock: all of it BEFORE the capture
    draw.set_end_time(t_end)
    ledger.set_time_rule(period)
    fields.set_time_rule(draw, period, reference_time_interval=4.0 * period)      # F(k,t) rows and references on a time grid

    def step():
        draw.fill()                                                        # one kernel: the variates, this step's dt -- or rest
        integrator.step_one()
        cavity.compute()
        molecular.compute()
        coulomb.compute()
        integrator.step_two()
        recorder.record()                                                  # S = sum |F| / m of this step, for the next dt
        ledger.record()                                                    # one kernel: a row where a system's clock says so
        fields.record()                                                    # one kernel: rho(k), F(k,t), references, by the clock
        trajectory.record()                                                # one kernel: a frame where a system's clock says so
        thermostat.step_async()

    cavity.compute()
    molecular.compute()
    coulomb.compute()
    integrator.prime()                                                     # a = F / m once, as HOOMD does at the start of a run
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    limit = int(t_end / dt_min) + 2                                        # no replica needs more steps than this
    replays = cavitymd.run_until_finished(graph.replay, draw, check_every=64, max_replays=limit + 64)
    clock = draw.state()
    assert clock["finished"].all() and (clock["elapsed"] >= t_end).all(), "a replica did not reach the end time"
    print(f"B={B}: t_end {t_end}, {replays} replays until every replica had finished")
    for k in range(B):
        print(f"  replica {k}: {int(clock['draws'][k])} steps, final clock {clock['elapsed'][k]:.3f}, last dt {clock['dt'][k]:.3f}")
    energy_rows, frames = ledger.rows(), trajectory.rows()
    series = ledger.read(count=int(energy_rows.min()))
    gaps = np.diff(series["time"], axis=1)
    print(f"energy rows per replica {int(energy_rows.min())} .. {int(energy_rows.max())}, frames {int(frames.min())} .. "
          f"{int(frames.max())}; smallest gap between energy rows {gaps.min() if gaps.size else float('nan'):.2f} "
          f"(output period {period})")
    fkt = fields.read(count=int(fields.rows().min()))
    lags = fields.lag_times(fkt)                                           # (B, rows, references): row time - reference time
    print(f"F(k,t) rows per replica {int(fields.rows().min())} .. {int(fields.rows().max())}, references "
          f"{int(fkt['n_references'][:, -1].min())} .. {int(fkt['n_references'][:, -1].max())}; longest lag {np.nanmax(lags):.1f}; "
          f"F / F(0) of replica 0 against its first reference: {np.round(fkt['F'][0, :4, 0] / fkt['rho2'][0, 0], 3).tolist()} ...")
    # A healthy value does not grow with the end time: the reservoirs hold exactly what the baths took (the Langevin tally is
    # taken with the velocity from after the kick), so this is the integrator's own error plus a zero-mean offset of the
    # photon's bath of the order of sqrt(gamma dt) kT.  A reservoir tallied before the kick would add 3 gamma kT t / m,
    # 9.5e-7 hartree per unit of time (tests/thermostatted_twin.py).
    drift = np.abs(series["universe_total"][:, -1] - series["universe_total"][:, 0])
    print(f"|change of the conserved energy| over the run: at most {drift.max():.3e} hartree")
    again = draw.state()
    graph.replay()                                                         # a replay past the end changes nothing
    assert draw.state().tobytes() == again.tobytes()


if __name__ == "__main__":
    main()
