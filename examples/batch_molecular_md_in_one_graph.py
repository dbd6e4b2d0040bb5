"""A complete MD step of B replicas of the reference's model, without electrostatics, captured into ONE graph: velocity-Verlet
step one, the cavity force, the harmonic bonds and Lennard-Jones pairs, step two (with the Langevin bath on the cavity
particle), the recorder, the energy ledger and the Bussi thermostat -- seven kernels of this library per step for all replicas,
plus the device-side draws of the variates.  The ledger writes every term of the conserved energy per step, so the conserved
quantity is a series.  It is examples/batch_md_in_one_graph.py with the molecular force launch between the cavity force and
step two, on lattice systems (no Lennard-Jones overlaps at the start) with the driver's O / N constants.

    python examples/batch_molecular_md_in_one_graph.py [B] [steps]

(Electrostatics -- PPPM, a real-space Ewald term -- would be a further force array of the integrator's items.)"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
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
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    assert torch.cuda.is_available(), "this example needs a GPU; the package has no CPU fallback"
    kT, dt = 3.167e-4, 5.0                                                 # 100 K in hartree; atomic units of time
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
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[f] for f in molecular.forces], langevin_index=photon)
    recorder = cavitymd.BatchRecorder(cavity, velocities, capacity=max(steps, 1))
    thermostat = cavitymd.BussiReservoirBatch(kT=kT, tau=1000.0)           # the molecular bath; the photon has its own
    thermostat.attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
    ledger = cavitymd.BatchEnergyLedger(cavity, velocities, terms=[("molecular", molecular)],
                                        reservoirs=[("bussi", thermostat), ("langevin", integrator)], capacity=max(steps, 1))

    def step():
        integrator.draw_inputs(dt, gamma=1e-3, kT=kT)                      # three uniforms per system, drawn on the device
        integrator.step_one()                                              # one kernel: kick, drift, wrap
        cavity.compute()                                                   # one kernel: the cavity force of all B systems
        molecular.compute()                                                # one kernel: bonds and Lennard-Jones of all B systems
        integrator.step_two()                                              # one kernel: sum of both, bath, a = F / m, kick
        recorder.record()                                                  # one kernel: one row per system into the series
        ledger.record()                                                    # one kernel: every term of the conserved energy
        thermostat.draw_inputs(0, dt)
        thermostat.step_async()                                            # one kernel: the thermostat step of all B systems

    cavity.compute()
    molecular.compute()
    integrator.prime()                                                     # a = F / m once, as HOOMD does at the start of a run
    integrator.draw_inputs(dt, gamma=1e-3, kT=kT)                          # warm-up of the draws outside the capture
    thermostat.draw_inputs(0, dt)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(steps):
        graph.replay()
    state = integrator.state()
    series = recorder.read()                                               # (B, steps) rows, one copy after all the replays
    energy = ledger.read()                                                 # (B, steps) rows of the energy ledger
    U = energy["molecular"]                                                # (B, steps)
    print(f"B={B}: {int(state['steps'][0])} MD steps per system from one captured graph, "
          f"{int(state['out_of_box'].sum())} coordinates left outside a box")
    # the conserved quantity: H plus what the two baths took (the thermostat's reservoir and the Langevin method's)
    H = series["kinetic_energy"] + series["energy"].sum(axis=2) + U        # (B, steps)
    baths = thermostat.total_reservoir_energy + state["langevin_reservoir"]
    scale = np.abs(H).max(axis=1)
    print(f"energy of system 0: first row {H[0, 0]:.6e}, last row {H[0, -1]:.6e} (bonds + Lennard-Jones {U[0, -1]:.6e})")
    print(f"baths of system 0: Bussi reservoir {thermostat.total_reservoir_energy[0]:.3e}, Langevin reservoir "
          f"{state['langevin_reservoir'][0]:.3e}")
    drift = (H[:, -1] + baths) - H[:, 0]
    print(f"drift of H + reservoirs over {steps} steps, relative to max |H|: worst system {np.abs(drift / scale).max():.3e}, "
          f"mean {np.abs(drift / scale).mean():.3e}")
    # the same quantity as a series: the ledger's universe_total of every step (its reservoirs are those the step's kernels saw)
    # What a healthy value looks like: the excursion does not grow with the length of the run.  The Langevin tally is taken with
    # the velocity from after the kick, so each reservoir holds exactly what its bath took, and what a row shows is the
    # integrator's own error plus a zero-mean offset of the photon's bath (the row is taken between the bath force's two
    # half-kicks) of the order of sqrt(gamma dt) kT, a few 1e-5 hartree here.  A reservoir tallied before the kick would add
    # 3 gamma kT t / m = 9.5e-7 hartree per unit of time: 4.8e-3 hartree over 1000 steps (tests/thermostatted_twin.py).
    universe = energy["universe_total"]
    excursion = np.abs(universe - universe[:, :1]).max(axis=1) / np.abs(energy["system_total"]).max(axis=1)
    print(f"universe_total over the whole series, worst excursion from its first row relative to max |system_total|: worst system "
          f"{excursion.max():.3e}, mean {excursion.mean():.3e}")


if __name__ == "__main__":
    main()
