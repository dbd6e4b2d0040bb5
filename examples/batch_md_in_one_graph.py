"""A complete MD step of B replicas captured into ONE graph: velocity-Verlet step one, the cavity force, step two (with the
Langevin bath on the cavity particle), the recorder and the Bussi thermostat -- five kernels of this library per step for all
replicas, plus the device-side draws of the variates.  Every per-step input is read from device memory, so each replay
advances the trajectory with fresh variates; the energy drift is read from the recorder's rows afterwards.

    python examples/batch_md_in_one_graph.py [B] [steps]

(The only force here is the cavity force: bonds, Lennard-Jones and electrostatics would be further force arrays of the
integrator's items.)"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cavitymd  # noqa: E402
from cavitymd import synthetic  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    assert torch.cuda.is_available(), "this example needs a GPU; the package has no CPU fallback"
    kT, dt = 3.167e-4, 5.0                                                 # 100 K in hartree; atomic units of time
    rng = np.random.default_rng(0)
    sysdefs, velocities = [], []
    for k in range(B):
        cfg = synthetic.config1(seed=k + 1)                                # N = 501, the reference's production size
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
        v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(kT / mass)[:, None]
        velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
    photon = int(np.flatnonzero(cfg["typeid"] == 2)[0])
    molecules = [np.flatnonzero(cfg["typeid"] != 2)] * B
    forces = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    integrator = cavitymd.VerletBatch(forces, velocities, langevin_index=photon)
    recorder = cavitymd.BatchRecorder(forces, velocities, capacity=max(steps, 1))
    thermostat = cavitymd.BussiReservoirBatch(kT=kT, tau=1000.0)           # the molecular bath; the photon has its own
    thermostat.attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)

    def step():
        integrator.draw_inputs(dt, gamma=1e-3, kT=kT)                      # three uniforms per system, drawn on the device
        integrator.step_one()                                              # one kernel: kick, drift, wrap
        forces.compute()                                                   # one kernel: the cavity force of all B systems
        integrator.step_two()                                              # one kernel: bath, a = F / m, kick
        recorder.record()                                                  # one kernel: one row per system into the series
        thermostat.draw_inputs(0, dt)
        thermostat.step_async()                                            # one kernel: the thermostat step of all B systems

    forces.compute()
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
    print(f"B={B}: {int(state['steps'][0])} MD steps per system from one captured graph, "
          f"{int(state['out_of_box'].sum())} coordinates left outside a box")
    # the conserved quantity: H plus what the two baths took (the thermostat's reservoir and the Langevin method's)
    H = series["kinetic_energy"] + series["energy"].sum(axis=2)            # (B, steps)
    baths = thermostat.total_reservoir_energy + state["langevin_reservoir"]
    scale = np.abs(H).max(axis=1)
    print(f"energy of system 0: first row {H[0, 0]:.6e}, last row {H[0, -1]:.6e}")
    print(f"baths of system 0: Bussi reservoir {thermostat.total_reservoir_energy[0]:.3e}, Langevin reservoir "
          f"{state['langevin_reservoir'][0]:.3e}")
    drift = (H[:, -1] + baths) - H[:, 0]
    print(f"drift of H + reservoirs over {steps} steps, relative to max |H|: worst system {np.abs(drift / scale).max():.3e}, "
          f"mean {np.abs(drift / scale).mean():.3e}")


if __name__ == "__main__":
    main()
