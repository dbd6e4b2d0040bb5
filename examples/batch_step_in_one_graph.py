"""Force batch + recorder + thermostat batch of B replicas captured into ONE graph: three kernels per step for all replicas.
The thermostat stays stochastic on replay because its variates are read from device memory, and the recorder appends one row
per replica and replay to a time series in device memory, read once after the replays.

    python examples/batch_step_in_one_graph.py [B] [steps]

(The integrator's position / velocity update between the two is the caller's and is left out: this shows the plumbing.)"""
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
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    assert torch.cuda.is_available(), "this example needs a GPU; the package has no CPU fallback"
    rng = np.random.default_rng(0)
    sysdefs, velocities = [], []
    for k in range(B):
        cfg = synthetic.config1(seed=k + 1)                                # N = 501, the reference's production size
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        v = np.ones((pd.getN(), 4))
        v[:, :3] = rng.normal(0.0, 1e-3, (pd.getN(), 3))
        velocities.append(torch.from_numpy(v).cuda())
    forces = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    recorder = cavitymd.BatchRecorder(forces, velocities, net_forces=forces.forces, capacity=max(steps, 1))
    thermostat = cavitymd.BussiReservoirBatch(kT=1e-6, tau=0.5)
    thermostat.attach(velocities, translational_dof=3.0 * 501 - 3.0)

    dt = 0.005
    forces.compute(0)                                                      # warm-up outside the capture
    thermostat.draw_inputs(0, dt)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        forces.compute(0)                                                  # one kernel: the cavity force of all B systems
        recorder.record()                                                  # one kernel: one row per system into the series
        thermostat.draw_inputs(0, dt)                                      # fresh variates, drawn on the device
        thermostat.step_async()                                            # one kernel: the thermostat step of all B systems
    for _ in range(steps):
        graph.replay()
    state = thermostat.device_state()                                      # after a capture: behind a device synchronisation
    print(f"B={B}: {state[0].steps} thermostat steps per system from one captured graph; "
          f"last alpha of system 0 = {state[0].last_alpha:.6f}, reservoir = {thermostat.total_reservoir_energy[0]:.3e}")
    series = recorder.read()                                               # (B, steps) rows, one copy after all the replays
    print(f"recorded rows per system: {recorder.rows().tolist()}")
    for label, row in (("first", series[0, 0]), ("last", series[0, -1])):
        print(f"system 0, {label} row (call {row['call']}): energies {row['energy'].tolist()}, "
              f"cavity T = {row['cavity_temperature']:.6e} K, kinetic energy = {row['kinetic_energy']:.6e}")


if __name__ == "__main__":
    main()
