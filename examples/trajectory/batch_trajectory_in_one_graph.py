"""examples/batch_coulomb_md_in_one_graph.py with an ADAPTIVE dt drawn on the device and a time-triggered trajectory: B replicas of
the reference's model under all three forces of its driver, one captured graph per step, and a frame of every replica's
positions, images and velocities whenever its own clock has advanced by the output period -- what the driver's hoomd.write.GSD
does with --gsd-output-period-ps (examples/05_advanced_run.py:1231-1246 of the reference), the initial frame first.  Under an
adaptive dt the host cannot know on which replay a frame is due without reading the device clock every step; here the recorder's
kernel reads that clock itself, so the loop below is nothing but ``graph.replay()``.

    python examples/trajectory/batch_trajectory_in_one_graph.py [B] [steps] [output period in atomic units of time]"""
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
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    period = float(sys.argv[3]) if len(sys.argv) > 3 else 250.0
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
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=15.0, accuracy=1e-5)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(molecular.forces, coulomb.forces)],
                                      langevin_index=photon, net_forces=True)
    recorder = cavitymd.BatchRecorder(cavity, velocities, net_forces=integrator.net_forces, capacity=max(steps, 1))
    thermostat = cavitymd.BussiReservoirBatch(kT=kT, tau=1000.0)
    thermostat.attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
    # dt = sqrt(tolerance / S) from the recorder's last row, clamped; the clock of every system is kept on the device
    draw = cavitymd.StepDraw(2024, integrator, thermostat, recorder, dt=dt, gamma=1e-3, kT=kT, tolerance=1e-3, dt_min=0.5,
                             dt_max=10.0)
    frames_expected = int(steps * 10.0 / period) + 2                       # no more than this many at dt_max
    trajectory = cavitymd.BatchTrajectoryRecorder(cavity, velocities, capacity=frames_expected, time_interval=period, clock=draw)

    def step():
        draw.fill()                                                        # one kernel: the variates and this step's dt
        integrator.step_one()
        cavity.compute()
        molecular.compute()
        coulomb.compute()
        integrator.step_two()
        recorder.record()                                                  # S = sum |F| / m of this step, for the next dt
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
    for _ in range(steps):
        graph.replay()
    clock = draw.state()
    rows = trajectory.rows()
    frames = trajectory.read(count=int(rows.min()))                        # (B, n): header columns, position, velocity, image
    print(f"B={B}: {steps} replays, elapsed time {clock['elapsed'].min():.1f} .. {clock['elapsed'].max():.1f}, last dt "
          f"{clock['dt'].min():.3f} .. {clock['dt'].max():.3f}; frames per system {int(rows.min())} .. {int(rows.max())}")
    t = frames["time"][0]
    print(f"system 0: frames written by calls {frames['call'][0][:6].tolist()} ... at times {np.round(t[:6], 2).tolist()} ...; "
          f"smallest gap {np.diff(t).min() if len(t) > 1 else float('nan'):.2f} (output period {period})")
    r = trajectory.unwrapped(frames)                                       # (B, n, N, 3): position + image * box
    moved = np.linalg.norm(r[:, -1] - r[:, 0], axis=-1)                    # (B, N)
    print(f"displacement between the first and the last common frame: molecular particles at most {moved[:, molecules[0]].max():.3f} "
          f"bohr, the cavity particle {moved[:, photon].max():.3f}")
    chunks = trajectory.gsd_chunks(0, -1)
    print("last frame of system 0 under GSD's chunk names: " + ", ".join(f"{k} {v.dtype}{list(v.shape)}" for k, v in chunks.items()))
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "batch_trajectory.npz")
    trajectory.save_npz(out)
    print(f"everything still held saved to {out}")


if __name__ == "__main__":
    main()
