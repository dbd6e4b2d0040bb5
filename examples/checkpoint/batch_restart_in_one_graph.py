"""Stop a batch run and take it up again: the Coulomb step of examples/trajectory/batch_trajectory_in_one_graph.py -- B replicas
under all three forces, an adaptive dt drawn on the device, the cavity particle's Langevin bath, the Bussi thermostat, the
recorder, the energy ledger and a time-triggered trajectory, one captured graph per step -- run for n steps, saved with
``BatchCheckpoint``, thrown away with every object and tensor, rebuilt from the same constructors, loaded and run for n more
steps.  The last line says whether the final state equals that of 2 n uninterrupted steps, bit for bit: what a job that died
on a queue-limited machine needs in order not to start from the lattice again.

    python examples/checkpoint/batch_restart_in_one_graph.py [B] [n] [checkpoint file]"""
import os
import sys
import tempfile

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
RECORDER_ROWS, LEDGER_ROWS, FRAMES, PERIOD = 64, 64, 8, 250.0                                        # the ring sizes of a long run


class Replicas:
    """Everything one process holds: the systems, the batch objects and the captured step.  Built from B and the seeds alone,
    so a new process builds the same."""

    def __init__(self, B: int, config=lambda k: synthetic.diatomic_lattice(6, 8.0, seed=k + 1)):
        kT, dt = 3.167e-4, 5.0                                             # 100 K in hartree; atomic units of time
        rng = np.random.default_rng(0)
        self.sysdefs, self.velocities, bonds, bond_typeid = [], [], [], []
        for k in range(B):
            cfg = config(k)                                                # 216 molecules + the photon: N = 433, box 48 bohr
            pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                                   cfg["box"], device="cuda")
            self.sysdefs.append(cavitymd.SystemDefinition(pd))
            mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
            v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(kT / mass)[:, None]
            self.velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
            b, t = synthetic.diatomic_bonds(cfg)
            bonds.append(b)
            bond_typeid.append(t)
        photon = int(np.flatnonzero(cfg["typeid"] == 2)[0])
        molecules = [np.flatnonzero(cfg["typeid"] != 2)] * B
        self.cavity = cavitymd.CavityForceBatch(self.sysdefs, cfg["params"])
        self.molecular = cavitymd.MolecularForceBatch(self.sysdefs, bonds, bond_typeid, harmonic=HARMONIC, lj=LJ)
        self.coulomb = cavitymd.CoulombForceBatch(self.sysdefs, bonds, r_cut=15.0, accuracy=1e-5)
        self.integrator = cavitymd.VerletBatch(self.cavity, self.velocities, langevin_index=photon, net_forces=True,
                                               extra_forces=[[m, c] for m, c in zip(self.molecular.forces, self.coulomb.forces)])
        self.recorder = cavitymd.BatchRecorder(self.cavity, self.velocities, net_forces=self.integrator.net_forces,
                                               capacity=RECORDER_ROWS)
        self.thermostat = cavitymd.BussiReservoirBatch(kT=kT, tau=1000.0)
        self.thermostat.attach(self.velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
        self.draw = cavitymd.StepDraw(2024, self.integrator, self.thermostat, self.recorder, dt=dt, gamma=1e-3, kT=kT,
                                      tolerance=1e-3, dt_min=0.5, dt_max=10.0)
        self.ledger = cavitymd.BatchEnergyLedger(self.cavity, self.velocities, terms=[self.molecular, self.coulomb],
                                                 reservoirs=[("bussi", self.thermostat), ("langevin", self.integrator)],
                                                 clock=self.draw, capacity=LEDGER_ROWS)
        self.trajectory = cavitymd.BatchTrajectoryRecorder(self.cavity, self.velocities, capacity=FRAMES, time_interval=PERIOD,
                                                           clock=self.draw, dtype="f64")
        # what a checkpoint holds: the systems' arrays and every object whose launches write state (the three force objects
        # keep nothing that a later launch reads)
        self.checkpoint = cavitymd.BatchCheckpoint(self.sysdefs, self.velocities, {
            "integrator": self.integrator, "draw": self.draw, "thermostat": self.thermostat, "recorder": self.recorder,
            "ledger": self.ledger, "trajectory": self.trajectory})
        self.cavity.compute()
        self.molecular.compute()
        self.coulomb.compute()
        self.integrator.prime()                                            # a = F / m once; a load replaces it
        torch.cuda.synchronize()
        self.graph = None

    def step(self):
        self.draw.fill()                                                   # one kernel: the variates and this step's dt
        self.integrator.step_one()
        self.cavity.compute()
        self.molecular.compute()
        self.coulomb.compute()
        self.integrator.step_two()
        self.recorder.record()
        self.ledger.record()
        self.trajectory.record()
        self.thermostat.step_async()

    def run(self, steps: int):
        if self.graph is None:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.step()
        for _ in range(steps):
            self.graph.replay()

    def final_state(self) -> dict:
        """what the two runs are compared by: everything a checkpoint would hold now, the recorder's ring as the rows it still
        holds without ``eval_sequence`` (a diagnostic column that restarts with the process)"""
        state = self.checkpoint.state()
        del state["object.recorder.snapshot"]
        rows = self.recorder.read().copy()
        rows["eval_sequence"] = 0
        state["recorder rows held"], state["recorder rows written"] = rows, self.recorder.rows()
        return {name: np.ascontiguousarray(a).tobytes() for name, a in state.items()}

    def close(self):
        self.graph = None
        for obj in (self.trajectory, self.ledger, self.draw, self.thermostat, self.recorder, self.integrator, self.coulomb,
                    self.molecular, self.cavity):
            obj.close()


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(tempfile.mkdtemp(), "batch_restart.npz")
    assert torch.cuda.is_available(), "this example needs a GPU; the package has no CPU fallback"

    whole = Replicas(B)                                                    # 2 n uninterrupted steps
    whole.run(2 * n)
    want = whole.final_state()
    elapsed = whole.draw.state()["elapsed"]
    whole.close()
    del whole

    first = Replicas(B)                                                    # n steps, then the job ends
    first.run(n)
    first.checkpoint.save(path)
    first.close()
    del first                                                              # every object and tensor is gone
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"B={B}: {n} replays saved to {path} ({os.path.getsize(path) / 2**20:.1f} MiB)")

    second = Replicas(B)                                                   # a new job: the same constructors, then the file
    second.checkpoint.load(path)
    second.run(n)                                                          # a new graph, n more steps
    got = second.final_state()
    print(f"elapsed time after {2 * n} steps: {elapsed.min():.1f} .. {elapsed.max():.1f}; "
          f"recorder rows {second.recorder.rows().tolist()[:4]} ..., frames {second.trajectory.rows().tolist()[:4]} ...")
    second.close()
    differ = sorted(name for name in want if got.get(name) != want[name])
    print(f"the restarted run equals the uninterrupted one: {not differ and got.keys() == want.keys()}"
          + (f" (differs in {differ})" if differ else ""))


if __name__ == "__main__":
    main()
