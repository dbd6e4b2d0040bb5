"""The batch run tests/test_gpu_checkpoint.py stops and resumes: B = 4 systems (diatomic lattices of N = 17, 55 and 433, each
with the photon, and one empty system) under the whole captured step, built by one function so that "the same constructors"
is one call, and observed by one function so that every comparison covers the same things.  Importing this module touches no
GPU."""
import numpy as np
import torch

import cavitymd
from cavitymd import synthetic

KT = 3.167e-4
HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=8.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=8.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=8.0)}
SERIES = ("recorder", "ledger", "fields", "trajectory")


def _empty_like(cfg):
    return dict(cfg, position=np.zeros((0, 3)), typeid=np.zeros(0, dtype=np.int32), charge=np.zeros(0),
                image=np.zeros((0, 3), dtype=np.int32))


class Run:
    """with_bath False: {draw (adaptive, reading the recorder), step one, cavity, molecular, Coulomb, step two with the cavity
    particle's Langevin row, recorder, ledger, field recorder, trajectory, Bussi batch}; with_bath True: a LangevinBathBatch on
    the molecules in place of step two, and no Bussi batch.  Everything is seeded: two Runs start from the same bits."""

    def __init__(self, with_bath: bool = False, draw_seed: int = 2024, n_systems: int = 4, recorder_capacity: int = 8, n_k: int = 5):
        rng = np.random.default_rng(7)
        lattices = [synthetic.diatomic_lattice(n, 8.0, seed=n) for n in (2, 3, 6)]          # N = 17, 55, 433
        cfgs = (lattices + [_empty_like(lattices[0])])[:n_systems]
        self.cfgs, self.with_bath = cfgs, with_bath
        self.sysdefs, self.velocities, bonds, bond_typeid, photons, molecules = [], [], [], [], [], []
        for cfg in cfgs:
            pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                                   cfg["box"], device="cuda")
            self.sysdefs.append(cavitymd.SystemDefinition(pd))
            n = pd.getN()
            mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
            self.velocities.append(torch.from_numpy(np.concatenate([np.zeros((n, 3)), mass[:, None]], axis=1)).cuda())
            b, t = synthetic.diatomic_bonds(cfg) if n else (np.zeros((0, 2), dtype=np.uint32), np.zeros(0, dtype=np.uint32))
            bonds.append(b)
            bond_typeid.append(t)
            photons.append(int(np.flatnonzero(cfg["typeid"] == 2)[0]) if n else None)
            molecules.append(np.flatnonzero(cfg["typeid"] != 2))
        B = len(cfgs)
        self.cavity = cavitymd.CavityForceBatch(self.sysdefs, lattices[0]["params"])
        self.molecular = cavitymd.MolecularForceBatch(self.sysdefs, bonds, bond_typeid, harmonic=HARMONIC, lj=LJ)
        self.coulomb = cavitymd.CoulombForceBatch(self.sysdefs, bonds, r_cut=6.0, accuracy=0.1)   # loose: K in the hundreds
        extra = [[m, c] for m, c in zip(self.molecular.forces, self.coulomb.forces)]
        self.integrator = cavitymd.VerletBatch(self.cavity, self.velocities, extra_forces=extra,
                                               langevin_index=None if with_bath else photons, net_forces=True)
        self.thermalizer = cavitymd.BatchThermalizer(self.velocities, KT, seed=11, cavity=self.cavity)
        self.recorder = cavitymd.BatchRecorder(self.cavity, self.velocities, net_forces=self.integrator.net_forces,
                                               capacity=recorder_capacity)
        self.thermostat = self.bath = None
        if with_bath:
            gammas = [((v[:, 3] > 1.5).to(torch.float64) * 1e-3).contiguous() if v.shape[0] else None for v in self.velocities]
            self.bath = cavitymd.LangevinBathBatch(self.integrator, gammas, KT, seed=77)
        else:
            self.thermostat = cavitymd.BussiReservoirBatch(kT=KT, tau=1000.0)
            self.thermostat.attach(self.velocities, translational_dof=[max(3.0 * len(m) - 3.0, 0.0) for m in molecules],
                                   members=molecules)
        self.draw = cavitymd.StepDraw(draw_seed, self.integrator, self.thermostat, self.recorder, dt=2.0, gamma=1e-3, kT=KT,
                                      tolerance=1e-3, dt_min=0.5, dt_max=4.0)
        reservoirs = [("bath", self.bath)] if with_bath else [("bussi", self.thermostat), ("langevin", self.integrator)]
        self.ledger = cavitymd.BatchEnergyLedger(self.cavity, self.velocities, terms=[self.molecular, self.coulomb],
                                                 reservoirs=reservoirs, clock=self.draw, capacity=8)
        positions = [s.getParticleData().getPositions() for s in self.sysdefs]
        self.fields = cavitymd.BatchFieldRecorder(positions, num_wavevectors=n_k, capacity=4, period=2, max_references=3,
                                                  reference_interval=3)
        self.trajectory = cavitymd.BatchTrajectoryRecorder(self.cavity, self.velocities, capacity=4, time_interval=1.0,
                                                           clock=self.draw, dtype="f64")
        self.objects = {"integrator": self.integrator, "thermalizer": self.thermalizer, "draw": self.draw,
                        "recorder": self.recorder, "ledger": self.ledger, "fields": self.fields, "trajectory": self.trajectory}
        self.objects.update({"bath": self.bath} if with_bath else {"thermostat": self.thermostat})
        self.checkpoint = cavitymd.BatchCheckpoint(self.sysdefs, self.velocities, self.objects)
        self.n_systems = B
        self.graph = None
        # the start of every run: seeded momenta, the forces of the lattice, a = F / m
        self.thermalizer.thermalize()
        self.cavity.compute()
        self.molecular.compute()
        self.coulomb.compute()
        self.integrator.prime()
        torch.cuda.synchronize()

    def step(self) -> None:
        self.draw.fill()
        self.integrator.step_one()
        self.cavity.compute()
        self.molecular.compute()
        self.coulomb.compute()
        (self.bath if self.with_bath else self.integrator).step_two()
        self.recorder.record()
        self.ledger.record()
        self.fields.record()
        self.trajectory.record()
        if self.thermostat is not None:
            self.thermostat.step_async()

    def capture(self) -> None:
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.step()

    def replay(self, times: int) -> None:
        for _ in range(times):
            self.graph.replay()

    def _held(self, name: str):
        """rows written, and per system every row its ring still holds (the full read of a series)"""
        rec = getattr(self, name)
        torch.cuda.synchronize()
        rows = rec.rows()
        held = []
        for k in range(self.n_systems):
            n = int(rows[k])
            first = max(n - rec.capacity, 0)
            a = rec.recorder.read(0, k, 1, first, n - first)[0] if n else np.zeros(0, dtype=np.uint8)
            if name == "recorder" and n:
                a = a.copy()
                a["eval_sequence"] = 0                                             # the one excluded column: diagnostic
            held.append(a.tobytes())
        return rows.tobytes(), held

    def observe(self) -> dict:
        """Everything the tests compare, as bytes: the arrays of every system (the empty one included), accel and the input
        rows, every object's state, and of the four series the row counters and every row still held; the field recorder's
        stored fields of every item."""
        torch.cuda.synchronize()
        out = {}
        for k, (s, v) in enumerate(zip(self.sysdefs, self.velocities)):
            pd = s.getParticleData()
            out[f"position.{k}"] = pd.getPositions().cpu().numpy().tobytes()
            out[f"image.{k}"] = pd.getImages().cpu().numpy().tobytes()
            out[f"velocity.{k}"] = v.cpu().numpy().tobytes()
            out[f"accel.{k}"] = self.integrator.accel[k].cpu().numpy().tobytes()
            out[f"net_force.{k}"] = self.integrator.net_forces[k].cpu().numpy().tobytes()
        out["integrator.inputs"] = self.integrator.inputs.cpu().numpy().tobytes()
        for name in ("integrator", "thermalizer", "draw") + (("bath",) if self.with_bath else ()):
            out[f"state.{name}"] = getattr(self, name).state().tobytes()
        if self.thermostat is not None:
            out["state.thermostat"] = bytes(self.thermostat._need().read(raise_refused=False)[0])
            out["thermostat.inputs"] = self.thermostat.inputs.cpu().numpy().tobytes()
        for name in SERIES:
            out[f"rows.{name}"], held = self._held(name)
            for k, a in enumerate(held):
                out[f"read.{name}.{k}"] = a
        for k in range(self.n_systems):
            now, refs, ref_rows = self.fields.fields(k)
            out[f"fields.{k}"] = now.tobytes() + refs.tobytes() + ref_rows.tobytes() + bytes([len(ref_rows)])
        return out

    def close(self) -> None:
        self.graph = None
        for name in ("trajectory", "fields", "ledger", "draw", "bath", "thermostat", "recorder", "thermalizer", "integrator",
                     "coulomb", "molecular", "cavity"):
            obj = getattr(self, name)
            if obj is not None:
                obj.close()
        self.objects = self.checkpoint = None
        self.sysdefs = self.velocities = None
