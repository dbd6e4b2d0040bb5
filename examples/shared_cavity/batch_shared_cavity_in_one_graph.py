"""Collective coupling in one captured graph: M periodic cells of charged harmonic dimers, each with its own box, and ONE photon
that feels the summed dipole of all of them (``SharedCavityForceBatch``).  The step is ``step_one``, the shared cavity force (two
launches), the bonds of every cell (``MolecularForceBatch``, one launch), ``step_two`` and the energy ledger, captured once and
replayed.  The cavity term is the only force that crosses the cells' boundaries, so no cell is conserved on its own: the
conserved quantity is the ledger's ``universe_total`` SUMMED over the cavity's members (the carrier's row holds the cavity's three
energies, the other members' rows hold zero there).  The last line prints the worst excursion of that sum, and of one cell alone.

    python examples/shared_cavity/batch_shared_cavity_in_one_graph.py [M] [steps] [dt]"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cavitymd  # noqa: E402

HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158)}                      # 'O-O' of examples/05_advanced_run.py:568-582 of the reference
MASS, CHARGE, BOX, DIMERS = 29166.0, 0.3, 20.0, 4
KT = 100.0 * 3.166811563e-6                                             # 100 K in hartree
PARAMS = {"omegac": 2000.0 / 219474.63, "couplstr": 1e-3, "phmass": 1.0}
TYPES, L_TYPEID = ["O", "L"], 1


def dimer_cells(M: int, seed: int = 0):
    """M cells of DIMERS dimers (charges +-CHARGE, one image per dimer); cell 0 carries the photon as its last particle."""
    rng = np.random.default_rng(seed)
    K = PARAMS["phmass"] * PARAMS["omegac"] ** 2
    cells = []
    for c in range(M):
        n = 2 * DIMERS + (c == 0)
        centre = rng.uniform(-0.5, 0.5, (DIMERS, 3)) * (BOX - 6.0)
        axis = rng.normal(size=(DIMERS, 3))
        half = 0.5 * HARMONIC[0]["r0"] * axis / np.linalg.norm(axis, axis=1)[:, None]
        pos, charge, mass = np.zeros((n, 3)), np.zeros(n), np.full(n, MASS)
        pos[0:2 * DIMERS:2], pos[1:2 * DIMERS:2] = centre - half, centre + half
        charge[0:2 * DIMERS:2], charge[1:2 * DIMERS:2] = CHARGE, -CHARGE
        image = np.zeros((n, 3), dtype=np.int32)
        image[:2 * DIMERS] = np.repeat(rng.integers(-1, 2, (DIMERS, 3)), 2, axis=0)
        typeid = np.zeros(n, dtype=np.int32)
        vel = rng.normal(size=(n, 3)) * np.sqrt(KT / MASS)
        if c == 0:
            typeid[-1], mass[-1] = L_TYPEID, PARAMS["phmass"]
            pos[-1] = rng.normal(size=3) * np.sqrt(KT / K)
            vel[-1] = rng.normal(size=3) * np.sqrt(KT / PARAMS["phmass"])
        cells.append({"position": pos, "image": image, "typeid": typeid, "charge": charge, "mass": mass, "velocity": vel,
                      "bonds": np.stack([np.arange(0, 2 * DIMERS, 2), np.arange(1, 2 * DIMERS, 2)], axis=1),
                      "box": (BOX, BOX, BOX), "types": list(TYPES), "params": dict(PARAMS)})
    return cells


class Cells:
    """The cells of ONE cavity on the GPU, the batch objects over them and the captured step."""

    def __init__(self, cells, dt: float, capacity: int, harmonic=None):
        self.sysdefs, self.velocities = [], []
        for cell in cells:
            pd = cavitymd.ParticleData.from_arrays(cell["position"], cell["typeid"], cell["charge"], cell["image"], cell["types"],
                                                   cell["box"], device="cuda")
            self.sysdefs.append(cavitymd.SystemDefinition(pd))
            self.velocities.append(torch.from_numpy(np.concatenate([cell["velocity"], cell["mass"][:, None]], axis=1)).cuda())
        M = len(cells)
        self.cavity = cavitymd.SharedCavityForceBatch(self.sysdefs, cavity_of=[0] * M, params=cells[0]["params"])
        self.molecular = cavitymd.MolecularForceBatch(self.sysdefs, [c["bonds"] for c in cells],
                                                      [np.zeros(len(c["bonds"]), dtype=np.int64) for c in cells],
                                                      harmonic=harmonic or HARMONIC, lj={})
        self.integrator = cavitymd.VerletBatch(self.cavity, self.velocities, extra_forces=[[f] for f in self.molecular.forces])
        self.ledger = cavitymd.BatchEnergyLedger(self.cavity, self.velocities, terms=[("bonds", self.molecular)], capacity=capacity)
        self.integrator.set_inputs(dt)                                     # no bath: NVE
        self.cavity.compute()
        self.molecular.compute()
        self.integrator.prime()                                            # a = F / m once
        torch.cuda.synchronize()
        self.graph = None

    def step(self):
        self.integrator.step_one()
        self.cavity.compute()                                              # two launches: the cells' dipoles, then the fold and the forces
        self.molecular.compute()
        self.integrator.step_two()
        self.ledger.record()

    def run(self, steps: int):
        if self.graph is None:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.step()
        for _ in range(steps):
            self.graph.replay()
        torch.cuda.synchronize()

    def universe_total(self):
        """(per-member (M, rows) column, its sum over the cavity's members (rows,)): only the sum is conserved"""
        rows = self.ledger.read()["universe_total"]
        return rows, rows.sum(axis=0)

    def close(self):
        self.graph = None
        for obj in (self.ledger, self.integrator, self.molecular, self.cavity):
            obj.close()


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 800
    dt = float(sys.argv[3]) if len(sys.argv) > 3 else 10.0
    assert torch.cuda.is_available(), "this example needs a GPU; the package has no CPU fallback"
    run = Cells(dimer_cells(M), dt, capacity=steps)
    run.run(steps)
    members, total = run.universe_total()
    alone = np.abs(members - members[:, :1]).max(axis=1)
    print(f"M={M} cells in one cavity, {steps} replays of dt={dt}: cavity-summed universe_total {total[0]:+.6e}, worst excursion "
          f"{np.abs(total - total[0]).max():.3e}; of one member alone {alone.max():.3e}")
    run.close()


if __name__ == "__main__":
    main()
