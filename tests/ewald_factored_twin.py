"""The NVE run of tests/test_gpu_ewald_reciprocal.py on the host: tests/device_start_twin.py's integrator of the 12 charged dimers
and the photon (cavity force, bonds and Lennard-Jones, Ewald, velocity Verlet, each its own numpy mirror) with the Ewald forces
taken from tests/coulomb_factored_mirror.py, the factored method, and -- for a run beside the GPU test's -- started from that
test's own state: the configuration's positions and water_systems.thermal's velocities, no thermalizer.
tests/test_ewald_reciprocal_abi.py holds its drift to second order without a GPU."""
import numpy as np

import coulomb_factored_mirror as factored
import coulomb_mirror
import device_start_twin as twin
import molecular_mirror
from verlet_mirror import mirror_accelerations, mirror_step_one, mirror_step_two
from water_systems import thermal as _thermal


class Dimers(twin.Dimers):
    """reciprocal: "factored" or "direct", which mirror gives the Ewald forces"""

    def __init__(self, reciprocal="factored"):
        super().__init__()
        self.reciprocal = reciprocal

    def forces(self, s):
        """[cavity, molecular, Coulomb] force arrays of the state s and (molecular, coulomb, cavity_potential)"""
        cfg = self.cfg
        cav = twin.cavity(cfg, s["pos"], s["image"])
        f = np.zeros((s["N"], 4))
        f[:, :3] = cav["force"][:, :3]
        m = molecular_mirror.forces(s["pos"][:, :3], cfg["typeid"], cfg["box"], self.tab, self.triples, self.S)
        args = (s["pos"][:, :3], cfg["charge"], cfg["box"], self.kappa, self.r_cut, self.k_cut, self.bonds)
        c = factored.values(*args) if self.reciprocal == "factored" else coulomb_mirror.forces(*args)[0]
        e = cav["energies"]
        return [f, m, c], (float(m[:, 3].sum()), float(c[:, 3].sum()), float((e[0] + e[1]) + e[2]))

    def run_thermal(self, dt, steps):
        """`steps` steps from the configuration's positions and thermal velocities -> (steps + 1, 4): kinetic_total, molecular,
        coulomb and cavity_potential at the start and after every step"""
        cfg = self.cfg
        n = len(cfg["charge"])
        v0, mass = _thermal(cfg)
        assert (mass == self.mass).all()
        pos = np.zeros((n, 4))
        pos[:, :3] = cfg["position"]
        s = {"N": n, "box": cfg["box"], "pos": pos, "vel": np.concatenate([v0, mass[:, None]], axis=1),
             "image": np.array(cfg["image"], dtype=np.int32), "net": None, "langevin": -1, "steps": 0, "out_of_box": 0,
             "reservoir": np.float64(0.0)}

        def row_of(U):
            return (float(0.5 * (mass * (s["vel"][:, :3] ** 2).sum(axis=1)).sum()),) + U

        row = self.verlet_input_make(dt)
        s["forces"], U = self.forces(s)
        mirror_accelerations(s)
        rows = [row_of(U)]
        for _ in range(steps):
            mirror_step_one(s, row)
            s["forces"], U = self.forces(s)
            mirror_step_two(s, row)
            rows.append(row_of(U))
        assert s["out_of_box"] == 0 and s["steps"] == steps
        return np.array(rows)
