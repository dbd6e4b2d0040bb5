"""The impulse multiple-time-step scheme (Verlet-I / r-RESPA) on the host: tests/device_start_twin.py's 12 charged dimers and
the photon, started as tests/ewald_factored_twin.py starts its thermal run, with the Ewald sum in its two parts
(tests/coulomb_parts_mirror.py).  One outer step is
    kick(long, n / 2);  n x {step one; cavity, molecular, short; step two};  long;  kick(long, n / 2)
with the kick of tests/verlet_kick_mirror.py and the half-steps of tests/verlet_mirror.py: what
examples/mts/batch_mts_coulomb_in_one_graph.py captures and tests/test_gpu_mts_step.py replays.  The velocities are whole only at
the end of an outer step, so the series has one row per outer step.  tests/test_coulomb_parts_abi.py holds its drift to second
order without a GPU, for n = 1, 2 and 4, and shows that a kick of weight 1 / 2 instead of n / 2 does not pass."""
import numpy as np

import coulomb_parts_mirror as parts
import device_start_twin as twin
import molecular_mirror
from verlet_kick_mirror import mirror_kick
from verlet_mirror import mirror_accelerations, mirror_step_one, mirror_step_two
from water_systems import thermal as _thermal


class Dimers(twin.Dimers):
    """method: "direct" or "factored", the reciprocal method of the long part"""

    def __init__(self, method="direct"):
        super().__init__()
        self.method = method

    def _coulomb_args(self, s):
        return (s["pos"][:, :3], self.cfg["charge"], self.cfg["box"], self.kappa, self.r_cut, self.k_cut, self.bonds)

    def inner_forces(self, s):
        """[cavity, molecular, short] of the state s and (molecular, ewald_short, cavity_potential)"""
        cfg = self.cfg
        cav = twin.cavity(cfg, s["pos"], s["image"])
        f = np.zeros((s["N"], 4))
        f[:, :3] = cav["force"][:, :3]
        m = molecular_mirror.forces(s["pos"][:, :3], cfg["typeid"], cfg["box"], self.tab, self.triples, self.S)
        c = parts.short(*self._coulomb_args(s))[0]
        e = cav["energies"]
        return [f, m, c], (float(m[:, 3].sum()), float(c[:, 3].sum()), float((e[0] + e[1]) + e[2]))

    def long_force(self, s):
        """the long array of the state s and ewald_long"""
        c = parts.long(*self._coulomb_args(s), method=self.method)[0]
        return c, float(c[:, 3].sum())

    def run_mts(self, dt, steps, n, weight=None):
        """`steps` MD steps (a multiple of n) in outer steps of n -> (steps / n + 1, 5): kinetic_total, molecular, ewald_short,
        ewald_long and cavity_potential at the start and after every outer step.  weight: of both kicks, n / 2 unless a
        mistake is planted."""
        assert steps % n == 0
        weight = 0.5 * n if weight is None else weight
        cfg = self.cfg
        N = len(cfg["charge"])
        v0, mass = _thermal(cfg)
        pos = np.zeros((N, 4))
        pos[:, :3] = cfg["position"]
        s = {"N": N, "box": cfg["box"], "pos": pos, "vel": np.concatenate([v0, mass[:, None]], axis=1),
             "image": np.array(cfg["image"], dtype=np.int32), "net": None, "langevin": -1, "steps": 0, "out_of_box": 0,
             "reservoir": np.float64(0.0)}

        def row_of(U, long_energy):
            kinetic = float(0.5 * (mass * (s["vel"][:, :3] ** 2).sum(axis=1)).sum())
            return (kinetic, U[0], U[1], long_energy, U[2])

        row = self.verlet_input_make(dt)
        s["forces"], U = self.inner_forces(s)
        mirror_accelerations(s)
        long, long_energy = self.long_force(s)
        rows = [row_of(U, long_energy)]
        for _ in range(steps // n):
            mirror_kick(s, row, long, weight)
            for _ in range(n):
                mirror_step_one(s, row)
                s["forces"], U = self.inner_forces(s)
                mirror_step_two(s, row)
            long, long_energy = self.long_force(s)
            mirror_kick(s, row, long, weight)
            rows.append(row_of(U, long_energy))
        assert s["out_of_box"] == 0 and s["steps"] == steps
        return np.array(rows)


def system_total(rows):
    """kinetic_total + potential_total of every row, the potential summed in the ledger's order of terms
    (molecular, ewald_short, ewald_long) and then the cavity"""
    return rows[:, 0] + (((rows[:, 1] + rows[:, 2]) + rows[:, 3]) + rows[:, 4])
