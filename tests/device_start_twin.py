"""A batch started on the device and taken through its first steps, on the host: the numpy mirrors of the contract composed in
the documented order of a start (include/cavmd.h, "the start of a batch") -- the cavity force for the dipole, the thermalizer,
every force again, a = F / m -- and then velocity-Verlet steps with a ledger row after each.  What
tests/test_device_start_twin.py checks without a GPU, so that the expectations, bands and time steps of
tests/test_gpu_device_start.py are rehearsed before a kernel is asked for them.

Nothing is restated here.  The thermalizer is tests/thermalize_mirror.py, the integrator tests/verlet_mirror.py, bonds and
Lennard-Jones tests/molecular_mirror.py, Ewald tests/coulomb_mirror.py, the cavity force oracle/numpy_mirror.py; only the
order of the calls and the ledger's sums (in plain numpy; the device's are compensated) are this file's.  The twin is not
compared with the device value for value: log and cospi differ between host and device, and Ewald carries the mirror's bound."""
import numpy as np

import coulomb_mirror
import device_start_cases as cases
import molecular_mirror
import thermalize_cases
import thermalize_mirror as mirror
from oracle import numpy_mirror as nm
from verlet_mirror import mirror_accelerations, mirror_step_one, mirror_step_two
from water_systems import HARMONIC, KT, LJ
from water_systems import thermal as _thermal


def cavity(cfg, pos, image):
    """the cavity force's evaluation of (pos (N, >= 3), image) -> the oracle's dict (force (N, 4), energies, dipole, q, Dq)"""
    pos4 = np.zeros((len(pos), 4))
    pos4[:, :3] = pos[:, :3]
    pos4[:, 3] = nm_type_tags(cfg["typeid"])
    p = cfg["params"]
    return nm.compute(pos4, cfg["charge"], image, cfg["box"], cfg["L_typeid"],
                      dict(couplstr=p["couplstr"], K=cases.spring_constant(p)), summation="fsum")


def nm_type_tags(typeid):
    t = np.asarray(typeid, dtype=np.int64) & 0xFFFFFFFF
    return t.astype(np.uint64).view(np.float64)


def start(cfg, vel, key, kT, draws=0, finite_q=True, zero_momentum=True):
    """{cavity force, thermalize} of one system on the host -> the thermalizer's item after the run (vel, pos, image are the
    started state).  The host's own dipole stands in for the result block's."""
    first = cavity(cfg, cfg["position"], np.asarray(cfg["image"]))
    item = thermalize_cases.photon_item(cfg, vel, key, first["dipole"], place_photon=True, finite_q=finite_q,
                                        zero_momentum=zero_momentum)
    item["kT"] = kT
    state = mirror.new_state()
    state["draws"] = draws
    run = mirror.thermalize(item, state)
    assert run["photon"] is not None and not run["photon"]["ambiguous"]
    return item


def first_row(cfg, vel, key, kT):
    """the three columns of the ledger's first row after one start with the cavity force alone, members = the molecules"""
    item = start(cfg, vel, key, kT)
    out = cavity(cfg, item["pos"], item["image"])
    v, m = item["vel"][:, :3], item["vel"][:, 3]
    ke = 0.5 * m * (v * v).sum(axis=1)
    p = out["photon_idx"]
    e = out["energies"]
    return dict(cavity_potential=(e[0] + e[1]) + e[2], kinetic_cavity=float(ke[p]), kinetic_group=float(np.delete(ke, p).sum()))


class Dimers:
    """cases.dimers_config started on the host at water_systems.KT and run with bonds, Lennard-Jones, Ewald and the cavity force"""

    def __init__(self):
        from cavitymd import _capi
        self.cfg, bonds, bond_typeid = cases.dimers_config()
        self.mass = _thermal(self.cfg)[1]
        self.bonds = bonds
        self.triples = np.concatenate([bonds, bond_typeid[:, None]], axis=1)
        r_cut = cases.DIMERS_R_CUT
        types = self.cfg["types"]
        self.tab = molecular_mirror.tables(_capi.molecular_params(
            len(types), {t: (p["k"], p["r0"]) for t, p in HARMONIC.items()},
            {(types.index(a), types.index(b)): (p["epsilon"], p["sigma"], min(p["r_cut"], r_cut)) for (a, b), p in LJ.items()}))
        self.S = _capi.molecular_order()[1]
        self.kappa, self.k_cut = _capi.coulomb_parameters(r_cut, cases.DIMERS_ACCURACY)
        self.r_cut = r_cut
        self.verlet_input_make = _capi.verlet_input_make

    def forces(self, s):
        """[cavity, molecular, Coulomb] force arrays of the state s and the ledger's (molecular, coulomb, cavity_potential)"""
        cfg = self.cfg
        cav = cavity(cfg, s["pos"], s["image"])
        f = np.zeros((s["N"], 4))
        f[:, :3] = cav["force"][:, :3]
        m = molecular_mirror.forces(s["pos"][:, :3], cfg["typeid"], cfg["box"], self.tab, self.triples, self.S)
        c = coulomb_mirror.forces(s["pos"][:, :3], cfg["charge"], cfg["box"], self.kappa, self.r_cut, self.k_cut, self.bonds)[0]
        e = cav["energies"]
        return [f, m, c], (float(m[:, 3].sum()), float(c[:, 3].sum()), float((e[0] + e[1]) + e[2]))

    def run(self, dt, steps):
        """one start, then `steps` steps -> (steps + 1, 4): kinetic_total, molecular, coulomb and cavity_potential of the row
        after the start and after every step"""
        cfg = self.cfg
        n = len(cfg["charge"])
        vel = np.concatenate([np.zeros((n, 3)), self.mass[:, None]], axis=1)
        item = start(cfg, vel, mirror.item_key(cases.DRIFT_SEED, 0), KT)
        s = {"N": n, "box": cfg["box"], "pos": item["pos"], "vel": item["vel"], "image": item["image"], "net": None,
             "langevin": -1, "steps": 0, "out_of_box": 0, "reservoir": np.float64(0.0)}

        def row_of(U):
            return (float(0.5 * (self.mass * (s["vel"][:, :3] ** 2).sum(axis=1)).sum()),) + U

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


def system_total(rows, coulomb=True):
    """kinetic_total + potential_total of every row; coulomb=False leaves that term out of the ledger (a planted mistake)"""
    return rows[:, 0] + ((rows[:, 1] + (rows[:, 2] if coulomb else 0.0)) + rows[:, 3])


def drift(series) -> float:
    """max |system_total - system_total[0]| over a series"""
    return float(np.abs(series - series[0]).max())
