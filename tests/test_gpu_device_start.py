"""A batch started on the device (cavitymd.BatchThermalizer) and taken through its first steps by the other batch objects.
Run with `-m gpu` on an MI355X.

tests/test_gpu_thermalize_batch.py holds the thermalizer to its own contract; here that contract is held to the kernels it has
to agree with.  tests/device_start_cases.py builds the inputs and derives every bound and band; tests/test_device_start_twin.py
rehearses them on the host with the contract's numpy mirrors:
  1. the photon placed at finite q sits at the cavity force kernel's zero: the two kernels agree on the sign, on K, on d leaving
     the photon out, on d being taken from unwrapped coordinates, and on q = pos + image * L;
  2. the documented start {cavity, thermalize, cavity, molecular, Coulomb, prime}, three times eagerly and three times from a
     graph, then two steps, eagerly and from a second graph;
  3. the first ledger row of 256 started systems: the spread of the photon and the velocities seen through the ledger;
  4. the ledger's system_total of an NVE run from a device start is conserved to velocity Verlet's second order."""
import numpy as np
import pytest
import torch

import cavitymd
import device_start_cases as cases
import thermalize_mirror as mirror
from gpu_support import same as _same
from water_systems import HARMONIC, KT, LJ
from water_systems import thermal as _thermal

pytestmark = pytest.mark.gpu
KB = cavitymd.PhysicalConstants.KB_HARTREE_PER_K


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sysdef(cfg):
    return cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"],
                                                                       cfg["types"], cfg["box"], device="cuda"))


def _restore(arrays, saved):
    """device-to-device copies on the current stream"""
    for a, s in zip(arrays, saved):
        a.copy_(s)


# ---- 1. the displaced equilibrium ----------------------------------------------------------------------------------------------------
def test_the_photon_placed_at_finite_q_sits_at_the_force_kernels_zero():
    """kT = 0: sigma and the spread are exact zeros, so the photon lands on x = ((-d) * g) / K and every velocity is +-0.  The
    bounds are device_start_cases' (one half-ulp rounding per operation of cavmd.h:64-71 and of the thermalizer's item 4)."""
    configs = cases.placed_configs()
    sysdefs = [_sysdef(cfg) for _, cfg, _ in configs]
    cavity = cavitymd.CavityForceBatch(sysdefs, [cfg["params"] for _, cfg, _ in configs])
    vel = [_cuda(v) for _, _, v in configs]
    pos = [sd.getParticleData().getPositions() for sd in sysdefs]
    image = [sd.getParticleData().getImages() for sd in sysdefs]
    pos0, image0 = [p.clone() for p in pos], [i.clone() for i in image]
    keys = [mirror.item_key(cases.PLACED_SEED, k) for k in range(len(configs))]
    bounds, images = {}, []
    worst = dict(photon=0.0, molecular=0.0, energy=0.0)
    live = dict(photon=np.inf, molecular=np.inf)
    for finite_q in (True, False):
        _restore(pos, pos0)
        _restore(image, image0)
        th = cavitymd.BatchThermalizer(vel, 0.0, seeds=keys, cavity=cavity, place_photon=True, finite_q=finite_q)
        cavity.compute()
        torch.cuda.synchronize()
        dipole_before = [np.array(r.dipole[:]) for r in cavity.results()]
        th.thermalize()
        cavity.compute()
        torch.cuda.synchronize()
        results, st = cavity.results(), th.state()
        for k, ((name, cfg, v), (_, _, g, has_photon)) in enumerate(zip(configs, cases.PLACED_SYSTEMS)):
            where = (name, finite_q)
            n, r = len(v), results[k]
            F, got_v = cavity.forces[k].cpu().numpy(), vel[k].cpu().numpy()
            got_p, got_i = pos[k].cpu().numpy(), image[k].cpu().numpy()
            assert int(st[k]["photon"]) == (n - 1 if has_photon else -1) and int(st[k]["skipped"]) == 0, where
            assert not got_v[:, :3].any() and _same(got_v[:, 3], v[:, 3]), where      # every thermalised velocity is +-0
            if not has_photon:                                                        # nothing placed, no cavity force
                assert _same(got_p, pos0[k].cpu().numpy()) and np.array_equal(got_i, image0[k].cpu().numpy()), where
                assert not F.any() and int(r.photon_idx) == -1, where
                continue
            d, q, E = np.array(r.dipole[:]), np.array(r.q[:]), np.array(r.energy[:])
            FL = np.array(r.photon_force[:])
            assert _same(d, dipole_before[k]), where                                  # the photon is not part of d
            assert _same(F[-1, :3], FL) and FL[2] == 0.0 and q[2] == 0.0, where
            assert _same(q, got_p[-1, :3] + got_i[-1] * np.asarray(cfg["box"])), where
            if g == 0.0:                                                              # exact zeros, as before
                assert not got_p[-1, :3].any() and not got_i[-1].any() and not F.any() and not E.any(), where
                continue
            K = cases.spring_constant(cfg["params"])
            charge = cfg["charge"][:-1]
            if finite_q:
                images.append(got_i[-1])
                bound_p = cases.photon_force_bound(K, g, q, d)
                bound_m = cases.molecular_force_bound(g, charge, q)
                bounds[k] = (bound_p, bound_m)
                total = (E[0] + E[1]) + E[2]
                ratios = (float((np.abs(FL[:2]) / bound_p).max()), float((np.abs(F[:-1, :2]) / bound_m).max()),
                          abs(total) / cases.energy_bound(E[2]))
                print(f"{name}: image {got_i[-1]}, |F_L| / bound {ratios[0]:.3f}, |F_i| / bound {ratios[1]:.3f}, "
                      f"|E_h + E_c + E_d| / bound {ratios[2]:.3f}")
                for key, x in zip(("photon", "molecular", "energy"), ratios):
                    worst[key] = max(worst[key], x)
                assert (np.abs(FL[:2]) <= bound_p).all(), (where, FL, bound_p)
                assert (np.abs(F[:-1, :2]) <= bound_m).all() and not F[:-1, 2:].any(), (where, ratios)
                assert abs(total) <= cases.energy_bound(E[2]), (where, E, total)
                assert np.array_equal(got_i[-1], cases.equilibrium(cfg, d)[1]), where  # and the wrap is item 4's
            else:                                                                     # liveness: q = 0 is far from the zero
                bound_p, bound_m = bounds[k]
                assert not got_p[-1, :3].any() and not got_i[-1].any(), where
                live["photon"] = min(live["photon"], float((np.abs(FL[:2]) / bound_p).min()))
                live["molecular"] = min(live["molecular"], float((np.abs(F[:-1, :2]) / bound_m).min()))
                assert (np.abs(FL[:2]) >= cases.LIVENESS * bound_p).all(), where
                assert (np.abs(F[:-1, :2]) >= cases.LIVENESS * bound_m).all(), where
        th.close()
    cavity.close()
    print(f"worst |F| / bound: photon {worst['photon']:.3f}, molecules {worst['molecular']:.3f}, energy {worst['energy']:.3f}; "
          f"at q = 0 the least |F| / bound: photon {live['photon']:.3e}, molecules {live['molecular']:.3e}")
    assert len(images) == 3 and cases.images_cover_both_signs_and_two_boxes(images)


# ---- the objects of 2. and 4. --------------------------------------------------------------------------------------------------------
class _Md:
    """cavity, molecular and Coulomb forces, the integrator over all three and the thermalizer of `cfgs`, as `_md` of
    tests/test_gpu_coulomb_batch.py builds them, with the masses in .w beforehand and every velocity zero"""

    def __init__(self, cfgs, bonds, bond_typeid, r_cut, accuracy, seed):
        self.cfgs = cfgs
        self.sysdefs = [_sysdef(c) for c in cfgs]
        self.velocities = []
        for c in cfgs:
            mass = _thermal(c)[1]
            self.velocities.append(_cuda(np.concatenate([np.zeros((len(mass), 3)), mass[:, None]], axis=1)))
        self.cavity = cavitymd.CavityForceBatch(self.sysdefs, [c["params"] for c in cfgs])
        lj = {pair: dict(p, r_cut=min(p["r_cut"], r_cut)) for pair, p in LJ.items()}
        self.mol = cavitymd.MolecularForceBatch(self.sysdefs, bonds, bond_typeid, HARMONIC, lj)
        self.coulomb = cavitymd.CoulombForceBatch(self.sysdefs, bonds, r_cut=r_cut, accuracy=accuracy)
        self.integrator = cavitymd.VerletBatch(self.cavity, self.velocities,
                                               extra_forces=[[m, c] for m, c in zip(self.mol.forces, self.coulomb.forces)])
        self.thermalizer = cavitymd.BatchThermalizer(self.velocities, KT, seed=seed, cavity=self.cavity, place_photon=True,
                                                     finite_q=True, zero_momentum=True)
        self.pos = [sd.getParticleData().getPositions() for sd in self.sysdefs]
        self.image = [sd.getParticleData().getImages() for sd in self.sysdefs]
        self.pos0, self.image0 = [p.clone() for p in self.pos], [i.clone() for i in self.image]

    def restore(self):
        _restore(self.pos, self.pos0)
        _restore(self.image, self.image0)

    def forces(self):
        self.cavity.compute()
        self.mol.compute()
        self.coulomb.compute()

    def start(self):
        """the documented order of a start (include/cavmd.h, "the start of a batch")"""
        self.cavity.compute()
        self.thermalizer.thermalize()
        self.forces()
        self.integrator.prime()

    def step(self):
        self.integrator.step_one()
        self.forces()
        self.integrator.step_two()

    def snapshot(self):
        torch.cuda.synchronize()
        arrays = (self.pos, self.image, self.velocities, self.integrator.accel, self.cavity.forces, self.mol.forces, self.coulomb.forces)
        return [[a[k].cpu().numpy().copy() for a in arrays] for k in range(len(self.cfgs))]

    def close(self):
        for obj in (self.thermalizer, self.integrator, self.coulomb, self.mol, self.cavity):
            obj.close()


def _equal(a, b) -> bool:
    return all(x.tobytes() == y.tobytes() for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def _unwrapped_photon(snap, cfg):
    pos, image = snap[0], snap[1]
    return pos[-1, :3] + image[-1] * np.asarray(cfg["box"]), np.abs(image[-1] * np.asarray(cfg["box"]))


# ---- 2. the documented start ---------------------------------------------------------------------------------------------------------
def test_the_documented_start_eager_and_from_a_graph_then_two_steps():
    """Three eager starts from the same initial positions against three replays of ONE captured start (prime is captured with
    the rest: it is step two's launch), each array byte for byte; then two steps from the third start, eagerly and from a
    second graph.  The photon's unwrapped position pos + image * L may move by at most |v| dt + 0.5 |a| dt^2 per step (step
    one's x += dt (v + 0.5 a dt)) plus START_ULPS spacings of |image| * L for forming it on the host: the image flags the
    thermalizer wrote are the ones the integrator continues from."""
    cfgs, bonds, bond_typeid = cases.start_lattices()
    md = _Md(cfgs, bonds, bond_typeid, 8.0, 1e-5, cases.START_SEED)
    dt = cases.START_DT
    md.integrator.set_inputs(dt)

    def two_steps(graph=None):
        snaps = []
        for _ in range(2):
            graph.replay() if graph is not None else md.step()
            snaps.append(md.snapshot())
        return snaps

    eager = []
    for _ in range(3):
        md.restore()
        md.start()
        eager.append(md.snapshot())
    assert md.thermalizer.state()["draws"].tolist() == [3, 3]
    eager_steps = two_steps()
    assert md.integrator.state()["steps"].tolist() == [2, 2] and md.integrator.state()["out_of_box"].tolist() == [0, 0]

    md.restore()
    md.thermalizer.reset()
    md.integrator.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        md.start()
    assert md.thermalizer.state()["draws"].tolist() == [0, 0]                          # a capture runs nothing
    replayed = []
    for _ in range(3):
        md.restore()
        graph.replay()
        replayed.append(md.snapshot())
    assert md.thermalizer.state()["draws"].tolist() == [3, 3]
    for r in range(3):
        assert _equal(replayed[r], eager[r]), r
    names = ("positions", "images", "velocities", "accel", "cavity force", "molecular force", "Coulomb force")
    for a in range(3):
        for b in range(a + 1, 3):
            for k in range(2):
                differ = [x.tobytes() != y.tobytes() for x, y in zip(eager[a][k], eager[b][k])]
                # only the photon moves between two starts: the molecular positions, hence bonds, LJ and Ewald, stay
                assert differ[0] and differ[2] and differ[3] and differ[4], (a, b, k, dict(zip(names, differ)))
    for k, cfg in enumerate(cfgs):
        p = eager[2][k]
        n = len(cfg["charge"])
        assert np.isfinite(np.concatenate([x.ravel() for x in p])).all() and p[5][:-1, :3].any() and p[6][:-1, :3].any(), k
        assert _same(p[0][:n - 1], md.pos0[k].cpu().numpy()[:n - 1]) and not p[1][:n - 1].any(), k   # the molecules stay put

    step_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(step_graph):
        md.step()
    assert md.integrator.state()["steps"].tolist() == [0, 0]
    replayed_steps = two_steps(step_graph)
    state = md.integrator.state()
    assert state["steps"].tolist() == [2, 2] and state["out_of_box"].tolist() == [0, 0]
    for s in range(2):
        assert _equal(replayed_steps[s], eager_steps[s]), s
    for k, cfg in enumerate(cfgs):
        before = eager[2][k]
        assert before[1][-1].any(), k                                                  # the photon starts outside its box
        for s in range(2):
            after = eager_steps[s][k]
            x0, scale0 = _unwrapped_photon(before, cfg)
            x1, scale1 = _unwrapped_photon(after, cfg)
            v, a = before[2][-1, :3], before[3][-1]
            allowed = np.abs(v) * dt + 0.5 * np.abs(a) * dt * dt \
                + cases.START_ULPS * np.spacing(np.maximum(np.maximum(scale0, scale1), np.maximum(np.abs(x0), np.abs(x1))))
            print(f"system {k}, step {s + 1}: photon image {after[1][-1]}, |move| {np.abs(x1 - x0)}, allowed {allowed}")
            assert (np.abs(x1 - x0) <= allowed).all(), (k, s, x0, x1, allowed)
            assert (x1 != x0).any(), (k, s)
            before = after
    md.close()


# ---- 3. the first ledger row -----------------------------------------------------------------------------------------------------------
def test_the_first_ledger_row_of_a_device_start_has_the_analytic_means():
    """256 systems of 40 molecules and the photon; one start with the cavity force alone, one ledger row.  The expectations
    and their six-sigma bands are derived in device_start_cases.ledger_expectations: cavity_potential = (K / 2) |q - q_eq|^2
    and kinetic_cavity are (kT / 2) chi^2_3; kinetic_group is (3 kT / 2)((n - 2) + (sum m)(sum 1 / m) / n^2), not
    (3 / 2)(n - 1) kT, because the momentum rule takes P / n off every momentum.  temperature is the header's expression of
    kinetic_group, bit for bit; that it equals T is not asserted."""
    configs = cases.ledger_configs()
    B, n = cases.LEDGER_B, cases.LEDGER_N
    sysdefs = [_sysdef(cfg) for cfg, _ in configs]
    cavity = cavitymd.CavityForceBatch(sysdefs, [cfg["params"] for cfg, _ in configs])
    host = np.array([v for _, v in configs])
    all_vel = _cuda(host)
    vel = [all_vel[k] for k in range(B)]
    integrator = cavitymd.VerletBatch(cavity, vel)
    th = cavitymd.BatchThermalizer(vel, cases.LEDGER_KT, seed=cases.LEDGER_SEED, cavity=cavity, place_photon=True, finite_q=True,
                                   zero_momentum=True)
    ledger = cavitymd.BatchEnergyLedger(cavity, vel, members=[np.arange(n)] * B, dof=cases.LEDGER_DOF, add_cavity_kinetic=True,
                                        capacity=2)
    cavity.compute()
    th.thermalize()
    cavity.compute()
    integrator.prime()
    ledger.record()
    rows = ledger.read()
    st = th.state()
    assert rows.shape == (B, 1) and st["photon"].tolist() == [n] * B and st["thermalised"].tolist() == [n] * B
    rows = rows[:, 0]
    assert np.isfinite(rows["system_total"]).all() and (rows["n_terms"] == 0).all()
    assert _same(rows["temperature"], cases.temperature(rows["kinetic_group"], cases.LEDGER_DOF, KB))
    assert _same(rows["kinetic_total"], rows["kinetic_group"] + rows["kinetic_cavity"])
    assert _same(rows["cavity_potential"], (rows["cavity"][:, 0] + rows["cavity"][:, 1]) + rows["cavity"][:, 2])
    expected = cases.ledger_expectations(host[:, :n, 3])
    print()
    for name, (mean, band) in expected.items():
        got = float(rows[name].mean())
        print(f"{name}: mean over {B} systems {got:.6e}, expected {mean:.6e}, |difference| {abs(got - mean):.3e} (band {band:.3e})")
        assert abs(got - mean) <= band, name
    for obj in (ledger, th, integrator, cavity):
        obj.close()


# ---- 4. the conserved column -----------------------------------------------------------------------------------------------------------
def test_the_ledgers_system_total_is_conserved_to_second_order_from_a_device_start():
    """12 charged dimers and the photon (the system of test_gpu_coulomb_batch's energy test), bonds, Lennard-Jones, Coulomb at
    accuracy 1e-8 and the cavity force, no bath, no thermostat, started on the device at that test's kT with finite_q.  The
    drift is max |system_total - system_total[0]| over the ledger's own series, one row per step written by a captured step:
    200 steps at dt = 10 against 400 at dt = 5 must give a ratio in [3, 5]; the twin's is in [3.5, 4.5] at these time steps
    (tests/test_device_start_twin.py).  The second run starts after thermalizer.reset(): the same bytes."""
    c, bonds, bond_typeid = cases.dimers_config()
    assert len(bonds) == 12 and len(c["charge"]) == 25
    md = _Md([c], [bonds], [bond_typeid], cases.DIMERS_R_CUT, cases.DIMERS_ACCURACY, cases.DRIFT_SEED)
    capacity = 2 * cases.DRIFT_STEPS + 1
    ledger = cavitymd.BatchEnergyLedger(md.cavity, md.velocities, terms=[("molecular", md.mol), ("coulomb", md.coulomb)],
                                        capacity=capacity)
    graph = None
    drift, starts = {}, []
    for dt, steps in ((cases.DRIFT_DT, cases.DRIFT_STEPS), (0.5 * cases.DRIFT_DT, 2 * cases.DRIFT_STEPS)):
        md.restore()
        md.thermalizer.reset()
        md.integrator.reset()
        ledger.reset()
        md.integrator.set_inputs(dt)
        md.start()
        ledger.record()
        start = md.snapshot()[0]
        starts.append((start[2].tobytes(), start[0][-1].tobytes(), start[1][-1].tobytes()))
        if graph is None:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                md.step()
                ledger.record()
        for _ in range(steps):
            graph.replay()
        rows = ledger.read()[0]
        state = md.integrator.state()
        assert len(rows) == steps + 1 and rows["call"].tolist() == list(range(1, steps + 2))
        assert state["steps"].tolist() == [steps] and state["out_of_box"].tolist() == [0]
        assert (rows["n_terms"] == 2).all() and np.isfinite(rows["system_total"]).all()
        assert rows["molecular"].any() and rows["coulomb"].any() and rows["kinetic_cavity"].all() and rows["cavity_potential"].all()
        total = rows["system_total"]
        drift[dt] = float(np.abs(total - total[0]).max())
    assert starts[0] == starts[1] and md.thermalizer.state()["draws"].tolist() == [1]
    ratio = drift[cases.DRIFT_DT] / drift[0.5 * cases.DRIFT_DT]
    print(f"\ndrift of system_total over {cases.DRIFT_STEPS} steps at dt = {cases.DRIFT_DT}: {drift[cases.DRIFT_DT]:.4e}; "
          f"at dt / 2: {drift[0.5 * cases.DRIFT_DT]:.4e}; ratio {ratio:.4f}")
    assert 3.0 <= ratio <= 5.0, (drift, ratio)
    ledger.close()
    md.close()
