"""Harmonic bonds and Lennard-Jones pairs of a batch of independent small systems in one launch (cavmd_molecular_*,
cavitymd.MolecularForceBatch) on the GPU.  Run with `-m gpu` on an MI355X.

The contract is the list of expressions in include/cavmd.h; tests/molecular_mirror.py restates it in element-wise numpy with
the published summation order, and every "bit for bit" check compares uint64 views:
  1. one ragged batch against the mirror, with every edge of the contract planted and counted;
  2. the closed-form answers through MolecularForceBatch, independent of the mirror;
  3. systems do not see each other, and set_items moves results with the items -- one at a time, and several at once with a
     larger largest N, a refused call and an item that becomes empty;
  4. {step one, cavity force, molecular force, step two} replayed from a graph against the same steps enqueued eagerly;
  5. the energy of an NVE run is conserved to velocity Verlet's second order, as a CPU twin's is."""
import numpy as np
import pytest
import torch

import cavitymd
import molecular_mirror as mirror
from cavitymd import _capi, synthetic
from gpu_support import same as _same
from molecular_ragged import ragged_batch_equals_the_mirror_bit_for_bit
from verlet_mirror import mirror_accelerations, mirror_step_one, mirror_step_two
from water_systems import HARMONIC, LJ
from water_systems import thermal as _thermal

pytestmark = pytest.mark.gpu


# ---- 1. one ragged batch --------------------------------------------------------------------------------------------------------
def test_one_ragged_batch_equals_the_mirror_bit_for_bit():
    ROWS, S = _capi.molecular_order()
    ragged_batch_equals_the_mirror_bit_for_bit(_capi.load(), (0, 1, 2, ROWS - 1, ROWS, ROWS + 1, 501, 2047, 2048))


# ---- 2. known answers -------------------------------------------------------------------------------------------------------------
def _one_system(position, typeid, box, types=("O", "N", "L")):
    n = len(typeid)
    pd = cavitymd.ParticleData.from_arrays(np.asarray(position, dtype=np.float64), typeid, np.zeros(n), np.zeros((n, 3), dtype=np.int32),
                                           list(types), box, device="cuda")
    return cavitymd.SystemDefinition(pd)


def test_known_answers_on_the_gpu():
    epsilon, sigma, K, r0, delta = 0.25, 1.5, 0.73204, 2.281655158, 0.125
    r_min = 2.0 ** (1.0 / 6.0) * sigma
    box = (16.0, 18.0, 20.0)
    sysdefs = [_one_system([[-0.75, 0.0, 0.0], [0.75, 0.0, 0.0]], [0, 0], box),                   # r = sigma
               _one_system([[0.0, 0.0, 0.0], [0.0, r_min, 0.0]], [0, 0], box),                    # the minimum
               _one_system([[1.0, 2.0, 3.0], [1.0 + r0 + delta, 2.0, 3.0]], [1, 1], box),         # one stretched bond, no LJ
               _one_system([[7.5, 0.0, 0.0], [7.5 + r0 + delta - 16.0, 0.0, 0.0]], [1, 1], box),  # the same across the boundary
               _one_system([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [0, 2, 1], box)]  # O, L, N: nothing listed
    bonds = [None, None, [[0, 1]], [[0, 1]], None]
    bond_typeid = [None, None, [0], [0], None]
    mol = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, harmonic={0: dict(k=K, r0=r0)},
                                       lj={("O", "O"): dict(epsilon=epsilon, sigma=sigma, r_cut=4.0)})
    mol.compute()
    E = mol.potential_energy().cpu().numpy()
    F = [f.cpu().numpy() for f in mol.forces]
    eshift = 4 * epsilon * ((sigma / 4.0) ** 12 - (sigma / 4.0) ** 6)
    assert np.allclose(F[0][:, 0], [-24 * epsilon / sigma, 24 * epsilon / sigma], rtol=1e-13) and not F[0][:, 1:3].any()
    assert np.isclose(E[0], -eshift, rtol=1e-12) and F[0][0, 3] == F[0][1, 3]
    assert np.abs(F[1][:, :3]).max() <= 1e-13 * 24 * epsilon / sigma and np.isclose(E[1], -epsilon - eshift, rtol=1e-13)
    for k in (2, 3):
        assert np.allclose(F[k][:, 0], [K * delta, -K * delta], rtol=1e-12) and not F[k][:, 1:3].any()
        assert np.allclose(F[k][:, 3], [0.25 * K * delta ** 2] * 2, rtol=1e-12) and np.isclose(E[k], 0.5 * K * delta ** 2, rtol=1e-12)
    assert not F[4].any() and E[4] == 0.0
    assert E.shape == (5,) and mol.potential_energy().device.type == "cuda"
    # without the shift the energy at sigma is 0
    plain = cavitymd.MolecularForceBatch(sysdefs[:1], None, None, harmonic={},
                                         lj={(0, 0): dict(epsilon=epsilon, sigma=sigma, r_cut=4.0)}, mode="none")
    plain.compute()
    assert abs(float(plain.potential_energy()[0])) <= 1e-15 * epsilon and _same(plain.forces[0].cpu().numpy()[:, :3], F[0][:, :3])
    plain.close()
    mol.close()


# ---- 3. independence ------------------------------------------------------------------------------------------------------------
def _lattice_batch(n_sides, seeds, spacing=8.0):
    cfgs = [synthetic.diatomic_lattice(n, spacing, seed=s) for n, s in zip(n_sides, seeds)]
    sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                           c["types"], c["box"], device="cuda")) for c in cfgs]
    bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
    return cfgs, sysdefs, [b[0] for b in bonds], [b[1] for b in bonds]


def test_systems_do_not_see_each_other_and_set_items_moves_results():
    cfgs, sysdefs, bonds, bond_typeid = _lattice_batch((4, 3, 4, 2), (1, 2, 3, 4))
    lj = {pair: dict(p, r_cut=8.0) for pair, p in LJ.items()}                    # the smallest box is 16 bohr
    mol = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, HARMONIC, lj)
    mol.compute()
    clean = [f.cpu().numpy().copy() for f in mol.forces]
    assert all(np.isfinite(f).all() and f[:-1, :3].any() for f in clean)
    sysdefs[1].getParticleData().getPositions()[10, 1] = float("nan")            # a bonded particle of system 1
    mol.compute()
    after = [f.cpu().numpy().copy() for f in mol.forces]
    for k in (0, 2, 3):
        assert _same(after[k], clean[k]), k
    assert not np.isfinite(after[1][10]).all() and not np.isfinite(after[1][11]).all()         # itself and its partner
    sysdefs[1].getParticleData().getPositions()[10, 1] = float(cfgs[1]["position"][10, 1])
    # swap items 0 and 3 (N = 129 and 17), each keeping its slot's force array: the results follow the items
    n = [len(c["charge"]) for c in cfgs]
    out = [torch.zeros((129, 4), dtype=torch.float64, device="cuda") for _ in range(2)]

    def item(k, force):
        triples = np.concatenate([bonds[k], bond_typeid[k][:, None]], axis=1)
        return _capi.molecular_item(n[k], sysdefs[k].getParticleData().getPositions().data_ptr(), force.data_ptr(), cfgs[k]["box"],
                                    triples)

    torch.cuda.synchronize()
    mol.molecular.set_items(0, [item(3, out[0])])
    mol.molecular.set_items(3, [item(0, out[1])])
    assert mol.molecular.sizes == [17, 55, 129, 129]
    mol.compute()
    torch.cuda.synchronize()
    assert _same(out[0].cpu().numpy()[:17], clean[3]) and _same(out[1].cpu().numpy(), clean[0])
    assert _same(mol.forces[1].cpu().numpy(), clean[1]) and _same(mol.forces[2].cpu().numpy(), clean[2])
    with pytest.raises(_capi.CavmdError) as e:                                   # a bond index beyond the new N: nothing changes
        mol.molecular.set_items(0, [_capi.molecular_item(17, sysdefs[3].getParticleData().getPositions().data_ptr(),
                                                         out[0].data_ptr(), cfgs[3]["box"], np.array([[0, 17, 0]]))])
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert mol._ws._lib.cavmd_destroy(mol._ws.handle) == _capi.CAVMD_ERR_INVALID_VALUE       # the workspace outlives nothing
    mol.compute()
    torch.cuda.synchronize()
    assert _same(out[0].cpu().numpy()[:17], clean[3])
    mol.close()


def test_set_items_grows_the_middle_refuses_whole_and_empties_an_item():
    """set_items over two items in the middle that raises the largest N (and with it the LDS of a launch and the number of
    workgroups); then a call that is refused at its second item, whose good first item must leave no trace; then an item that
    becomes empty.  Expected values: the mirror for new systems, and what the same systems gave before the call."""
    ROWS, S = _capi.molecular_order()
    cfgs, sysdefs, bonds, bond_typeid = _lattice_batch((2, 2, 3, 2), (1, 2, 3, 4))
    spare_cfgs, spare_sysdefs, spare_bonds, spare_bond_typeid = _lattice_batch((4, 2), (5, 6))
    lj = {pair: dict(p, r_cut=8.0) for pair, p in LJ.items()}                    # the smallest box is 16 bohr
    mol = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, HARMONIC, lj)
    batch = mol.molecular
    assert batch.sizes == [17, 17, 55, 17] and batch.launch_order == [2, 0, 1, 3]
    mol.compute()
    first = [f.cpu().numpy().copy() for f in mol.forces]
    assert all(np.isfinite(f).all() and f[:-1, :3].any() for f in first)

    def item(c, sd, b, t, force, bad=False):
        triples = np.concatenate([b, t[:, None]], axis=1)
        if bad:
            triples = np.concatenate([triples, [[0, len(c["charge"]), 0]]])         # a pair index equal to N
        return _capi.molecular_item(len(c["charge"]), sd.getParticleData().getPositions().data_ptr(), force.data_ptr(), c["box"],
                                    triples)

    # grow in the middle: items 1 and 2 become the spare systems of 129 and 17 particles, each with a fresh output array
    out = [torch.zeros((len(c["charge"]), 4), dtype=torch.float64, device="cuda") for c in spare_cfgs]
    torch.cuda.synchronize()
    batch.set_items(1, [item(spare_cfgs[j], spare_sysdefs[j], spare_bonds[j], spare_bond_typeid[j], out[j]) for j in range(2)])
    assert batch.sizes == [17, 129, 17, 17] and batch.launch_order == [1, 0, 2, 3]
    mol.compute()
    torch.cuda.synchronize()
    assert _same(mol.forces[0].cpu().numpy(), first[0]) and _same(mol.forces[3].cpu().numpy(), first[3])
    tab = mirror.tables(mol.params)
    grown = [o.cpu().numpy().copy() for o in out]
    for j, c in enumerate(spare_cfgs):
        triples = np.concatenate([spare_bonds[j], spare_bond_typeid[j][:, None]], axis=1)
        want = mirror.forces(c["position"], c["typeid"], c["box"], tab, triples, S)
        assert grown[j].shape == want.shape and _same(grown[j], want), (j, np.abs(grown[j] - want).max())

    # a refused call changes nothing: its first item (the N = 55 system) is good, its second names particle N
    scratch = [torch.zeros((55, 4), dtype=torch.float64, device="cuda"), torch.zeros((17, 4), dtype=torch.float64, device="cuda")]
    with pytest.raises(_capi.CavmdError) as e:
        batch.set_items(1, [item(cfgs[2], sysdefs[2], bonds[2], bond_typeid[2], scratch[0]),
                            item(cfgs[3], sysdefs[3], bonds[3], bond_typeid[3], scratch[1], bad=True)])
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert batch.sizes == [17, 129, 17, 17]
    mol.compute()
    torch.cuda.synchronize()
    assert _same(mol.forces[0].cpu().numpy(), first[0]) and _same(mol.forces[3].cpu().numpy(), first[3])
    assert _same(out[0].cpu().numpy(), grown[0]) and _same(out[1].cpu().numpy(), grown[1])
    assert not scratch[0].cpu().numpy().any() and not scratch[1].cpu().numpy().any()

    # item 0 becomes empty: its old force array is no longer written, the others do not notice
    batch.set_items(0, [_capi.molecular_item(0, 0, 0, cfgs[0]["box"], None)])
    assert batch.sizes == [0, 129, 17, 17] and batch.launch_order == [1, 2, 3, 0]
    mol.compute()
    torch.cuda.synchronize()
    assert _same(mol.forces[0].cpu().numpy(), first[0])
    assert _same(out[0].cpu().numpy(), grown[0]) and _same(out[1].cpu().numpy(), grown[1])
    assert _same(mol.forces[3].cpu().numpy(), first[3])
    mol.close()


# ---- 4. capture -------------------------------------------------------------------------------------------------------------------
def _md(cfgs, sysdefs, bonds, bond_typeid, rng_seed=7):
    """cavity force, molecular force and integrator over `sysdefs`, with thermal velocities -> (cavity, mol, integrator, vel)"""
    velocities, start = [], []
    for c in cfgs:
        v0, mass = _thermal(c, rng_seed)
        start.append((v0, mass))
        velocities.append(torch.from_numpy(np.concatenate([v0, mass[:, None]], axis=1)).cuda())
    cavity = cavitymd.CavityForceBatch(sysdefs, [c["params"] for c in cfgs])
    mol = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, HARMONIC, LJ)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[f] for f in mol.forces])
    return cavity, mol, integrator, velocities, start


def _snapshot(sysdefs, velocities, cavity, mol, integrator):
    torch.cuda.synchronize()
    out = []
    for k, sd in enumerate(sysdefs):
        pd = sd.getParticleData()
        out.append((pd.getPositions().cpu().numpy().tobytes(), pd.getImages().cpu().numpy().tobytes(),
                    velocities[k].cpu().numpy().tobytes(), cavity.forces[k].cpu().numpy().tobytes(),
                    mol.forces[k].cpu().numpy().tobytes(), integrator.accel[k].cpu().numpy().tobytes()))
    return out


def test_captured_step_replays_like_the_eager_one():
    REPLAYS, dt = 50, 10.0
    results = []
    for captured in (False, True):
        cfgs, sysdefs, bonds, bond_typeid = _lattice_batch((4, 4), (11, 12))
        cavity, mol, integrator, velocities, _ = _md(cfgs, sysdefs, bonds, bond_typeid)
        integrator.set_inputs(dt)
        cavity.compute()
        mol.compute()
        integrator.prime()
        torch.cuda.synchronize()

        def step():
            integrator.step_one()
            cavity.compute()
            mol.compute()
            integrator.step_two()

        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            assert integrator.state()["steps"].tolist() == [0, 0]                # capturing ran nothing
            for _ in range(REPLAYS):
                graph.replay()
        else:
            for _ in range(REPLAYS):
                step()
        results.append(_snapshot(sysdefs, velocities, cavity, mol, integrator))
        state = integrator.state()
        assert state["steps"].tolist() == [REPLAYS] * 2 and state["out_of_box"].tolist() == [0, 0]
        moved = mol.forces[0].cpu().numpy()
        assert np.isfinite(moved).all() and moved[:-1, :3].any() and not moved[-1].any()       # the photon: zeros
        integrator.close()
        mol.close()
        cavity.close()
    assert results[0] == results[1]


# ---- 5. energy ----------------------------------------------------------------------------------------------------------------------
ENERGY_DT, ENERGY_STEPS = 20.0, 24


def _twin_fluctuation(cfg, v0, mass, bonds, bond_typeid, tab, S, ref, oracle_mod, dt, steps):
    """max |H(t) - H(0)| of the CPU twin: mirror forces, the oracle's cavity force, the Verlet mirror"""
    n, p = len(cfg["charge"]), cfg["params"]
    prm = ref.make_params(p["omegac"], p["couplstr"], p["phmass"])
    triples = np.concatenate([bonds, bond_typeid[:, None]], axis=1)
    s = {"N": n, "box": cfg["box"], "pos": np.concatenate([cfg["position"], np.zeros((n, 1))], axis=1),
         "vel": np.concatenate([v0, mass[:, None]], axis=1), "image": np.array(cfg["image"], dtype=np.int32), "net": None,
         "langevin": -1, "steps": 0, "out_of_box": 0, "reservoir": np.float64(0.0)}

    def force():
        out = ref.compute(oracle_mod.pack_pos(s["pos"][:, :3], cfg["typeid"]), cfg["charge"], s["image"], cfg["box"], 2, prm)
        f = np.zeros((n, 4))
        f[:, :3] = out["force"][:, :3]
        m = mirror.forces(s["pos"][:, :3], cfg["typeid"], cfg["box"], tab, triples, S)
        return [f, m], float(np.sum(out["energies"])) + float(m[:, 3].sum())

    def hamiltonian(U):
        return 0.5 * float((mass * (s["vel"][:, :3] ** 2).sum(axis=1)).sum()) + U

    row = _capi.verlet_input_make(dt)
    s["forces"], U = force()
    mirror_accelerations(s)
    H = [hamiltonian(U)]
    for _ in range(steps):
        mirror_step_one(s, row)
        s["forces"], U = force()
        mirror_step_two(s, row)
        H.append(hamiltonian(U))
    H = np.array(H)
    return float(np.abs(H - H[0]).max())


def test_nve_energy_is_conserved_to_second_order(ref, oracle_mod):
    """NVE, B = 3 lattice systems of 4 x 4 x 4 molecules plus the photon (N = 129), no bath, no thermostat;
    H = KE + the three cavity energies + sum of .w, read eagerly every step.  dt = 20 and 24 steps (48 at dt / 2) were chosen
    on the CPU twin: its max |H(t) - H(0)| at dt over that at dt / 2 is
        3.9977, 3.9868, 3.9993
    for the three systems, inside [3.5, 4.5] (velocity Verlet's second order, ten orders above rounding), with
        6.0206e-04, 4.1444e-04, 2.3107e-03
    hartree at dt.  The GPU run must give a ratio in [3, 5] and at most twice the twin's fluctuation at dt: both follow the
    same trajectory up to summation-order rounding in the cavity dipole."""
    S = _capi.molecular_order()[1]
    cfgs, _, bonds, bond_typeid = _lattice_batch((4, 4, 4), (21, 22, 23))
    fluct = {}
    for dt, steps in ((ENERGY_DT, ENERGY_STEPS), (0.5 * ENERGY_DT, 2 * ENERGY_STEPS)):
        cfgs, sysdefs, bonds, bond_typeid = _lattice_batch((4, 4, 4), (21, 22, 23))
        cavity, mol, integrator, velocities, start = _md(cfgs, sysdefs, bonds, bond_typeid)
        masses = [torch.from_numpy(m).cuda() for _, m in start]

        def hamiltonian():
            ke = torch.stack([0.5 * (masses[k] * (velocities[k][:, :3] ** 2).sum(dim=1)).sum() for k in range(3)])
            return ke.cpu().numpy() + cavity.energies().sum(axis=1) + mol.potential_energy().cpu().numpy()

        integrator.set_inputs(dt)
        cavity.compute()
        mol.compute()
        integrator.prime()
        H = [hamiltonian()]
        for _ in range(steps):
            integrator.step_one()
            cavity.compute()
            mol.compute()
            integrator.step_two()
            H.append(hamiltonian())
        H = np.array(H)
        fluct[dt] = np.abs(H - H[0]).max(axis=0)
        assert integrator.state()["out_of_box"].tolist() == [0, 0, 0]
        tab = mirror.tables(mol.params)
        integrator.close()
        mol.close()
        cavity.close()
    twin = {dt: np.array([_twin_fluctuation(cfgs[k], start[k][0], start[k][1], bonds[k], bond_typeid[k], tab, S, ref, oracle_mod,
                                            dt, steps) for k in range(3)])
            for dt, steps in ((ENERGY_DT, ENERGY_STEPS), (0.5 * ENERGY_DT, 2 * ENERGY_STEPS))}
    twin_ratio = twin[ENERGY_DT] / twin[0.5 * ENERGY_DT]
    ratio = fluct[ENERGY_DT] / fluct[0.5 * ENERGY_DT]
    print(f"\ntwin: fluctuation at dt {twin[ENERGY_DT]}, ratio {twin_ratio}; GPU: fluctuation at dt {fluct[ENERGY_DT]}, ratio {ratio}")
    assert np.all((twin_ratio >= 3.5) & (twin_ratio <= 4.5)), twin_ratio
    assert np.all((ratio >= 3.0) & (ratio <= 5.0)), ratio
    assert np.all(fluct[ENERGY_DT] <= 2.0 * twin[ENERGY_DT]), (fluct[ENERGY_DT], twin[ENERGY_DT])
