"""Ewald Coulomb forces of a batch of independent small systems in two launches (cavmd_coulomb_*, cavitymd.CoulombForceBatch) on
the GPU.  Run with `-m gpu` on an MI355X.

The contract is the list of expressions in include/cavmd.h; tests/coulomb_mirror.py restates it in numpy and derives, alongside,
the rounding bound a correct fp64 evaluation stays within (tests/test_coulomb_abi.py checks that mirror against physics):
  1. one ragged batch within the mirror's bound, entry by entry, with every edge of the contract planted and counted;
  2. the rock-salt cell through CoulombForceBatch: the Madelung constant, independent of the mirror;
  3. systems do not see each other, set_items moves results with the items (one at a time, and several at once with a larger
     largest N, a refused call and an item that becomes empty), and an evaluation repeats bit for bit;
  4. {step one, cavity, molecular, Coulomb, step two} replayed from a graph against the same steps enqueued eagerly;
  5. the energy of an NVE run with bonds, Lennard-Jones and Coulomb is conserved to velocity Verlet's second order."""
import numpy as np
import pytest
import torch

import cavitymd
import coulomb_mirror as mirror
from cavitymd import _capi, synthetic
from coulomb_ragged import ragged_batch_stays_within_the_mirror_bound
from gpu_support import same as _same
from water_systems import HARMONIC, LJ
from water_systems import thermal as _thermal

pytestmark = pytest.mark.gpu

MADELUNG = 1.7475645946331822


# ---- 1. one ragged batch --------------------------------------------------------------------------------------------------------
def test_one_ragged_batch_stays_within_the_mirror_bound():
    ROWS, S, KROWS, T = _capi.coulomb_order()
    ragged_batch_stays_within_the_mirror_bound(_capi.load(), (0, 1, 2, ROWS - 1, ROWS, ROWS + 1, 501, 2047, 2048),
                                               (0, 1, 4096, KROWS - 1, KROWS, KROWS + 1, 300, 0, 200))


# ---- 2. rock salt -----------------------------------------------------------------------------------------------------------------
def _system(position, charge, box):
    n = len(charge)
    pd = cavitymd.ParticleData.from_arrays(np.asarray(position, dtype=np.float64), np.zeros(n, dtype=np.int32), np.asarray(charge),
                                           np.zeros((n, 3), dtype=np.int32), ["O", "N", "L"], box, device="cuda")
    return cavitymd.SystemDefinition(pd)


def test_rock_salt_gives_the_madelung_constant():
    g = np.arange(4)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    q = np.where(ijk.sum(axis=1) % 2 == 0, 1.0, -1.0)
    coulomb = cavitymd.CoulombForceBatch([_system(ijk - 2.0, q, (4.0, 4.0, 4.0))], None, r_cut=2.0, kappa=2.0, k_cut=18.209)
    assert coulomb.k_counts == [3309]
    coulomb.compute()
    E = float(coulomb.potential_energy()[0])
    F = coulomb.forces[0].cpu().numpy()
    madelung = -2.0 * E / 64
    print(f"\nMadelung constant on the GPU: {madelung!r}, off by {madelung - MADELUNG:.3e}; largest force {np.abs(F[:, :3]).max():.3e}")
    assert abs(madelung - MADELUNG) <= 2e-7
    assert np.abs(F[:, :3]).max() < 1e-12
    assert np.allclose(F[:, 3], F[0, 3], rtol=1e-12)                               # every ion carries the same share
    coulomb.close()
    with pytest.raises(ValueError):
        cavitymd.CoulombForceBatch([_system(ijk - 2.0, q, (4.0, 4.0, 4.0))], None, r_cut=2.0, accuracy=1e-6, kappa=2.0)


# ---- 3. independence ------------------------------------------------------------------------------------------------------------
def _lattice_batch(n_sides, seeds, spacing=8.0):
    cfgs = [synthetic.diatomic_lattice(n, spacing, seed=s) for n, s in zip(n_sides, seeds)]
    sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                           c["types"], c["box"], device="cuda")) for c in cfgs]
    bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
    return cfgs, sysdefs, [b[0] for b in bonds], [b[1] for b in bonds]


def test_systems_do_not_see_each_other_and_set_items_moves_results():
    cfgs, sysdefs, bonds, _ = _lattice_batch((4, 3, 4, 2), (1, 2, 3, 4))
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=8.0, accuracy=1e-4)   # smallest box 16 bohr; largest 32: K = 3000-odd
    coulomb.compute()
    clean = [f.cpu().numpy().copy() for f in coulomb.forces]
    assert all(np.isfinite(f).all() and f[:-1, :3].any() and not f[-1].any() for f in clean)   # the photon has no charge
    coulomb.compute()                                                              # the same input gives the same bits
    assert all(_same(f.cpu().numpy(), c) for f, c in zip(coulomb.forces, clean))
    sysdefs[1].getParticleData().getPositions()[10, 1] = float("nan")
    coulomb.compute()
    after = [f.cpu().numpy().copy() for f in coulomb.forces]
    for k in (0, 2, 3):
        assert _same(after[k], clean[k]), k
    assert np.isnan(after[1][:-1, 3]).all()                                        # S(k) carries the NaN to every charge of item 1
    sysdefs[1].getParticleData().getPositions()[10, 1] = float(cfgs[1]["position"][10, 1])
    # swap items 0 and 3 (N = 129 and 17), each keeping its slot's force array: the results follow the items
    n = [len(c["charge"]) for c in cfgs]
    out = [torch.zeros((129, 4), dtype=torch.float64, device="cuda") for _ in range(2)]

    def item(k, force, ex=None):
        pd = sysdefs[k].getParticleData()
        return _capi.coulomb_item(n[k], pd.getPositions().data_ptr(), pd.getCharges().data_ptr(), force.data_ptr(), cfgs[k]["box"],
                                  coulomb.kappa, coulomb.r_cut, coulomb.k_cut, bonds[k] if ex is None else ex)

    torch.cuda.synchronize()
    coulomb.coulomb.set_items(0, [item(3, out[0])])
    coulomb.coulomb.set_items(3, [item(0, out[1])])
    assert coulomb.coulomb.sizes == [17, 55, 129, 129]
    coulomb.compute()
    torch.cuda.synchronize()
    assert _same(out[0].cpu().numpy()[:17], clean[3]) and _same(out[1].cpu().numpy(), clean[0])
    assert _same(coulomb.forces[1].cpu().numpy(), clean[1]) and _same(coulomb.forces[2].cpu().numpy(), clean[2])
    with pytest.raises(_capi.CavmdError) as e:                                     # an index beyond the new N: nothing changes
        coulomb.coulomb.set_items(0, [item(3, out[0], np.array([[0, 17]]))])
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert coulomb._ws._lib.cavmd_destroy(coulomb._ws.handle) == _capi.CAVMD_ERR_INVALID_VALUE
    coulomb.compute()
    torch.cuda.synchronize()
    assert _same(out[0].cpu().numpy()[:17], clean[3])
    coulomb.close()


def test_set_items_grows_the_middle_refuses_whole_and_empties_an_item():
    """set_items over two items in the middle that raises the largest N (and with it the LDS of a launch and the number of
    workgroups of both launches); then a call that is refused at its second item, whose good first item must leave no trace;
    then an item that becomes empty.  Expected values: the mirror (within the bound it returns) for new systems, and what the
    same systems gave before the call."""
    cfgs, sysdefs, bonds, _ = _lattice_batch((2, 2, 3, 2), (1, 2, 3, 4))
    spare_cfgs, spare_sysdefs, spare_bonds, _ = _lattice_batch((4, 2), (5, 6))
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=8.0, accuracy=1e-4)   # smallest box 16 bohr
    batch = coulomb.coulomb
    assert batch.sizes == [17, 17, 55, 17] and batch.launch_order == [2, 0, 1, 3]
    coulomb.compute()
    first = [f.cpu().numpy().copy() for f in coulomb.forces]
    assert all(np.isfinite(f).all() and f[:-1, :3].any() for f in first)

    def item(c, sd, ex, force):
        pd = sd.getParticleData()
        return _capi.coulomb_item(len(c["charge"]), pd.getPositions().data_ptr(), pd.getCharges().data_ptr(), force.data_ptr(),
                                  c["box"], coulomb.kappa, coulomb.r_cut, coulomb.k_cut, ex)

    def offsets_for(k_counts):
        return list(np.cumsum([0] + [K + 1 for K in k_counts])[:-1])

    assert batch.structure_device_ptr()[1] == offsets_for(coulomb.k_counts)

    # grow in the middle: items 1 and 2 become the spare systems of 129 and 17 particles, each with a fresh output array
    out = [torch.zeros((len(c["charge"]), 4), dtype=torch.float64, device="cuda") for c in spare_cfgs]
    new_items = [item(spare_cfgs[j], spare_sysdefs[j], spare_bonds[j], out[j]) for j in range(2)]
    k_counts = [coulomb.k_counts[0]] + [_capi.coulomb_k_count(it) for it in new_items] + [coulomb.k_counts[3]]
    torch.cuda.synchronize()
    batch.set_items(1, new_items)
    assert batch.sizes == [17, 129, 17, 17] and batch.launch_order == [1, 0, 2, 3]
    grown_offsets = batch.structure_device_ptr()[1]
    assert grown_offsets == offsets_for(k_counts) and k_counts[1] > k_counts[2] > 0
    coulomb.compute()
    torch.cuda.synchronize()
    assert _same(coulomb.forces[0].cpu().numpy(), first[0]) and _same(coulomb.forces[3].cpu().numpy(), first[3])
    grown = [o.cpu().numpy().copy() for o in out]
    for j, c in enumerate(spare_cfgs):
        want, bound = mirror.forces(c["position"], c["charge"], c["box"], coulomb.kappa, coulomb.r_cut, coulomb.k_cut, spare_bonds[j])
        err = np.abs(grown[j] - want)
        print(f"\nnew item {1 + j}: N = {len(c['charge'])}, K = {k_counts[1 + j]}, largest error / bound = "
              f"{float((err[bound > 0] / bound[bound > 0]).max()):.4f}")
        assert grown[j].shape == want.shape and np.isfinite(grown[j]).all() and (err <= bound).all(), j

    # a refused call changes nothing: its first item (the N = 55 system) is good, its second names particle N
    scratch = [torch.zeros((55, 4), dtype=torch.float64, device="cuda"), torch.zeros((17, 4), dtype=torch.float64, device="cuda")]
    with pytest.raises(_capi.CavmdError) as e:
        batch.set_items(1, [item(cfgs[2], sysdefs[2], bonds[2], scratch[0]),
                            item(cfgs[3], sysdefs[3], np.concatenate([bonds[3], [[0, 17]]]), scratch[1])])
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert batch.sizes == [17, 129, 17, 17] and batch.structure_device_ptr()[1] == grown_offsets
    coulomb.compute()
    torch.cuda.synchronize()
    assert _same(coulomb.forces[0].cpu().numpy(), first[0]) and _same(coulomb.forces[3].cpu().numpy(), first[3])
    assert _same(out[0].cpu().numpy(), grown[0]) and _same(out[1].cpu().numpy(), grown[1])
    assert not scratch[0].cpu().numpy().any() and not scratch[1].cpu().numpy().any()

    # item 0 becomes empty: its old force array is no longer written, the others do not notice
    batch.set_items(0, [_capi.coulomb_item(0, 0, 0, 0, cfgs[0]["box"], coulomb.kappa, coulomb.r_cut, coulomb.k_cut, None)])
    assert batch.sizes == [0, 129, 17, 17] and batch.launch_order == [1, 2, 3, 0]
    offsets = batch.structure_device_ptr()[1]
    assert offsets == offsets_for([0] + k_counts[1:]) and offsets[1] - offsets[0] == 1
    coulomb.compute()
    torch.cuda.synchronize()
    assert _same(coulomb.forces[0].cpu().numpy(), first[0])
    assert _same(out[0].cpu().numpy(), grown[0]) and _same(out[1].cpu().numpy(), grown[1])
    assert _same(coulomb.forces[3].cpu().numpy(), first[3])
    coulomb.close()


# ---- 4. capture -------------------------------------------------------------------------------------------------------------------
def _md(cfgs, sysdefs, bonds, bond_typeid, r_cut, accuracy):
    """cavity force, molecular force, Coulomb force and integrator over `sysdefs`, with thermal velocities"""
    velocities, masses = [], []
    for c in cfgs:
        v0, mass = _thermal(c)
        masses.append(torch.from_numpy(mass).cuda())
        velocities.append(torch.from_numpy(np.concatenate([v0, mass[:, None]], axis=1)).cuda())
    cavity = cavitymd.CavityForceBatch(sysdefs, [c["params"] for c in cfgs])
    lj = {pair: dict(p, r_cut=min(p["r_cut"], r_cut)) for pair, p in LJ.items()}
    mol = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, HARMONIC, lj)
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=r_cut, accuracy=accuracy)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(mol.forces, coulomb.forces)])
    return cavity, mol, coulomb, integrator, velocities, masses


def test_captured_step_replays_like_the_eager_one():
    STEPS, dt = 8, 10.0
    results = []
    for captured in (False, True):
        cfgs, sysdefs, bonds, bond_typeid = _lattice_batch((3, 2), (11, 12))
        cavity, mol, coulomb, integrator, velocities, _ = _md(cfgs, sysdefs, bonds, bond_typeid, 8.0, 1e-5)
        integrator.set_inputs(dt)
        cavity.compute()
        mol.compute()
        coulomb.compute()
        integrator.prime()
        torch.cuda.synchronize()

        def step():
            integrator.step_one()
            cavity.compute()
            mol.compute()
            coulomb.compute()
            integrator.step_two()

        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            assert integrator.state()["steps"].tolist() == [0, 0]                  # capturing ran nothing
            for _ in range(STEPS):
                graph.replay()
        else:
            for _ in range(STEPS):
                step()
        torch.cuda.synchronize()
        results.append([(sd.getParticleData().getPositions().cpu().numpy().tobytes(), velocities[k].cpu().numpy().tobytes(),
                         coulomb.forces[k].cpu().numpy().tobytes()) for k, sd in enumerate(sysdefs)])
        assert integrator.state()["steps"].tolist() == [STEPS] * 2
        moved = coulomb.forces[0].cpu().numpy()
        assert np.isfinite(moved).all() and moved[:-1, :3].any()
        integrator.close()
        coulomb.close()
        mol.close()
        cavity.close()
    assert results[0] == results[1]


# ---- 5. energy ----------------------------------------------------------------------------------------------------------------------
def _dimers(seed):
    """12 charged dimers and the photon: the first 12 molecules of a 3 x 3 x 3 lattice, in its 24-bohr box"""
    c = synthetic.diatomic_lattice(3, 8.0, seed=seed)
    keep = list(range(24)) + [len(c["charge"]) - 1]
    c = dict(c, position=c["position"][keep], typeid=c["typeid"][keep], charge=c["charge"][keep], image=c["image"][keep])
    sysdef = cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"], c["types"],
                                                                         c["box"], device="cuda"))
    bonds, bond_typeid = synthetic.diatomic_bonds(c)
    return c, sysdef, bonds, bond_typeid


def test_nve_energy_is_conserved_to_second_order():
    """NVE, 12 charged dimers plus the photon with bonds, Lennard-Jones and Coulomb (and the cavity force the integrator is
    built on), no bath, no thermostat; H = KE + the cavity energies + both sums of .w, read eagerly every step.  The drift is
    max |H(t) - H(0)| over the 200 steps at dt and over the same time (400 steps) at dt / 2: velocity Verlet's second order
    makes their ratio 4, and the test asks for [3, 5]."""
    DT, STEPS = 10.0, 200
    drift = {}
    for dt, steps in ((DT, STEPS), (0.5 * DT, 2 * STEPS)):
        c, sysdef, bonds, bond_typeid = _dimers(31)
        assert len(bonds) == 12 and len(c["charge"]) == 25
        cavity, mol, coulomb, integrator, velocities, masses = _md([c], [sysdef], [bonds], [bond_typeid], 12.0, 1e-8)

        def hamiltonian():
            ke = 0.5 * (masses[0] * (velocities[0][:, :3] ** 2).sum(dim=1)).sum()
            return float(ke) + float(cavity.energies().sum()) + float(mol.potential_energy()[0]) + float(coulomb.potential_energy()[0])

        integrator.set_inputs(dt)
        cavity.compute()
        mol.compute()
        coulomb.compute()
        integrator.prime()
        H = [hamiltonian()]
        for _ in range(steps):
            integrator.step_one()
            cavity.compute()
            mol.compute()
            coulomb.compute()
            integrator.step_two()
            H.append(hamiltonian())
        H = np.array(H)
        drift[dt] = float(np.abs(H - H[0]).max())
        assert integrator.state()["out_of_box"].tolist() == [0] and np.isfinite(H).all()
        integrator.close()
        coulomb.close()
        mol.close()
        cavity.close()
    ratio = drift[DT] / drift[0.5 * DT]
    print(f"\nenergy drift over {STEPS} steps at dt = {DT}: {drift[DT]:.4e}; at dt / 2: {drift[0.5 * DT]:.4e}; ratio {ratio:.4f}")
    assert 3.0 <= ratio <= 5.0, (drift, ratio)
