"""The factored reciprocal-space method of the Ewald Coulomb batch (cavmd_ewald_set_reciprocal,
cavitymd.CoulombForceBatch(reciprocal="factored")) on the GPU.  Run with `-m gpu` on an MI355X.

The contract is include/cavmd.h's: the direct method's expressions with cos(k.x) and sin(k.x) taken from per-axis phase factors
in a stated order of multiplications.  tests/coulomb_factored_mirror.py restates it in numpy and derives the rounding bound
(tests/test_ewald_reciprocal_abi.py holds that mirror to the direct one and to physics first):
  1. one ragged batch within the factored mirror's bound, entry by entry, sizes on every boundary of the two kernels;
  2. both methods on one batch: forces and S(k) within the sum of the bounds, direct bits back after switching back;
  3. an evaluation repeats bit for bit;  4. systems do not see each other;
  5. 50 replays of a captured step equal 50 eager steps, the switch is refused during capture, a captured graph keeps its method;
  6. the per-axis limit: refused beyond it, right at it; a replay captured for a smaller M gives NaN, nothing out of bounds;
  7. set_items under the factored method;
  8. the Madelung constant and second-order energy conservation through CoulombForceBatch(reciprocal="factored")."""
import numpy as np
import pytest
import torch

import cavitymd
import coulomb_factored_mirror as factored
import coulomb_mirror as mirror
from cavitymd import _capi, synthetic
from coulomb_ragged import KAPPA, R_CUT, ragged_system
from gpu_support import same as _same
from gpu_support import stream as _stream
from water_systems import HARMONIC, LJ
from water_systems import thermal as _thermal

pytestmark = pytest.mark.gpu

MADELUNG = 1.7475645946331822
DIRECT, FACTORED = _capi.EWALD_RECIPROCAL_DIRECT, _capi.EWALD_RECIPROCAL_FACTORED


class Ragged:
    """A batch of host systems (coulomb_ragged.ragged_system's dictionaries) on the device, created with the direct method as
    every batch is."""

    def __init__(self, systems, kappa=KAPPA, r_cut=R_CUT):
        self.systems, self.kappa, self.r_cut = systems, kappa, r_cut
        self.pos, self.charge, self.force = [], [], []
        for s in systems:
            p = np.zeros((max(s["N"], 1), 4))
            p[:s["N"], :3] = s["x"]
            p[:, 3] = 123.0                                                        # .w is ignored
            self.pos.append(torch.from_numpy(p).cuda())
            self.charge.append(torch.from_numpy(np.concatenate([s["q"], [0.0]])).cuda())
            self.force.append(torch.full((max(s["N"], 1), 4), 7.0, dtype=torch.float64, device="cuda"))
        self.ws = _capi.Workspace(1)
        self.batch = _capi.Coulomb(self.ws, [self.item(k) for k in range(len(systems))])

    def item(self, k, system=None, force=None):
        s = self.systems[k] if system is None else system
        live = s["N"] != 0
        f = self.force[k] if force is None else force
        return _capi.coulomb_item(s["N"], self.pos[k].data_ptr() if live else 0, self.charge[k].data_ptr() if live else 0,
                                  f.data_ptr() if live else 0, s["box"], self.kappa, self.r_cut, s["k_cut"], s["ex"])

    def compute(self):
        self.batch.compute(_stream())
        torch.cuda.synchronize()
        return [f.cpu().numpy()[:s["N"]].copy() for f, s in zip(self.force, self.systems)]

    def structure(self):
        """per item its (K + 1, 2) entries of the structure-factor table"""
        torch.cuda.synchronize()
        ptr, offsets = self.batch.structure_device_ptr()
        counts = [(0 if s["N"] == 0 else s["K"]) + 1 for s in self.systems]
        assert ptr and offsets == list(np.cumsum([0] + counts)[:-1])

        class Table:
            __cuda_array_interface__ = {"data": (ptr, False), "shape": (sum(counts), 2), "typestr": "<f8", "strides": None, "version": 2}

        table = torch.as_tensor(Table(), device="cuda").clone().cpu().numpy()
        return [table[o:o + c] for o, c in zip(offsets, counts)]

    def mirrors(self, k):
        """((F, bound) of the direct mirror, (F, bound) of the factored one) for item k"""
        s = self.systems[k]
        args = (s["x"], s["q"], s["box"], self.kappa, self.r_cut, s["k_cut"], s["ex"])
        direct = mirror.forces(*args)
        return direct, factored.forces(*args, direct=direct)

    def close(self):
        self.batch.close()
        self.ws.close()


def _ratio(err, bound):
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _within(got, want, bound, what):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want)
    assert (err <= bound).all(), (what, _ratio(err, bound))
    return _ratio(err, bound)


def _with_edges(s):
    """a particle at x = -L / 2 exactly on every axis (index 18, which no planted edge uses) and a particle without charge"""
    if s["N"] > 19:
        s["x"][18] = -0.5 * np.array(s["box"])
        s["q"][19] = 0.0
    return s


def _segment_lengths(s):
    """the lengths of the item's segments, in k order"""
    if s["N"] == 0 or s["K"] == 0:
        return []
    m = mirror.k_vectors(s["box"], s["k_cut"])[0]
    return np.bincount(np.cumsum(factored.segments(m) == np.arange(len(m))) - 1).tolist()


def _n_segments(s):
    return len(_segment_lengths(s))


def _thin(n, M, rng, box=(4.0, 4.0, 100.0)):
    """n particles in a long thin box whose kept vectors are (0, 0, 1 .. M), ONE row: k_cut between the M-th and the (M + 1)-th"""
    k_cut = mirror.TWO_PI * (M + 0.5) / box[2]
    assert k_cut < mirror.TWO_PI / max(box[0], box[1])
    m = mirror.k_vectors(box, k_cut)[0]
    assert len(m) == M and (m[:, :2] == 0).all() and m[-1, 2] == M
    x = rng.uniform(-0.5, 0.5, (n, 3)) * np.array(box)
    return {"N": n, "K": M, "box": box, "k_cut": k_cut, "x": x, "q": rng.uniform(-1.0, 1.0, n), "ex": np.zeros((0, 2), dtype=np.uint32)}


# ---- 1. one ragged batch --------------------------------------------------------------------------------------------------------
def test_one_ragged_batch_stays_within_the_factored_mirror_bound():
    """Sizes on every boundary: N around ROWS of either launch 2 and around the tile of launch 1; K around SEG vectors in all, K
    with SEGROWS segments (one full workgroup of launch 1), one fewer and one more (K = 376, 371, 377 in the even items' box,
    counted below); and, since a k_cut says nothing about the rows it makes, three thin boxes whose vectors are ONE row of
    SEG - 1, SEG and SEG + 1: a segment one short, a full one, and a full one with a second of one vector (counted below, as are
    the rows of the ragged boxes that split into full segments and a rest).  Largest error / bound measured on an MI355X: 0.0084 (profiles/coulomb_batch/README.md)."""
    ROWS = _capi.coulomb_order()[0]
    TILE, SEG, MAX_M, EROWS, SEGROWS = _capi.ewald_order()
    assert (SEG, SEGROWS) == (8, 64)                                               # the K below were chosen for these
    sizes = (0, 1, 2, 17, ROWS - 1, ROWS, EROWS + 1, TILE - 1, TILE, TILE + 1, 501, 2048, 130, 3 * TILE + 5)
    counts = (0, 1, 2, SEG - 1, 376, SEG, 371, SEG + 1, 377, 300, 2 * SEG + 1, 200, 0, 1000)
    rng = np.random.default_rng(20261021)
    systems = [_with_edges(ragged_system(k, n, K, rng)) for k, (n, K) in enumerate(zip(sizes, counts))]
    systems += [_thin(40, M, rng, box=(8.0, 8.0, 100.0)) for M in (SEG - 1, SEG, SEG + 1)]
    assert [_n_segments(systems[k]) for k in (4, 6, 8)] == [SEGROWS, SEGROWS - 1, SEGROWS + 1]
    assert [_segment_lengths(s) for s in systems[-3:]] == [[SEG - 1], [SEG], [SEG, 1]]
    lengths = _segment_lengths(systems[13])                                        # M = (4, 8, 12): rows of up to 25 vectors
    assert any(lengths[g:g + 4] == [SEG, SEG, SEG, 1] for g in range(len(lengths))) and SEG - 1 in lengths
    assert _n_segments(systems[13]) > 2 * SEGROWS                                  # several workgroups in launch 1
    r = Ragged(systems)
    assert r.batch.reciprocal == DIRECT                                            # a new batch uses the direct method
    r.batch.set_reciprocal(FACTORED)
    assert r.batch.reciprocal == FACTORED
    got = r.compute()
    worst = 0.0
    for k, s in enumerate(systems):
        want, bound = r.mirrors(k)[1]
        ratio = _within(got[k], want, bound, (k, s["N"], s["K"]))
        worst = max(worst, ratio)
        print(f"\nitem {k}: N = {s['N']}, K = {s['K']}, largest error / bound = {ratio:.4f}")
        if s["N"] == 0:
            assert (r.force[k].cpu().numpy() == 7.0).all()                         # an empty item: nothing is written
        if s["N"] > 19 and k < len(sizes):                                         # (the ragged systems carry the planted edges)
            assert (got[k][19] == 0.0).all() and (got[k][17] == 0.0).all()         # no charge: an entry that compares equal to 0
            assert (s["x"][18] == -0.5 * np.array(s["box"])).all() and got[k][18, :3].any()
    print(f"\nlargest error / bound of the batch: {worst:.4f}")
    r.close()


# ---- 2., 3. two methods on one batch, repeatability ---------------------------------------------------------------------------
def _small_batch(seed=20261022):
    rng = np.random.default_rng(seed)
    return [_with_edges(ragged_system(k, n, K, rng)) for k, (n, K) in enumerate(((65, 300), (17, 63), (0, 0), (200, 376), (40, 0)))]


def test_two_methods_on_one_batch_and_a_repeat_is_bit_for_bit():
    systems = _small_batch()
    r, never_set = Ragged(systems), Ragged(systems)
    first = r.compute()
    first_S = r.structure()
    r.batch.set_reciprocal(FACTORED)
    second = r.compute()
    second_S = r.structure()
    for k, s in enumerate(systems):
        (Fd, bd), (Ff, bf) = r.mirrors(k)
        _within(first[k], Fd, bd, ("direct", k))
        _within(second[k], Ff, bf, ("factored", k))
        # every force entry of the two methods differs by at most the sum of the two bounds
        assert (np.abs(first[k] - second[k]) <= bd + bf).all(), k
        if s["N"] and s["K"]:
            assert not _same(first[k], second[k]), k                               # another evaluation, not the same one
        Sd, sbd = factored.structure_factors(s["x"], s["q"], s["box"], s["k_cut"], "direct")
        Sf, sbf = factored.structure_factors(s["x"], s["q"], s["box"], s["k_cut"], "factored")
        K = 0 if s["N"] == 0 else s["K"]
        assert (np.abs(first_S[k][:K] - Sd) <= sbd).all() and (np.abs(second_S[k][:K] - Sf) <= sbf).all(), k
        assert (np.abs(first_S[k][:K] - second_S[k][:K]) <= sbd + sbf).all(), k
        if s["N"]:                                                                 # launch 2 of either method stores {Q, 0}
            assert second_S[k][K, 1] == 0.0 and _same(second_S[k][K], first_S[k][K]) and np.isclose(second_S[k][K, 0], s["q"].sum(), atol=1e-12)
    # 3. a second factored compute on unchanged input repeats the first bit for bit
    again = r.compute()
    assert all(_same(a, b) for a, b in zip(again, second)) and all(_same(a, b) for a, b in zip(r.structure(), second_S))
    # switching back gives the first direct result bit for bit; a batch never set and one set to DIRECT explicitly agree
    r.batch.set_reciprocal(DIRECT)
    back = r.compute()
    assert all(_same(a, b) for a, b in zip(back, first)) and all(_same(a, b) for a, b in zip(r.structure(), first_S))
    assert never_set.batch.reciprocal == DIRECT
    untouched = never_set.compute()
    assert all(_same(a, b) for a, b in zip(untouched, first))
    with pytest.raises(_capi.CavmdError) as e:
        r.batch.set_reciprocal(2)
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE and r.batch.reciprocal == DIRECT
    r.close()
    never_set.close()


# ---- 4. independence ------------------------------------------------------------------------------------------------------------
def test_a_nan_coordinate_stays_inside_its_system():
    systems = _small_batch(20261023)
    r = Ragged(systems)
    r.batch.set_reciprocal(FACTORED)
    clean = r.compute()
    clean_S = r.structure()
    r.pos[0][10, 1] = float("nan")
    dirty = r.compute()
    dirty_S = r.structure()
    for k in range(1, len(systems)):
        assert _same(dirty[k], clean[k]) and _same(dirty_S[k], clean_S[k]), k
    charged = systems[0]["q"] != 0.0
    assert np.isnan(dirty[0][charged, 3]).all()                                    # S(k) carries the NaN to every charge of item 0
    r.close()


# ---- 5. capture -------------------------------------------------------------------------------------------------------------------
def _lattice_batch(n_sides, seeds, spacing=8.0):
    cfgs = [synthetic.diatomic_lattice(n, spacing, seed=s) for n, s in zip(n_sides, seeds)]
    sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                           c["types"], c["box"], device="cuda")) for c in cfgs]
    bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
    return cfgs, sysdefs, [b[0] for b in bonds], [b[1] for b in bonds]


def _md(cfgs, sysdefs, bonds, bond_typeid, r_cut, accuracy, reciprocal):
    """cavity force, molecular force, Coulomb force and integrator over `sysdefs`, with thermal velocities"""
    velocities, masses = [], []
    for c in cfgs:
        v0, mass = _thermal(c)
        masses.append(torch.from_numpy(mass).cuda())
        velocities.append(torch.from_numpy(np.concatenate([v0, mass[:, None]], axis=1)).cuda())
    cavity = cavitymd.CavityForceBatch(sysdefs, [c["params"] for c in cfgs])
    lj = {pair: dict(p, r_cut=min(p["r_cut"], r_cut)) for pair, p in LJ.items()}
    mol = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, HARMONIC, lj)
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=r_cut, accuracy=accuracy, reciprocal=reciprocal)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(mol.forces, coulomb.forces)])
    return cavity, mol, coulomb, integrator, velocities, masses


def test_fifty_replays_equal_fifty_eager_steps_and_a_graph_keeps_its_method():
    STEPS, dt = 50, 10.0
    results, kept = [], {}
    for captured in (False, True):
        cfgs, sysdefs, bonds, bond_typeid = _lattice_batch((3, 2), (11, 12))
        cavity, mol, coulomb, integrator, velocities, _ = _md(cfgs, sysdefs, bonds, bond_typeid, 8.0, 1e-5, "factored")
        assert coulomb.reciprocal == "factored"
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
                with pytest.raises(_capi.CavmdError) as e:                         # the batch's last stream is capturing
                    coulomb.coulomb.set_reciprocal(DIRECT)
                assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
            assert coulomb.reciprocal == "factored" and integrator.state()["steps"].tolist() == [0, 0]   # capturing ran nothing
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
        if captured:
            # a graph captured with one method keeps it after the switch: positions frozen, the Coulomb launches alone
            coulomb.set_reciprocal("direct")
            coulomb.compute()
            torch.cuda.synchronize()
            kept["direct"] = [f.cpu().numpy().copy() for f in coulomb.forces]
            only = torch.cuda.CUDAGraph()
            with torch.cuda.graph(only):
                coulomb.compute()
            coulomb.set_reciprocal("factored")
            coulomb.compute()
            torch.cuda.synchronize()
            kept["factored"] = [f.cpu().numpy().copy() for f in coulomb.forces]
            only.replay()
            torch.cuda.synchronize()
            kept["replayed"] = [f.cpu().numpy().copy() for f in coulomb.forces]
        integrator.close()
        coulomb.close()
        mol.close()
        cavity.close()
    assert results[0] == results[1]
    assert all(_same(a, b) for a, b in zip(kept["replayed"], kept["direct"]))
    assert not all(_same(a, b) for a, b in zip(kept["replayed"], kept["factored"]))


# ---- 6. capacity ------------------------------------------------------------------------------------------------------------------
def test_the_per_axis_limit_is_refused_beyond_and_right_at_it():
    MAX_M = _capi.ewald_order()[2]
    rng = np.random.default_rng(20261024)
    at, beyond, plain = _thin(40, MAX_M, rng), _thin(40, MAX_M + 1, rng), _thin(40, 5, rng)
    # a box with M exactly at the limit passes the bound of test 1
    r = Ragged([at, plain], kappa=1.5, r_cut=2.0)
    r.batch.set_reciprocal(FACTORED)
    got = r.compute()
    for k in range(2):
        want, bound = r.mirrors(k)[1]
        print(f"\nM = {r.systems[k]['K']}: largest error / bound = {_within(got[k], want, bound, k):.4f}")
    # with the factored method selected, set_items with an item beyond the limit is refused whole: its good first item leaves no trace
    spare = torch.full((40, 4), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(_capi.CavmdError) as e:
        r.batch.set_items(0, [r.item(0, system=plain, force=spare), r.item(1, system=beyond)])
    assert e.value.status == _capi.CAVMD_ERR_CAPACITY and r.batch.reciprocal == FACTORED
    assert all(_same(a, b) for a, b in zip(r.compute(), got)) and (spare.cpu().numpy() == 7.0).all()
    r.close()
    # a batch that holds such an item: the switch is refused, method and results are unchanged
    r = Ragged([plain, beyond], kappa=1.5, r_cut=2.0)
    first = r.compute()
    with pytest.raises(_capi.CavmdError) as e:
        r.batch.set_reciprocal(FACTORED)
    assert e.value.status == _capi.CAVMD_ERR_CAPACITY and r.batch.reciprocal == DIRECT
    assert all(_same(a, b) for a, b in zip(r.compute(), first))
    for k in range(2):
        want, bound = r.mirrors(k)[0]
        _within(first[k], want, bound, k)
    # under the direct method the same set_items is fine, and the switch is refused afterwards as well
    r.batch.set_items(0, [r.item(0, system=beyond)])
    with pytest.raises(_capi.CavmdError) as e:
        r.batch.set_reciprocal(FACTORED)
    assert e.value.status == _capi.CAVMD_ERR_CAPACITY
    r.close()
    # the Python class names the axis and its M
    pd = cavitymd.ParticleData.from_arrays(beyond["x"], np.zeros(40, dtype=np.int32), beyond["q"], np.zeros((40, 3), dtype=np.int32),
                                           ["O", "N", "L"], beyond["box"], device="cuda")
    with pytest.raises(ValueError, match=rf"M = {MAX_M + 1} along z"):
        cavitymd.CoulombForceBatch([cavitymd.SystemDefinition(pd)], None, r_cut=2.0, kappa=1.5, k_cut=beyond["k_cut"], reciprocal="factored")
    with pytest.raises(ValueError, match="reciprocal"):
        cavitymd.CoulombForceBatch([cavitymd.SystemDefinition(pd)], None, r_cut=2.0, kappa=1.5, k_cut=beyond["k_cut"], reciprocal="mesh")


def test_a_replay_captured_for_a_smaller_m_gives_nan_and_leaves_the_rest_alone():
    """The stale-capture guard of both factored kernels: a launch keeps the LDS it was captured with, sized by the largest M
    of the batch then.  After set_items gave item 1 a box with a larger M (legal: within the limit), the replay writes NaN to
    that item's structure factors and forces -- never an out-of-bounds access -- and leaves item 0's bits as they were; an
    eager compute, which sizes its LDS anew, is right again."""
    MAX_M = _capi.ewald_order()[2]
    rng = np.random.default_rng(20261026)
    r = Ragged([_thin(40, 5, rng), _thin(40, 5, rng)], kappa=1.5, r_cut=2.0)
    r.batch.set_reciprocal(FACTORED)
    clean = r.compute()
    clean_S = r.structure()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.batch.compute(_stream())
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same(f.cpu().numpy(), c) for f, c in zip(r.force, clean))
    large = _thin(40, MAX_M, rng)
    r.systems[1] = large
    p = np.zeros((40, 4))
    p[:, :3] = large["x"]
    r.pos[1] = torch.from_numpy(p).cuda()
    r.charge[1] = torch.from_numpy(np.concatenate([large["q"], [0.0]])).cuda()
    r.batch.set_items(1, [r.item(1)])
    graph.replay()
    torch.cuda.synchronize()
    S = r.structure()
    assert _same(r.force[0].cpu().numpy(), clean[0]) and _same(S[0], clean_S[0])
    assert np.isnan(r.force[1].cpu().numpy()).all() and np.isnan(S[1][:MAX_M]).all()
    got = r.compute()                                                              # an eager launch has the LDS the tables need
    want, bound = r.mirrors(1)[1]
    _within(got[1], want, bound, "after the eager compute")
    assert _same(got[0], clean[0])
    r.close()


# ---- 7. set_items -------------------------------------------------------------------------------------------------------------------
def test_set_items_under_the_factored_method():
    """One item replaced; two at once with a larger largest N (more LDS, more workgroups in both launches); an item that becomes
    empty.  New systems within the factored mirror's bound, untouched ones bit for bit, structure offsets as reported."""
    rng = np.random.default_rng(20261025)
    systems = [ragged_system(k, n, K, rng) for k, (n, K) in enumerate(((17, 63), (17, 9), (55, 300), (17, 0)))]
    spares = [ragged_system(k, n, K, rng) for k, (n, K) in ((0, (40, 17)), (1, (129, 377)), (2, (17, 200)))]
    r = Ragged(systems)
    r.batch.set_reciprocal(FACTORED)
    first = r.compute()

    def put(k, s):
        """system s becomes item k (fresh device arrays, kept alive in r)"""
        r.systems[k] = s
        p = np.zeros((max(s["N"], 1), 4))
        p[:s["N"], :3] = s["x"]
        r.pos[k] = torch.from_numpy(p).cuda()
        r.charge[k] = torch.from_numpy(np.concatenate([s["q"], [0.0]])).cuda()
        r.force[k] = torch.full((max(s["N"], 1), 4), 7.0, dtype=torch.float64, device="cuda")
        return r.item(k)

    def check(new, old):
        got = r.compute()
        r.structure()                                                              # asserts the offsets
        for k in new:
            want, bound = r.mirrors(k)[1]
            print(f"\nnew item {k}: N = {r.systems[k]['N']}, K = {r.systems[k]['K']}, largest error / bound = "
                  f"{_within(got[k], want, bound, k):.4f}")
        for k in old:
            assert _same(got[k], first[k]), k

    torch.cuda.synchronize()
    r.batch.set_items(3, [put(3, spares[0])])
    assert r.batch.sizes == [17, 17, 55, 40] and r.batch.reciprocal == FACTORED
    check([3], [0, 1, 2])
    r.batch.set_items(1, [put(1, spares[1]), put(2, spares[2])])
    assert r.batch.sizes == [17, 129, 17, 40] and r.batch.launch_order == [1, 3, 0, 2]
    check([1, 2, 3], [0])
    empty = dict(systems[0], N=0, K=0, x=np.zeros((0, 3)), q=np.zeros(0), ex=np.zeros((0, 2), dtype=np.uint32))
    r.batch.set_items(0, [put(0, empty)])
    assert r.batch.sizes == [0, 129, 17, 40]
    check([1, 2, 3], [])
    assert (r.force[0].cpu().numpy() == 7.0).all()
    r.close()


# ---- 8. physics ---------------------------------------------------------------------------------------------------------------------
def test_rock_salt_gives_the_madelung_constant():
    g = np.arange(4)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    q = np.where(ijk.sum(axis=1) % 2 == 0, 1.0, -1.0)
    pd = cavitymd.ParticleData.from_arrays(np.asarray(ijk - 2.0, dtype=np.float64), np.zeros(64, dtype=np.int32), q,
                                           np.zeros((64, 3), dtype=np.int32), ["O", "N", "L"], (4.0, 4.0, 4.0), device="cuda")
    coulomb = cavitymd.CoulombForceBatch([cavitymd.SystemDefinition(pd)], None, r_cut=2.0, kappa=2.0, k_cut=18.209, reciprocal="factored")
    assert coulomb.k_counts == [3309] and coulomb.reciprocal == "factored"
    coulomb.compute()
    E = float(coulomb.potential_energy()[0])
    F = coulomb.forces[0].cpu().numpy()
    madelung = -2.0 * E / 64
    print(f"\nMadelung constant on the GPU, factored: {madelung!r}, off by {madelung - MADELUNG:.3e}; largest force {np.abs(F[:, :3]).max():.3e}")
    assert abs(madelung - MADELUNG) <= 2e-7
    assert np.abs(F[:, :3]).max() < 1e-12
    assert np.allclose(F[:, 3], F[0, 3], rtol=1e-12)                               # every ion carries the same share
    coulomb.close()


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
    """The construction and the tolerance of tests/test_gpu_coulomb_batch.py's test of the same name, with the factored method,
    beside its CPU twin: tests/ewald_factored_twin.py runs the same system from the same start on the host (the host integrator
    of tests/device_start_twin.py with the factored mirror's Ewald forces); tests/test_ewald_reciprocal_abi.py holds that
    twin's drift ratio to [3.5, 4.5] without a GPU.  Here the GPU run's energy is held to the twin's step by step at dt: the
    two evaluate the same expressions and differ by rounding per step (device and host erfc, exp, sincos; fold orders), so their
    energies stay together far below the integrator's own drift -- 1e-3 of it leaves thirteen orders of magnitude over one
    rounding.  A run with the direct method on the GPU is held to the factored one in the same way.
    Measured on an MI355X: drift 1.5256e-4 at dt and 3.8141e-5 at dt / 2, ratio 3.9998, which are the twin's figures as well;
    the GPU run and the twin 2.5e-16 apart, the two methods on the GPU 1.5e-16."""
    import device_start_twin as twin
    import ewald_factored_twin
    DT, STEPS = 10.0, 200
    drift, energies = {}, {}
    for method in ("factored", "direct"):
        for dt, steps in ((DT, STEPS), (0.5 * DT, 2 * STEPS)):
            if method == "direct" and dt != DT:
                continue
            c, sysdef, bonds, bond_typeid = _dimers(31)
            assert len(bonds) == 12 and len(c["charge"]) == 25
            cavity, mol, coulomb, integrator, velocities, masses = _md([c], [sysdef], [bonds], [bond_typeid], 12.0, 1e-8, method)

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
            assert integrator.state()["out_of_box"].tolist() == [0] and np.isfinite(H).all()
            if method == "factored":
                drift[dt] = float(np.abs(H - H[0]).max())
            if dt == DT:
                energies[method] = H
            integrator.close()
            coulomb.close()
            mol.close()
            cavity.close()
    ratio = drift[DT] / drift[0.5 * DT]
    host = twin.system_total(ewald_factored_twin.Dimers("factored").run_thermal(DT, STEPS))
    from_twin = float(np.abs(energies["factored"] - host).max())
    apart = float(np.abs(energies["factored"] - energies["direct"]).max())
    print(f"\nfactored: energy drift over {STEPS} steps at dt = {DT}: {drift[DT]:.4e}; at dt / 2: {drift[0.5 * DT]:.4e}; ratio {ratio:.4f}; "
          f"the CPU twin's drift {twin.drift(host):.4e}; largest |H_gpu - H_twin| over the run: {from_twin:.3e}; "
          f"largest |H_factored - H_direct| on the GPU: {apart:.3e}")
    assert 3.0 <= ratio <= 5.0, (drift, ratio)
    assert from_twin <= 1e-3 * drift[DT], (from_twin, drift[DT])
    assert apart <= 1e-3 * drift[DT], (apart, drift[DT])
