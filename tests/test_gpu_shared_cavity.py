"""Several systems of a batch coupled to one shared cavity mode (cavmd_shared_cavity_*, cavitymd.SharedCavityForceBatch) on
the GPU.  Run with `-m gpu` on an MI355X.

  1  a cavity of one member is cavmd_batch_compute's evaluation of that item, byte for byte (sequence and n_partials apart)
  2  a cavity of many members against the CPU oracle on the concatenation of its members, P1 to P5 of tests/parity_support.py
     at tol = 1e-10, the dipole within 2 ulp of the exact sum; what the result blocks of carrier and other members hold
  3  the coupling crosses cells: a charge moved in cell a changes the forces in cell b by -g q_i (g/K) q_j delta
  4  a cavity whose carrier has no photon: zero forces and energies, the other cavities untouched
  5  capture: two kernel nodes, replays equal eager evaluations, the refusals, a replay follows set_items; the capacity rule
  6  the captured step of examples/shared_cavity against the numpy twin (tests/shared_cavity_twin.py)
  7  the example runs"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi
import shared_cavity_cases as cases
from parity_support import check_parity, ref_eval

pytestmark = pytest.mark.gpu

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TOL = 1e-10


def _evaluate(table, items=None):
    ws = _capi.Workspace(1)
    obj = _capi.SharedCavity(ws, table.items() if items is None else items)
    obj.compute(0)
    res = obj.results(0)
    return ws, obj, res


# ---- 1. one member is the batch ---------------------------------------------------------------------------------------------
def _single_member_table():
    members = []
    for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4097):
        for where in sorted({0, n // 2, n - 1}) + [None]:          # the photon first, in the middle, last or absent
            members.append((cases.member_cfg(n, seed=13 * n + (where or 0) + (where is None), photon_at=where), len(members), True))
    two = cases.member_cfg(1500, seed=5, photon_at=700, photon_charge=0.75)   # two L-typed particles: the first is the photon
    two["typeid"][1400] = cases.L_TYPEID
    members.append((two, len(members), True))
    return cases.Table(members, _capi)


def test_a_cavity_of_one_member_is_the_batch_byte_for_byte():
    table = _single_member_table()
    B = len(table.cfgs)
    ws, obj, res = _evaluate(table)
    batch = _capi.Batch(ws, [table.batch_item(k) for k in range(B)], history_depth=2)
    batch.compute(0)
    want = batch.results()
    torch.cuda.synchronize()
    assert obj.count() == B and [obj.carrier(c) for c in range(B)] == list(range(B))
    assert table.guards_intact()
    two_L = 0
    for k in range(B):
        assert res[k].sequence == 1 and res[k].n_partials == 1 and want[k].n_partials == 1
        assert cases.block_equal(res[k], want[k]), (k, table.n[k])
        assert table.forces(k).tobytes() == table.forces(k, table.store2).tobytes(), (k, table.n[k])
        two_L += res[k].n_photon_typed == 2
    assert two_L == 1 and sum(r.photon_idx < 0 for r in res) == 10


# ---- 2. many members against the concatenation --------------------------------------------------------------------------------
SMALL = {2: [1025, 0], 3: [257, 1, 64], 16: None, 17: None}       # ragged N, 0 and 1025 among them
LARGE = (255, 256, 257, 1024)                                       # N = 3 per member


def _many_member_table(no_photon_in=None, seed=0):
    """Cavities of 2, 3, 16, 17, 255, 256, 257 and 1024 members, interleaved in item order; boxes and images differ per member;
    the carrier is the first, a middle or the last member of its cavity."""
    rng = np.random.default_rng(100 + seed)
    slots = []                                                      # (cavity, position among the cavity's members)
    sizes = list(SMALL) + list(LARGE)
    for c, M in enumerate(sizes):
        slots += [(c, j) for j in range(M)]
    order = rng.permutation(len(slots))
    # a cavity's members in ascending item order are its slots in the order they come up
    seen = {c: 0 for c in range(len(sizes))}
    members = []
    for s in order:
        c, _ = slots[s]
        M, j = sizes[c], seen[c]
        seen[c] += 1
        carrier_at = [0, M // 2, M - 1][c % 3]
        if M in SMALL:
            ragged = SMALL[M] or [int(x) for x in np.random.default_rng(M).choice([0, 1, 3, 64, 257, 300], M)]
            n = ragged[j]
        else:
            n = 3
        is_carrier = j == carrier_at
        if is_carrier and n == 0:
            n = 2
        box = tuple(float(x) for x in rng.uniform(9.0, 33.0, 3))
        photon_at = None
        if is_carrier and c != no_photon_in:
            photon_at = [0, n // 2, n - 1][(c // 3) % 3]
        cfg = cases.member_cfg(n, seed=1000 * c + j + 7, photon_at=photon_at, L=box, image_range=2 + c % 3)
        members.append((cfg, c, is_carrier))
    return cases.Table(members, _capi), sizes


def _check_cavity(table, res, c, ref, oracle_mod, cell_dipoles):
    """P1 to P5 of the cavity against the oracle on the concatenation; the blocks of carrier and other members"""
    ks = table.members_of(c)
    cfg, start = cases.concatenated([table.cfgs[k] for k in ks])
    carrier = next(k for k in ks if table.is_carrier[k])
    r = res[carrier]
    at = int(start[ks.index(carrier)])
    gpu = {"photon_idx": at + r.photon_idx if r.photon_idx >= 0 else -1,
           "force": np.concatenate([table.forces(k) for k in ks]).reshape(-1, 4), "energies": np.array(r.energy[:]),
           "dipole": np.array(r.dipole[:])}
    refout = ref_eval(ref, oracle_mod, cfg)
    check_parity(cfg, gpu, refout, tol=TOL)
    assert r.n_partials == len(ks) and r.n_particles == table.n[carrier]
    total = np.zeros(3)
    for k in ks:
        b = res[k]
        assert bytes(b)[24:64] == bytes(r)[24:64], (c, k)                     # q and Dq: identical bits in every member's block
        assert b.n_particles == table.n[k] and b.sequence == r.sequence
        total += np.array(b.energy[:])
        cell = table.cfgs[k]
        if table.n[k]:
            pidx = r.photon_idx if k == carrier else -1
            hi, _ = ref.dipole_exact(oracle_mod.pack_pos(cell["position"], cell["typeid"]), cell["charge"], cell["image"], cell["box"], pidx)
            assert np.all(np.abs(cell_dipoles[k] - hi) <= 2 * np.spacing(np.abs(hi)) + 1e-300), (c, k)
        else:
            assert not cell_dipoles[k].any()
        if k != carrier:
            assert not any(b.energy[:]) and not any(b.photon_force[:]) and b.photon_idx == -1 and b.n_photon_typed == 0
            assert b.n_partials == 1
            assert np.array_equal(np.array(b.dipole[:]), cell_dipoles[k]) and np.array_equal(np.array(b.total_dipole[:]), cell_dipoles[k])
    assert np.array_equal(total, np.array(r.energy[:]))                       # the sum over the members is the carrier's
    return refout


def _cell_dipoles(obj, B):
    out = torch.empty((B, 4), dtype=torch.float64, device="cuda")
    view = torch.as_tensor(cavitymd.shared_cavity._DeviceArray(obj.cell_dipoles_device_ptr(), (B, 4)), device="cuda")
    out.copy_(view)
    return out.cpu().numpy()[:, :3]


@pytest.fixture(scope="module")
def many():
    table, sizes = _many_member_table()
    ws, obj, res = _evaluate(table)
    torch.cuda.synchronize()
    forces = [table.forces(k).copy() for k in range(len(table.cfgs))]
    return {"table": table, "sizes": sizes, "ws": ws, "obj": obj, "res": [bytes(r) for r in res], "forces": forces,
            "cell": _cell_dipoles(obj, len(table.cfgs))}


def test_many_members_against_the_concatenated_system(many, ref, oracle_mod):
    table, obj = many["table"], many["obj"]
    res = [_capi.Result.from_buffer_copy(b) for b in many["res"]]
    assert obj.count() == len(many["sizes"]) and table.guards_intact()
    assert sorted(len(table.members_of(c)) for c in range(obj.count())) == sorted(many["sizes"])
    for c in range(obj.count()):
        assert table.is_carrier[obj.carrier(c)] and table.cavity[obj.carrier(c)] == c
        _check_cavity(table, res, c, ref, oracle_mod, many["cell"])


# ---- 3. the coupling crosses cells ------------------------------------------------------------------------------------------------
def test_a_charge_moved_in_one_cell_changes_the_forces_in_another(many):
    table, obj = many["table"], many["obj"]
    c = many["sizes"].index(3)
    ks = table.members_of(c)
    a = next(k for k in ks if not table.is_carrier[k] and table.n[k] > 1)
    b = next(k for k in ks if k != a and table.n[k] > 1)
    j = 0
    delta = np.array([0.375, -0.25, 0.5])
    table.move(a, j, delta)
    try:
        table.poison()
        obj.compute(0)
        res = obj.results(0)
        p = table.prm[c]
        g, K = p.couplstr, p.K
        qj = table.cfgs[a]["charge"][j]
        before, after = many["forces"][b], table.forces(b)
        mol = table.cfgs[b]["typeid"] != cases.L_TYPEID
        qi = table.cfgs[b]["charge"][mol]
        want = (-g * qi)[:, None] * ((g / K) * qj * delta[:2])[None, :]
        r0 = _capi.Result.from_buffer_copy(many["res"][next(k for k in ks if table.is_carrier[k])])
        scale = g * np.abs(qi) * (np.abs(np.array(r0.q[:2])).max() + (g / K) * np.abs(np.array(r0.dipole[:2])).max())
        assert np.abs(want).max() > 1e3 * TOL * scale.max()                    # the change asked for is far above the tolerance
        assert np.all(np.abs((after - before)[mol, :2] - want) <= 2 * TOL * scale[:, None])
        assert not np.array_equal(after, before)
        for k in range(len(table.cfgs)):                                       # every other cavity keeps its bytes
            if table.cavity[k] != c:
                assert table.forces(k).tobytes() == many["forces"][k].tobytes(), k
                assert cases.block_equal(res[k], many["res"][k], but=("sequence",)), k
    finally:
        table.move(a, j, -delta)


# ---- 4. no photon in one cavity ------------------------------------------------------------------------------------------------
def test_a_cavity_without_a_photon_is_zero_and_leaves_the_others_alone(many, ref, oracle_mod):
    dark = many["sizes"].index(17)
    table, sizes = _many_member_table(no_photon_in=dark)
    ws, obj, res = _evaluate(table)
    torch.cuda.synchronize()
    cell = _cell_dipoles(obj, len(table.cfgs))
    assert table.guards_intact()
    for k in table.members_of(dark):
        assert not table.forces(k).any() and not any(res[k].energy[:]) and res[k].photon_idx == -1
        assert not any(res[k].q[:]) and not any(res[k].Dq[:]) and not any(res[k].photon_force[:])
    for c in range(obj.count()):
        if c != dark:
            _check_cavity(table, res, c, ref, oracle_mod, cell)
            for k in table.members_of(c):                                      # and the bytes of the run with every photon there
                assert table.forces(k).tobytes() == many["forces"][k].tobytes(), k


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------
def _three_cavities():
    members = []
    for c, M in enumerate((3, 2, 1)):
        for j in range(M):
            n = [5, 300, 64][j % 3] + c
            members.append((cases.member_cfg(n, seed=50 * c + j, photon_at=(n - 1 if j == 0 else None)), c, j == 0))
    return cases.Table(members, _capi)


def test_a_captured_evaluation_is_two_kernel_nodes_and_replays_like_eager_calls():
    table = _three_cavities()
    B = len(table.cfgs)
    ws = _capi.Workspace(1)
    obj = _capi.SharedCavity(ws, table.items())
    with pytest.raises(_capi.CavmdError) as e:
        obj.results(0)
    assert e.value.status == _capi.CAVMD_ERR_NOT_COMPUTED

    def refused_in_capture(stream):
        obj.compute(stream)
        out = []
        for call in (lambda: obj.set_items(0, [table.item(0)]), lambda: obj.results(stream)):
            with pytest.raises(_capi.CavmdError) as e:
                call()
            out.append(e.value.status)
        return out

    types, statuses = cases.captured_node_types(refused_in_capture)
    assert types == [0, 0], types                                              # exactly two kernel nodes, nothing else
    assert statuses == [_capi.CAVMD_ERR_INVALID_VALUE] * 2
    obj.compute(0)                                                             # (the object's last stream is an uncaptured one again)
    torch.cuda.synchronize()

    def eager(items):
        fresh = _capi.SharedCavity(ws, items)
        table.poison()
        fresh.compute(0)
        res = fresh.results(0)
        out = [bytes(r) for r in res], [table.forces(k).tobytes() for k in range(B)]
        fresh.close()
        return out

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obj.compute(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    for rep in range(3):                                                       # positions move between replays
        for k in range(B):
            table.move(k, rep % table.n[k], rng.uniform(-0.5, 0.5, 3))
        want = eager(table.items())
        table.poison()
        graph.replay()
        torch.cuda.synchronize()
        res = obj.results(0)
        assert [table.forces(k).tobytes() for k in range(B)] == want[1], rep
        assert all(cases.block_equal(res[k], want[0][k], but=("sequence",)) for k in range(B)), rep
    # item 1 leaves cavity 0 for cavity 2: the replay follows the new table
    moved = table.item(1, cavity=2)
    obj.set_items(1, [moved])
    items = table.items()
    items[1] = moved
    want = eager(items)
    table.poison()
    graph.replay()
    torch.cuda.synchronize()
    res = obj.results(0)
    assert [table.forces(k).tobytes() for k in range(B)] == want[1]
    assert all(cases.block_equal(res[k], want[0][k], but=("sequence",)) for k in range(B))
    assert res[obj.carrier(0)].n_partials == 2 and res[obj.carrier(2)].n_partials == 2
    # a table that is refused changes nothing
    with pytest.raises(_capi.CavmdError) as e:
        obj.set_items(0, [table.item(0, cavity=1)])                            # cavity 0 without a carrier, cavity 1 with two
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    table.poison()
    graph.replay()
    torch.cuda.synchronize()
    assert [table.forces(k).tobytes() for k in range(B)] == want[1]


def test_the_1025th_member_is_refused_through_create():
    cfg = cases.member_cfg(2, seed=1, photon_at=1)
    other = cases.member_cfg(1, seed=2)
    table = cases.Table([(cfg, 0, True)] + [(other, 0, False)] * 1024, _capi)
    ws = _capi.Workspace(1)
    with pytest.raises(_capi.CavmdError) as e:
        _capi.SharedCavity(ws, table.items())
    assert e.value.status == _capi.CAVMD_ERR_CAPACITY
    obj = _capi.SharedCavity(ws, table.items()[:1024])
    assert obj.count() == 1 and obj.carrier(0) == 0


# ---- the Python class -------------------------------------------------------------------------------------------------------------
def test_the_python_class_end_to_end():
    from parity_support import to_device
    cfgs = [cases.member_cfg(40, seed=1, photon_at=39), cases.member_cfg(30, seed=2), cases.member_cfg(20, seed=3, photon_at=0),
            cases.member_cfg(10, seed=4)]
    for k in (1, 3):
        cfgs[k]["types"] = ["O", "N"]                                          # no type named L: not a carrier
    shared = cavitymd.SharedCavityForceBatch([to_device(c) for c in cfgs], [0, 0, 1, 1], cases.PRM)
    assert len(shared) == 4 and shared.n_cavities == 2 and shared.carriers == [0, 2] and shared.batch.sizes == [40, 30, 20, 10]
    shared.compute()
    e = shared.energies()
    res = shared.results()
    assert e.shape == (2, 3) and np.array_equal(e[1], np.array(res[2].energy[:])) and e.all()
    d = shared.cell_dipoles.cpu().numpy()
    assert d.shape == (4, 3) and np.array_equal(d[1], np.array(res[1].dipole[:]))
    assert np.allclose(d[0] + d[1], np.array(res[0].dipole[:]), rtol=1e-12, atol=0.0)
    assert [f.shape for f in shared.forces] == [(40, 4), (30, 4), (20, 4), (10, 4)]
    assert shared.batch.results_device_ptr() != 0
    shared.refresh(cavity_of={1: 1})                                           # system 1 moves to cavity 1
    shared.compute()
    assert shared.results()[2].n_partials == 3 and shared.cavity_of == [0, 1, 1, 1]
    shared.close()
    with pytest.raises(RuntimeError):
        shared.compute()


# ---- 6. the step -----------------------------------------------------------------------------------------------------------------
EXAMPLE = os.path.join(ROOT, "examples", "shared_cavity", "batch_shared_cavity_in_one_graph.py")
MEASURED_RELATIVE_DIFFERENCE = 2.389e-14     # on the MI355X against the twin (the docstring of the test below)
ALLOWED_RELATIVE_DIFFERENCE = 16.0 * MEASURED_RELATIVE_DIFFERENCE


def _example():
    import importlib.util
    spec = importlib.util.spec_from_file_location("batch_shared_cavity_in_one_graph", EXAMPLE)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_captured_step_follows_the_twin_and_only_the_cavity_sum_is_conserved():
    """The example's graph on the twin's configuration (seed 0, M = 3, dt = 10, 800 steps = 8000 a.u.): the ledger's universe_total
    summed over the cavity's members against the twin's energy after every step.  Measured on the MI355X: the largest relative
    difference over the 800 rows is 2.389e-14 (the twin is plain numpy, its sums in another order than the kernels'); allowed is 16
    times that, 3.822e-13.  The excursion of the cavity sum came out as the twin's own, 1.7231e-05, in a band of 3 times that; the
    three members alone moved by 5.010e-04, 1.897e-04 and 4.438e-04."""
    import shared_cavity_twin as twin
    steps = int(round(twin.SPAN / 10.0))
    want = twin.run(0, 10.0)[0]
    run = _example().Cells(twin.start(0), 10.0, capacity=steps, harmonic={0: dict(k=twin.BOND_K, r0=twin.BOND_R0)})
    try:
        run.run(steps)
        members, total = run.universe_total()
    finally:
        run.close()
    assert total.shape == want.shape == (steps,) and members.shape == (twin.M, steps)
    relative = float((np.abs(total - want) / np.abs(want)).max())
    excursion = twin.excursion(total)
    alone = [twin.excursion(m) for m in members]
    band = twin.BAND * twin.MEASURED[0][0]
    print(f"\nlargest relative difference from the twin {relative:.3e} (allowed {ALLOWED_RELATIVE_DIFFERENCE:.3e}); excursion of the "
          f"cavity sum {excursion:.4e} (twin {twin.excursion(want):.4e}, band {band:.4e}); of the members alone "
          + " ".join(f"{a:.3e}" for a in alone))
    assert relative <= ALLOWED_RELATIVE_DIFFERENCE
    assert excursion <= band
    assert all(a > band for a in alone)                                        # the members exchange energy


# ---- 7. the example ----------------------------------------------------------------------------------------------------------------
def test_the_example_runs_in_a_fresh_process():
    done = subprocess.run([sys.executable, EXAMPLE, "3", "100", "10"], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    line = done.stdout.strip().splitlines()[-1]
    assert line.startswith("M=3 cells in one cavity, 100 replays of dt=10.0: cavity-summed universe_total") and "worst excursion" in line
    worst = float(line.split("worst excursion ")[1].split(";")[0])
    alone = float(line.rsplit(" ", 1)[1])
    assert 0.0 < worst < alone, line                                           # only the sum over the cavity is conserved
