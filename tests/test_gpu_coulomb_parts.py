"""The two parts of the Ewald sum on the GPU (cavmd_mts_coulomb_set_long_forces, cavmd_mts_coulomb_compute_parts).  Run with
`-m gpu` on an MI355X.

The contract is include/cavmd.h's ("the two parts of the Ewald sum"); tests/coulomb_parts_mirror.py restates it in numpy and
derives the two bounds (tests/test_coulomb_parts_abi.py holds that mirror to tests/coulomb_mirror.py first):
  1. one ragged batch, N and K on every boundary of the kernels: SHORT and LONG inside their bounds entry by entry under both
     reciprocal methods, SHORT + LONG beside cavmd_coulomb_compute, a repeat bit for bit;
  2. SHORT's x, y, z equal cavmd_coulomb_compute's without k-vectors and exclusions;
  3. cavmd_coulomb_compute on a split batch: an unsplit batch's bytes, the long arrays untouched;
  4. systems do not see each other;  5. set_items keeps the long pointers;
  6. 50 replays of {short, long} equal 50 eager calls;  7. a replay captured for a smaller N gives NaN in both arrays;
  8. every refusal that needs a live batch."""
import numpy as np
import pytest
import torch

import coulomb_mirror as mirror
import coulomb_parts_mirror as parts
from cavitymd import _capi
from coulomb_ragged import KAPPA, R_CUT, ragged_system
from gpu_support import same as _same
from gpu_support import stream as _stream

pytestmark = pytest.mark.gpu

SHORT, LONG = _capi.COULOMB_PART_SHORT, _capi.COULOMB_PART_LONG
BOTH = SHORT | LONG
DIRECT, FACTORED = _capi.EWALD_RECIPROCAL_DIRECT, _capi.EWALD_RECIPROCAL_FACTORED
INV = _capi.CAVMD_ERR_INVALID_VALUE


class Ragged:
    """coulomb_ragged.ragged_system's dictionaries on the device; split: every item gets a long array as well"""

    def __init__(self, systems, split=True):
        self.systems = systems
        self.pos, self.charge, self.force, self.long = [], [], [], []
        for s in systems:
            self._arrays(s)
        self.ws = _capi.Workspace(1)
        self.batch = _capi.Coulomb(self.ws, [self.item(k) for k in range(len(systems))])
        if split:
            self.batch.set_long_forces(self.long_ptrs())

    def _arrays(self, s, k=None):
        p = np.zeros((max(s["N"], 1), 4))
        p[:s["N"], :3] = s["x"]
        p[:, 3] = 123.0                                                            # .w is ignored
        new = (torch.from_numpy(p).cuda(), torch.from_numpy(np.concatenate([s["q"], [0.0]])).cuda(),
               torch.full((max(s["N"], 1), 4), 7.0, dtype=torch.float64, device="cuda"),
               torch.full((max(s["N"], 1), 4), 9.0, dtype=torch.float64, device="cuda"))
        for arrays, t in zip((self.pos, self.charge, self.force, self.long), new):
            if k is None:
                arrays.append(t)
            else:
                arrays[k] = t

    def put(self, k, s):
        """system s becomes item k, on fresh device arrays but for the long array, which the batch keeps -> the item"""
        kept = self.long[k]
        self.systems[k] = s
        self._arrays(s, k)
        self.long[k] = kept
        return self.item(k)

    def item(self, k):
        s = self.systems[k]
        live = s["N"] != 0
        return _capi.coulomb_item(s["N"], self.pos[k].data_ptr() if live else 0, self.charge[k].data_ptr() if live else 0,
                                  self.force[k].data_ptr() if live else 0, s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"])

    def long_ptrs(self):
        return [f.data_ptr() if s["N"] else 0 for f, s in zip(self.long, self.systems)]

    def read(self, arrays):
        torch.cuda.synchronize()
        return [f.cpu().numpy()[:s["N"]].copy() for f, s in zip(arrays, self.systems)]

    def compute_parts(self, which=BOTH):
        self.batch.compute_parts(_stream(), which)
        return self.read(self.force), self.read(self.long)

    def compute(self):
        self.batch.compute(_stream())
        return self.read(self.force)

    def structure(self):
        torch.cuda.synchronize()
        ptr, offsets = self.batch.structure_device_ptr()
        counts = [(0 if s["N"] == 0 else s["K"]) + 1 for s in self.systems]

        class Table:
            __cuda_array_interface__ = {"data": (ptr, False), "shape": (sum(counts), 2), "typestr": "<f8", "strides": None, "version": 2}

        table = torch.as_tensor(Table(), device="cuda").clone().cpu().numpy()
        return [table[o:o + c] for o, c in zip(offsets, counts)]

    def args(self, k):
        s = self.systems[k]
        return (s["x"], s["q"], s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"])

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


def _ragged_systems():
    """N in {0, 1, ROWS - 1, ROWS, ROWS + 1, 257, 433} and K in {0, 1, KROWS - 1, KROWS, KROWS + 1, 300}: 257 is one more
    than a workgroup of launch 1 has lanes, 433 the profile's system; an item with particles and no k-vector besides."""
    ROWS, _, KROWS, _ = _capi.coulomb_order()
    assert (ROWS, KROWS) == (16, 64)
    sizes = (0, 1, ROWS - 1, ROWS, ROWS + 1, 257, 433, 40)
    counts = (0, 1, KROWS - 1, KROWS, KROWS + 1, 300, 300, 0)
    rng = np.random.default_rng(20261101)
    return [ragged_system(k, n, K, rng) for k, (n, K) in enumerate(zip(sizes, counts))]


@pytest.fixture(scope="module")
def ragged():
    systems = _ragged_systems()
    trace = {}
    reference = []
    for s in systems:
        args = (s["x"], s["q"], s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"])
        reference.append({"whole": mirror.forces(*args, trace), "short": parts.short(*args),
                          "direct": parts.long(*args, method="direct"), "factored": parts.long(*args, method="factored")})
    # the batch carries exclusions inside the cut-off, beyond it and across the boundary, and particles without charge
    assert trace["excluded_pair_inside_cutoff"] >= 4 and trace["excluded_pair_beyond_cutoff"] >= 4
    assert trace["exclusion_across_boundary"] >= 4 and trace["zero_charge"] >= 4 and trace["four_exclusions"] >= 2
    r = Ragged(systems)
    yield r, reference
    r.close()


# ---- 1. one ragged batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["direct", "factored"])
def test_short_and_long_stay_within_their_mirror_bounds(ragged, method):
    """Largest error / bound measured on an MI355X: see profiles/coulomb_parts/README.md."""
    r, reference = ragged
    r.batch.set_reciprocal(_capi.EWALD_RECIPROCAL[method])
    for f, g in zip(r.force, r.long):
        f.fill_(7.0)
        g.fill_(9.0)
    short, long = r.compute_parts(BOTH)
    whole = r.compute()                                                            # overwrites the short arrays: read above
    worst = {"short": 0.0, "long": 0.0, "sum": 0.0}
    for k, s in enumerate(r.systems):
        ref = reference[k]
        a = _within(short[k], ref["short"][0], ref["short"][1], ("short", k))
        b = _within(long[k], ref[method][0], ref[method][1], ("long", method, k))
        # SHORT + LONG beside the combined evaluation of the same batch: the sum of the two parts' bounds
        c = _within(short[k] + long[k], whole[k], ref["short"][1] + ref[method][1], ("short + long", method, k))
        worst = {"short": max(worst["short"], a), "long": max(worst["long"], b), "sum": max(worst["sum"], c)}
        print(f"\nitem {k}: N = {s['N']}, K = {s['K']}: largest error / bound: short {a:.4f}, long ({method}) {b:.4f}; "
              f"|short + long - compute| / (b_short + b_long) {c:.4f}")
        if s["N"] == 0:
            assert (r.force[k].cpu().numpy() == 7.0).all() and (r.long[k].cpu().numpy() == 9.0).all()   # nothing is written
        if s["N"] > 17:
            for i in (17, max(s["N"] // 2, 18)):                                   # no charge: entries that compare equal to 0
                assert s["q"][i] == 0.0 and (short[k][i] == 0.0).all() and (long[k][i] == 0.0).all(), (k, i)
            assert short[k][:, :3].any() and long[k][:, :3].any()
    print(f"\nlargest error / bound of the batch ({method}): short {worst['short']:.4f}, long {worst['long']:.4f}, "
          f"short + long beside compute {worst['sum']:.4f}")
    # the owner of particle 0 stored {Q, 0}, as the combined evaluation does
    r.compute_parts(LONG)
    for k, (S, s) in enumerate(zip(r.structure(), r.systems)):
        if s["N"]:
            assert S[s["K"], 1] == 0.0 and np.isclose(S[s["K"], 0], s["q"].sum(), atol=1e-12), k
    # a repeat on unchanged input is bit for bit; one part at a time gives the bits of both together and leaves the other array
    again = r.compute_parts(BOTH)
    assert all(_same(x, y) for x, y in zip(again[0], short)) and all(_same(x, y) for x, y in zip(again[1], long))
    for f in r.force + r.long:
        f.fill_(5.0)
    s_only = r.compute_parts(SHORT)
    assert all(_same(x, y) for x, y in zip(s_only[0], short)) and all((x == 5.0).all() for x in s_only[1])
    for f in r.force:
        f.fill_(5.0)
    l_only = r.compute_parts(LONG)
    assert all(_same(x, y) for x, y in zip(l_only[1], long)) and all((x == 5.0).all() for x in l_only[0])
    r.batch.set_reciprocal(DIRECT)


# ---- 2. SHORT beside the combined evaluation without k-vectors and exclusions ------------------------------------------------
def test_short_equals_compute_without_k_vectors_and_exclusions():
    bare = [dict(s, K=0, k_cut=0.0, ex=np.zeros((0, 2), dtype=np.uint32)) for s in _ragged_systems()]
    r = Ragged(bare)
    short, _ = r.compute_parts(SHORT)
    whole = r.compute()
    for k, s in enumerate(bare):
        assert (short[k][:, :3] == whole[k][:, :3]).all(), k                        # the same terms, partition and fold
        if s["N"]:
            w = whole[k][:, 3] - parts.self_and_background(s["q"], s["box"], KAPPA)
            bs, bw = parts.short(*r.args(k))[1][:, 3], mirror.forces(*r.args(k))[1][:, 3]
            assert (np.abs(short[k][:, 3] - w) <= bs + bw).all(), k
    assert sum(int(f[:, :3].any()) for f in short) >= 4
    r.close()


# ---- 3. the combined evaluation does not know of the split -------------------------------------------------------------------
def test_compute_on_a_split_batch_is_an_unsplit_batch_and_leaves_the_long_arrays_alone(ragged):
    r, _ = ragged
    plain = Ragged(r.systems, split=False)
    for method in (DIRECT, FACTORED):
        r.batch.set_reciprocal(method)
        plain.batch.set_reciprocal(method)
        for f in r.long:
            f.fill_(3.25)
        assert all(_same(a, b) for a, b in zip(r.compute(), plain.compute())), method
        assert all((f.cpu().numpy() == 3.25).all() for f in r.long), method
    r.batch.set_reciprocal(DIRECT)
    with pytest.raises(_capi.CavmdError) as e:                                     # no long arrays: no parts
        plain.batch.compute_parts(_stream(), BOTH)
    assert e.value.status == INV
    plain.close()


# ---- 4. independence ----------------------------------------------------------------------------------------------------------
def _small_batch(seed):
    rng = np.random.default_rng(seed)
    return [ragged_system(k, n, K, rng) for k, (n, K) in enumerate(((65, 300), (17, 63), (0, 0), (200, 65), (40, 0)))]


def test_a_nan_coordinate_stays_inside_its_item():
    r = Ragged(_small_batch(20261102))
    clean = r.compute_parts(BOTH)
    r.pos[0][10, 1] = float("nan")
    dirty = r.compute_parts(BOTH)
    for k in range(1, len(r.systems)):
        assert _same(dirty[0][k], clean[0][k]) and _same(dirty[1][k], clean[1][k]), k
    charged = r.systems[0]["q"] != 0.0
    assert np.isnan(dirty[1][0][charged, 3]).all()                                 # S(k) carries the NaN to every charge of item 0
    # (SHORT of item 0 stays finite: a NaN distance is not inside the cut-off, so the pair is skipped, as the contract has it)
    assert np.isfinite(dirty[0][0]).all() and not _same(dirty[0][0], clean[0][0])
    r.close()


# ---- 5. set_items ---------------------------------------------------------------------------------------------------------------
def test_set_items_keeps_the_long_pointers():
    rng = np.random.default_rng(20261103)
    r = Ragged(_small_batch(20261104))
    first = r.compute_parts(BOTH)
    spare = ragged_system(1, 17, 9, rng)                                           # same N, other positions, charges and K
    r.batch.set_items(1, [r.put(1, spare)])
    got = r.compute_parts(BOTH)
    _within(got[0][1], *parts.short(*r.args(1)), "new short")
    _within(got[1][1], *parts.long(*r.args(1)), "new long")                        # written where the long pointer was before
    assert not _same(got[1][1], first[1][1])
    for k in (0, 3, 4):
        assert _same(got[0][k], first[0][k]) and _same(got[1][k], first[1][k]), k
    # a new item may not take its own long array as d_force, nor bring particles to a long pointer that is NULL
    bad = r.item(1)
    bad.d_force = r.long[1].data_ptr()
    with pytest.raises(_capi.CavmdError) as e:
        r.batch.set_items(1, [bad])
    assert e.value.status == INV
    with pytest.raises(_capi.CavmdError) as e:
        r.batch.set_items(2, [r.item(1)])                                          # item 2 has N == 0 and no long array
    assert e.value.status == INV
    again = r.compute_parts(BOTH)
    assert all(_same(a, b) for a, b in zip(again[0] + again[1], got[0] + got[1]))
    r.close()


# ---- 6., 7. capture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["direct", "factored"])
def test_fifty_replays_equal_fifty_eager_calls(method):
    """Between the evaluations every position moves (a torch operation outside the graph), so a replay that did not read its
    inputs when it runs would show."""
    results = []
    for captured in (False, True):
        r = Ragged(_small_batch(20261105))
        r.batch.set_reciprocal(_capi.EWALD_RECIPROCAL[method])
        r.compute_parts(BOTH)
        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                r.batch.compute_parts(_stream(), SHORT)
                r.batch.compute_parts(_stream(), LONG)
                with pytest.raises(_capi.CavmdError) as e:                         # the batch's last stream is capturing
                    r.batch.set_long_forces(r.long_ptrs())
                assert e.value.status == INV
        for step in range(50):
            for p, s in zip(r.pos, r.systems):
                if s["N"]:
                    p[:s["N"], :3] += 1e-3 * (1 + step % 3)
            if captured:
                graph.replay()
            else:
                r.batch.compute_parts(_stream(), SHORT)
                r.batch.compute_parts(_stream(), LONG)
        results.append([a.tobytes() for a in r.read(r.force) + r.read(r.long) + r.structure()])
        assert np.isfinite(r.read(r.long)[0]).all()
        r.close()
    assert results[0] == results[1]


def test_a_replay_captured_for_a_smaller_n_writes_nan_to_both_arrays():
    """The stale-capture guard of the existing launches: the captured launches keep their workgroups (2 + 2 of ROWS = 16) and
    the LDS of N = 20.  After set_items gave item 1 N = 40, the new table starts with item 1's three workgroups: all of its rows
    get NaN in both arrays, never an out-of-bounds access; the fourth workgroup is item 0's first, whose rows keep their bits."""
    rng = np.random.default_rng(20261106)
    r = Ragged([ragged_system(k, 20, 9, rng) for k in range(2)])
    clean = r.compute_parts(BOTH)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.batch.compute_parts(_stream(), BOTH)
    graph.replay()
    assert all(_same(a, b) for a, b in zip(r.read(r.force) + r.read(r.long), clean[0] + clean[1]))
    large = ragged_system(1, 40, 9, rng)
    r.long[1] = torch.full((40, 4), 9.0, dtype=torch.float64, device="cuda")
    r.batch.set_long_forces([r.long[0].data_ptr(), r.long[1].data_ptr()])           # (room for 40 rows before the item grows)
    r.batch.set_items(1, [r.put(1, large)])
    graph.replay()
    short, long = r.read(r.force), r.read(r.long)
    assert np.isnan(short[1]).all() and np.isnan(long[1]).all()
    assert _same(short[0], clean[0][0]) and _same(long[0], clean[1][0])
    got = r.compute_parts(BOTH)                                                    # an eager launch has the LDS the table needs
    _within(got[0][1], *parts.short(*r.args(1)), "short after the eager call")
    _within(got[1][1], *parts.long(*r.args(1)), "long after the eager call")
    r.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_live_batch():
    r = Ragged(_small_batch(20261107), split=False)
    good = r.long_ptrs()

    def refused(call, *args):
        with pytest.raises(_capi.CavmdError) as e:
            call(*args)
        assert e.value.status == INV, e.value.status

    for which in (SHORT, LONG, BOTH):                                              # no long arrays yet
        refused(r.batch.compute_parts, _stream(), which)
    refused(r.batch.set_long_forces, good[:-1])                                    # a wrong n_items
    refused(r.batch.set_long_forces, good + [good[0]])
    refused(r.batch.set_long_forces, [good[0] + 8] + good[1:])                     # a misaligned pointer
    refused(r.batch.set_long_forces, [r.force[0].data_ptr()] + good[1:])           # the item's own d_force
    refused(r.batch.set_long_forces, [0] + good[1:])                               # NULL for an item with particles
    refused(r.batch.compute_parts, _stream(), BOTH)                                # nothing was changed by the refused calls
    r.batch.set_long_forces(good)
    for which in (0, 4, 7, 0xFFFFFFFF):
        refused(r.batch.compute_parts, _stream(), which)
    first = r.compute_parts(BOTH)
    assert good[2] == 0                                                            # (NULL for the empty item is fine)
    r.batch.set_long_forces([0] * len(good))                                       # all NULL drops the split
    refused(r.batch.compute_parts, _stream(), BOTH)
    r.batch.set_long_forces(good)
    again = r.compute_parts(BOTH)
    assert all(_same(a, b) for a, b in zip(again[0] + again[1], first[0] + first[1]))
    r.close()
