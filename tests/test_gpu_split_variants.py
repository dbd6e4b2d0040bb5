"""Every lane split include/cavmd.h allows, and a launch captured before set_items and replayed after it, for the molecular
force batch (cavmd_molecular_*) and the Ewald Coulomb batch (cavmd_coulomb_*).  Run with `-m gpu` on an MI355X.

The splits are compile-time constants, so a process only ever sees one of them in the product library.  The Makefile's
`split_variants` builds the product three more times (cavitymd._capi.SPLIT_VARIANTS); with the default build every allowed
value of CAVMD_MOLECULAR_J_SPLIT, CAVMD_COULOMB_J_SPLIT and CAVMD_COULOMB_K_SPLIT then runs here once:
  1. each build's ragged batch against the mirrors (tests/molecular_ragged.py and tests/coulomb_ragged.py),
     at sizes on that build's own ROWS and KROWS boundaries, and a second compute repeating the first bit for bit;
  2. per build and per batch, a compute captured into a graph, a set_items outside any capture, and a replay of the OLD graph:
     same sizes and other arrays; a shrunk item; an item grown past the captured LDS; for Coulomb a smaller and a larger K;
     and a new capture after each change of size.  What is expected comes from a second, freshly created batch over the same
     items, evaluated eagerly: part 1 has compared such a batch with the mirror;
  3. set_items while the batch's stream is capturing is refused, and the batch evaluates as before afterwards.
Nothing here is meant to fault: every step uses the library as include/cavmd.h documents it."""
import numpy as np
import pytest
import torch

import coulomb_ragged
import molecular_ragged
from cavitymd import _capi
from gpu_support import same as _same
from gpu_support import stream as _stream
from split_builds import BUILDS, k_counts_for, k_values_for, replay_k_counts, sizes_for

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GUARD = 8   # rows of sentinel before, between and after the items' force arrays
SPARE = 3   # rows a force array is longer than its item


def load_build(name):
    return _capi.load() if name == "product" else _capi.load_split_variant(name)


@pytest.fixture(scope="session", params=list(BUILDS))
def build(request):
    """(name, library) of one of the four builds; the order each answers is the table's."""
    lib = load_build(request.param)
    S_mol, S, T = BUILDS[request.param]
    assert _capi.molecular_order(lib) == (256 // S_mol, S_mol) and _capi.coulomb_order(lib) == (256 // S, S, 256 // T, T)
    return request.param, lib


# ---- 1. every split against the mirrors ----------------------------------------------------------------------------------------
def test_molecular_split_equals_the_mirror_bit_for_bit(build):
    name, lib = build
    ROWS, S = _capi.molecular_order(lib)
    sizes = sizes_for(ROWS)
    assert sum(1 for n in sizes if n > 19) >= 2 and {ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1, 64, 501} <= set(sizes)
    molecular_ragged.ragged_batch_equals_the_mirror_bit_for_bit(lib, sizes, repeat=True)


def test_coulomb_split_stays_within_the_mirror_bound(build):
    """Entry by entry within the bound tests/coulomb_mirror.py derives, with no tolerance added.  The largest error / bound of
    the build is printed; profiles/coulomb_batch/README.md ("Split tests") is where the four figures are recorded."""
    name, lib = build
    ROWS, S, KROWS, T = _capi.coulomb_order(lib)
    sizes = sizes_for(ROWS)
    counts = k_counts_for(sizes, KROWS)
    assert sum(1 for n in sizes if n > 19) >= 2
    # both sides of the KROWS boundary and the boundary itself, from the K the items actually get (N = 0 keeps none)
    kept = {K for n, K in zip(sizes, counts) if n > 0}
    assert {KROWS - 1, KROWS, KROWS + 1, 2 * KROWS + 1} <= kept and set(counts) == set(k_values_for(KROWS))
    assert any(0 < K < KROWS for K in kept) and any(KROWS < K <= 2 * KROWS for K in kept) and any(K > 2 * KROWS for K in kept)
    worst = coulomb_ragged.ragged_batch_stays_within_the_mirror_bound(lib, sizes, counts, repeat=True)
    print(f"\nbuild {name} (S = {S}, T = {T}): K per item {counts}, largest error / bound = {worst:.4f}")


# ---- 2. replay across set_items --------------------------------------------------------------------------------------------------
class Arena:
    """The force arrays of a batch in ONE allocation filled with the sentinel: GUARD rows, then per item its rows and GUARD
    rows more.  An array is longer than its item, so a write past N or past an array lands on a sentinel that is looked at."""

    def __init__(self, caps):
        self.caps, self.offsets = list(caps), []
        rows = GUARD
        for cap in self.caps:
            self.offsets.append(rows)
            rows += cap + GUARD
        self.buffer = torch.full((rows, 4), SENTINEL, dtype=torch.float64, device="cuda")

    def ptr(self, k):
        return self.buffer.data_ptr() + 32 * self.offsets[k]

    def refill(self):
        self.buffer.fill_(SENTINEL)

    def read(self):
        torch.cuda.synchronize()
        return self.buffer.cpu().numpy()

    def expected(self, rows):
        """the whole buffer with the sentinel everywhere but in `rows`: {item: (row indices, their values)}"""
        want = np.full((self.buffer.shape[0], 4), SENTINEL)
        for k, (index, values) in rows.items():
            index = np.asarray(index, dtype=np.int64)
            assert index.size == 0 or index.max() < self.caps[k]
            want[self.offsets[k] + index] = values
        return want


def _agree(got, want):
    """bit for bit, a NaN standing for any NaN"""
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and _same(np.where(nan, 0.0, got), np.where(nan, 0.0, want)))


class MolecularKind:
    name = "molecular"

    def __init__(self, lib):
        self.lib = lib
        self.rows = _capi.molecular_order(lib)[0]
        self.params = molecular_ragged.ragged_params()

    def system(self, k, n, rng, K=None, other_list=False):
        s = molecular_ragged.ragged_system(k, n, rng)
        if other_list:                                                           # the last ordinary bond gives way to another
            s["bonds"] = np.concatenate([s["bonds"][:-1], np.array([[n - 10, n - 8, 1]], dtype=np.uint32)])
        s["pos"] = torch.from_numpy(molecular_ragged.pos4(s)).cuda()
        return s

    def item(self, s, force_ptr):
        return _capi.molecular_item(s["N"], s["pos"].data_ptr(), force_ptr, s["box"], s["bonds"])

    def create(self, ws, items):
        return _capi.Molecular(ws, self.params, items)


class CoulombKind:
    name = "coulomb"

    def __init__(self, lib):
        self.lib = lib
        self.rows, _, self.k_rows, _ = _capi.coulomb_order(lib)

    def system(self, k, n, rng, K=None, other_list=False):
        s = coulomb_ragged.ragged_system(k, n, K, rng)
        if other_list:                                                           # the last ordinary exclusion gives way to another
            s["ex"] = np.concatenate([s["ex"][:-1], np.array([[n - 10, n - 8]], dtype=np.uint32)])
        p = np.zeros((n, 4))
        p[:, :3] = s["x"]
        s["pos"], s["charge"] = torch.from_numpy(p).cuda(), torch.from_numpy(s["q"].copy()).cuda()
        return s

    def item(self, s, force_ptr):
        it = _capi.coulomb_item(s["N"], s["pos"].data_ptr(), s["charge"].data_ptr(), force_ptr, s["box"], coulomb_ragged.KAPPA,
                                coulomb_ragged.R_CUT, s["k_cut"], s["ex"])
        assert coulomb_ragged.k_count(self.lib, it) == s["K"]
        return it

    def create(self, ws, items):
        return _capi.Coulomb(ws, items)


KINDS = {"molecular": MolecularKind, "coulomb": CoulombKind}


@pytest.fixture(params=list(KINDS))
def kind(request, build):
    return KINDS[request.param](build[1])


def _structure(batch, systems):
    """the structure-factor table of a Coulomb batch: per item its (K + 1, 2) entries"""
    torch.cuda.synchronize()
    ptr, offsets = batch.structure_device_ptr()
    total = sum(s["K"] + 1 for s in systems)
    assert offsets == list(np.cumsum([0] + [s["K"] + 1 for s in systems])[:-1])

    class Table:
        __cuda_array_interface__ = {"data": (ptr, False), "shape": (total, 2), "typestr": "<f8", "strides": None, "version": 2}

    table = torch.as_tensor(Table(), device="cuda").clone().cpu().numpy()
    return [table[o:o + s["K"] + 1] for o, s in zip(offsets, systems)]


class Session:
    """A batch over `systems` with its arena: one eager compute, one compute captured into a graph, and a first replay that
    must equal the eager result bit for bit."""

    def __init__(self, kind, systems, caps, captured=True):
        self.kind, self.systems = kind, list(systems)
        self.arena = Arena(caps)
        self.ws = _capi.Workspace(1, lib=kind.lib)
        self.batch = kind.create(self.ws, [kind.item(s, self.arena.ptr(k)) for k, s in enumerate(self.systems)])
        self.graph = None
        self.batch.compute(_stream())
        self.eager = self.arena.read()
        for k, s in enumerate(self.systems):                                     # every entry up to N, none from N on
            rows = self.eager[self.arena.offsets[k]:self.arena.offsets[k] + self.arena.caps[k]]
            assert np.isfinite(rows[:s["N"]]).all() and not (rows[:s["N"], :3] == SENTINEL).any(), k
        assert _agree(self.eager, self.arena.expected({k: (np.arange(s["N"]), self._rows(self.eager, k, s["N"]))
                                                        for k, s in enumerate(self.systems)}))
        if captured:
            self.capture()
            assert _same(self.replay(), self.eager)

    def _rows(self, buffer, k, n):
        return buffer[self.arena.offsets[k]:self.arena.offsets[k] + n]

    def capture(self):
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.batch.compute(_stream())
        self.captured_sizes = [s["N"] for s in self.systems]
        if isinstance(self.kind, CoulombKind):
            self.captured_counts = [s["K"] for s in self.systems]

    def set(self, k, system):
        """set_items outside any capture; replays are not launches the library knows of, so the caller waits for them"""
        torch.cuda.synchronize()
        self.batch.set_items(k, [self.kind.item(system, self.arena.ptr(k))])
        self.systems[k] = system

    def replay(self):
        self.arena.refill()
        self.graph.replay()
        return self.arena.read()

    def fresh(self):
        """a freshly created batch over the same items with an arena of the same layout, evaluated eagerly"""
        other = Session(self.kind, self.systems, self.arena.caps, captured=False)
        other.structure = _structure(other.batch, other.systems) if isinstance(self.kind, CoulombKind) else None
        other.close()
        return other

    def all_rows(self, fresh):
        return self.arena.expected({k: (np.arange(s["N"]), self._rows(fresh.eager, k, s["N"])) for k, s in enumerate(self.systems)})

    def close(self):
        torch.cuda.synchronize()
        self.graph = None
        self.batch.close()
        self.ws.close()


def _workgroups(sizes, rows):
    """(item, first row) per workgroup in the documented order: items by N descending, ties in item order, ceil(N / rows) each"""
    return [(k, first) for k in _capi.batch_launch_order(sizes) for first in range(0, sizes[k], rows)]


def _reached(captured_sizes, sizes, rows):
    """{item: rows} the workgroups of a launch captured for `captured_sizes` reach in the table of `sizes`"""
    grid = max(len(_workgroups(captured_sizes, rows)), 1)
    out = {k: [] for k in range(len(sizes))}
    for k, first in _workgroups(sizes, rows)[:grid]:
        out[k].extend(range(first, min(first + rows, sizes[k])))
    return out


def _start(kind, grown=0):
    """the three items N = (2 ROWS + 1, 40, 17) with the edge-planting helpers' data; item 2's array has room for `grown`"""
    rng = np.random.default_rng(20261019)
    sizes = (2 * kind.rows + 1, 40, 17)
    counts = replay_k_counts(kind.k_rows)[0] if isinstance(kind, CoulombKind) else (None,) * 3
    systems = [kind.system(k, n, rng, K) for k, (n, K) in enumerate(zip(sizes, counts))]
    caps = [sizes[0] + SPARE, sizes[1] + SPARE, max(sizes[2], grown) + SPARE]
    return rng, systems, Session(kind, systems, caps)


def test_replay_follows_other_arrays_of_the_same_sizes(kind):
    rng, systems, session = _start(kind)
    other = kind.system(1, 40, rng, systems[1].get("K"), other_list=True)      # other positions (and charges), another list
    assert other["box"] == systems[1]["box"] and other.get("k_cut") == systems[1].get("k_cut")
    lists = [s.get("bonds", s.get("ex")) for s in (other, systems[1])]
    assert not np.array_equal(other["x"], systems[1]["x"]) and not np.array_equal(*lists) and len(lists[0]) == len(lists[1])
    session.set(1, other)
    fresh = session.fresh()
    assert not _same(fresh.eager, session.eager)                                 # the new arrays give other forces
    assert _same(session.replay(), fresh.eager)
    session.close()


def test_replay_follows_a_shrunk_item(kind):
    rng, systems, session = _start(kind)
    session.set(0, kind.system(0, 5, rng, systems[0].get("K")))                  # fewer workgroups, another launch order
    assert _capi.batch_launch_order(session.batch.sizes) == [1, 2, 0] and session.systems[0]["box"] == systems[0]["box"]
    fresh = session.fresh()
    got = session.replay()
    assert _agree(got, session.all_rows(fresh))                                  # first N entries; sentinels from N on and in the guards
    assert _same(got, fresh.eager)
    session.close()


def _grown_sizes(kind):
    """N = 2 ROWS + 1 + 2 max(ROWS, 2) for item 2.  A launch has LDS for the largest N it was captured with, rounded up to even,
    which is item 1's 40 where ROWS is 4 or 16: where the size above does not exceed it (ROWS = 4 gives 17, no growth at all), a
    second case of as many rows beyond that LDS follows, so that every build meets the NaN path."""
    lds_n = (max(2 * kind.rows + 1, 40) + 1) & ~1
    first = 2 * kind.rows + 1 + 2 * max(kind.rows, 2)
    return lds_n, [first] if first > lds_n else [first, lds_n + 1 + 2 * max(kind.rows, 2)]


def test_replay_fills_an_item_grown_past_the_captured_lds_with_nan(kind):
    lds_n, cases = _grown_sizes(kind)
    assert cases[-1] > lds_n
    for grown in cases:
        rng, systems, session = _start(kind, grown)
        session.set(2, kind.system(2, grown, rng, systems[2].get("K")))
        assert session.systems[2]["box"] == systems[2]["box"] and session.systems[2].get("k_cut") == systems[2].get("k_cut")
        sizes = [s["N"] for s in session.systems]
        fresh = session.fresh()
        reached = _reached(session.captured_sizes, sizes, kind.rows)
        if grown > lds_n:
            assert 0 < len(reached[2]) and sum(len(r) for r in reached.values()) < sum(sizes)   # some rows are reached, some are not
        want = session.arena.expected({k: (rows, np.nan if sizes[k] > lds_n else session._rows(fresh.eager, k, sizes[k])[rows])
                                       for k, rows in reached.items()})
        got = session.replay()
        assert _agree(got, want), (grown, np.argwhere(np.isnan(got) != np.isnan(want))[:4])
        # capture again after a call that changes the sizes: everything, bit for bit
        session.capture()
        assert _same(session.replay(), fresh.eager)
        session.close()


def _k_workgroups(sizes, counts, k_rows):
    """(item, first k) per workgroup of launch 1, in the documented order (none for an item without particles)"""
    return [(k, first) for k in _capi.batch_launch_order(sizes) if sizes[k] for first in range(0, counts[k], k_rows)]


def test_coulomb_replay_after_k_changes(build):
    kind = CoulombKind(build[1])
    _, smaller, larger = replay_k_counts(kind.k_rows)
    rng, systems, session = _start(kind)
    sizes = [s["N"] for s in systems]
    # a smaller k_cut for item 1: launch 1's grid reaches every k-block, with workgroups to spare
    session.set(1, kind.system(1, 40, rng, smaller))
    fresh = session.fresh()
    assert _same(session.replay(), fresh.eager)
    assert all(_same(a, b) for a, b in zip(_structure(session.batch, session.systems), fresh.structure))
    # a larger one: launch 1's captured grid ends before the table does
    session.set(1, kind.system(1, 40, rng, larger))
    counts = [s["K"] for s in session.systems]
    grid = len(_k_workgroups(session.captured_sizes, session.captured_counts, kind.k_rows))
    table = _k_workgroups(sizes, counts, kind.k_rows)
    assert 0 < grid <= len(table) - 2
    fresh = session.fresh()
    got = session.replay()
    structure = _structure(session.batch, session.systems)
    want = [np.zeros_like(t) for t in fresh.structure]                           # the table is allocated zeroed
    for k, first in table[:grid]:
        want[k][first:min(first + kind.k_rows, counts[k])] = fresh.structure[k][first:min(first + kind.k_rows, counts[k])]
    for k in range(3):                                                           # {Q, 0}: launch 2 reaches block 0 of every item
        want[k][counts[k]] = fresh.structure[k][counts[k]]
        assert fresh.structure[k][counts[k], 0] != 0.0 and fresh.structure[k][counts[k], 1] == 0.0
    assert sum(min(kind.k_rows, counts[k] - first) for k, first in table[grid:]) >= 2 and any((w[:-1] != 0.0).any() for w in want)
    for k in range(3):
        assert _same(structure[k], want[k]), (k, counts[k])
    # the forces of a half-evaluated table are promised nothing but their place: N entries, the rest untouched
    written = session.arena.expected({k: (np.arange(n), 0.0) for k, n in enumerate(sizes)})
    assert np.array_equal(got[written == SENTINEL], written[written == SENTINEL])
    # capture again after a call that changes K: everything, bit for bit
    session.capture()
    assert _same(session.replay(), fresh.eager)
    assert all(_same(a, b) for a, b in zip(_structure(session.batch, session.systems), fresh.structure))
    session.close()


# ---- 3. set_items while capturing ----------------------------------------------------------------------------------------------
def test_set_items_is_refused_while_the_stream_is_capturing(kind):
    rng, systems, session = _start(kind)
    other = kind.system(1, 40, rng, systems[1].get("K"))
    item = kind.item(other, session.arena.ptr(1))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        session.batch.compute(_stream())
        with pytest.raises(_capi.CavmdError) as e:                               # the stream of the last launch is capturing
            session.batch.set_items(1, [item])
        assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert session.batch.sizes == [s["N"] for s in systems]
    # nothing changed: the new graph, the old one and an eager compute all give what the batch gave before
    session.arena.refill()
    graph.replay()
    assert _same(session.arena.read(), session.eager)
    assert _same(session.replay(), session.eager)
    session.arena.refill()
    session.batch.compute(_stream())
    assert _same(session.arena.read(), session.eager)
    del graph
    session.close()
