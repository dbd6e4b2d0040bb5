"""One ragged batch of the molecular force batch (cavmd_molecular_*) against tests/molecular_mirror.py bit for bit, with every
edge of the contract planted and counted: tests/test_gpu_molecular_batch.py runs it on the product library,
tests/test_gpu_split_variants.py on every lane-split build.  Importing this module touches no GPU."""
import numpy as np
import torch

import cavitymd
import molecular_mirror as mirror
from cavitymd import _capi
from gpu_support import same as _same
from gpu_support import stream as _stream

PHOTON, N_TYPES = 3, 4


def ragged_params():
    """three interacting types, the photon (type 3) listed with nobody, and the pair (2, 2) left unlisted as well"""
    return _capi.molecular_params(N_TYPES, {0: (0.7, 1.2), 1: (1.4, 0.9)},
                                  {(0, 0): (1e-3, 1.0, 3.0), (0, 1): (2e-3, 0.8, 3.0), (1, 1): (5e-4, 1.1, 3.0),
                                   (0, 2): (1e-3, 0.9, 3.0), (1, 2): (3e-3, 0.7, 2.0)})


def ragged_system(k, n, rng):
    """Host arrays of item k: random wrapped positions in a box with three different lengths (Lx = 8 and Lz = 16 are powers of
    two), the photon in the middle, and as many of the planted edges as the system has particles for."""
    box = (8.0, 10.0 + 2.0 * (k % 2), 16.0)
    x = rng.uniform(-0.5, 0.5, (n, 3)) * np.array(box)
    t = rng.integers(0, 3, n)
    planted = [
        # (index, position, type)
        (0, (0.0, 0.0, 0.0), 0), (1, (3.0, 0.0, 0.0), 0),                        # rsq == rcutsq exactly: skipped
        (2, (0.0, 1.0, 5.0), 0), (3, (np.nextafter(3.0, 0.0), 1.0, 5.0), 1),     # its neighbour inside: contributes
        (4, (-2.0, -3.0, 7.0), 0), (5, (2.0, -3.0, 7.0), 0),                     # d == -L/2 seen from 4, +L/2 seen from 5
        (6, (1.0, 2.0, -4.0), 1), (7, (1.0, 2.0, 4.0), 1),                       # the same on z, bonded: the term is not cut off
        (8, (1.0, 3.0, -5.0), 0), (9, (1.0, 3.0, -3.8), 0),                      # bonded inside the cut-off: bond term, no LJ term
        (10, (3.5, -1.0, -7.0), 1), (11, (-3.5, -1.0, -7.0), 1),                 # a bond across the periodic boundary
        (12, (-1.0, -4.0, 2.0), 2), (13, (-1.0, -4.0, 3.0), 0), (14, (-1.0, -3.0, 2.0), 1), (15, (-2.0, -4.0, 2.0), 2),
        (16, (-1.0, -4.0, 1.0), 2),                                              # 12 has four bonds; (2, 2) is unlisted
        (17, (2.0, 2.0, 2.0), 7), (18, (2.0, 2.5, 2.0), -1),                     # type ids not below n_types
    ]
    for i, pos, typ in planted:
        if i < n:
            x[i], t[i] = pos, typ
    if n > 19:
        t[max(n // 2, 19)] = PHOTON
    bonds = [(6, 7, 1), (8, 9, 0), (10, 11, 1), (12, 13, 0), (14, 12, 1), (12, 15, 0), (16, 12, 1)]
    bonds = [b for b in bonds if max(b[0], b[1]) < n]
    bonds += [(i, i + 1, i % 2) for i in range(20, n - 1, 7)]                     # some ordinary bonds among the random ones
    return {"N": n, "box": box, "x": x, "t": t, "bonds": np.array(bonds, dtype=np.uint32).reshape(-1, 3)}


def pos4(s):
    pos = np.zeros((s["N"], 4))
    pos[:, :3] = s["x"]
    pos[:, 3] = cavitymd.state.type_tag_as_double(s["t"])
    return pos


def ragged_batch_equals_the_mirror_bit_for_bit(lib, sizes, repeat=False):
    """One batch of systems of `sizes` particles (501 among them), created on the loaded library `lib`, against the mirror run
    with that build's S.  repeat: a second compute on unchanged input must repeat the first bit for bit."""
    S = _capi.molecular_order(lib)[1]
    rng = np.random.default_rng(20241018)
    prm = ragged_params()
    tab = mirror.tables(prm)
    systems = [ragged_system(k, n, rng) for k, n in enumerate(sizes)]
    pos = [torch.from_numpy(pos4(s)).cuda() for s in systems]
    force = [torch.full((max(s["N"], 1), 4), 7.0, dtype=torch.float64, device="cuda") for s in systems]
    ws = _capi.Workspace(1, lib=lib)
    batch = _capi.Molecular(ws, prm, [_capi.molecular_item(s["N"], pos[k].data_ptr() if s["N"] else 0,
                                                           force[k].data_ptr() if s["N"] else 0, s["box"], s["bonds"])
                                      for k, s in enumerate(systems)])
    assert batch.launch_order == sorted(range(len(sizes)), key=lambda i: -sizes[i])
    batch.compute(_stream())
    torch.cuda.synchronize()
    trace = {}
    for k, s in enumerate(systems):
        want = mirror.forces(s["x"], s["t"], s["box"], tab, s["bonds"], S, trace)
        got = force[k].cpu().numpy()[:s["N"]]
        assert got.shape == want.shape and _same(got, want), (k, s["N"], np.abs(got - want).max() if s["N"] else 0)
        assert np.isfinite(got).all(), k
        if s["N"] == 0:
            assert (force[k].cpu().numpy() == 7.0).all()                          # an empty item: nothing is written
        if s["N"] > 19:
            for i in (17, 18, max(s["N"] // 2, 19)):                              # out-of-range ids and the photon: exact zeros
                assert s["t"][i] in (7, -1, PHOTON) and not got[i].any(), (k, i)
    # every planted edge was met, by every system large enough to carry it
    big = sum(1 for n in sizes if n > 19)
    assert big >= 2                                                              # or the counts below would ask for nothing
    assert trace["rsq_equals_rcutsq"] >= 2 * big and trace["just_inside_cutoff"] >= 2 * big
    assert trace["d_equals_plus_half"] >= big and trace["d_equals_minus_half"] >= big
    assert trace["bonded_pair_inside_cutoff"] >= 2 * big and trace["bond_across_boundary"] >= 3 * big
    assert trace["four_bonds"] >= big and trace["unlisted_pair"] > 0 and trace["type_out_of_range"] >= 2 * big
    # ... and behaved as the contract says: the first four planted particles alone
    s = systems[sizes.index(501)]
    only = dict(s, x=s["x"][:4].copy(), t=s["t"][:4].copy(), N=4, bonds=np.zeros((0, 3), dtype=np.uint32))
    F = mirror.forces(only["x"], only["t"], only["box"], tab, only["bonds"], S)
    assert not F[0].any() and not F[1].any()                                     # rsq == rcutsq, and 0-2 / 1-3 are farther
    assert F[2, 0] != 0.0 and F[2, 0] == -F[3, 0]                                 # one ulp inside: the term is there
    if repeat:
        first = [f.cpu().numpy() for f in force]
        batch.compute(_stream())
        torch.cuda.synchronize()
        assert all(_same(f.cpu().numpy(), g) for f, g in zip(force, first))
    batch.close()
    ws.close()
