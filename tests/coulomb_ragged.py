"""One ragged batch of the Ewald Coulomb batch (cavmd_coulomb_*) within the bound tests/coulomb_mirror.py derives, with every
edge of the contract planted and counted: tests/test_gpu_coulomb_batch.py runs it on the product library,
tests/test_gpu_split_variants.py on every lane-split build.  Importing this module touches no GPU."""
import ctypes

import numpy as np
import torch

import coulomb_mirror as mirror
from cavitymd import _capi
from gpu_support import same as _same
from gpu_support import stream as _stream

R_CUT, KAPPA = 3.0, 1.0


def ragged_system(k, n, K, rng):
    """Host arrays of item k: random wrapped positions and charges in a box with three different lengths (Lx = 8 exactly; Ly
    and Lz stretched until a k_cut keeps exactly K vectors), and as many of the planted edges as the system has particles for."""
    box, k_cut = mirror.box_and_k_cut_for((8.0, 10.0 + 2.0 * (k % 2), 16.0), K)
    x = rng.uniform(-0.5, 0.5, (n, 3)) * np.array(box)
    q = rng.uniform(-1.0, 1.0, n)
    planted = [
        # (index, position)
        (0, (0.0, 0.0, 0.0)), (1, (3.0, 0.0, 0.0)),                                # rsq == r_cut^2 exactly: skipped
        (2, (0.0, 1.0, 5.0)), (3, (np.nextafter(3.0, 0.0), 1.0, 5.0)),             # its neighbour one ulp inside: contributes
        (4, (-2.0, -3.0, 7.0)), (5, (2.0, -3.0, 7.0)),                             # d == -L/2 seen from 4, +L/2 seen from 5
        (8, (1.0, 3.0, -5.0)), (9, (1.0, 3.0, -3.8)),                              # excluded inside the cut-off: erf term only
        (10, (3.5, -1.0, -7.0)), (11, (-3.5, -1.0, -7.0)),                         # an exclusion across the periodic boundary
        (12, (-1.0, -4.0, 2.0)), (13, (-1.0, -4.0, 3.0)), (14, (-1.0, -3.0, 2.0)), (15, (-2.0, -4.0, 2.0)),
        (16, (-1.0, -4.0, 1.0)),                                                   # 12 has four exclusions
    ]
    for i, pos in planted:
        if i < n:
            x[i] = pos
    for i in (0, 1, 2, 3, 4, 5):                                                   # the edge pairs carry charges that count
        if i < n:
            q[i] = 0.5 + 0.1 * i
    if n > 17:
        q[17] = 0.0                                                                # a particle without charge
        q[max(n // 2, 18)] = 0.0
    ex = [(8, 9), (10, 11), (12, 13), (14, 12), (12, 15), (16, 12)]
    ex = [e for e in ex if max(e) < n]
    ex += [(i, i + 1) for i in range(20, n - 1, 7)]                                # ordinary exclusions among the random ones
    return {"N": n, "K": K, "box": box, "k_cut": k_cut, "x": x, "q": q, "ex": np.array(ex, dtype=np.uint32).reshape(-1, 2)}


def k_count(lib, item) -> int:
    K = ctypes.c_uint32()
    _capi.check(lib.cavmd_coulomb_k_count(ctypes.byref(item), ctypes.byref(K)), "cavmd_coulomb_k_count")
    return int(K.value)


def ragged_batch_stays_within_the_mirror_bound(lib, sizes, counts, repeat=False):
    """One batch of systems of `sizes` particles (501 among them) and `counts` kept k-vectors, created on the loaded library
    `lib`, entry by entry within the mirror's bound -> the largest error / bound.  repeat: a second compute on unchanged input
    must repeat the first bit for bit."""
    rng = np.random.default_rng(20261018)
    systems = [ragged_system(k, n, K, rng) for k, (n, K) in enumerate(zip(sizes, counts))]
    pos, charge, force = [], [], []
    for s in systems:
        p = np.zeros((max(s["N"], 1), 4))
        p[:s["N"], :3] = s["x"]
        p[:, 3] = 123.0                                                            # .w is ignored
        pos.append(torch.from_numpy(p).cuda())
        charge.append(torch.from_numpy(np.concatenate([s["q"], [0.0]])).cuda())
        force.append(torch.full((max(s["N"], 1), 4), 7.0, dtype=torch.float64, device="cuda"))
    ws = _capi.Workspace(1, lib=lib)
    items = [_capi.coulomb_item(s["N"], pos[k].data_ptr() if s["N"] else 0, charge[k].data_ptr() if s["N"] else 0,
                                force[k].data_ptr() if s["N"] else 0, s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"])
             for k, s in enumerate(systems)]
    assert [k_count(lib, it) for it in items] == [0 if s["N"] == 0 else s["K"] for s in systems]
    batch = _capi.Coulomb(ws, items)
    assert batch.launch_order == sorted(range(len(sizes)), key=lambda i: -sizes[i])
    batch.compute(_stream())
    torch.cuda.synchronize()
    ptr, offsets = batch.structure_device_ptr()
    assert ptr and offsets == list(np.cumsum([0] + [(0 if s["N"] == 0 else s["K"]) + 1 for s in systems])[:-1])
    trace, worst = {}, 0.0
    for k, s in enumerate(systems):
        want, bound = mirror.forces(s["x"], s["q"], s["box"], KAPPA, R_CUT, s["k_cut"], s["ex"], trace)
        got = force[k].cpu().numpy()[:s["N"]]
        assert got.shape == want.shape and np.isfinite(got).all(), k
        err = np.abs(got - want)
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        worst = max(worst, ratio)
        print(f"\nitem {k}: N = {s['N']}, K = {s['K']}, largest error / bound = {ratio:.4f}, largest error = {err.max() if s['N'] else 0:.3e}")
        assert (err <= bound).all(), (k, s["N"], s["K"], ratio)
        if s["N"] == 0:
            assert (force[k].cpu().numpy() == 7.0).all()                           # an empty item: nothing is written
        if s["N"] > 17:
            for i in (17, max(s["N"] // 2, 18)):                                   # no charge: an entry that compares equal to 0
                assert s["q"][i] == 0.0 and (got[i] == 0.0).all(), (k, i)
    print(f"\nlargest error / bound of the batch: {worst:.4f}")
    # every planted edge was met, by every system large enough to carry it
    big = sum(1 for n in sizes if n > 17)
    assert sum(1 for n in sizes if n > 19) >= 2                                    # or the counts below would ask for nothing
    assert trace["rsq_equals_rcutsq"] >= 2 * big and trace["just_inside_cutoff"] >= 2 * big
    assert trace["d_equals_plus_half"] >= big and trace["d_equals_minus_half"] >= big
    assert trace["excluded_pair_inside_cutoff"] >= 2 * big and trace["exclusion_across_boundary"] >= 2 * big
    assert trace["four_exclusions"] >= big and trace["zero_charge"] >= 2 * big
    # ... and behaved as the contract says: the first four planted particles alone, without a reciprocal part
    s = systems[sizes.index(501)]
    F, _ = mirror.forces(s["x"][:4], s["q"][:4], s["box"], KAPPA, R_CUT, 0.0)
    assert not F[0, :3].any() and not F[1, :3].any()                               # rsq == r_cut^2, and 0-2 / 1-3 are farther
    assert F[2, 0] != 0.0 and F[2, 0] == -F[3, 0]                                  # one ulp inside: the term is there
    # the exclusion removes the pair's whole Coulomb interaction: erf term and no erfc term
    two = mirror.forces(s["x"][8:10], [1.0, 1.0], s["box"], KAPPA, R_CUT, 0.0, [(0, 1)])[0]
    r = 1.2
    from scipy.special import erf
    assert np.isclose(two[:, 3].sum() + 2.0 * KAPPA / mirror.SQRT_PI + np.pi / (np.prod(s["box"]) * KAPPA ** 2) * 2.0,
                      -erf(KAPPA * r) / r, rtol=1e-13)
    if repeat:
        first = [f.cpu().numpy() for f in force]
        batch.compute(_stream())
        torch.cuda.synchronize()
        assert all(_same(f.cpu().numpy(), g) for f, g in zip(force, first))
    batch.close()
    ws.close()
    return worst
