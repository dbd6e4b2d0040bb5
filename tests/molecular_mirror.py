"""A numpy mirror of the molecular force contract of include/cavmd.h (cavmd_molecular_*): harmonic bonds and Lennard-Jones
pairs under the minimum image, with the published summation order.  Element-wise numpy only -- numpy's element-wise operations
round once each and do not fuse -- vectorised over i, with an explicit Python loop over j in the published order: partial
s = j % S collects j = s, s + S, ... left to right, P = ((p0 + p1) + p2) + ..., F = B + P.  S comes from the library
(``_capi.molecular_order()``): it is part of the contract, not of the kernel's tuning."""
import numpy as np

MAX_BONDS = 4


def pair_constants(epsilon, sigma, r_cut, shift=True):
    """cavmd_molecular_pair_make, operation by operation -> (lj1, lj2, lj1_12, lj2_6, rcutsq, eshift)"""
    epsilon, sigma, r_cut = np.float64(epsilon), np.float64(sigma), np.float64(r_cut)
    s2 = sigma * sigma
    s6 = (s2 * s2) * s2
    lj2 = (np.float64(4.0) * epsilon) * s6
    lj1 = lj2 * s6
    lj1_12 = np.float64(12.0) * lj1
    lj2_6 = np.float64(6.0) * lj2
    rcutsq = r_cut * r_cut
    eshift = np.float64(0.0)
    if shift and rcutsq > 0.0:
        r2inv = np.float64(1.0) / rcutsq
        r6inv = (r2inv * r2inv) * r2inv
        eshift = r6inv * ((lj1 * r6inv) - lj2)
    return lj1, lj2, lj1_12, lj2_6, rcutsq, eshift


def tables(params):
    """The constants of a ``_capi.MolecularParams``, bit for bit, as arrays: the mirror starts from the library's bits."""
    names = ("lj1", "lj2", "lj1_12", "lj2_6", "rcutsq", "eshift")
    out = {name: np.array([[getattr(params.pair[a][b], name) for b in range(8)] for a in range(8)], dtype=np.float64)
           for name in names}
    out["n_types"], out["n_bond_types"] = int(params.n_types), int(params.n_bond_types)
    out["K"] = np.array([params.bond[k].K for k in range(8)], dtype=np.float64)
    out["r0"] = np.array([params.bond[k].r0 for k in range(8)], dtype=np.float64)
    return out


def partner_table(n, bonds):
    """(partner, bond type), each (n, 4), -1 where empty: the bonds that name a particle, in list order."""
    partner = np.full((n, MAX_BONDS), -1, dtype=np.int64)
    btype = np.zeros((n, MAX_BONDS), dtype=np.int64)
    count = np.zeros(n, dtype=np.int64)
    for a, b, t in np.asarray(bonds, dtype=np.int64).reshape(-1, 3):
        for me, other in ((a, b), (b, a)):
            partner[me, count[me]] = other
            btype[me, count[me]] = t
            count[me] += 1
    return partner, btype


def min_image(d, L):
    h = L * 0.5
    return np.where(d >= h, d - L, np.where(d < -h, d + L, d))


def forces(position, typeid, box, tab, bonds, S, trace=None):
    """(N, 4): force and the particle's share of the energy.  position (N, 3) wrapped, typeid (N,) integers as stored in
    pos.w, bonds (n_b, 3).  trace: a dict that receives counts of the edge cases met (for tests that plant them)."""
    x = np.ascontiguousarray(position, dtype=np.float64)
    n = x.shape[0]
    L = [np.float64(v) for v in box]
    t = np.asarray(typeid, dtype=np.int64) & 0xFFFFFFFF           # the kernel compares type ids as unsigned
    typed = t < tab["n_types"]
    tc = np.where(typed, t, 0)
    partner, btype = partner_table(n, bonds)
    idx = np.arange(n)
    seen = {"rsq_equals_rcutsq": 0, "just_inside_cutoff": 0, "d_equals_plus_half": 0, "d_equals_minus_half": 0,
            "bonded_pair_inside_cutoff": 0, "bond_across_boundary": 0, "four_bonds": int(np.count_nonzero(partner[:, 3] >= 0)),
            "unlisted_pair": 0, "type_out_of_range": int(np.count_nonzero(~typed))}
    p = np.zeros((S, n, 4))
    with np.errstate(all="ignore"):
        for j in range(n):
            s = j % S
            raw = [x[:, c] - x[j, c] for c in range(3)]
            d = [min_image(raw[c], L[c]) for c in range(3)]
            rsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            bonded = (partner == j).any(axis=1)
            eligible = (idx != j) & ~bonded & typed & bool(typed[j])
            rc = tab["rcutsq"][tc, tc[j]]
            ok = eligible & (rsq < rc)
            if trace is not None:
                seen["rsq_equals_rcutsq"] += int(np.count_nonzero(eligible & (rsq == rc) & (rc > 0)))
                seen["just_inside_cutoff"] += int(np.count_nonzero(ok & (rsq > rc - 4 * np.spacing(rc))))
                seen["unlisted_pair"] += int(np.count_nonzero(eligible & (rc == 0)))
                seen["bonded_pair_inside_cutoff"] += int(np.count_nonzero(bonded & typed & bool(typed[j]) & (rsq < rc)))
                for c in range(3):
                    seen["d_equals_plus_half"] += int(np.count_nonzero(eligible & (raw[c] == L[c] * 0.5)))
                    seen["d_equals_minus_half"] += int(np.count_nonzero(eligible & (raw[c] == -(L[c] * 0.5))))
            r2inv = 1.0 / rsq
            r6inv = (r2inv * r2inv) * r2inv
            fdivr = (r2inv * r6inv) * ((tab["lj1_12"][tc, tc[j]] * r6inv) - tab["lj2_6"][tc, tc[j]])
            e = r6inv * ((tab["lj1"][tc, tc[j]] * r6inv) - tab["lj2"][tc, tc[j]]) - tab["eshift"][tc, tc[j]]
            for c in range(3):
                p[s, :, c] = np.where(ok, p[s, :, c] + d[c] * fdivr, p[s, :, c])
            p[s, :, 3] = np.where(ok, p[s, :, 3] + 0.5 * e, p[s, :, 3])
        P = p[0].copy()
        for s in range(1, S):
            P = P + p[s]
        B = np.zeros((n, 4))
        for k in range(MAX_BONDS):
            has = partner[:, k] >= 0
            if n == 0 or not has.any():
                continue
            q = np.where(has, partner[:, k], 0)
            raw = [x[:, c] - x[q, c] for c in range(3)]
            d = [min_image(raw[c], L[c]) for c in range(3)]
            seen["bond_across_boundary"] += int(np.count_nonzero(has & np.any([d[c] != raw[c] for c in range(3)], axis=0)))
            rsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            K, r0 = tab["K"][btype[:, k]], tab["r0"][btype[:, k]]
            r = np.sqrt(rsq)
            fdivr = K * (r0 / r - 1.0)
            e = (0.5 * K) * ((r0 - r) * (r0 - r))
            for c in range(3):
                B[:, c] = np.where(has, B[:, c] + d[c] * fdivr, B[:, c])
            B[:, 3] = np.where(has, B[:, 3] + 0.5 * e, B[:, 3])
        F = B + P
    if trace is not None:
        for name, count in seen.items():
            trace[name] = trace.get(name, 0) + count
    return F
