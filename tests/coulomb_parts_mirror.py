"""The two parts of the Ewald sum (include/cavmd.h, "the two parts of the Ewald sum") restated in numpy: what
tests/test_gpu_coulomb_parts.py compares cavmd_mts_coulomb_compute_parts with, and what tests/test_coulomb_parts_abi.py holds to
tests/coulomb_mirror.py first.  Every expression is coulomb_mirror's; only the grouping is this file's.

short() and long() return F (n, 4) and a bound (n, 4) of coulomb_mirror's form, taken over the part's own absolute terms:
    short   2 eps (n + 16) abs_short                      abs_short: the erfc terms of the pairs inside the cut-off
    long    2 eps ((n + K) + 16 + phase) abs_long         abs_long: the erf terms of the exclusion partners, the reciprocal
                                                          terms, and in .w the self and background terms
n (+ K) covers worst-case summation on both sides in any order and 16 the few-ulp library functions, as in coulomb_mirror.  The
phase argument's rounding enters the reciprocal terms alone, so the short part carries neither K nor a phase term; for the
long part phase = 2 theta_max = 2 k_cut |x|_max under the direct method and G of tests/coulomb_factored_mirror.py under the
factored one.  abs_short + abs_long is coulomb_mirror's abs, so the two bounds sum to at most its bound.  Derived, not tuned
to any kernel."""
import numpy as np
from scipy.special import erf, erfc

import coulomb_factored_mirror as factored
import coulomb_mirror as mirror

EPS = mirror.EPS


def _pairs(x, q, box, exclusions):
    n = len(q)
    L = np.asarray(box, dtype=np.float64)
    ex = mirror.exclusion_matrix(n, exclusions)[0] if len(exclusions) else np.zeros((n, n), dtype=bool)
    d = mirror.min_image(x[:, None, :] - x[None, :, :], L)
    rsq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return ex, d, rsq, q[:, None] * q[None, :]


def short(x, q, box, kappa, r_cut, k_cut=0.0, exclusions=()):
    """-> (F (n, 4), bound (n, 4)) of SHORT; k_cut plays no part (the signature is coulomb_mirror.forces's)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    n = len(q)
    F, A = np.zeros((n, 4)), np.zeros((n, 4))
    if n == 0:
        return F, A
    ex, d, rsq, qq = _pairs(x, q, box, exclusions)
    inside = ~np.eye(n, dtype=bool) & ~ex & (rsq < r_cut * r_cut)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(rsq)
        g = (2.0 * kappa / mirror.SQRT_PI) * np.exp(-(kappa * r) ** 2)
        u_c = erfc(kappa * r) / r
        e = np.where(inside, qq * u_c, 0.0)
        fdivr = np.where(inside, qq * (u_c + g) / rsq, 0.0)
        e_abs = np.where(inside, np.abs(qq) * u_c, 0.0)
        f_abs = np.where(inside, np.abs(qq) * (u_c + g) / rsq, 0.0)
    F[:, :3] += (d * fdivr[..., None]).sum(axis=1)
    A[:, :3] += (np.abs(d) * f_abs[..., None]).sum(axis=1)
    F[:, 3] += 0.5 * e.sum(axis=1)
    A[:, 3] += 0.5 * e_abs.sum(axis=1)
    return F, 2.0 * EPS * (n + 16.0) * A


def long(x, q, box, kappa, r_cut, k_cut, exclusions=(), method="direct"):
    """-> (F (n, 4), bound (n, 4)) of LONG under `method` ("direct" or "factored"); r_cut plays no part"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    L = np.asarray(box, dtype=np.float64)
    n = len(q)
    F, A = np.zeros((n, 4)), np.zeros((n, 4))
    if n == 0:
        return F, A
    V = (L[0] * L[1]) * L[2]
    ex, d, rsq, qq = _pairs(x, q, box, exclusions)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(rsq)
        g = (2.0 * kappa / mirror.SQRT_PI) * np.exp(-(kappa * r) ** 2)
        u_f = erf(kappa * r) / r
        e = np.where(ex, -qq * u_f, 0.0)
        fdivr = np.where(ex, -qq * (u_f - g) / rsq, 0.0)
        e_abs = np.where(ex, np.abs(qq) * u_f, 0.0)
        f_abs = np.where(ex, np.abs(qq) * (u_f + g) / rsq, 0.0)
    F[:, :3] += (d * fdivr[..., None]).sum(axis=1)
    A[:, :3] += (np.abs(d) * f_abs[..., None]).sum(axis=1)
    F[:, 3] += 0.5 * e.sum(axis=1)
    A[:, 3] += 0.5 * e_abs.sum(axis=1)

    m, k, k2 = mirror.k_vectors(L, k_cut)
    K = len(k2)
    q_abs = np.abs(q).sum()
    if K:
        a_k = (4.0 * np.pi / V) * np.exp(-k2 / (4.0 * kappa * kappa)) / k2
        if method == "factored":
            c, s = factored.phases(x, box, m)
        else:
            theta = x @ k.T
            c, s = np.cos(theta), np.sin(theta)
        Sa, Sb = q @ c, q @ s
        w = a_k * (Sa * s - Sb * c)
        F[:, :3] += 2.0 * q[:, None] * (w @ k)
        F[:, 3] += q * ((a_k * (Sa * c + Sb * s)).sum(axis=1))
        A[:, :3] += np.abs(q)[:, None] * (a_k @ np.abs(k))[None, :] * q_abs
        A[:, 3] += np.abs(q) * a_k.sum() * q_abs
    Q = q.sum()
    F[:, 3] += -(kappa / mirror.SQRT_PI) * q * q - np.pi * q * Q / (2.0 * V * kappa * kappa)
    A[:, 3] += (kappa / mirror.SQRT_PI) * q * q + np.pi * np.abs(q) * q_abs / (2.0 * V * kappa * kappa)
    if method == "factored":
        phase = factored.phase_term(x, box, m)
    else:
        phase = 2.0 * k_cut * float(np.sqrt((x * x).sum(axis=1)).max())
    return F, 2.0 * EPS * ((n + K) + 16.0 + phase) * A


def self_and_background(q, box, kappa):
    """the .w terms lane 0 adds in the combined evaluation and in LONG -> (n,)"""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    L = np.asarray(box, dtype=np.float64)
    V = (L[0] * L[1]) * L[2]
    return -(kappa / mirror.SQRT_PI) * q * q - np.pi * q * q.sum() / (2.0 * V * kappa * kappa)
