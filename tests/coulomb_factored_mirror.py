"""The FACTORED reciprocal-space method of the Ewald Coulomb batch (include/cavmd.h, "the reciprocal-space method of a Coulomb
batch") restated in numpy with explicit real arithmetic: the base angles, the order and the number of the complex
multiplications are the header's.  Everything that is not cos(k.x) / sin(k.x) is tests/coulomb_mirror.py's.

forces() returns F (n, 4) and a bound (n, 4): coulomb_mirror.forces's bound
    2 eps ((n + K) + 16 + 2 theta_max) abs
with the phase term 2 theta_max replaced by G.  G bounds, in units of eps = 2^-52, the absolute error of cos theta and sin theta
as the factored method obtains them, against the exact phase of the exact product k1_c x_c; term by term:
  * phi_c = fl(k1_c * x_c) with k1_c = fl((2 pi * 1) / L_c): two roundings, each of relative size eps / 2, so
    |d phi_c| <= eps |phi_c|.  (2 pi * 1 is exact, and the double nearest 2 pi is the constant of both methods.)
  * E_c(1) = sincos(phi_c): the argument's error moves the point on the circle by |d phi_c|, and a few-ulp sincos adds at most
    eps per component (the direct bound's "16" covers the library functions; this eps is counted again here because it is
    amplified below).  So E_c(1) is off by at most eps (|phi_c| + 1).
  * E_c(m) is E_c(1) to the |m|-th power: an error d of the base grows to |m| d (first order, |E| = 1).  Over the three axes
    that is sum_c M_c (phi_max_c + 1) eps, with M_c the item's largest |m_c| and phi_max_c = k1_c max_j |x_c|.
  * every complex multiplication a * b = (a.re b.re - a.im b.im, a.re b.im + a.im b.re) rounds two products and one sum per
    component: |error| <= (eps / 2) (|a.re b.re| + |a.im b.im|) + (eps / 2) |result| <= eps |a| |b| per component (Cauchy-
    Schwarz), i.e. 1 eps for factors on the unit circle.  The stated constant is C_MUL = 2 eps per multiplication: 1 eps as
    derived and 1 eps for the factors' own moduli, which drift from 1 by at most the error already accumulated (< 1e-12 at
    the sizes the library accepts, so the second eps is generous by orders of magnitude).  The multiplications behind a phase
    number at most n_mul = Mx + My + Mz + SEG - 2 (the header's count, at its largest).
  G = sum_c M_c (phi_max_c + 1) + C_MUL n_mul.
An error e of cos / sin enters a reciprocal term twice, through S(k) (at most e sum_j |q_j|) and through particle i's own phase,
hence 2 e on the term's absolute value -- the factor 2 in front, as in the direct bound.  The bound is derived, not tuned to any
kernel."""
import numpy as np

import coulomb_mirror as mirror

EPS = mirror.EPS
SEGMENT = 8          # CAVMD_EWALD_SEGMENT (tests/test_ewald_reciprocal_abi.py compares with the library's)
C_MUL = 2.0          # eps per complex multiplication, see above


def segments(m):
    """The header's segments of the kept vectors m (K, 3) -> (start (K,) int64: for every k the index of its segment's first
    vector).  A row (mx, my) of consecutive mz is cut into runs of at most SEGMENT from its first mz on."""
    K = len(m)
    start = np.zeros(K, dtype=np.int64)
    for k in range(1, K):
        same_row = m[k, 0] == m[k - 1, 0] and m[k, 1] == m[k - 1, 1] and m[k, 2] == m[k - 1, 2] + 1
        start[k] = start[k - 1] if same_row and k - start[k - 1] < SEGMENT else k
    return start


def cmul(a, b):
    """(re, im) * (re, im), every operation rounded"""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def phases(x, box, m):
    """cos and sin of k.x as the factored method obtains them -> (c (n, K), s (n, K)).  Vectorised over particles, and over
    segments for the vectors at the same distance from their segment's start: the operations on every element are the
    header's, in its order."""
    n, K = len(x), len(m)
    cs, sn = np.zeros((n, K)), np.zeros((n, K))
    if K == 0:
        return cs, sn
    L = np.asarray(box, dtype=np.float64)
    tables = []
    for c in range(3):
        k1 = (mirror.TWO_PI * 1.0) / L[c]
        phi = k1 * x[:, c]
        e1 = (np.cos(phi), np.sin(phi))
        table = [(np.ones(n), np.zeros(n)), e1]
        for _ in range(2, int(np.abs(m[:, c]).max()) + 1):
            table.append(cmul(table[-1], e1))
        tables.append((np.array([t[0] for t in table]), np.array([t[1] for t in table])))    # (M + 1, n) each

    def power(c, mc):
        """E_c(mc) for an array of mc -> (re, im), each (len(mc), n)"""
        re, im = tables[c][0][np.abs(mc)], tables[c][1][np.abs(mc)]
        return re, np.where((mc < 0)[:, None], -im, im)

    start = segments(m)
    first = np.flatnonzero(start == np.arange(K))                                # the first vector of every segment
    segment_of = np.cumsum(start == np.arange(K)) - 1
    p = cmul(cmul(power(0, m[first, 0]), power(1, m[first, 1])), power(2, m[first, 2]))
    e1z = (tables[2][0][1][None, :], tables[2][1][1][None, :])
    for t in range(SEGMENT):
        at = np.flatnonzero(np.arange(K) - start == t)
        if len(at) == 0:
            break
        cs[:, at], sn[:, at] = p[0][segment_of[at]].T, p[1][segment_of[at]].T
        p = cmul(p, e1z)
    return cs, sn


def phase_term(x, box, m):
    """G of the module docstring"""
    L = np.asarray(box, dtype=np.float64)
    M = np.abs(m).max(axis=0) if len(m) else np.zeros(3)
    phi_max = (mirror.TWO_PI / L) * np.abs(x).max(axis=0)
    n_mul = max(float(M.sum()) + SEGMENT - 2.0, 0.0)
    return float((M * (phi_max + 1.0)).sum() + C_MUL * n_mul)


def values(x, q, box, kappa, r_cut, k_cut, exclusions=()):
    """F (n, 4) of the factored method, without the bound: what a host integrator asks at every step"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    L = np.asarray(box, dtype=np.float64)
    if len(q) == 0:
        return np.zeros((0, 4))
    # everything but the reciprocal sum: the direct mirror without k-vectors
    F = mirror.forces(x, q, box, kappa, r_cut, 0.0, exclusions)[0]
    m, k, k2 = mirror.k_vectors(L, k_cut)
    if len(k2):
        V = (L[0] * L[1]) * L[2]
        a_k = (4.0 * np.pi / V) * np.exp(-k2 / (4.0 * kappa * kappa)) / k2
        c, s = phases(x, box, m)
        Sa, Sb = q @ c, q @ s
        w = a_k * (Sa * s - Sb * c)
        F[:, :3] += 2.0 * q[:, None] * (w @ k)
        F[:, 3] += q * ((a_k * (Sa * c + Sb * s)).sum(axis=1))
    return F


def forces(x, q, box, kappa, r_cut, k_cut, exclusions=(), direct=None):
    """-> (F (n, 4), bound (n, 4)).  `direct`: what coulomb_mirror.forces returned for the same arguments, if the caller has it."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    n = len(q)
    if n == 0:
        return np.zeros((0, 4)), np.zeros((0, 4))
    F = values(x, q, box, kappa, r_cut, k_cut, exclusions)
    m = mirror.k_vectors(box, k_cut)[0]
    K = len(m)
    # the direct bound with its phase term replaced: abs = bound / (2 eps (...)) is the sum of the terms' absolute values
    _, bound = mirror.forces(x, q, box, kappa, r_cut, k_cut, exclusions) if direct is None else direct
    theta_max = k_cut * float(np.sqrt((x * x).sum(axis=1)).max())
    absolute = bound / (2.0 * EPS * ((n + K) + 16.0 + 2.0 * theta_max))
    return F, 2.0 * EPS * ((n + K) + 16.0 + phase_term(x, box, m)) * absolute


def structure_factors(x, q, box, k_cut, method="factored"):
    """S(k) = sum_j q_j exp(i k.x_j) of either method -> (S (K, 2), bound: one number for every slot and both components).
    The bound is the force bound's reasoning for one sum of n terms q_j cos theta_j: eps ((n + 16) + phase) sum_j |q_j|, where
    (n + 16) eps covers the summation in any order and the few-ulp functions as in coulomb_mirror, and the phase error of one
    cos / sin -- 2 theta_max eps for the direct method (coulomb_mirror's term), G eps for the factored one -- enters once, not
    twice as in a force term."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    m, k, _ = mirror.k_vectors(box, k_cut)
    n, K = len(q), len(m)
    if n == 0 or K == 0:
        return np.zeros((K, 2)), 0.0
    if method == "factored":
        c, s = phases(x, box, m)
        phase = phase_term(x, box, m)
    else:
        theta = x @ k.T
        c, s = np.cos(theta), np.sin(theta)
        phase = 2.0 * k_cut * float(np.sqrt((x * x).sum(axis=1)).max())
    return np.stack([q @ c, q @ s], axis=1), EPS * ((n + 16.0) + phase) * float(np.abs(q).sum())
