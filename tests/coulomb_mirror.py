"""The Ewald Coulomb contract of include/cavmd.h (section "Ewald Coulomb forces of a batch") restated in numpy, with
scipy.special.erfc / erf: what tests/test_gpu_coulomb_batch.py compares the kernels with, and what tests/test_coulomb_abi.py
checks against physics first (the Madelung constant, kappa-independence, F = -dE/dx).

forces() returns F (n, 4) and, computed alongside, a bound (n, 4) on what a correct evaluation in fp64 may differ by:
    bound = 2 eps ((n + K) + 16 + 2 theta_max) abs
abs is the sum of the absolute values of all terms that enter the component (for the reciprocal part |q_i| a_k |k_c| sum_j |q_j|,
in .w without |k_c|); (n + K) covers worst-case summation on both sides in any order, 16 the few-ulp library functions (erfc,
erf, exp, sincos, sqrt, the divisions), and 2 theta_max = 2 k_cut |x|_max the amplification of the phase argument's rounding.
The bound is derived, not tuned to any kernel."""
import numpy as np
from scipy.special import erf, erfc

EPS = 2.0 ** -52
TWO_PI = 2.0 * 3.141592653589793
SQRT_PI = 1.7724538509055159
MAX_EXCLUSIONS = 4


def k_vectors(box, k_cut):
    """The kept k-vectors in the contract's order (mx, then my, then mz ascending) -> (m (K, 3) int64, k (K, 3), k2 (K,)).
    k_c = (2 pi m_c) / L_c and k2 = (kx kx + ky ky) + kz kz in the library's operations, so the kept set is the library's."""
    L = np.asarray(box, dtype=np.float64)
    M = [int(k_cut * l / TWO_PI) + 1 for l in L]
    mx, my, mz = np.meshgrid(np.arange(0, M[0] + 1), np.arange(-M[1], M[1] + 1), np.arange(-M[2], M[2] + 1), indexing="ij")
    m = np.stack([mx.ravel(), my.ravel(), mz.ravel()], axis=1).astype(np.int64)
    half = (m[:, 0] > 0) | ((m[:, 0] == 0) & (m[:, 1] > 0)) | ((m[:, 0] == 0) & (m[:, 1] == 0) & (m[:, 2] > 0))
    k = (TWO_PI * m.astype(np.float64)) / L
    k2 = (k[:, 0] * k[:, 0] + k[:, 1] * k[:, 1]) + k[:, 2] * k[:, 2]
    keep = half & (k2 > 0.0) & (k2 <= k_cut * k_cut)
    return m[keep], k[keep], k2[keep]


def k_cut_for(box, K):
    """A k_cut that keeps exactly K vectors of `box` (K >= 0), between the K-th and the (K + 1)-th k2 of the half space; None
    if they are equal (k2 does not change with the signs of my and mz, so the counts a k_cut can reach come in shells)."""
    if K == 0:
        return 0.0
    guess = (12.0 * np.pi ** 2 * (K + 64) / float(np.prod(box))) ** (1.0 / 3.0) * 1.5 + TWO_PI / min(box)
    k2 = np.sort(k_vectors(box, guess)[2])
    assert len(k2) > K
    if not k2[K] > k2[K - 1] * (1.0 + 1e-9):
        return None
    k_cut = float(np.sqrt(0.5 * (k2[K - 1] + k2[K])))
    assert len(k_vectors(box, k_cut)[2]) == K
    return k_cut


def box_and_k_cut_for(box, K, tries=2000):
    """(box', k_cut) with exactly K kept vectors: Ly and Lz of `box` are stretched by up to a half (drawn from a generator
    seeded with K; the first try is `box` itself) until a shell boundary falls after exactly K vectors."""
    rng = np.random.default_rng(K)
    for t in range(tries):
        s = rng.uniform(1.0, 1.5, 2) if t else (1.0, 1.0)
        b = (float(box[0]), float(box[1]) * float(s[0]), float(box[2]) * float(s[1]))
        k_cut = k_cut_for(b, K)
        if k_cut is not None:
            return b, k_cut
    raise AssertionError(f"no box near {box} keeps exactly {K} k-vectors")


def min_image(d, L):
    h = L * 0.5
    return np.where(d >= h, d - L, np.where(d < -h, d + L, d))


def exclusion_matrix(n, exclusions):
    ex = np.zeros((n, n), dtype=bool)
    count = np.zeros(n, dtype=np.int64)
    pairs = np.asarray(exclusions, dtype=np.int64)
    pairs = pairs.reshape(-1, pairs.shape[-1] if pairs.ndim == 2 else 2)[:, :2]      # a third column (a bond type) is ignored
    for a, b in pairs:
        ex[a, b] = ex[b, a] = True
        count[a] += 1
        count[b] += 1
    assert count.max(initial=0) <= MAX_EXCLUSIONS
    return ex, count


def forces(x, q, box, kappa, r_cut, k_cut, exclusions=(), trace=None):
    """-> (F (n, 4), bound (n, 4)).  `trace`, if given, counts the edges of the contract this system met."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    L = np.asarray(box, dtype=np.float64)
    n = len(q)
    F, A = np.zeros((n, 4)), np.zeros((n, 4))
    if n == 0:
        return F, A
    V = (L[0] * L[1]) * L[2]
    ex, ex_count = exclusion_matrix(n, exclusions) if len(exclusions) else (np.zeros((n, n), dtype=bool), np.zeros(n, dtype=np.int64))
    raw = x[:, None, :] - x[None, :, :]
    d = min_image(raw, L)
    rsq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    other = ~np.eye(n, dtype=bool)
    inside = other & ~ex & (rsq < r_cut * r_cut)
    qq = q[:, None] * q[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(rsq)
        g = (2.0 * kappa / SQRT_PI) * np.exp(-(kappa * r) ** 2)
        u_c, u_f = erfc(kappa * r) / r, erf(kappa * r) / r
        e = np.where(inside, qq * u_c, np.where(ex, -qq * u_f, 0.0))
        fdivr = np.where(inside, qq * (u_c + g) / rsq, np.where(ex, -qq * (u_f - g) / rsq, 0.0))
        e_abs = np.where(inside, np.abs(qq) * u_c, np.where(ex, np.abs(qq) * u_f, 0.0))
        f_abs = np.where(inside, np.abs(qq) * (u_c + g) / rsq, np.where(ex, np.abs(qq) * (u_f + g) / rsq, 0.0))
    F[:, :3] += (d * fdivr[..., None]).sum(axis=1)
    A[:, :3] += (np.abs(d) * f_abs[..., None]).sum(axis=1)
    F[:, 3] += 0.5 * e.sum(axis=1)
    A[:, 3] += 0.5 * e_abs.sum(axis=1)

    m, k, k2 = k_vectors(L, k_cut)
    K = len(k2)
    q_abs = np.abs(q).sum()
    if K:
        a_k = (4.0 * np.pi / V) * np.exp(-k2 / (4.0 * kappa * kappa)) / k2
        theta = x @ k.T                                                     # (n, K)
        c, s = np.cos(theta), np.sin(theta)
        Sa, Sb = q @ c, q @ s                                               # (K,)
        w = a_k * (Sa * s - Sb * c)                                         # (n, K)
        F[:, :3] += 2.0 * q[:, None] * (w @ k)
        F[:, 3] += q * ((a_k * (Sa * c + Sb * s)).sum(axis=1))
        A[:, :3] += np.abs(q)[:, None] * (a_k @ np.abs(k))[None, :] * q_abs
        A[:, 3] += np.abs(q) * a_k.sum() * q_abs
    Q = q.sum()
    F[:, 3] += -(kappa / SQRT_PI) * q * q - np.pi * q * Q / (2.0 * V * kappa * kappa)
    A[:, 3] += (kappa / SQRT_PI) * q * q + np.pi * np.abs(q) * q_abs / (2.0 * V * kappa * kappa)
    theta_max = k_cut * float(np.sqrt((x * x).sum(axis=1)).max())
    bound = 2.0 * EPS * ((n + K) + 16.0 + 2.0 * theta_max) * A

    if trace is not None:
        def add(name, v):
            trace[name] = trace.get(name, 0) + int(v)
        h = L * 0.5
        add("rsq_equals_rcutsq", (other & ~ex & (rsq == r_cut * r_cut)).sum())
        add("just_inside_cutoff", (inside & (rsq >= np.nextafter(r_cut, 0.0) ** 2 * (1.0 - 4.0 * EPS))).sum())
        add("d_equals_plus_half", (other[..., None] & (raw == h)).sum())
        add("d_equals_minus_half", (other[..., None] & (raw == -h)).sum())
        add("excluded_pair_inside_cutoff", (ex & (rsq < r_cut * r_cut)).sum())
        add("excluded_pair_beyond_cutoff", (ex & (rsq >= r_cut * r_cut)).sum())
        add("exclusion_across_boundary", (ex[..., None] & (raw != d)).any(axis=2).sum())
        add("four_exclusions", (ex_count == MAX_EXCLUSIONS).sum())
        add("zero_charge", (q == 0.0).sum())
    return F, bound


def energy(x, q, box, kappa, r_cut, k_cut, exclusions=()):
    return float(forces(x, q, box, kappa, r_cut, k_cut, exclusions)[0][:, 3].sum())
