"""The inputs tests/test_gpu_device_start.py runs on the device -- a batch started by ``BatchThermalizer`` and taken through its
first steps by the other batch objects -- built from seeds with numpy alone, so that tests/test_device_start_twin.py can
rehearse them on a machine WITHOUT a GPU; and, next to them, the bounds and bands both files assert, each with its derivation.
Importing this module touches no GPU.

  1. the photon placed at finite q against the cavity force kernel's zero: five systems and three rounding bounds;
  2. the documented start, eager and from a graph: two diatomic lattices;
  3. the first ledger row of a device start: 256 systems and three analytic means with their six-sigma bands;
  4. the ledger's system_total from a device start: 12 charged dimers."""
import numpy as np

import thermalize_cases as cases
import thermalize_mirror as mirror

EPS = 2.0 ** -52                    # the spacing of doubles at 1; one correctly rounded operation errs by at most u = EPS / 2
assert EPS == mirror.EPS


# ---- 1. the displaced equilibrium ----------------------------------------------------------------------------------------------------
# The four photon systems of thermalize_cases and one more whose larger couplstr carries the photon far outside the box.
IMAGES_SYSTEM = ("g_images", 96, 5e-3, True)
PLACED_SYSTEMS = cases.PHOTON_SYSTEMS + (IMAGES_SYSTEM,)
PLACED_SEED = 20261021
LIVENESS = 2.0 ** 20

# The bounds.  u = EPS / 2; d is the dipole of the result block (the same bits in the thermalizer and in the force kernel: the
# photon is not part of it); delta_k are single roundings, |delta_k| <= u; second-order terms are left to the slack between
# the first-order constant and the c chosen.
#
#   placement (thermalize item 4, kT = 0 so the spread is an exact zero):
#       x   = fl(fl((-d) g) / K)                = -(g d / K)(1 + delta_1)(1 + delta_2)
#       S   = fl(i L)                            the same double in the thermalizer and in the force kernel
#       pos = fl(x - S)                         = (x - S)(1 + delta_3)
#   the force kernel (cavmd.h:64, r = pos + image * L):
#       q   = fl(pos + S)                       = (pos + S)(1 + delta_4)
#   With i = 0: S = 0 and q = x exactly.  With i != 0: |x| >= L / 2 >= |pos| (up to a rounding), so
#       |q - x| <= u |pos| + u |q| <= 2 u |x|,  q = x (1 + theta),  |theta| <= 2 u,   K q = -(g d)(1 + eta),  |eta| <= 4 u.
#
#   F_L,c = fl(fl(-K q) - fl(g d)) (cavmd.h:71)   = [(g d)(1 + eta)(1 + delta_5) - (g d)(1 + delta_6)](1 + delta_7)
#       |F_L,c| <= (4 + 1 + 1) u |g d| = 6 u |g d| = 3 u (|K q| + |g d|) = 1.5 EPS (|K q| + |g d|):            c = 2
#       (a fused multiply-add drops delta_5 or delta_6 and only lowers this.)
C_PHOTON = 2
#   Dq_c = fl(q + fl(fl(g / K) d)) (cavmd.h:70) = [-(g d / K)(1 + delta_1)(1 + delta_2)(1 + theta) + (g d / K)(1 + delta_a)(1 + delta_b)](1 + delta_c)
#       |Dq_c| <= (1 + 1 + 2 + 1 + 1) u |g d / K| = 6 u |q_c|;  F_i,c = fl(fl(-g c_i) Dq_c) adds two relative roundings:
#       |F_i,c| <= 6 u g |c_i| |q_c| (1 + 2 u) = 3 EPS g |c_i| |q_c| (1 + 2 u):                                  c = 4
C_MOLECULAR = 4
#   the energies (cavmd.h:68), with q_c = -(g / K) d_c (1 + eta_c): in real arithmetic E_h = sum_c E_d,c (1 + eta_c)^2,
#   E_c = -2 sum_c E_d,c (1 + eta_c), so E_h + E_c + E_d = sum_c E_d,c eta_c^2, second order.  What is left is the rounding
#   of the three evaluations, none of which cancels inside (q_c d_c < 0 in both components, q_z = 0 exactly):
#       E_h = fl((0.5 K)(q_x q_x + q_y q_y + 0))          two products, one sum, one product (0.5 K is exact): 3 u E_d
#       E_c = fl(g (d_x q_x + d_y q_y + 0))                the same count on |E_c| = 2 E_d:                      6 u E_d
#       E_d = fl((0.5 fl(fl(g g) / K))(d_x d_x + d_y d_y + 0))   two more for g g / K:                          5 u E_d
#       (E_h + E_c) + E_d                                  one rounding of about -E_d, then an exact difference:   u E_d
#       |E_h + E_c + E_d| <= 15 u E_d = 7.5 EPS E_d:                                                             c = 8
C_ENERGY = 8


def placed_configs():
    """(name, snapshot dict, velocities (N, 4)) per system of PLACED_SYSTEMS: thermalize_cases' four, then the fifth built the
    same way; the photon, where there is one, is the LAST particle and has the mass params['phmass'] = 1"""
    from cavitymd import synthetic
    out = list(cases.photon_configs())
    name, n_molecular, g, _ = IMAGES_SYSTEM
    cfg = synthetic.random_charged_box(n_molecular, seed=100 + len(out), params=synthetic.default_params(couplstr=g))
    rng = np.random.default_rng(12)
    n = len(cfg["typeid"])
    vel = np.zeros((n, 4))
    vel[:, :3] = rng.normal(0.0, 1.0, (n, 3))
    vel[:, 3] = rng.uniform(1.0, 30.0, n)
    vel[-1, 3] = cfg["params"]["phmass"]
    out.append((name, cfg, vel))
    return out


def spring_constant(params) -> float:
    from cavitymd import _capi
    return float(_capi.make_params(params["omegac"], params["couplstr"], params["phmass"]).K)


def equilibrium(cfg, dipole=None):
    """(x, image) of the photon placed at finite q with kT = 0 -- item 4's expressions on `dipole` (default: the host's)"""
    d = np.asarray(cases.host_dipole(cfg) if dipole is None else dipole, dtype=np.float64)
    x = ((-d) * np.float64(cfg["params"]["couplstr"])) / np.float64(spring_constant(cfg["params"]))
    x[2] = 0.0
    _, i, _ = mirror.wrap(x, np.asarray(cfg["box"], dtype=np.float64))
    return x, i.astype(np.int64)


def images_cover_both_signs_and_two_boxes(images) -> bool:
    """over a batch's photon images: some component <= -1, some >= +1, some |i| >= 2"""
    i = np.concatenate([np.asarray(x).reshape(-1) for x in images])
    return bool((i <= -1).any() and (i >= 1).any() and (np.abs(i) >= 2).any())


def photon_force_bound(K, g, q, d):
    """(2,) on |photon_force[c]|, c = 0, 1, from the evaluation's own q and d"""
    q, d = np.asarray(q, dtype=np.float64), np.asarray(d, dtype=np.float64)
    return C_PHOTON * EPS * (np.abs(K * q[:2]) + np.abs(g * d[:2]))


def molecular_force_bound(g, charge, q):
    """(n, 2) on the x and y components of the cavity force on the molecules"""
    q = np.asarray(q, dtype=np.float64)
    return C_MOLECULAR * EPS * abs(g) * np.abs(np.asarray(charge, dtype=np.float64))[:, None] * np.abs(q[:2])[None, :]


def energy_bound(E_d) -> float:
    return C_ENERGY * EPS * float(E_d)


# ---- 2. the documented start --------------------------------------------------------------------------------------------------------
START_LATTICES = ((3, 41), (2, 42))        # (n_side, seed): N = 55 and 17
START_SPACING = 8.0
START_COUPLING = 4e-3                      # carries the displaced equilibrium of both lattices outside their boxes
START_SEED = 77
START_DT = 10.0
START_ULPS = 4                             # "a few ulp of |image| * L" in the bound on the photon's unwrapped move


def start_lattices():
    from cavitymd import synthetic
    cfgs = [synthetic.diatomic_lattice(n, START_SPACING, seed=s, params=synthetic.default_params(couplstr=START_COUPLING))
            for n, s in START_LATTICES]
    bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
    return cfgs, [b[0] for b in bonds], [b[1] for b in bonds]


# ---- 3. the first ledger row ----------------------------------------------------------------------------------------------------------
LEDGER_B, LEDGER_N, LEDGER_G, LEDGER_SEED = 256, 40, 1e-3, 9
LEDGER_KT = cases.KT
LEDGER_DOF = 3 * LEDGER_N - 3


def ledger_configs():
    """(snapshot dict, velocities (41, 4) with zero velocities) per system: masses uniform in (1, 30), the photon's phmass"""
    from cavitymd import synthetic
    rng = np.random.default_rng(17)
    out = []
    for k in range(LEDGER_B):
        cfg = synthetic.random_charged_box(LEDGER_N, seed=k, params=synthetic.default_params(couplstr=LEDGER_G))
        vel = np.zeros((LEDGER_N + 1, 4))
        vel[:, 3] = rng.uniform(1.0, 30.0, LEDGER_N + 1)
        vel[-1, 3] = cfg["params"]["phmass"]
        out.append((cfg, vel))
    return out


def ledger_expectations(masses, kT=LEDGER_KT):
    """name -> (expected mean over the batch, six standard errors of that mean); masses: (B, n), the molecules' alone.

    cavity_potential.  E_h + E_c + E_d = (K / 2)((q_x + g d_x / K)^2 + (q_y + g d_y / K)^2 + q_z^2) = (K / 2) |q - q_eq|^2, and
    the start puts q - q_eq = sqrt(kT / K) n with three standard normals: (kT / 2) chi^2_3, mean (3 / 2) kT, variance
    (kT / 2)^2 * 3 * 2 = (3 / 2) kT^2.
    kinetic_cavity.  v = sqrt(kT / m) n: (m / 2) |v|^2 = (kT / 2) chi^2_3 again.
    kinetic_group.  Per component p_i = m_i v_i = sqrt(m_i kT) n_i, P = sum_j p_j, and the header's rule leaves
    p_i' = p_i - P / n (P / n off every MOMENTUM, not P / M off every velocity).  var p_i' = m_i kT (1 - 2 / n) + (sum_j m_j) kT / n^2,
    so E sum_i p_i'^2 / (2 m_i) = (kT / 2)((n - 2) + (sum m)(sum 1 / m) / n^2) per component, three components:
        (3 kT / 2)((n - 2) + (sum m)(sum 1 / m) / n^2),
    which is (3 / 2)(n - 1) kT only for equal masses (Cauchy-Schwarz: (sum m)(sum 1 / m) >= n^2).  Its band takes the variance
    of 3 (n - 1) independent squares (kT / 2) chi^2_1, each of variance kT^2 / 2; the O(1 / n) correction of that variance
    is far inside six sigma."""
    masses = np.asarray(masses, dtype=np.float64)
    B, n = masses.shape
    chi3 = 6.0 * np.sqrt(1.5) * kT / np.sqrt(B)
    group = 1.5 * kT * ((n - 2) + masses.sum(axis=1) * (1.0 / masses).sum(axis=1) / n ** 2)
    return {"cavity_potential": (1.5 * kT, chi3), "kinetic_cavity": (1.5 * kT, chi3),
            "kinetic_group": (float(group.mean()), 6.0 * np.sqrt(1.5 * (n - 1)) * kT / np.sqrt(B))}


def temperature(kinetic_group, dof, kB):
    """the header's expression, one rounding per operation"""
    return (np.float64(2.0) * np.asarray(kinetic_group, dtype=np.float64)) / (np.float64(dof) * np.float64(kB))


# ---- 4. the conserved column ---------------------------------------------------------------------------------------------------------
DIMERS_SEED = 31
DIMERS_R_CUT, DIMERS_ACCURACY = 12.0, 1e-8
DRIFT_DT, DRIFT_STEPS = 10.0, 200          # and DRIFT_DT / 2 over 2 * DRIFT_STEPS: the twin's ratio is in [3.5, 4.5] at these
DRIFT_SEED = 4


def dimers_config(seed=DIMERS_SEED):
    """12 charged dimers and the photon: the first 12 molecules of a 3 x 3 x 3 lattice, in its 24-bohr box -- the host arrays
    of `_dimers` of tests/test_gpu_coulomb_batch.py, expression for expression -> (snapshot dict, bonds, bond_typeid)"""
    from cavitymd import synthetic
    c = synthetic.diatomic_lattice(3, 8.0, seed=seed)
    keep = list(range(24)) + [len(c["charge"]) - 1]
    c = dict(c, position=c["position"][keep], typeid=c["typeid"][keep], charge=c["charge"][keep], image=c["image"][keep])
    bonds, bond_typeid = synthetic.diatomic_bonds(c)
    return c, bonds, bond_typeid
