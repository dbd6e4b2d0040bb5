"""The inputs tests/test_gpu_thermalize_batch.py runs on the device, built from seeds with numpy alone, so that
tests/test_thermalize_abi.py can hold the mirror (tests/thermalize_mirror.py) to the same bands and rule out an ambiguous wrap
on a machine WITHOUT a GPU.  Importing this module touches no GPU."""
import numpy as np

import thermalize_mirror as mirror

T = mirror.TILE
KT = 9.5e-4
SEED = 20261020

# ---- 1. the ragged batch: every size at which the kernel takes another path, every member variant, planted masses ---------------
SIZES = (1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 0)
VARIANTS = ("null", "null", "subset", "planted", "empty", "beyond", "null", "subset_planted", "null", "null")
BEYOND = 3                         # entries of the "beyond" list at or past N
PLANTED = 4                        # masses 0, negative, NaN, infinite


def flags(zero_momentum=False, place_photon=False, finite_q=False, photon_velocity=True):
    return dict(zero_momentum=zero_momentum, place_photon=place_photon, finite_q=finite_q, photon_velocity=photon_velocity)


def ragged():
    """one mirror item per system of the ragged batch, without a result block; item k draws under item_key(SEED, k)"""
    rng = np.random.default_rng(7)
    systems = []
    for k, (n, variant) in enumerate(zip(SIZES, VARIANTS)):
        vel = np.zeros((n, 4))
        vel[:, :3] = rng.normal(0.0, 1.0, (n, 3))                  # what an untouched row keeps
        vel[:, 3] = rng.uniform(1.0, 30.0, n)
        members = None
        if variant in ("subset", "subset_planted"):
            members = rng.permutation(n)[:n // 3]
        elif variant == "empty":
            members = np.zeros(0, dtype=np.int64)
        elif variant == "beyond":
            members = rng.permutation(np.concatenate([rng.permutation(n)[:100], [n, n + 7, 70000]]))
        if variant in ("planted", "subset_planted"):
            bad = np.array([3, n // 2, n - 2, 7])
            vel[bad, 3] = [0.0, -2.0, np.nan, np.inf]
            if members is not None:
                members = rng.permutation(np.union1d(members, bad))
        if members is not None:
            members = members.astype(np.uint32)
        systems.append(dict(N=n, vel=vel, members=members, kT=KT * (1.0 + 0.125 * k), seed=mirror.item_key(SEED, k), result=None,
                            **flags()))
    return systems


# ---- 3. the photon: q = 0 and finite q, g = 0 and g != 0, no photon ----------------------------------------------------------------
PHOTON_SYSTEMS = (("g", 40, 1e-3, True), ("g0", 41, 0.0, True), ("no_photon", 64, 1e-3, False), ("g_large", 513, 2e-3, True))


def photon_configs():
    """(name, snapshot dict of cavitymd.synthetic, velocities (N, 4)) per system; the photon, where there is one, is the LAST
    particle and has the mass params['phmass'] = 1"""
    from cavitymd import synthetic
    rng = np.random.default_rng(11)
    out = []
    for k, (name, n_molecular, g, has_photon) in enumerate(PHOTON_SYSTEMS):
        cfg = synthetic.random_charged_box(n_molecular, seed=100 + k, params=synthetic.default_params(couplstr=g))
        if not has_photon:
            cfg = dict(cfg, position=cfg["position"][:-1], typeid=cfg["typeid"][:-1], charge=cfg["charge"][:-1],
                       image=cfg["image"][:-1], types=["O", "N"])
        n = len(cfg["typeid"])
        vel = np.zeros((n, 4))
        vel[:, :3] = rng.normal(0.0, 1.0, (n, 3))
        vel[:, 3] = rng.uniform(1.0, 30.0, n)
        if has_photon:
            vel[-1, 3] = cfg["params"]["phmass"]
        out.append((name, cfg, vel))
    return out


def host_dipole(cfg):
    """the molecular dipole as the driver takes it (:458-460), photon excluded: what the device's result block holds up to
    the rounding of the sum"""
    box = np.asarray(cfg["box"])
    molecular = np.asarray(cfg["typeid"]) != cfg["L_typeid"]
    unwrapped = cfg["position"] + cfg["image"] * box[None, :]
    return np.einsum("i,ij->j", cfg["charge"][molecular], unwrapped[molecular])


def photon_item(cfg, vel, key, dipole, n_particles=None, **which):
    """the mirror's item of one photon system under `flags(**which)`; dipole: the result block's"""
    from cavitymd import _capi
    n = len(cfg["typeid"])
    where = np.nonzero(np.asarray(cfg["typeid"]) == cfg["L_typeid"])[0] if "L" in cfg["types"] else []
    p = cfg["params"]
    pos = np.zeros((n, 4))
    pos[:, :3] = cfg["position"]
    return dict(N=n, vel=vel.copy(), members=None, kT=KT, seed=key, pos=pos, image=np.array(cfg["image"], dtype=np.int32),
                L=np.asarray(cfg["box"], dtype=np.float64), K=_capi.make_params(p["omegac"], p["couplstr"], p["phmass"]).K,
                g=p["couplstr"],
                result=dict(n_particles=n if n_particles is None else n_particles, photon_idx=int(where[0]) if len(where) else -1,
                            dipole=np.asarray(dipole, dtype=np.float64)), **flags(**which))


# ---- 5. Maxwell-Boltzmann: 256 systems of N = 300 ------------------------------------------------------------------------------------
STAT_B, STAT_N, STAT_SEED = 256, 300, 5


def stat_masses():
    return np.random.default_rng(13).uniform(1.0, 30.0, (STAT_B, STAT_N))


def standardised(vel, kT):
    """v sqrt(m / kT) of (B, N, 4) velocities"""
    return vel[..., :3] * np.sqrt(vel[..., 3] / kT)[..., None]


def bands(z):
    """name -> (|deviation|, bound) of (B, N, 3) standardised variates.  The bounds are analytic, six standard errors with n the
    number of variates (or of pairs): a standard normal has variance 1, var(x^2) = 2, var(x^4) = 105 - 9 = 96, and the product of
    two independent ones has variance 1."""
    flat = z.ravel()
    n = flat.size
    out = {"mean": (abs(flat.mean()), 6.0 / np.sqrt(n)),
           "variance": (abs(flat.var() - 1.0), 6.0 * np.sqrt(2.0 / n)),
           "fourth moment": (abs((flat ** 4).mean() - 3.0), 6.0 * np.sqrt(96.0 / n))}
    for a, b in ((0, 1), (0, 2), (1, 2)):
        prod = z[..., a] * z[..., b]
        out[f"components {a}{b}"] = (abs(prod.mean()), 6.0 / np.sqrt(prod.size))
    for c in range(3):
        prod = z[:, :-1, c] * z[:, 1:, c]
        out[f"neighbours {c}"] = (abs(prod.mean()), 6.0 / np.sqrt(prod.size))
    return out
