"""The constants of the reference driver's molecular model and the thermal start the MD tests of the molecular, Coulomb,
batch-owner and split-variant GPU modules share.  Importing this module touches no GPU."""
import numpy as np

# the driver's constants (examples/05_advanced_run.py:568-582 of the reference); types 0 = 'O', 1 = 'N', 2 = 'L' (unlisted)
HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=15.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=15.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=15.0)}
KT = 3.167e-4


def thermal(cfg, rng_seed=7):
    """(velocities at 100 K, masses): the photon's mass is 1"""
    rng = np.random.default_rng(rng_seed + int(cfg["seed"]))
    n = len(cfg["charge"])
    mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
    return rng.normal(size=(n, 3)) * np.sqrt(KT / mass)[:, None], mass
