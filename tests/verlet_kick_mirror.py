"""cavmd_mts_verlet_kick of include/cavmd.h restated in element-wise numpy, which rounds once per operation and does not fuse:
    h = weight * dt;  minv = 1.0 / m;  v_c = v_c + (f_c * minv) * h
on a system of tests/verlet_mirror.py (a dict of host arrays).  Only vel[:, :3] changes.  tests/test_gpu_verlet_kick.py compares
the kernel with it bit for bit; the host twin of the impulse scheme (tests/mts_twin.py) kicks with it."""
import numpy as np


def mirror_kick(s, row, force, weight) -> None:
    """force: (N, >= 3) or None (a NULL pointer: the item is left untouched)"""
    if s["N"] == 0 or row.skip or force is None:
        return
    h = np.float64(weight) * np.float64(row.dt)
    minv = 1.0 / s["vel"][:, 3]
    s["vel"][:, :3] = s["vel"][:, :3] + (np.asarray(force)[:, :3] * minv[:, None]) * h
