"""The contract of cavmd_bath_step_two (include/cavmd.h, "a Langevin bath on any set of particles of a batch") restated in
element-wise numpy, which rounds once per operation and does not fuse: step two of tests/verlet_mirror.py with the group's bath
between its items 3 and 5.  The net force is verlet_mirror.mirror_net_force, the generator and the words-to-doubles step are
draw_mirror.philox / unit; only the counter layout, the bath's expressions and the tally are this file's.  The item's tally T is
taken with math.fsum, the correctly rounded sum: the kernel's compensated sum must lie within 2 ulp of it.

A system is the dict of verlet_mirror (N, vel, forces, net, accel, langevin, steps, reservoir); its bath is a dict
(gamma: (n_bath,) array or None, kT, seed, draws, coupled, reservoir)."""
import math

import numpy as np

import draw_mirror
from draw_mirror import KEY_STRIDE, item_key  # noqa: F401  (the bath's callers take both from here)
from verlet_mirror import mirror_net_force

PURPOSE = 0x80000000


def block(seed, draws, j, b):
    """The four words of counter (draws low, draws high, j, 0x80000000 + b) under the key (seed low, seed high); j an array."""
    j = np.asarray(j, dtype=np.uint64)
    return draw_mirror.block(seed, np.full(j.shape, draws, dtype=np.uint64), j, np.full(j.shape, PURPOSE + b, dtype=np.uint64))


def variates(seed, draws, j):
    """(len(j), 3) variates in [-1, 1): u_x from w0,w1 and u_y from w2,w3 of block 0, u_z from w0,w1 of block 1"""
    w0, w1 = block(seed, draws, j, 0), block(seed, draws, j, 1)
    return np.stack([2.0 * draw_mirror.unit(w0[..., 0], w0[..., 1]) - 1.0, 2.0 * draw_mirror.unit(w0[..., 2], w0[..., 3]) - 1.0,
                     2.0 * draw_mirror.unit(w1[..., 0], w1[..., 1]) - 1.0], axis=-1)


def coupled_particles(s, row, bath) -> np.ndarray:
    """indices j < min(bath N, N) with gamma_j > 0 that are not the row's Langevin particle (NaN > 0 is False)"""
    if bath["gamma"] is None:
        return np.zeros(0, dtype=np.int64)
    n = min(len(bath["gamma"]), s["N"])
    with np.errstate(invalid="ignore"):
        on = bath["gamma"][:n] > 0.0
    if s["langevin"] >= 0 and row.langevin_gamma != 0.0 and s["langevin"] < n:
        on[s["langevin"]] = False
    return np.nonzero(on)[0]


def mirror_bath_step_two(s, row, bath, uniforms=None, tally_velocity="after"):
    """Step two with the bath.  Returns (tallies of the coupled particles, fsum of them), or None where the item is left
    untouched.  uniforms: None (the contract's Philox variates) or a callable (j -> (len(j), 3)) for planted mistakes.
    tally_velocity: "after" is the contract; "before" is verlet_mirror.mirror_step_two's planted mistake, for the twins."""
    assert tally_velocity in ("after", "before")
    if s["N"] == 0 or row.skip:
        return None
    dt, gamma, coeff = np.float64(row.dt), np.float64(row.langevin_gamma), np.float64(row.langevin_coeff)
    minv = 1.0 / s["vel"][:, 3]
    F = mirror_net_force(s["forces"])
    if s["net"] is not None:
        s["net"] = F.copy()                                  # without any bath term
    F = F[:, :3].copy()
    j = s["langevin"]
    bathed = j >= 0 and gamma != 0.0
    if bathed:                                               # the row's bath, as verlet_mirror.mirror_step_two has it
        before_row = s["vel"][j, :3].copy()
        bd_row = np.array(row.uniform[:], dtype=np.float64) * coeff - gamma * before_row
        F[j] = F[j] + bd_row
    on = np.zeros(0, dtype=np.int64)
    if bath["gamma"] is not None:
        on = coupled_particles(s, row, bath)
        if len(on):
            g = bath["gamma"][on]
            u = variates(bath["seed"], bath["draws"], on) if uniforms is None else uniforms(on)
            with np.errstate(invalid="ignore", divide="ignore"):
                c = np.sqrt(((6.0 * g) * np.float64(bath["kT"])) / dt)
            before = s["vel"][on, :3].copy()                 # the force: from BEFORE the kick
            bd = u * c[:, None] - g[:, None] * before
            F[on] = F[on] + bd
    a = F * minv[:, None]
    s["accel"] = a
    s["vel"][:, :3] = s["vel"][:, :3] + (0.5 * a) * dt
    if bathed:                                               # the tallies: from AFTER the kick, the velocity just stored
        v = s["vel"][j, :3] if tally_velocity == "after" else before_row
        tally = (bd_row[0] * v[0] + bd_row[1] * v[1]) + bd_row[2] * v[2]
        s["reservoir"] = s["reservoir"] - tally * dt
    tallies = np.zeros(0)
    if bath["gamma"] is not None:
        if len(on):
            v = s["vel"][on, :3] if tally_velocity == "after" else before
            tallies = (bd[:, 0] * v[:, 0] + bd[:, 1] * v[:, 1]) + bd[:, 2] * v[:, 2]
        T = np.float64(math.fsum(tallies.tolist()))
        bath["coupled"] = len(on)
        bath["reservoir"] = bath["reservoir"] - T * dt
        bath["draws"] += 1
    s["steps"] += 1
    return tallies, (math.fsum(tallies.tolist()) if bath["gamma"] is not None else 0.0)
