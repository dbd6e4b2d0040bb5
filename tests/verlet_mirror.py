"""The velocity-Verlet half-steps of include/cavmd.h (cavmd_verlet_*: HOOMD-blue's ConstantVolume half-steps plus its Langevin
bath on one particle) restated in element-wise numpy, which rounds once per operation and does not fuse.  A system is a dict
of host arrays (N, box, pos, vel, image, forces, net, accel, langevin, steps, out_of_box, reservoir); tests/test_gpu_verlet_batch.py
builds them and compares the kernels with this mirror bit for bit."""
import numpy as np


def mirror_net_force(forces):
    F = forces[0].copy()
    for f in forces[1:]:
        F = F + f                                            # left to right, .w included
    return F


def mirror_accelerations(s) -> None:
    """steps 1, 2, 3 and 5 of step two"""
    if s["N"] == 0:
        return
    minv = 1.0 / s["vel"][:, 3]
    F = mirror_net_force(s["forces"])
    if s["net"] is not None:
        s["net"] = F.copy()
    s["accel"] = F[:, :3] * minv[:, None]


def mirror_step_one(s, row, classify=None) -> None:
    if s["N"] == 0 or row.skip:
        return
    dt = np.float64(row.dt)
    for c in range(3):
        L = np.float64(s["box"][c])
        v = s["vel"][:, c] + (0.5 * s["accel"][:, c]) * dt
        x = s["pos"][:, c] + dt * v
        hi = L * 0.5
        lo = -hi
        if classify is not None:
            classify(c, x, lo, hi, L)
        up = x >= hi
        down = ~up & (x < lo)
        x = np.where(up, x - L, np.where(down, x + L, x))
        s["image"][:, c] += up.astype(np.int32) - down.astype(np.int32)
        s["out_of_box"] += int(np.count_nonzero(~((x >= lo) & (x < hi))))
        s["vel"][:, c] = v
        s["pos"][:, c] = x


def mirror_step_two(s, row, tally_velocity="after") -> None:
    """tally_velocity: "after" is the contract; "before" (the velocity the force is formed with) is kept as a planted mistake
    for the twins, under which langevin_reservoir heats by 3 gamma kT dt / m per step and the ledger's total drifts."""
    assert tally_velocity in ("after", "before")
    if s["N"] == 0 or row.skip:
        return
    dt, gamma, coeff = np.float64(row.dt), np.float64(row.langevin_gamma), np.float64(row.langevin_coeff)
    minv = 1.0 / s["vel"][:, 3]
    F = mirror_net_force(s["forces"])
    if s["net"] is not None:
        s["net"] = F.copy()
    F = F[:, :3].copy()
    j = s["langevin"]
    bathed = j >= 0 and gamma != 0.0
    if bathed:
        before = s["vel"][j, :3].copy()                      # the force: from BEFORE the kick
        bd = np.array(row.uniform[:], dtype=np.float64) * coeff - gamma * before
        F[j] = F[j] + bd
    a = F * minv[:, None]
    s["accel"] = a
    s["vel"][:, :3] = s["vel"][:, :3] + (0.5 * a) * dt
    if bathed:
        v = s["vel"][j, :3] if tally_velocity == "after" else before   # the tally: from AFTER the kick, the velocity just stored
        tally = (bd[0] * v[0] + bd[1] * v[1]) + bd[2] * v[2]
        s["reservoir"] = s["reservoir"] - tally * dt
    s["steps"] += 1
