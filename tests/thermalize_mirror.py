"""The contract of cavmd_thermalize_run (include/cavmd.h, "the start of a batch") restated in element-wise numpy, which rounds
once per operation and does not fuse.  The generator, the words-to-doubles step, the normal and its bound are draw_mirror's
(philox, block, normal, NORMAL_REL, EPS); only the counter layout, the member rule, the momentum and the photon's expressions
are this file's.

What is exact and what is not.  The generator words, every + - * / sqrt and floor are the same IEEE operations here and on
the device: compared bit for bit.  log and cospi are library functions on either side, so a normal n differs by at most
NORMAL_REL |n| (draw_mirror derives that), and with one more rounding on either side

    velocity           v = sigma n, sigma exact on both sides:           |dv| <= (NORMAL_REL + EPS) |v|
    photon coordinate  x = x0 + s n, s = sqrt(kT / K) and x0 exact; then pos = x - i L with i and i L the same on both sides:
                       |dpos| <= (NORMAL_REL + EPS) |s n| + 2 EPS |x|     (one EPS for the sum, one for the difference:
                       |pos| <= |x| whenever i != 0, and pos = x when i = 0)

provided the wrap takes the same image on both sides: a coordinate whose (x + L/2) / L lies within WRAP_MARGIN of an integer
is `ambiguous`.  The momentum P is taken with math.fsum, the correctly rounded sum: the kernel's compensated sum must lie within
2 ulp of it.  None of this is fitted to what a GPU returned.

An item is a dict: N, vel (N, 4) with the mass in column 3, members (None or an index array), kT, seed, the four flags
(zero_momentum, place_photon, finite_q, photon_velocity), and for the photon pos (N, 4), image (N, 3) int32, L (3,), K, g and
result (None, or a dict n_particles, photon_idx, dipole (3,)).  Its state is a dict (draws, thermalised, skipped, momentum,
photon)."""
import math

import numpy as np

import draw_mirror
from draw_mirror import EPS, NORMAL_REL, item_key  # noqa: F401  (the thermalizer's callers take item_key from here)

PURPOSE_VELOCITY = 0xC0000000
PURPOSE_POSITION = 0xC0000008
TILE = 512                          # CAVMD_THERMALIZE_TILE: entries of a member set per tile of the kernel
WRAP_MARGIN = 1e-9
VELOCITY_REL = NORMAL_REL + EPS


def new_state():
    return dict(draws=0, thermalised=0, skipped=0, momentum=np.zeros(3), photon=-1)


def block(seed, draws, j, purpose):
    """The four words of counter (draws low, draws high, j, purpose) under the key (seed low, seed high); j an array."""
    j = np.asarray(j, dtype=np.uint64)
    return draw_mirror.block(seed, np.full(j.shape, draws, dtype=np.uint64), j, np.full(j.shape, purpose, dtype=np.uint64))


def normals(seed, draws, j, purpose):
    """(len(j), 3) normals: component c of particle j from ONE block, purpose + c (item 1)"""
    j = np.asarray(j, dtype=np.uint64)
    d = np.full(j.shape, draws, dtype=np.uint64)
    return np.stack([draw_mirror.normal(seed, d, j, np.full(j.shape, purpose + c, dtype=np.uint64)) for c in range(3)], axis=-1)


def photon_of(item) -> int:
    """item 4's photon: only with a result block of this N that names one"""
    r = item.get("result")
    if r is None or int(r["n_particles"]) != item["N"] or not 0 <= int(r["photon_idx"]) < item["N"]:
        return -1
    return int(r["photon_idx"])


def mass_ok(m):
    with np.errstate(invalid="ignore"):
        return (m > 0.0) & np.isfinite(m)


def member_set(item, photon):
    """(the j the kernel writes, the number of entries it skips) -- item 2"""
    N = item["N"]
    if item["members"] is None:
        entries = np.array([j for j in range(N) if j != photon], dtype=np.int64)
    else:
        entries = np.asarray(item["members"], dtype=np.int64).reshape(-1)
    inside = entries[entries < N]
    written = inside[mass_ok(item["vel"][inside, 3])] if len(inside) else inside
    return written, len(entries) - len(written)


def remove_momentum(vel, written, P):
    """item 3's second half on the rows `written`, in place: v_c = v_c - (P_c / n) / m"""
    share = np.asarray(P, dtype=np.float64) / np.float64(len(written))
    vel[written, :3] = vel[written, :3] - share[None, :] / vel[written, 3][:, None]


def wrap(x, L):
    """the driver's wrap_position: (position, image flags as doubles, the distance of (x + L/2) / L from an integer)"""
    u = (x + L / 2.0) / L
    i = np.floor(u)
    return x - i * L, i, np.minimum(u - i, (i + 1.0) - u)


def place(item, p, draws, dipole=None):
    """item 4's placement of photon p -> dict x (unwrapped), pos, image, bound (on |device pos - pos|), ambiguous.
    dipole: None for the result block's, or the device's own."""
    K, g, kT = np.float64(item["K"]), np.float64(item["g"]), np.float64(item["kT"])
    L = np.asarray(item["L"], dtype=np.float64)
    d = np.asarray(item["result"]["dipole"] if dipole is None else dipole, dtype=np.float64)
    x = np.zeros(3)
    if item["finite_q"]:
        x = ((-d) * g) / K
        x[2] = 0.0
    spread = np.zeros(3)
    if g != 0.0:
        spread = np.sqrt(kT / K) * normals(item["seed"], draws, [p], PURPOSE_POSITION)[0]
        x = x + spread
    pos, i, margin = wrap(x, L)
    return dict(x=x, pos=pos, image=i.astype(np.int32), bound=VELOCITY_REL * np.abs(spread) + 2.0 * EPS * np.abs(x),
                ambiguous=bool((margin <= WRAP_MARGIN).any()))


def thermalize(item, state, dipole=None):
    """One run of one item, in place (vel, pos, image, state).  Returns None for N == 0 (the item is untouched), else a dict:
    written (the rows item 2 wrote), bound ((N, 3) on |device v - v| for a run WITHOUT zero_momentum; 0 on untouched rows),
    addends ((len(written), 3): m v_c before the momentum went out), photon (what place() returned, or None)."""
    N = item["N"]
    if N == 0:
        return None
    draws, kT = state["draws"], np.float64(item["kT"])
    vel = item["vel"]
    p = photon_of(item)
    written, skipped = member_set(item, p)
    bound = np.zeros((N, 3))
    addends = np.zeros((0, 3))
    if len(written):
        m = vel[written, 3]
        sigma = np.sqrt(kT / m)
        vel[written, :3] = sigma[:, None] * normals(item["seed"], draws, written, PURPOSE_VELOCITY)
        bound[written] = VELOCITY_REL * np.abs(vel[written, :3])
        addends = m[:, None] * vel[written, :3]
    P = np.zeros(3)
    if item["zero_momentum"] and len(written):
        P = np.array([math.fsum(addends[:, c].tolist()) for c in range(3)])
        remove_momentum(vel, written, P)
    placed = None
    if p >= 0:
        if item["photon_velocity"] and mass_ok(vel[p, 3]):
            vel[p, :3] = np.sqrt(kT / vel[p, 3]) * normals(item["seed"], draws, [p], PURPOSE_VELOCITY)[0]
            bound[p] = VELOCITY_REL * np.abs(vel[p, :3])
        if item["place_photon"]:
            placed = place(item, p, draws, dipole)
            item["pos"][p, :3] = placed["pos"]
            item["image"][p] = placed["image"]
    state.update(draws=draws + 1, thermalised=len(written), skipped=skipped, momentum=P, photon=p)
    return dict(written=written, bound=bound, addends=addends, photon=placed)
