"""M cells of charged harmonic dimers in one shared cavity on the host: velocity Verlet in plain numpy.  The reference for the
captured step of tests/test_gpu_shared_cavity.py (the graph of examples/shared_cavity/batch_shared_cavity_in_one_graph.py), and
what tests/test_shared_cavity_twin.py proves first without a GPU.

Every cell is a periodic box of edge L with its own 4 dimers (charges +-Q, a harmonic bond under the minimum image); cell 0
carries the photon as its last particle.  The cavity term is the formulas of include/cavmd.h (cavmd_shared_cavity): with r
unwrapped by each cell's own box, d_c = sum_i q_i r_i, D = sum_c d_c, E = 1/2 K q.q + g D_xy.q_xy + 1/2 (g^2/K) D_xy.D_xy,
F_i = -g q_i (q_xy + (g/K) D_xy) on every molecule of every cell and F_L = -K q - g D_xy on the photon.  The step is step one
(v += a dt / 2, x += v dt, one wrap per axis with the image following), the forces, step two (a = F / m, v += a dt / 2); the
energy is taken after step two.

The planted mistake "own_dipole": every cell's molecules feel q_xy + (g/K) d_c of their OWN cell instead of D.  The photon
still feels D, so the cells no longer exchange energy through it consistently and the energy is not conserved.

Measured with this file (host, numpy; never a GPU run), from the repository's root:
    PYTHONPATH=tests python tests/shared_cavity_twin.py
M = 3, span 8000 a.u., seeds 0..3 -- excursion of the energy at dt = 10, at dt = 20, their ratio, and with the planted mistake
at dt = 10 (tests/test_shared_cavity_twin.py fails if MEASURED is not that run's figures):"""
import numpy as np

M, DIMERS = 3, 4
Q, MASS = 0.3, 29166.0
BOND_K, BOND_R0 = 0.73204, 2.281655158
BOX = 20.0
IMAGES = 1                                   # images drawn from -1 .. 1
KT = 100.0 * 3.166811563e-6                  # 100 K in hartree
OMEGA = 2000.0 / 219474.63                   # 2000 cm^-1
G, PHMASS = 1e-3, 1.0
K_SPRING = PHMASS * OMEGA * OMEGA
SPAN = 8000.0
SEEDS = (0, 1, 2, 3)
TYPES = ["O", "L"]
L_TYPEID = 1

# seed -> (excursion at dt = 10, at dt = 20, with "own_dipole" at dt = 10); M = 1, seed 0: MEASURED_ALONE
MEASURED = {
    0: (1.7231e-05, 6.8278e-05, 2.0593e-01),   # ratio 3.962, mistake 11951x
    1: (1.0477e-04, 4.0996e-04, 2.4784e-01),   # ratio 3.913, mistake 2366x
    2: (1.5898e-05, 6.2625e-05, 1.8549e-01),   # ratio 3.939, mistake 11667x
    3: (1.0209e-04, 3.9200e-04, 2.3932e-01),   # ratio 3.840, mistake 2344x
}
MEASURED_ALONE = (1.3175e-05, 5.1229e-05)      # ratio 3.888
BAND = 3.0                                   # the margin of tests/thermostatted_twin.py: 3 times the twin's own excursion


def start(seed, cells=M):
    """The cells at time 0: per cell a dict of position (wrapped), image, typeid, charge, mass, velocity, bonds, box, types."""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for c in range(cells):
        n = 2 * DIMERS + (c == 0)
        pos = np.zeros((n, 3))
        centre = rng.uniform(-0.5, 0.5, (DIMERS, 3)) * (BOX - 6.0)
        axis = rng.normal(size=(DIMERS, 3))
        axis /= np.linalg.norm(axis, axis=1)[:, None]
        half = 0.5 * (BOND_R0 + rng.uniform(-0.05, 0.05, DIMERS))[:, None] * axis
        pos[0:2 * DIMERS:2] = centre - half
        pos[1:2 * DIMERS:2] = centre + half
        charge = np.zeros(n)
        charge[0:2 * DIMERS:2], charge[1:2 * DIMERS:2] = Q, -Q
        mass = np.full(n, MASS)
        typeid = np.zeros(n, dtype=np.int32)
        image = np.zeros((n, 3), dtype=np.int32)                          # one image per dimer: a molecule is whole when unwrapped
        image[:2 * DIMERS] = np.repeat(rng.integers(-IMAGES, IMAGES + 1, (DIMERS, 3)), 2, axis=0)
        vel = rng.normal(size=(n, 3)) * np.sqrt(KT / MASS)
        if c == 0:
            typeid[-1], mass[-1] = L_TYPEID, PHMASS
            pos[-1] = rng.normal(size=3) * np.sqrt(KT / K_SPRING)
            vel[-1] = rng.normal(size=3) * np.sqrt(KT / PHMASS)
        bonds = np.stack([np.arange(0, 2 * DIMERS, 2), np.arange(1, 2 * DIMERS, 2)], axis=1)
        out.append({"position": pos, "image": image, "typeid": typeid, "charge": charge, "mass": mass, "velocity": vel,
                    "bonds": bonds, "box": (BOX, BOX, BOX), "types": list(TYPES), "L_typeid": L_TYPEID,
                    "params": {"omegac": OMEGA, "couplstr": G, "phmass": PHMASS}})
    return out


def forces(cells, mistake=None):
    """(per-cell (n, 3) forces, potential energy): the bonds of every cell and the one cavity term over all of them"""
    F, U = [], 0.0
    dipoles = []
    for cell in cells:
        x, box = cell["position"], np.asarray(cell["box"])
        f = np.zeros_like(x)
        a, b = cell["bonds"][:, 0], cell["bonds"][:, 1]
        d = x[b] - x[a]
        d -= box * np.round(d / box)                                   # the minimum image
        r = np.linalg.norm(d, axis=1)
        U += float((0.5 * BOND_K * (r - BOND_R0) ** 2).sum())
        pull = (BOND_K * (r - BOND_R0) / r)[:, None] * d               # on a, towards b
        np.add.at(f, a, pull)
        np.add.at(f, b, -pull)
        F.append(f)
        mol = cell["typeid"] != L_TYPEID
        r_unwrapped = x + cell["image"] * box
        dipoles.append((cell["charge"][mol, None] * r_unwrapped[mol]).sum(axis=0))
    D = np.sum(dipoles, axis=0)
    photon = int(np.flatnonzero(cells[0]["typeid"] == L_TYPEID)[0])
    q = cells[0]["position"][photon] + cells[0]["image"][photon] * np.asarray(cells[0]["box"])
    U += 0.5 * K_SPRING * float(q @ q) + G * float(D[:2] @ q[:2]) + 0.5 * (G * G / K_SPRING) * float(D[:2] @ D[:2])
    for c, cell in enumerate(cells):
        felt = dipoles[c] if mistake == "own_dipole" else D
        Dq = q[:2] + (G / K_SPRING) * felt[:2]
        mol = cell["typeid"] != L_TYPEID
        F[c][mol, :2] += (-G * cell["charge"][mol])[:, None] * Dq[None, :]
    F[0][photon] = np.array([-K_SPRING * q[0] - G * D[0], -K_SPRING * q[1] - G * D[1], -K_SPRING * q[2]])
    return F, U


def energy(cells, U):
    return U + sum(float((0.5 * c["mass"] * (c["velocity"] ** 2).sum(axis=1)).sum()) for c in cells)


def run(seed, dt, span=SPAN, cells=M, mistake=None):
    """The energy after every step of `span` / dt steps, (steps,); and the energy of the start"""
    state = [dict(c, position=c["position"].copy(), image=c["image"].copy(), velocity=c["velocity"].copy())
             for c in start(seed, cells)]
    steps = int(round(span / dt))
    F, U = forces(state, mistake)
    E0 = energy(state, U)
    trace = np.zeros(steps)
    for s in range(steps):
        for c, cell in enumerate(state):
            box = np.asarray(cell["box"])
            cell["velocity"] += (F[c] / cell["mass"][:, None]) * (0.5 * dt)
            cell["position"] += cell["velocity"] * dt
            up, down = cell["position"] >= 0.5 * box, cell["position"] < -0.5 * box
            cell["position"] -= box * up
            cell["position"] += box * down
            cell["image"] += up.astype(np.int32) - down.astype(np.int32)
        F, U = forces(state, mistake)
        for c, cell in enumerate(state):
            cell["velocity"] += (F[c] / cell["mass"][:, None]) * (0.5 * dt)
        trace[s] = energy(state, U)
    return trace, E0


def excursion(trace) -> float:
    """max |E - E[0]| over the rows of a trace"""
    return float(np.abs(trace - trace[0]).max())


def measure(seed, cells=M):
    fine, coarse = run(seed, 10.0, cells=cells)[0], run(seed, 20.0, cells=cells)[0]
    out = [excursion(fine), excursion(coarse)]
    if cells > 1:
        out.append(excursion(run(seed, 10.0, cells=cells, mistake="own_dipole")[0]))
    return tuple(out)


if __name__ == "__main__":
    for seed in SEEDS:
        m = measure(seed)
        print(f"    {seed}: ({m[0]:.4e}, {m[1]:.4e}, {m[2]:.4e}),   # ratio {m[1] / m[0]:.3f}, mistake {m[2] / m[0]:.0f}x")
    a = measure(0, cells=1)
    print(f"MEASURED_ALONE = ({a[0]:.4e}, {a[1]:.4e})   # ratio {a[1] / a[0]:.3f}")
