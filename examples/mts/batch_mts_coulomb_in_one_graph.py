"""The long part of the Ewald sum every n-th step: the impulse multiple-time-step scheme (Verlet-I / r-RESPA) for B systems of
charged dimers, one OUTER step captured into one graph.  The reciprocal sum takes most of a step of
examples/batch_coulomb_md_in_one_graph.py and is smooth on the scale of a bond vibration; a split ``CoulombForceBatch`` keeps it
in an array of its own, and ``VerletBatch.kick`` applies it around n plain velocity-Verlet steps with everything else:

    kick(long, n / 2);  n x {step one; cavity, molecular, short; step two};  long;  kick(long, n / 2);  ledger

The ledger has the reference's two columns, ``ewald_short`` and ``ewald_long``.  The velocities are whole at the end of an outer
step, so the ledger writes one row per outer step.  NVE, fixed dt: the scheme is defined for a dt that stays the same through an
outer step (``StepDraw``'s fixed mode); under the adaptive rule it is unsupported, and a run clock's end time inside an outer
step would leave that system with an unmatched opening kick.  The example prints, for n = 1 and n = 4, the worst excursion of
``universe_total`` and the time per MD step.

    python examples/mts/batch_mts_coulomb_in_one_graph.py [B] [md_steps]"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cavitymd  # noqa: E402
from cavitymd import synthetic  # noqa: E402

# examples/05_advanced_run.py:568-582 of the reference
HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}      # 'O-O', 'N-N'
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=12.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=12.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=12.0)}                       # pairs with 'L': not listed


def run(B, md_steps, n, dt=10.0, kT=3.167e-4):
    """md_steps MD steps of B systems in outer steps of n -> (worst excursion of universe_total, microseconds per MD step)"""
    rng = np.random.default_rng(0)
    sysdefs, velocities, bonds, bond_typeid = [], [], [], []
    for k in range(B):
        cfg = synthetic.diatomic_lattice(3, 8.0, seed=k + 1)               # 27 dimers + the photon: N = 55, box 24 bohr
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
        v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(kT / mass)[:, None]
        velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
        b, t = synthetic.diatomic_bonds(cfg)
        bonds.append(b)
        bond_typeid.append(t)
    cavity = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    molecular = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, harmonic=HARMONIC, lj=LJ)
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=12.0, accuracy=1e-8, split=True)
    # the integrator's own forces are the cavity's, the molecular and the SHORT part; the long part only ever kicks
    integrator = cavitymd.VerletBatch(cavity, velocities,
                                      extra_forces=[[m, s] for m, s in zip(molecular.forces, coulomb.short.forces)])
    outer_steps = md_steps // n
    ledger = cavitymd.BatchEnergyLedger(cavity, velocities, terms=[("molecular", molecular), ("ewald_short", coulomb.short),
                                                                   ("ewald_long", coulomb.long)], capacity=outer_steps + 1)

    def outer():
        integrator.kick(coulomb.long, 0.5 * n)                             # one kernel: v += (f_long / m) (n / 2) dt
        for _ in range(n):
            integrator.step_one()
            cavity.compute()
            molecular.compute()
            coulomb.compute(parts="short")                                 # one kernel
            integrator.step_two()
        coulomb.compute(parts="long")                                      # two kernels: structure factors, the long part
        integrator.kick(coulomb.long, 0.5 * n)
        ledger.record()

    integrator.set_inputs(dt)
    cavity.compute()
    molecular.compute()
    coulomb.compute(parts="both")
    integrator.prime()                                                     # a = F / m of the integrator's own forces
    integrator.kick_table(coulomb.long)                                    # the kick's pointer table: an upload, before the capture
    ledger.record()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outer()
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(outer_steps):
        graph.replay()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    energy = ledger.read()                                                 # (B, outer_steps + 1) rows
    state = integrator.state()
    assert int(state["steps"][0]) == outer_steps * n and int(state["out_of_box"].sum()) == 0
    universe = energy["universe_total"]
    excursion = float(np.abs(universe - universe[:, :1]).max())
    print(f"n = {n}: B = {B}, {outer_steps * n} MD steps; ewald_short {energy['ewald_short'][0, -1]:.6e}, ewald_long "
          f"{energy['ewald_long'][0, -1]:.6e}; worst excursion of universe_total {excursion:.3e} hartree; "
          f"{1e6 * elapsed / (outer_steps * n):.1f} us per MD step")
    for obj in (ledger, integrator, coulomb, molecular, cavity):
        obj.close()
    return excursion, 1e6 * elapsed / (outer_steps * n)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    md_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 160
    assert torch.cuda.is_available(), "this example needs a GPU; the package has no CPU fallback"
    assert md_steps % 4 == 0, "md_steps: a multiple of 4"
    for n in (1, 4):
        run(B, md_steps, n)


if __name__ == "__main__":
    main()
