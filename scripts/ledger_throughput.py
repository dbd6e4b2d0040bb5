"""What the energy ledger adds to a replay of the captured MD step, against the torch bookkeeping it replaces.

usage: python scripts/ledger_throughput.py [--sizes 8,64,512] [--sweeps 200] [--repeats 3] [--only ledger] [--json PATH]
                                           [--readme PATH]

For every B: B systems of examples/batch_coulomb_md_in_one_graph.py (216 diatomics and the photon, N = 433) and its full step --
draws, step one, cavity force, bonds and Lennard-Jones, Ewald Coulomb, step two with the Langevin bath, recorder, Bussi
thermostat -- captured three times over the SAME objects and alternated `--repeats` times in this one process:
  step               the step with no per-step energy at all: the floor;
  step+torch         the step as the example had it before the ledger: the two torch reductions of .w, their add, an index_copy_
                     into a caller-made tensor and an add_ on a device-side row counter (five torch launches);
  step+ledger        the step with one cavmd_ledger_record in their place.
Every replay ends in a stream synchronise and is timed on the host clock around it (`--sweeps` replays per repeat, after a
warm-up).  Printed per B and variant: median, p10 and p90 microseconds per replay, and the two differences from the floor.
`--only ledger` replays that graph alone, for `rocprofv3 --kernel-trace --stats -- python scripts/ledger_throughput.py --only
ledger`.  `--readme` writes the table of profiles/ledger/README.md from this run.  A measurement path: it needs a GPU and has no
fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cavitymd  # noqa: E402
from cavitymd import synthetic  # noqa: E402

HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=15.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=15.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=15.0)}
VARIANTS = ("step", "step+torch", "step+ledger")


def build(B, replays):
    """the example's objects for B systems, and one captured graph per variant over them"""
    kT, dt = 3.167e-4, 5.0
    rng = np.random.default_rng(0)
    sysdefs, velocities, bonds, bond_typeid = [], [], [], []
    for k in range(B):
        cfg = synthetic.diatomic_lattice(6, 8.0, seed=k + 1)
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
        v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(kT / mass)[:, None]
        velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
        b, t = synthetic.diatomic_bonds(cfg)
        bonds.append(b)
        bond_typeid.append(t)
    photon = int(np.flatnonzero(cfg["typeid"] == 2)[0])
    molecules = [np.flatnonzero(cfg["typeid"] != 2)] * B
    cavity = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    molecular = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, harmonic=HARMONIC, lj=LJ)
    coulomb = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=15.0, accuracy=1e-5)
    integrator = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(molecular.forces, coulomb.forces)],
                                      langevin_index=photon)
    recorder = cavitymd.BatchRecorder(cavity, velocities, capacity=256)
    thermostat = cavitymd.BussiReservoirBatch(kT=kT, tau=1000.0)
    thermostat.attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
    ledger = cavitymd.BatchEnergyLedger(cavity, velocities, terms=[molecular, coulomb], reservoirs=[thermostat, integrator],
                                        capacity=256)
    potential = torch.zeros((replays, B), dtype=torch.float64, device="cuda")      # one row per replay of step+torch, no more
    row = torch.zeros((), dtype=torch.int64, device="cuda")

    def step(energy):
        integrator.draw_inputs(dt, gamma=1e-3, kT=kT)
        integrator.step_one()
        cavity.compute()
        molecular.compute()
        coulomb.compute()
        integrator.step_two()
        recorder.record()
        if energy == "step+torch":
            potential.index_copy_(0, row.reshape(1), (molecular.potential_energy() + coulomb.potential_energy())[None])
            row.add_(1)
        elif energy == "step+ledger":
            ledger.record()
        thermostat.draw_inputs(0, dt)
        thermostat.step_async()

    cavity.compute()
    molecular.compute()
    coulomb.compute()
    integrator.prime()
    integrator.draw_inputs(dt, gamma=1e-3, kT=kT)
    thermostat.draw_inputs(0, dt)
    molecular.potential_energy() + coulomb.potential_energy()
    ledger.record()
    torch.cuda.synchronize()
    graphs = {}
    for name in VARIANTS:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(name)
        graphs[name] = graph
    keep = (sysdefs, velocities, cavity, molecular, coulomb, integrator, recorder, thermostat, ledger, potential, row)
    return graphs, keep


def measure(B, sweeps, repeats, only):
    warm = 10
    graphs, keep = build(B, warm + sweeps * repeats)
    if only:
        graphs = {"step+" + only: graphs["step+" + only]}
    sync = torch.cuda.synchronize
    for g in graphs.values():
        for _ in range(warm):
            g.replay()
        sync()
    times = {k: [] for k in graphs}
    for _ in range(repeats):
        for name, g in graphs.items():          # alternated
            for _ in range(sweeps):
                t0 = time.perf_counter()
                g.replay()
                sync()
                times[name].append(time.perf_counter() - t0)
    ledger, integrator = keep[8], keep[5]
    if "step+ledger" in graphs:
        last = ledger.read()[:, -1]
        assert np.isfinite(last["universe_total"]).all() and (last["kinetic_group"] > 0).all() and (last["n_terms"] == 2).all()
    assert int(integrator.state()["out_of_box"].sum()) == 0
    out = {}
    for name, v in times.items():
        us = np.array(v) * 1e6
        out[name] = {"B": B, "variant": name, "replays": len(v), "median_us": float(np.median(us)),
                     "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90))}
    for obj in (ledger, keep[6], integrator, keep[4], keep[3], keep[2]):
        obj.close()
    keep[7].detach()
    return out


def write_readme(path, rows, sweeps, repeats):
    """the measured table of profiles/ledger/README.md, between its two markers"""
    lines = ["| B | step | step + torch bookkeeping | step + ledger | torch adds | ledger adds |", "|---|---|---|---|---|---|"]
    for B in sorted({r["B"] for r in rows}):
        r = {x["variant"]: x for x in rows if x["B"] == B}
        cell = lambda x: f"{x['median_us']:.1f} ({x['p10_us']:.1f}-{x['p90_us']:.1f})"   # noqa: E731
        floor = r["step"]["median_us"]
        lines.append(f"| {B} | {cell(r['step'])} | {cell(r['step+torch'])} | {cell(r['step+ledger'])} | "
                     f"{r['step+torch']['median_us'] - floor:+.1f} | {r['step+ledger']['median_us'] - floor:+.1f} |")
    lines.append("")
    lines.append(f"Microseconds per replay, median (p10-p90) of {repeats} x {sweeps} replays, the three graphs alternated in one process.")
    text = open(path).read()
    begin, end = "<!-- measured: begin -->", "<!-- measured: end -->"
    head, rest = text.split(begin)
    tail = rest.split(end)[1]
    with open(path, "w") as f:
        f.write(head + begin + "\n" + "\n".join(lines) + "\n" + end + tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,64,512")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("ledger", "torch"), default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--readme", default=None, help="rewrite the measured table of this README (profiles/ledger/README.md)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ledger_throughput.py measures on a GPU; there is no fallback"
    print(f"N=433 replays/repeat={args.sweeps} repeats={args.repeats}")
    print(f"{'B':>6s} {'variant':<14s} {'median us':>10s} {'p10':>9s} {'p90':>9s}")
    rows = []
    for B in [int(x) for x in args.sizes.split(",") if x]:
        got = measure(B, args.sweeps, args.repeats, args.only)
        for name, r in got.items():
            rows.append(r)
            print(f"{B:6d} {name:<14s} {r['median_us']:10.2f} {r['p10_us']:9.2f} {r['p90_us']:9.2f}", flush=True)
        if not args.only:
            floor = got["step"]
            print(f"{B:6d} torch bookkeeping adds {got['step+torch']['median_us'] - floor['median_us']:.2f} us, the ledger "
                  f"{got['step+ledger']['median_us'] - floor['median_us']:.2f} us per replay; step p10..p90 "
                  f"{floor['p10_us']:.2f}..{floor['p90_us']:.2f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"n": 433, "rows": rows}, f, indent=1)
    if args.readme and not args.only:
        write_readme(args.readme, rows, args.sweeps, args.repeats)


if __name__ == "__main__":
    main()
