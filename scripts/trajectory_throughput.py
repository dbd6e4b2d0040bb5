"""What the trajectory recorder costs in the captured MD step, what a recording call moves, and what a caller does without it
(DESIGN.md 3.7l).

usage: python scripts/trajectory_throughput.py [--B 512] [--sweeps 200] [--repeats 3] [--only record] [--json PATH]

B systems of N = 501 (synthetic.config1: 250 diatomics and the photon) under the full step of
examples/batch_coulomb_md_in_one_graph.py -- draws, step one, cavity force, bonds and Lennard-Jones, Ewald Coulomb, step two,
recorder, Bussi thermostat.  Variants, alternated `--repeats` times in this one process, every replay or call ending in a stream
synchronise and timed on the host clock around it (`--sweeps` per repeat, after a warm-up):
  (a) step                 the captured step without a trajectory node: the baseline (the parent has no such object);
      step+idle record     the same step with one cavmd_trajectory_record node whose frames are never due: what a user pays on
                           every step between frames;
  (b) record f32, f64      a graph of ONE recording call (every system forced): bytes read and written are printed beside it;
  (c) sync+clone           what a caller can do today: synchronise, then clone the 3 B position, velocity and image tensors.
`--only record` runs (b) and (c) alone, `--sweeps` times each, for
`rocprofv3 --kernel-trace --stats -- python scripts/trajectory_throughput.py --only record`, whose kernel times go beside the
bytes.  A measurement path: it needs a GPU and has no fallback."""
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
NEVER = 2 ** 40                      # a period no run reaches: the node decides, moves two counters and leaves


def systems(B):
    kT = 3.167e-4
    rng = np.random.default_rng(0)
    sysdefs, velocities, bonds, bond_typeid = [], [], [], []
    for k in range(B):
        cfg = synthetic.config1(seed=k + 1)
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
        v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(kT / mass)[:, None]
        velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
        b, t = synthetic.diatomic_bonds(cfg)
        bonds.append(b)
        bond_typeid.append(t)
    return cfg, sysdefs, velocities, bonds, bond_typeid


def step_graphs(cfg, sysdefs, velocities, bonds, bond_typeid):
    """the example's step captured twice over the same objects: without and with a trajectory node that never records"""
    B, kT, dt = len(sysdefs), 3.167e-4, 0.5
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
    idle = cavitymd.BatchTrajectoryRecorder(cavity, velocities, capacity=1, period=NEVER)

    def step(with_node):
        integrator.draw_inputs(dt, gamma=1e-3, kT=kT)
        integrator.step_one()
        cavity.compute()
        molecular.compute()
        coulomb.compute()
        integrator.step_two()
        if with_node:
            idle.record()
        recorder.record()
        thermostat.draw_inputs(0, dt)
        thermostat.step_async()

    cavity.compute()
    molecular.compute()
    coulomb.compute()
    integrator.prime()
    integrator.draw_inputs(dt, gamma=1e-3, kT=kT)
    thermostat.draw_inputs(0, dt)
    idle.record()
    torch.cuda.synchronize()
    graphs = {}
    for name, with_node in (("step", False), ("step+idle record", True)):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step(with_node)
        graphs[name] = g.replay
    keep = (cavity, molecular, coulomb, integrator, recorder, thermostat, idle)
    return graphs, keep


def record_calls(sysdefs, velocities):
    """(b) one forced recording call per format, captured; (c) synchronise and clone"""
    calls, keep, moved = {}, [], {}
    B, N = len(sysdefs), sysdefs[0].getParticleData().getN()
    for dtype, e in (("f32", 4), ("f64", 8)):
        t = cavitymd.BatchTrajectoryRecorder(sysdefs, velocities, capacity=2, dtype=dtype)
        t.record(force=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t.record(force=True)
        calls["record " + dtype] = g.replay
        keep += [t, g]
        pad16 = lambda x: -(-x // 16) * 16       # noqa: E731
        moved["record " + dtype] = dict(read=B * N * (32 + 32 + 12), written=B * (64 + 2 * pad16(3 * N * e) + pad16(12 * N)))
    arrays = [s.getParticleData().getPositions() for s in sysdefs] + list(velocities) \
        + [s.getParticleData().getImages() for s in sysdefs]

    def clone():
        torch.cuda.synchronize()
        return [a.clone() for a in arrays]

    calls["sync+clone"] = clone
    moved["sync+clone"] = dict(read=B * N * (32 + 32 + 12), written=B * N * (32 + 32 + 12))
    return calls, keep, moved


def measure(calls, sweeps, repeats, warm=10):
    sync = torch.cuda.synchronize
    for f in calls.values():
        for _ in range(warm):
            f()
        sync()
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for name, f in calls.items():            # alternated
            for _ in range(sweeps):
                t0 = time.perf_counter()
                f()
                sync()
                times[name].append(time.perf_counter() - t0)
    out = {}
    for name, v in times.items():
        us = np.array(v) * 1e6
        out[name] = {"variant": name, "calls": len(v), "median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)),
                     "p90_us": float(np.percentile(us, 90))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("record",), default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "trajectory_throughput.py measures on a GPU; there is no fallback"
    cfg, sysdefs, velocities, bonds, bond_typeid = systems(args.B)
    print(f"B={args.B} N={sysdefs[0].getParticleData().getN()} calls/repeat={args.sweeps} repeats={args.repeats}")
    rows = {}
    calls, keep_b, moved = record_calls(sysdefs, velocities)
    rows.update(measure(calls, args.sweeps, 1 if args.only else args.repeats))
    for t in keep_b[::2]:
        assert list(t.rows()) == [t.rows()[0]] * args.B and int(t.rows()[0]) > 0
    if not args.only:
        graphs, keep_a = step_graphs(cfg, sysdefs, velocities, bonds, bond_typeid)
        rows.update(measure(graphs, args.sweeps, args.repeats))
        idle = keep_a[-1]
        assert list(idle.rows()) == [0] * args.B                     # the node never recorded
    print(f"{'variant':<18s} {'median us':>10s} {'p10':>9s} {'p90':>9s} {'MB read':>9s} {'MB written':>11s}")
    for name, r in rows.items():
        m = moved.get(name)
        r.update(m or {})
        tail = f" {m['read'] / 1e6:9.2f} {m['written'] / 1e6:11.2f}" if m else ""
        print(f"{name:<18s} {r['median_us']:10.2f} {r['p10_us']:9.2f} {r['p90_us']:9.2f}{tail}")
    if not args.only:
        a, b = rows["step"], rows["step+idle record"]
        print(f"the idle node adds {b['median_us'] - a['median_us']:+.2f} us per replay; step p10..p90 {a['p10_us']:.2f}..{a['p90_us']:.2f}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"B": args.B, "rows": list(rows.values())}, f, indent=1)


if __name__ == "__main__":
    main()
