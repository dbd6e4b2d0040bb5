"""What the run clock costs and what it buys (profiles/run_clock/README.md).

usage: python scripts/run_clock_timing.py ab    [--tree DIR] [--sizes 64,500] [--sweeps 200]
       python scripts/run_clock_timing.py rules [--sizes 64,500] [--sweeps 200] [--repeats 3]
       python scripts/run_clock_timing.py buys  [--B 64] [--t-end 400]

The systems are those of examples/batch_coulomb_md_in_one_graph.py (216 diatomics and the photon, N = 433).  Every replay ends
in a stream synchronise and is timed on the host clock around it; a measurement path: it needs a GPU and has no fallback.

ab     the captured step of that example -- no rule set anywhere -- for the package under DIR (default: this tree): one JSON
       line per B with the median, the smallest and the largest of `--sweeps` replays.  Run it alternately for the parent
       commit's tree and this one, each in a fresh process: "no rule set must cost nothing".
rules  five graphs over the SAME objects, alternated in one process: the step alone; with the ledger at period 1; with the
       ledger under a time rule whose interval is about four steps (most calls write no row); with a field recorder (50
       wavevectors) at period 1; with a field recorder under a time rule of the same interval; and
       ``StepDraw.fill()`` alone as a one-kernel graph, of an object without end times against one whose end times are set (to
       a time never reached, so every item still draws).
buys   B replicas under the adaptive dt run to one t_end: the spread of step counts, the replays until all had finished, and
       the wall time of ``run_until_finished`` at check_every = 64, 256, 1024 against a loop that reads the B clocks after
       every replay (each from the same saved start)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=15.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=15.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=15.0)}
KT, DT = 3.167e-4, 5.0


def systems(B):
    """the example's B systems with their three forces, integrator, recorder and thermostat"""
    rng = np.random.default_rng(0)
    sysdefs, velocities, bonds, bond_typeid = [], [], [], []
    for k in range(B):
        cfg = synthetic.diatomic_lattice(6, 8.0, seed=k + 1)
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, pd.getN()))
        v = rng.normal(size=(pd.getN(), 3)) * np.sqrt(KT / mass)[:, None]
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
                                      langevin_index=photon, net_forces=True)
    recorder = cavitymd.BatchRecorder(cavity, velocities, net_forces=integrator.net_forces, capacity=64)
    thermostat = cavitymd.BussiReservoirBatch(kT=KT, tau=1000.0)
    thermostat.attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
    cavity.compute()
    molecular.compute()
    coulomb.compute()
    integrator.prime()
    return dict(sysdefs=sysdefs, velocities=velocities, cavity=cavity, molecular=molecular, coulomb=coulomb, integrator=integrator,
                recorder=recorder, thermostat=thermostat)


def captured(step):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def timed_replays(graph, sweeps):
    out = []
    for _ in range(sweeps):
        t0 = time.perf_counter()
        graph.replay()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def summary(us):
    us = np.asarray(us)
    return dict(median_us=float(np.median(us)), min_us=float(us.min()), max_us=float(us.max()), p10_us=float(np.percentile(us, 10)),
                p90_us=float(np.percentile(us, 90)))


def mode_ab(args):
    for B in args.sizes:
        s = systems(B)

        def step():
            s["integrator"].draw_inputs(DT, gamma=1e-3, kT=KT)
            s["integrator"].step_one()
            s["cavity"].compute()
            s["molecular"].compute()
            s["coulomb"].compute()
            s["integrator"].step_two()
            s["recorder"].record()
            s["thermostat"].draw_inputs(0, DT)
            s["thermostat"].step_async()

        s["integrator"].draw_inputs(DT, gamma=1e-3, kT=KT)
        s["thermostat"].draw_inputs(0, DT)
        graph = captured(step)
        timed_replays(graph, 20)
        print(json.dumps(dict(mode="ab", tree=args.tree, B=B, sweeps=args.sweeps, **summary(timed_replays(graph, args.sweeps)))), flush=True)
        assert int(s["integrator"].state()["out_of_box"].sum()) == 0
        del graph


def mode_rules(args):
    for B in args.sizes:
        s = systems(B)
        draw = cavitymd.StepDraw(2024, s["integrator"], s["thermostat"], s["recorder"], dt=DT, gamma=1e-3, kT=KT, tolerance=1e-3,
                                 dt_min=0.5, dt_max=10.0)
        make = lambda: cavitymd.BatchEnergyLedger(s["cavity"], s["velocities"], terms=[s["molecular"], s["coulomb"]],   # noqa: E731
                                                  reservoirs=[s["thermostat"], s["integrator"]], clock=draw, capacity=256)
        ledgers = {"step": None, "step+ledger": make(), "step+timed ledger": make()}
        ledgers["step+timed ledger"].set_time_rule(4.0 * DT)
        positions = [sd.getParticleData().getPositions() for sd in s["sysdefs"]]
        for name in ("step+fields", "step+timed fields"):
            ledgers[name] = cavitymd.BatchFieldRecorder(positions, capacity=256, reference_interval=0)
        ledgers["step+timed fields"].set_time_rule(draw, 4.0 * DT, 40.0 * DT)

        def step(ledger):
            draw.fill()
            s["integrator"].step_one()
            s["cavity"].compute()
            s["molecular"].compute()
            s["coulomb"].compute()
            s["integrator"].step_two()
            s["recorder"].record()
            if ledger is not None:
                ledger.record()
            s["thermostat"].step_async()

        graphs = {name: captured(lambda ledger=ledger: step(ledger)) for name, ledger in ledgers.items()}
        # fill() alone: two more draw objects over tables of their own, so that the step's clocks are not touched
        tables = [torch.zeros((B, 8), dtype=torch.float64, device="cuda") for _ in range(4)]
        fills = {"fill": cavitymd.StepDraw(7, tables[0], tables[1], dt=DT, gamma=1e-3, kT=KT, set_T=KT, tau=1000.0, dof=645.0),
                 "fill+end times": cavitymd.StepDraw(7, tables[2], tables[3], dt=DT, gamma=1e-3, kT=KT, set_T=KT, tau=1000.0, dof=645.0)}
        fills["fill+end times"].set_end_time(1e30)
        graphs.update({name: captured(d.fill) for name, d in fills.items()})
        for g in graphs.values():
            timed_replays(g, 10)
        times = {name: [] for name in graphs}
        for _ in range(args.repeats):
            for name, g in graphs.items():
                times[name] += timed_replays(g, args.sweeps)
        rows = {name: int(l.rows().min()) for name, l in ledgers.items() if l is not None}
        calls = 10 + args.repeats * args.sweeps
        for name, us in times.items():
            extra = dict(rows_written=rows[name], calls=calls) if name in rows else {}
            print(json.dumps(dict(mode="rules", B=B, variant=name, **summary(us), **extra)), flush=True)
        assert int(s["integrator"].state()["out_of_box"].sum()) == 0
        assert fills["fill"].state()["draws"].tolist() == fills["fill+end times"].state()["draws"].tolist()
        del graphs


def mode_buys(args):
    B, t_end = args.B, args.t_end
    s = systems(B)
    draw = cavitymd.StepDraw(2024, s["integrator"], s["thermostat"], s["recorder"], dt=DT, gamma=1e-3, kT=KT, tolerance=1e-3,
                             dt_min=0.5, dt_max=10.0)
    draw.set_end_time(t_end)
    objects = {"integrator": s["integrator"], "draw": draw, "recorder": s["recorder"], "thermostat": s["thermostat"]}
    checkpoint = cavitymd.BatchCheckpoint(s["sysdefs"], s["velocities"], objects)

    def step():
        draw.fill()
        s["integrator"].step_one()
        s["cavity"].compute()
        s["molecular"].compute()
        s["coulomb"].compute()
        s["integrator"].step_two()
        s["recorder"].record()
        s["thermostat"].step_async()

    graph = captured(step)
    start = checkpoint.state()
    limit = int(t_end / 0.5) + 2

    def from_start():
        checkpoint.load_state(start)
        s["cavity"].compute()
        s["molecular"].compute()
        s["coulomb"].compute()
        torch.cuda.synchronize()

    from_start()
    t0 = time.perf_counter()
    replays = 0
    while replays < limit:                                                 # the loop the run clock replaces: B clocks per replay
        graph.replay()
        replays += 1
        if (draw.state()["elapsed"] >= t_end).all():
            break
    wall = time.perf_counter() - t0
    steps = draw.state()["draws"].astype(np.int64)
    print(json.dumps(dict(mode="buys", B=B, t_end=t_end, loop="clocks read after every replay", replays=replays, wall_s=wall,
                          steps_min=int(steps.min()), steps_median=float(np.median(steps)), steps_max=int(steps.max()))), flush=True)
    for check_every in (64, 256, 1024):
        from_start()
        t0 = time.perf_counter()
        replays = cavitymd.run_until_finished(graph.replay, draw, check_every=check_every, max_replays=limit + check_every)
        wall = time.perf_counter() - t0
        state = draw.state()
        assert state["finished"].all() and (state["elapsed"] >= t_end).all()
        assert (state["draws"].astype(np.int64) == steps).all()            # the same steps, whichever loop drove them
        print(json.dumps(dict(mode="buys", B=B, t_end=t_end, loop=f"run_until_finished, check_every={check_every}", replays=replays,
                              wall_s=wall, clock_min=float(state["elapsed"].min()), clock_max=float(state["elapsed"].max()))), flush=True)
    del graph


def main():
    global np, torch, cavitymd, synthetic
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("ab", "rules", "buys"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (mode ab)")
    ap.add_argument("--sizes", default="64,500", type=lambda x: [int(v) for v in x.split(",") if v])
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--t-end", type=float, default=400.0)
    args = ap.parse_args()
    sys.path[:0] = [args.tree, os.path.join(args.tree, "cav-hoomd_amd")]
    import numpy as np
    import torch

    import cavitymd
    from cavitymd import synthetic
    assert torch.cuda.is_available(), "run_clock_timing.py measures on a GPU; there is no fallback"
    {"ab": mode_ab, "rules": mode_rules, "buys": mode_buys}[args.mode](args)


if __name__ == "__main__":
    main()
