"""Microseconds per replay of the captured MD step of examples/batch_coulomb_md_in_one_graph.py (B replicas of N = 433: step one,
cavity force, bonds and Lennard-Jones, Ewald Coulomb, step two, recorder, thermostat), B = 8, 64, 500, with the step's inputs

  (a) drawn by torch: ``VerletBatch.draw_inputs`` and ``BussiReservoirBatch.draw_inputs`` (rand, randn, _standard_gamma,
      where, slice and constant copies), and
  (b) drawn by ONE launch of the library: ``StepDraw.fill`` (cavmd_draw_fill), fixed dt,

and the draws alone (a graph that holds nothing but ``fill``, fixed and adaptive; one that holds the two torch calls).  It also
counts the nodes of both steps' graphs where the runtime's graph dump gives any ("not available" otherwise).

Method: the two graphs are built on the SAME systems and alternated sample by sample, so that a drift of the clocks hits both:
20 warm-up replays each, then 15 samples of 20 replays between two events on the stream; a sample is the elapsed time / 20;
the table gives the median and the min .. max of the samples.  The trajectory advances while it is timed.

    python scripts/step_draw_throughput.py [--out profiles/step_draw/table.txt] [--batches 8,64,500]
"""
import argparse
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cavitymd  # noqa: E402
from cavitymd import synthetic  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "examples"))
from batch_coulomb_md_in_one_graph import HARMONIC, LJ  # noqa: E402

KT, DT, GAMMA, WARMUP, SAMPLES, INNER = 3.167e-4, 5.0, 1e-3, 20, 15, 20


def build(B):
    rng = np.random.default_rng(0)
    sysdefs, velocities, bonds, bond_typeid = [], [], [], []
    for k in range(B):
        cfg = synthetic.diatomic_lattice(6, 8.0, seed=k + 1)               # N = 433, as the example
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
    s = {"B": B}
    s["cavity"] = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    s["molecular"] = cavitymd.MolecularForceBatch(sysdefs, bonds, bond_typeid, harmonic=HARMONIC, lj=LJ)
    s["coulomb"] = cavitymd.CoulombForceBatch(sysdefs, bonds, r_cut=15.0, accuracy=1e-5)
    s["integrator"] = cavitymd.VerletBatch(s["cavity"], velocities,
                                           extra_forces=[[m, c] for m, c in zip(s["molecular"].forces, s["coulomb"].forces)],
                                           langevin_index=photon, net_forces=True)
    s["recorder"] = cavitymd.BatchRecorder(s["cavity"], velocities, net_forces=s["integrator"].net_forces, capacity=64)
    s["thermostat"] = cavitymd.BussiReservoirBatch(kT=KT, tau=1000.0)
    s["thermostat"].attach(velocities, translational_dof=3.0 * len(molecules[0]) - 3.0, members=molecules)
    s["draw"] = cavitymd.StepDraw(12345, s["integrator"], s["thermostat"], dt=DT, gamma=GAMMA, kT=KT)
    s["adaptive"] = cavitymd.StepDraw(12345, s["integrator"], s["thermostat"], s["recorder"], dt=DT, gamma=GAMMA, kT=KT,
                                      tolerance=1e-3, dt_min=DT, dt_max=DT)   # the rule runs; the clamp keeps the step the example's
    for name in ("cavity", "molecular", "coulomb"):
        s[name].compute()
    s["integrator"].prime()
    return s


def body(s):
    s["integrator"].step_one()
    s["cavity"].compute()
    s["molecular"].compute()
    s["coulomb"].compute()
    s["integrator"].step_two()
    s["recorder"].record()


def step_torch(s):
    s["integrator"].draw_inputs(DT, gamma=GAMMA, kT=KT)
    body(s)
    s["thermostat"].draw_inputs(0, DT)
    s["thermostat"].step_async()


def step_fill(s):
    s["draw"].fill()
    body(s)
    s["thermostat"].step_async()


def capture(run, s):
    run(s)                                                                  # once outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(s)
    return graph


def sample(graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(INNER):
        graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / INNER


def alternate(graphs):
    """name -> (median, min, max) in us per replay; the graphs take turns, sample by sample"""
    for graph in graphs.values():
        for _ in range(WARMUP):
            graph.replay()
    torch.cuda.synchronize()
    samples = {name: [] for name in graphs}
    for _ in range(SAMPLES):
        for name, graph in graphs.items():
            samples[name].append(sample(graph))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in samples.items()}


def graph_nodes(run, s):
    """nodes (kernels, copies, memsets) of the graph `run` captures, from the runtime's dot dump of one more, untimed capture;
    None where the runtime gives none"""
    import re
    import tempfile
    try:
        graph = torch.cuda.CUDAGraph()
        graph.enable_debug_mode()
        with torch.cuda.graph(graph):
            run(s)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "graph.dot")
            graph.debug_dump(path)
            text = open(path).read()
    except Exception:
        return None
    return len([line for line in text.splitlines() if re.search(r"\[.*label", line) and "->" not in line]) or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="8,64,500")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script needs a GPU"
    fmt = lambda t: f"{t[0]:10.1f} ({t[1]:.1f} .. {t[2]:.1f})"  # noqa: E731
    lines = [f"# us per replay of the captured Coulomb step, N = 433, dt = {DT}: median (min .. max) of {SAMPLES} samples of {INNER} "
             f"replays after {WARMUP} warm-up replays, the variants alternated sample by sample",
             f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"{'B':>4}  {'variant':<44} {'us per replay':>28}"]
    for B in [int(x) for x in args.batches.split(",")]:
        s = build(B)
        graphs = {"step, torch draw_inputs x 2 (parent)": capture(step_torch, s), "step, one StepDraw.fill": capture(step_fill, s)}
        t = alternate(graphs)
        alone = alternate({"fill alone, fixed dt": capture(lambda s: s["draw"].fill(), s),
                           "fill alone, adaptive dt": capture(lambda s: s["adaptive"].fill(), s),
                           "torch draw_inputs x 2 alone": capture(lambda s: (s["integrator"].draw_inputs(DT, gamma=GAMMA, kT=KT),
                                                                             s["thermostat"].draw_inputs(0, DT)), s)})
        for name, v in list(t.items()) + list(alone.items()):
            lines.append(f"{B:>4}  {name:<44} {fmt(v):>28}")
            print(lines[-1], flush=True)
        a, b = t["step, torch draw_inputs x 2 (parent)"][0], t["step, one StepDraw.fill"][0]
        lines.append(f"{B:>4}  one fill against the torch draws, whole step: {a - b:+.1f} us ({b / a:.3f} of the parent's step)")
        print(lines[-1], flush=True)
        nodes = {"torch draw_inputs x 2": graph_nodes(step_torch, s), "one StepDraw.fill": graph_nodes(step_fill, s)}
        lines.append(f"{B:>4}  nodes in the captured step: " + ", ".join(f"{name}: {n if n is not None else 'not available'}"
                                                                       for name, n in nodes.items()))
        print(lines[-1], flush=True)
        state, vstate = s["draw"].state(), s["integrator"].state()
        assert int(vstate["out_of_box"].sum()) == 0 and int(state["exhausted"].sum()) == 0
        for name in ("adaptive", "draw", "thermostat", "recorder", "integrator", "coulomb", "molecular", "cavity"):
            s[name].close()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
