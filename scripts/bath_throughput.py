"""Microseconds per replay of the captured {step one, cavity force batch, step two} of B replicas of N = 501 (config 1: 500
molecular particles and the photon), B = 8, 64, 500, with a Langevin bath on all 500 molecular particles of every replica and
step two being

  (a) ``VerletBatch.step_two`` (cavmd_verlet_step_two) with NO bath: the parent's kernel, the price of no bath;
  (b) ``LangevinBathBatch.step_two`` (cavmd_bath_step_two): the bath drawn inside step two;
  (c) what a user did before: ``torch.rand`` plus the element-wise bath force on stacked tensors, written into a further force
      array of the integrator, then (a).

Method: the three graphs are built on the SAME systems and alternated sample by sample, so that a drift of the clocks hits all:
20 warm-up replays each, then 15 samples of 20 replays between two events on the stream; a sample is the elapsed time / 20;
the table gives the median and the min .. max of the samples.  The trajectory advances while it is timed (the variants share
positions and velocities; each integrator keeps its own accelerations, so the physics of the mixture means nothing).

    python scripts/bath_throughput.py [--out profiles/bath_batch/table.txt] [--batches 8,64,500] [--only b]
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

KT, DT, GAMMA, WARMUP, SAMPLES, INNER = 3.167e-4, 2.0, 1e-3, 20, 15, 20


def build(B):
    rng = np.random.default_rng(0)
    sysdefs, rows = [], []
    for k in range(B):
        cfg = synthetic.config1(seed=k + 1)
        pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                               cfg["box"], device="cuda")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        n = pd.getN()
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
        v = rng.normal(size=(n, 3)) * np.sqrt(KT / mass)[:, None]
        rows.append(np.concatenate([v, mass[:, None]], axis=1))
    assert n == 501
    molecular = torch.from_numpy(np.tile(cfg["typeid"] != 2, B)).cuda()
    s = {"B": B, "N": n}
    s["vel"] = torch.from_numpy(np.concatenate(rows)).cuda()                 # (B N, 4): every velocity array is a row-slice
    s["bath_force"] = torch.zeros((B * n, 4), dtype=torch.float64, device="cuda")
    # gamma_j = GAMMA m_j on the molecular particles (x = gamma dt / 2 m = 1e-3), 0 on the photon
    s["gamma"] = torch.where(molecular, GAMMA * s["vel"][:, 3], torch.zeros_like(s["vel"][:, 3])).contiguous()
    s["coeff"] = torch.sqrt(((6.0 * s["gamma"]) * KT) / DT)
    velocities = [s["vel"][k * n:(k + 1) * n] for k in range(B)]
    s["cavity"] = cavitymd.CavityForceBatch(sysdefs, cfg["params"])
    s["plain"] = cavitymd.VerletBatch(s["cavity"], velocities)
    s["extra"] = cavitymd.VerletBatch(s["cavity"], velocities, extra_forces=[[s["bath_force"][k * n:(k + 1) * n]] for k in range(B)])
    s["bath"] = cavitymd.LangevinBathBatch(s["plain"], [s["gamma"][k * n:(k + 1) * n] for k in range(B)], KT, seed=12345)
    s["cavity"].compute()
    for name in ("plain", "extra"):
        s[name].prime()
        s[name].set_inputs(DT)
    return s


def step_no_bath(s):
    s["plain"].step_one()
    s["cavity"].compute()
    s["plain"].step_two()


def step_bath(s):
    s["plain"].step_one()
    s["cavity"].compute()
    s["bath"].step_two()


def step_torch(s):
    s["extra"].step_one()
    s["cavity"].compute()
    u = torch.rand((s["B"] * s["N"], 3), dtype=torch.float64, device="cuda")
    s["bath_force"][:, :3] = (2.0 * u - 1.0) * s["coeff"][:, None] - s["gamma"][:, None] * s["vel"][:, :3]
    s["extra"].step_two()


VARIANTS = {"a": ("(a) cavmd_verlet_step_two, no bath (parent)", step_no_bath), "b": ("(b) cavmd_bath_step_two", step_bath),
            "c": ("(c) torch.rand + bath force array, then (a)", step_torch)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="8,64,500")
    ap.add_argument("--only", default="abc", help="the variants to capture, e.g. b for a profiler run of the new kernel alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script needs a GPU"
    fmt = lambda t: f"{t[0]:10.1f} ({t[1]:.1f} .. {t[2]:.1f})"  # noqa: E731
    lines = [f"# us per replay of the captured {{step one, cavity force batch, step two}}, N = 501, 500 coupled, dt = {DT}: median "
             f"(min .. max) of {SAMPLES} samples of {INNER} replays after {WARMUP} warm-up replays, the variants alternated sample by "
             f"sample",
             f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"{'B':>4}  {'variant':<48} {'us per replay':>28}"]
    for B in [int(x) for x in args.batches.split(",")]:
        s = build(B)
        t = alternate({VARIANTS[v][0]: capture(VARIANTS[v][1], s) for v in args.only})
        for name, v in t.items():
            lines.append(f"{B:>4}  {name:<48} {fmt(v):>28}")
            print(lines[-1], flush=True)
        if set("abc") <= set(args.only):
            a, b, c = (t[VARIANTS[v][0]][0] for v in "abc")
            lines.append(f"{B:>4}  the bath in step two costs {b - a:+.1f} us over no bath; against the torch bath force {b - c:+.1f} us "
                         f"({b / c:.3f} of its step)")
            print(lines[-1], flush=True)
        if "b" in args.only:
            state = s["bath"].state()
            assert state["coupled"].tolist() == [500] * B and int(s["plain"].state()["out_of_box"].sum()) == 0
        for name in ("bath", "extra", "plain", "cavity"):
            s[name].close()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
