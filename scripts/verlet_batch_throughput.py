"""Microseconds per MD step {velocity-Verlet step one, cavity force, step two} of B replicas of N = 501, B = 8, 64, 500.

Compared: the batch integrator (cavitymd.VerletBatch, two launches per step for all replicas) against the only integration the
tree had before it, the torch element-wise update of tests/test_gpu_dynamics.py (unwrapped positions, images re-derived with
floor), applied (a) per system in a Python loop and (b) once on tensors stacked over the replicas.  The force is one
CavityForceBatch launch per step in every variant, so the differences are the integrator's alone.  Every variant is timed
eagerly and replayed from a captured graph.

Method: per variant 20 warm-up steps, then 15 samples of 20 steps each between two events on the stream; a sample is the
elapsed time / 20; the table gives the median and the min .. max of the samples.  The trajectory advances while it is timed.

    python scripts/verlet_batch_throughput.py [--out profiles/verlet_batch/table.txt] [--batches 8,64,500]
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

DT, WARMUP, SAMPLES, INNER = 5.0, 20, 15, 20


def build(B, stacked=False):
    """B config-1 replicas; stacked: positions, images, velocities and forces of all replicas are views of one tensor each"""
    cfgs = [synthetic.config1(seed=k + 1) for k in range(B)]
    n = len(cfgs[0]["charge"])
    rng = np.random.default_rng(42)
    pos = np.zeros((B, n, 4))
    vel = np.zeros((B, n, 4))
    img = np.zeros((B, n, 3), dtype=np.int32)
    for k, cfg in enumerate(cfgs):
        mass = np.where(cfg["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
        pos[k, :, :3] = cfg["position"]
        pos[k, :, 3] = cavitymd.state.type_tag_as_double(cfg["typeid"])
        img[k] = cfg["image"]
        vel[k, :, :3] = rng.normal(size=(n, 3)) * np.sqrt(3.167e-4 / mass)[:, None]
        vel[k, :, 3] = mass
    pos, vel, img = torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda(), torch.from_numpy(img).cuda()
    sysdefs = []
    for k, cfg in enumerate(cfgs):
        chg = torch.from_numpy(np.ascontiguousarray(cfg["charge"], dtype=np.float64)).cuda()
        sysdefs.append(cavitymd.SystemDefinition(cavitymd.ParticleData(pos[k], chg, img[k], cfg["types"], cfg["box"])))
    forces = cavitymd.CavityForceBatch(sysdefs, cfgs[0]["params"])
    frc = None
    if stacked:
        # the force batch writes into views of ONE (B, N, 4) tensor, so that the stacked update reads it without a gather
        frc = torch.zeros((B, n, 4), dtype=torch.float64, device="cuda")
        forces._force = [frc[k] for k in range(B)]
        forces.refresh()
    L = torch.tensor(cfgs[0]["box"], dtype=torch.float64, device="cuda")
    return {"B": B, "pos": pos, "vel": vel, "img": img, "frc": frc, "forces": forces, "L": L}


def ours(s):
    integrator = cavitymd.VerletBatch(s["forces"], [s["vel"][k] for k in range(s["B"])])
    integrator.set_inputs(DT)
    s["forces"].compute()
    integrator.prime()
    s["keep"] = integrator

    def step():
        integrator.step_one()
        s["forces"].compute()
        integrator.step_two()
    return step


def torch_per_system(s):
    """tests/test_gpu_dynamics.py's update, one system after the other; one force launch for all"""
    B, L, forces = s["B"], s["L"], s["forces"]
    pos, vel, img = [s["pos"][k] for k in range(B)], [s["vel"][k] for k in range(B)], [s["img"][k] for k in range(B)]
    r = [(pos[k][:, :3] + img[k] * L).clone() for k in range(B)]
    m = [vel[k][:, 3:4] for k in range(B)]
    F = forces.forces
    forces.compute()

    def step():
        for k in range(B):
            vel[k][:, :3] += 0.5 * DT * F[k][:, :3] / m[k]
            r[k] += DT * vel[k][:, :3]
            image = torch.floor((r[k] + L / 2) / L)
            pos[k][:, :3] = r[k] - image * L
            img[k].copy_(image.to(torch.int32))
        forces.compute()
        for k in range(B):
            vel[k][:, :3] += 0.5 * DT * F[k][:, :3] / m[k]
    return step


def torch_stacked(s):
    """the same update once on (B, N, .) tensors"""
    L, forces, pos, vel, img, F = s["L"], s["forces"], s["pos"], s["vel"], s["img"], s["frc"]
    r = (pos[:, :, :3] + img * L).clone()
    m = vel[:, :, 3:4]
    forces.compute()

    def step():
        vel[:, :, :3] += 0.5 * DT * F[:, :, :3] / m
        r.add_(DT * vel[:, :, :3])
        image = torch.floor((r + L / 2) / L)
        pos[:, :, :3] = r - image * L
        img.copy_(image.to(torch.int32))
        forces.compute()
        vel[:, :, :3] += 0.5 * DT * F[:, :, :3] / m
    return step


def time_steps(run):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    samples = []
    for _ in range(SAMPLES):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(INNER):
            run()
        stop.record()
        stop.synchronize()
        samples.append(start.elapsed_time(stop) * 1e3 / INNER)
    return float(np.median(samples)), float(min(samples)), float(max(samples))


def measure(make, B, stacked=False):
    """(eager, captured) timings of one variant on a fresh set of replicas"""
    out = []
    for captured in (False, True):
        s = build(B, stacked)
        step = make(s)
        torch.cuda.synchronize()
        if captured:
            step()                                                          # once outside the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            out.append(time_steps(graph.replay))
        else:
            out.append(time_steps(step))
        assert bool(torch.isfinite(s["vel"]).all()) and bool(torch.isfinite(s["pos"][:, :, :3]).all())
        if "keep" in s:
            state = s["keep"].state()
            assert int(state["out_of_box"].sum()) == 0 and int(state["steps"].min()) >= WARMUP + SAMPLES * INNER
            s["keep"].close()
        s["forces"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="8,64,500")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script needs a GPU"
    lines = [f"# us per MD step {{step one, cavity force, step two}}, N = 501, dt = {DT}: median (min .. max) of {SAMPLES} samples of "
             f"{INNER} steps after {WARMUP} warm-up steps",
             f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"{'B':>4}  {'variant':<34} {'eager':>28} {'captured graph':>28}"]
    for B in [int(x) for x in args.batches.split(",")]:
        rows = [("VerletBatch (2 launches + force)", measure(ours, B)),
                ("torch element-wise, per system", measure(torch_per_system, B)),
                ("torch element-wise, stacked", measure(torch_stacked, B, stacked=True))]
        for name, (eager, captured) in rows:
            fmt = lambda t: f"{t[0]:10.1f} ({t[1]:.1f} .. {t[2]:.1f})"  # noqa: E731
            lines.append(f"{B:>4}  {name:<34} {fmt(eager):>28} {fmt(captured):>28}")
            print(lines[-1], flush=True)
        base = rows[0][1][1][0]
        lines.append(f"{B:>4}  captured, relative to VerletBatch: per system x{rows[1][1][1][0] / base:.1f}, stacked "
                     f"x{rows[2][1][1][0] / base:.2f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
