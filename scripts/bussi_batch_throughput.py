"""One batched thermostat launch against the sequential sweep it replaces.

usage: python scripts/bussi_batch_throughput.py [--sizes 1,8,64,256,512,2048] [--n 501] [--sweeps 200] [--repeats 3]
                                                [--ragged] [--only batched|sequential] [--parent-lib PATH] [--json PATH]

For every B: B independent velocity arrays of n particles.  Ways to step all of them once ("a sweep"), alternated `--repeats`
times in this one process:
  sequential         B calls of cavmd_bussi_step_device on B workspaces, one stream (two launches each): what a caller had
                     before the batch existed;
  sequential@parent  the same loop through a libcavmd.so built from the parent commit (`--parent-lib`), in the same run;
  batched            one cavmd_bussi_batch_step (its input rows already on the device).
Every sweep ends in a stream synchronise and is timed on the host clock around it (`--sweeps` sweeps per repeat, after a
warm-up of every shape).  tau is large and the variates are fixed, so the velocities stay bounded over any number of sweeps.
Printed per B and variant: median, p10 and p90 microseconds per sweep and system steps per second.  `--ragged` adds one mixed
batch (sizes 64..4096).  `--only` runs one variant alone, for `rocprofv3 --kernel-trace --stats -- python
scripts/bussi_batch_throughput.py --only batched`.  A measurement path: it needs a GPU and has no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cavitymd import _capi  # noqa: E402

RAGGED = [64, 128, 256, 501, 501, 501, 501, 1024, 1024, 2048, 4096] * 6  # 66 systems
DT, TAU, R, GAMMA_OVER_SHAPE = 0.005, 50.0, 0.1, 1.0


class System:
    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        v = np.zeros((n, 4))
        v[:, 3] = 1.0
        v[:, :3] = rng.normal(0.0, 1e-3, (n, 3))
        self.n = n
        self.vel = torch.from_numpy(v).cuda()
        self.dof = 3.0 * n - 3.0
        self.kT = float((v[:, :3] ** 2).sum() / self.dof)
        self.gamma = GAMMA_OVER_SHAPE * (self.dof - 1.0) / 2.0
        self.ws = None
        self.parent_ws = None


def _parent(path):
    lib = ctypes.CDLL(path)
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    lib.cavmd_create.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.cavmd_bussi_step_device.argtypes = [vp, vp, vp, vp, ctypes.c_size_t] + [dbl] * 6
    lib.cavmd_destroy.argtypes = [vp]
    assert not hasattr(lib, "cavmd_bussi_batch_step"), "--parent-lib must be the library of the parent commit"
    return lib


def measure(systems, sweeps, repeats, only, parent):
    B = len(systems)
    for s in systems:
        if s.ws is None:
            s.ws = _capi.Workspace(s.n)
        if parent is not None and s.parent_ws is None:
            s.parent_ws = ctypes.c_void_p()
            assert parent.cavmd_create(-1, s.n, ctypes.byref(s.parent_ws)) == 0
    holder = _capi.Workspace(1)
    batch = _capi.BussiBatch(holder, [_capi.bussi_batch_item(s.vel.data_ptr(), 0, s.n, s.dof) for s in systems])
    arr = (_capi.BussiBatchInput * B)(*[_capi.bussi_batch_input_make(DT, s.kT, TAU, R, s.gamma) for s in systems])
    rows = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.float64).reshape(B, 8).copy()).cuda()
    rows_ptr = rows.data_ptr()
    lib = _capi.load()
    calls = [(s.ws.handle, None, s.vel.data_ptr(), None, s.n, s.dof, DT, s.kT, TAU, R, s.gamma) for s in systems]

    def sequential():
        f = lib.cavmd_bussi_step_device
        for c in calls:
            f(*c)

    def batched():
        batch.step(0, rows_ptr)

    variants = {"sequential": sequential, "batched": batched}
    if parent is not None:
        pcalls = [(s.parent_ws,) + c[1:] for s, c in zip(systems, calls)]

        def sequential_parent():
            f = parent.cavmd_bussi_step_device
            for c in pcalls:
                f(*c)

        variants = {"sequential@parent": sequential_parent, "sequential": sequential, "batched": batched}
    if only:
        variants = {only: variants[only]}
    sync = torch.cuda.synchronize
    for fn in variants.values():              # warm-up of every shape and code path
        for _ in range(10):
            fn()
        sync()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for name, fn in variants.items():     # alternated
            for _ in range(sweeps):
                t0 = time.perf_counter()
                fn()
                sync()
                times[name].append(time.perf_counter() - t0)
    out = {}
    n_total = sum(s.n for s in systems)
    for name, v in times.items():
        us = np.array(v) * 1e6
        med = float(np.median(us))
        out[name] = {"B": B, "particles": n_total, "sweeps": len(v), "median_us": med, "p10_us": float(np.percentile(us, 10)),
                     "p90_us": float(np.percentile(us, 90)), "system_steps_per_s": B / (med * 1e-6)}
    states = batch.read()
    assert all(np.isfinite(x.last_alpha) and x.refused == 0 for x in states)
    batch.close()
    holder.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256,512,2048")
    ap.add_argument("--n", type=int, default=501, help="particles per system")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--only", choices=("batched", "sequential"), default=None)
    ap.add_argument("--parent-lib", default=None, help="libcavmd.so built from the parent commit: its sequential loop is timed too")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bussi_batch_throughput.py measures on a GPU; there is no fallback"
    parent = _parent(args.parent_lib) if (args.parent_lib and not args.only) else None
    sizes = [int(x) for x in args.sizes.split(",") if x]
    pool = [System(args.n, seed) for seed in range(1, max(sizes) + 1)]
    out = {"n": args.n, "rows": []}
    print(f"n={args.n} sweeps/repeat={args.sweeps} repeats={args.repeats} parent={'yes' if parent is not None else 'no'}")
    print(f"{'B':>6s} {'variant':<18s} {'median us':>10s} {'p10':>9s} {'p90':>9s} {'sys steps/s':>12s}")
    cases = [(f"{B}", pool[:B]) for B in sizes]
    if args.ragged:
        cases.append(("ragged", [System(n, 1000 + k) for k, n in enumerate(RAGGED)]))
    for label, systems in cases:
        rows = measure(systems, args.sweeps, args.repeats, args.only, parent)
        for name, r in rows.items():
            r["case"] = label
            r["variant"] = name
            out["rows"].append(r)
            print(f"{label:>6s} {name:<18s} {r['median_us']:10.2f} {r['p10_us']:9.2f} {r['p90_us']:9.2f} "
                  f"{r['system_steps_per_s']:12.0f}")
        ref = rows.get("sequential@parent", rows.get("sequential"))
        if ref is not None and "batched" in rows:
            b = rows["batched"]
            print(f"{label:>6s} {ref['variant']}/batched = {ref['median_us'] / b['median_us']:.2f}x; batched p90 {b['p90_us']:.2f} "
                  f"{'<' if b['p90_us'] < ref['p10_us'] else '>='} {ref['variant']} p10 {ref['p10_us']:.2f}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
