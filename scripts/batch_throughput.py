"""One batched launch against the sequential sweep it replaces.

usage: python scripts/batch_throughput.py [--sizes 1,8,64,256,512,2048] [--n 500] [--sweeps 200] [--repeats 3]
                                          [--ragged] [--only batched|sequential] [--json PATH]

For every B: B independent systems of N = n + 1 particles (synthetic.diatomic_box, seeds 1..B), each with its own device
arrays.  Two ways to evaluate all of them once ("a sweep"), alternated `--repeats` times in this one process:
  sequential   B calls of cavmd_compute_hoomd on B workspaces, one stream: what a caller had before the batch existed;
  batched      one cavmd_batch_compute.
Every sweep ends in a stream synchronise and is timed on the host clock around it (`--sweeps` sweeps per repeat, after a
warm-up of every shape).  Printed per B and variant: median, p10 and p90 microseconds per sweep, system evaluations per
second, and the fraction of 8 TB/s that 84 N bytes per system amount to.  `--ragged` adds one mixed batch (sizes 64..4096).
`--only` runs one variant alone, for `rocprofv3 --kernel-trace --stats -- python scripts/batch_throughput.py --only batched`.
A measurement path: it needs a GPU and has no fallback."""
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
from cavitymd import _capi, synthetic  # noqa: E402

try:
    from cavitymd import _cavitymd as _ext  # the enqueue CavityForceComputeHIP uses (pybind11 over the C ABI)
except ImportError:
    _ext = None

PEAK_BYTES_PER_S = 8.0e12
BYTES_PER_PARTICLE = 84  # pos 32 + charge 8 + image 12 read, force 32 written
RAGGED = [64, 128, 256, 501, 501, 501, 501, 1024, 1024, 2048, 4096] * 6  # 66 systems


class System:
    def __init__(self, n_molecular, seed):
        cfg = synthetic.diatomic_box(n_molecular, seed=seed, box_length=40.0)
        self.pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                                    cfg["box"], device="cuda")
        self.n = self.pd.getN()
        self.frc = torch.empty((self.n, 4), dtype=torch.float64, device="cuda")
        p = cfg["params"]
        self.prm = _capi.make_params(p["omegac"], p["couplstr"], p["phmass"])
        self.box = [float(x) for x in cfg["box"]]
        self.ptrs = (self.pd.getPositions().data_ptr(), self.pd.getCharges().data_ptr(), self.pd.getImages().data_ptr(),
                     self.frc.data_ptr())
        self.ws = None

    def item(self):
        return _capi.batch_item(self.n, *self.ptrs, self.box, 2, self.prm)


def measure(systems, sweeps, repeats, only):
    B = len(systems)
    for s in systems:
        if s.ws is None:
            s.ws = _capi.Workspace(s.n)
            s.ws.set_tunable("small_system_max_n", max(1024, min(s.n, 1 << 20)))  # the single-block kernel at every size here
    holder = _capi.Workspace(1)
    batch = _capi.Batch(holder, [s.item() for s in systems], history_depth=2)

    if _ext is not None:
        calls = [(s.ws.handle.value, 0, s.n, s.ptrs[0], s.ptrs[1], s.ptrs[2], s.box[0], s.box[1], s.box[2], 2, s.prm.omegac,
                  s.prm.couplstr, s.prm.K, s.prm.phmass, s.ptrs[3]) for s in systems]

        def sequential():
            f = _ext.compute_hoomd
            for c in calls:
                f(*c)
    else:
        def sequential():
            for s in systems:
                s.ws.compute_hoomd(0, s.n, s.ptrs[0], s.ptrs[1], s.ptrs[2], s.box, 2, s.prm, s.ptrs[3])

    def batched():
        batch.compute(0)

    variants = {"sequential": sequential, "batched": batched}
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
    rows = {}
    n_total = sum(s.n for s in systems)
    for name, v in times.items():
        us = np.array(v) * 1e6
        med = float(np.median(us))
        rows[name] = {"B": B, "particles": n_total, "sweeps": len(v), "median_us": med, "p10_us": float(np.percentile(us, 10)),
                      "p90_us": float(np.percentile(us, 90)), "system_evals_per_s": B / (med * 1e-6),
                      "fraction_of_peak_bandwidth": BYTES_PER_PARTICLE * n_total / (med * 1e-6) / PEAK_BYTES_PER_S}
    batch.close()
    holder.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256,512,2048")
    ap.add_argument("--n", type=int, default=500, help="molecular particles per system (N = n + 1)")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--only", choices=("batched", "sequential"), default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "batch_throughput.py measures on a GPU; there is no fallback"
    sizes = [int(x) for x in args.sizes.split(",") if x]
    pool = [System(args.n, seed) for seed in range(1, max(sizes) + 1)]
    out = {"binding": "pybind11" if _ext is not None else "ctypes", "N": args.n + 1, "rows": []}
    print(f"N={args.n + 1} sweeps/repeat={args.sweeps} repeats={args.repeats} binding={out['binding']}")
    print(f"{'B':>6s} {'variant':<11s} {'median us':>10s} {'p10':>9s} {'p90':>9s} {'sys evals/s':>12s} {'of 8 TB/s':>10s}")
    cases = [(f"{B}", pool[:B]) for B in sizes]
    if args.ragged:
        cases.append(("ragged", [System(n - 1 if n % 2 else n, 1000 + k) for k, n in enumerate(RAGGED)]))
    for label, systems in cases:
        rows = measure(systems, args.sweeps, args.repeats, args.only)
        for name, r in rows.items():
            r["case"] = label
            r["variant"] = name
            out["rows"].append(r)
            print(f"{label:>6s} {name:<11s} {r['median_us']:10.2f} {r['p10_us']:9.2f} {r['p90_us']:9.2f} "
                  f"{r['system_evals_per_s']:12.0f} {r['fraction_of_peak_bandwidth']:10.4f}")
        if "sequential" in rows and "batched" in rows:
            s, b = rows["sequential"], rows["batched"]
            print(f"{label:>6s} sequential/batched = {s['median_us'] / b['median_us']:.2f}x; sequential p10-p90 spread "
                  f"{s['p90_us'] - s['p10_us']:.2f} us, gain {s['median_us'] - b['median_us']:.2f} us")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
