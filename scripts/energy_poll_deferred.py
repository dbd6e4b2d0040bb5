"""What reading the energies after every step costs, with and without the result history.

usage: python scripts/energy_poll_deferred.py [--n 1000000] [--steps 2000] [--repeats 5] [--only a|b|c]

One workspace, driven through the C ABI at N = n + 1 over bench.py's ring of 7 HBM-cold frames (synthetic.config3 device
arrays, positions perturbed frame to frame).  Three loops, alternated, `--repeats` times each:
  (a) enqueue only;
  (b) enqueue + cavmd_energies() every step (the reference's EnergyTracker at period 1, read synchronously);
  (c) enqueue step k + cavmd_energies_at(k - 1) (cavitymd.EnergyHistory: one step of latency, no wait for step k).
Prints the median and min/max evaluations per second of each loop and the (c)/(a) ratio.  `--only c` runs loop (c)
alone (for `rocprofv3 --kernel-trace --stats -- python scripts/energy_poll_deferred.py --only c`)."""
import argparse
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
    from cavitymd import _cavitymd as _ext  # the enqueue bench.py's compute objects use (pybind11 over the C ABI)
except ImportError:
    _ext = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000, help="molecular particles (N = n + 1)")
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    args = ap.parse_args()

    cfg = synthetic.config3(n_molecular=args.n)
    n = len(cfg["charge"])
    p = cfg["params"]
    prm = _capi.make_params(p["omegac"], p["couplstr"], p["phmass"])
    L = [float(x) for x in cfg["box"]]
    L_typeid = cfg["L_typeid"]
    frames, cur = [], cfg
    for k in range(args.frames):
        if k:
            cur = synthetic.perturb(cur, k)
        pd = cavitymd.ParticleData.from_arrays(cur["position"], cur["typeid"], cur["charge"], cur["image"], cur["types"],
                                               cur["box"], device="cuda")
        frc = torch.empty((n, 4), dtype=torch.float64, device="cuda")
        frames.append((pd.getPositions().data_ptr(), pd.getCharges().data_ptr(), pd.getImages().data_ptr(), frc.data_ptr(),
                       pd, frc))
    ws = _capi.Workspace(n)
    h = ws.handle.value
    nf = len(frames)

    if _ext is not None:
        def enqueue(s):
            f = frames[s % nf]
            _ext.compute_hoomd(h, 0, n, f[0], f[1], f[2], L[0], L[1], L[2], L_typeid, prm.omegac, prm.couplstr, prm.K,
                               prm.phmass, f[3])
    else:
        def enqueue(s):
            f = frames[s % nf]
            ws.compute_hoomd(0, n, f[0], f[1], f[2], L, L_typeid, prm, f[3])

    def loop(kind, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "a":
            for s in range(steps):
                enqueue(s)
        elif kind == "b":
            for s in range(steps):
                enqueue(s)
                ws.energies()
        else:
            first = ws.last_sequence() + 1
            for s in range(steps):
                enqueue(s)
                if s:
                    ws.energies_at(first + s - 1)
            ws.energies_at(first + steps - 1)
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)

    kinds = [args.only] if args.only else ["a", "b", "c"]
    for k in kinds:                       # warm-up: every frame, code path and the getters touched once
        loop(k, 2 * nf)
    rates = {k: [] for k in kinds}
    for _ in range(args.repeats):
        for k in kinds:
            rates[k].append(loop(k, args.steps))

    label = {"a": "(a) enqueue only", "b": "(b) enqueue + energies() every step",
             "c": "(c) enqueue k + energies_at(k-1)"}
    dev = ws.device_info()
    print(f"N={n} frames={nf} steps={args.steps} repeats={args.repeats} device={dev['arch']} "
          f"binding={'pybind11' if _ext is not None else 'ctypes'} result_history={ws.get_tunable('result_history')}")
    med = {}
    for k in kinds:
        v = np.array(rates[k])
        med[k] = float(np.median(v))
        print(f"{label[k]:<40s} median {med[k]:9.0f} evals/s ({1e6 / med[k]:6.2f} us)   min {v.min():9.0f}   max {v.max():9.0f}"
              f"   all {' '.join(f'{x:.0f}' for x in v)}")
    if "a" in med and "c" in med:
        print(f"(c)/(a) = {med['c'] / med['a']:.3f}")
    if "a" in med and "b" in med:
        print(f"(b)/(a) = {med['b'] / med['a']:.3f}")


if __name__ == "__main__":
    main()
