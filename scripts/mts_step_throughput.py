"""The captured outer step of the impulse multiple-time-step scheme against the captured plain step, in ONE process, the graphs
taking turns sample by sample so that clocks and caches treat them alike.  The systems are those of
scripts/coulomb_batch_throughput.py: diatomic lattices of 6 x 6 x 6 molecules plus the photon (N = 433, a 48-bohr box,
r_cut = 15, accuracy 1e-5: about 3400 k-vectors), bonded pairs excluded.

    python scripts/mts_step_throughput.py [--B 8 64 512] [--samples 11] [--n 2 4] [--parent-lib PATH/libcavmd.so]

    plain   {step one, cavity, molecular, Coulomb (two kernels), step two}, the step of examples/batch_coulomb_md_in_one_graph.py
            without its recorders and baths.  With --parent-lib its objects are created on THAT library (a build of the commit
            before the split existed), loaded next to this tree's; without it, on this tree's, whose kernels for that step have
            the same device code (profiles/coulomb_parts/device_code.txt).
    n       {kick; n x {step one, cavity, molecular, SHORT, step two}; LONG (two kernels); kick} on a split batch

One JSON line per B and reciprocal method; times are device time in microseconds per MD step (an outer step counts n), as median
and 10th and 90th percentile of the samples.  The expectation the scheme was proposed with is that the p90 at n = 4 lies below
the plain step's p10; `n4_p90_below_plain_p10` says whether it does.  --markdown prints the same as a table."""
import argparse
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

from coulomb_batch_throughput import ACCURACY, HARMONIC, LJ, R_CUT, timed  # noqa: E402  (the sibling script: same systems)

METHODS = ("direct", "factored")


def spread(samples, steps):
    import numpy as np
    s = 1e3 * np.asarray(samples) / steps
    return {"median_us": float(np.median(s)), "p10_us": float(np.percentile(s, 10)), "p90_us": float(np.percentile(s, 90))}


@contextlib.contextmanager
def library(path):
    """Objects created inside are created on the library at `path` (None: this tree's).  An older build lacks the newest
    entry points: those it has get their prototypes, and nothing here calls the others on it."""
    from cavitymd import _capi
    if path is None:
        yield
        return
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in _capi._PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    ours = _capi.load()
    _capi._lib = lib
    try:
        yield
    finally:
        _capi._lib = ours


def systems(B):
    import numpy as np
    import torch

    import cavitymd
    from cavitymd import synthetic
    cfgs = [synthetic.diatomic_lattice(6, 8.0, seed=k + 1) for k in range(B)]
    sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                           c["types"], c["box"], device="cuda")) for c in cfgs]
    bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
    rng = np.random.default_rng(0)
    velocities = []
    for c in cfgs:
        n = len(c["charge"])
        mass = np.where(c["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
        v = rng.normal(size=(n, 3)) * np.sqrt(3.167e-4 / mass)[:, None]
        velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
    return cfgs, sysdefs, bonds, velocities


def build(B, method, split):
    """cavity, molecular, Coulomb and integrator over fresh copies of the B systems"""
    import cavitymd
    cfgs, sysdefs, bonds, velocities = systems(B)
    cavity = cavitymd.CavityForceBatch(sysdefs, cfgs[0]["params"])
    mol = cavitymd.MolecularForceBatch(sysdefs, [b[0] for b in bonds], [b[1] for b in bonds], HARMONIC, LJ)
    extra = dict(split=True) if split else {}
    coulomb = cavitymd.CoulombForceBatch(sysdefs, [b[0] for b in bonds], r_cut=R_CUT, accuracy=ACCURACY, reciprocal=method, **extra)
    integ = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(mol.forces, coulomb.forces)])
    integ.set_inputs(1.0)                                 # a short step: the systems barely move while the step is timed
    cavity.compute()
    mol.compute()
    coulomb.compute()
    integ.prime()
    return {"cavity": cavity, "mol": mol, "coulomb": coulomb, "integ": integ, "keep": (cfgs, sysdefs, velocities)}


def capture(body):
    import torch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


def measure(args):
    import torch
    lines = []
    for B in args.B:
        for method in METHODS:
            with library(args.parent_lib):
                plain = build(B, method, split=False)
            mts = build(B, method, split=True)
            mts["integ"].kick_table(mts["coulomb"].long)

            def plain_step(o=plain):
                o["integ"].step_one()
                o["cavity"].compute()
                o["mol"].compute()
                o["coulomb"].compute()
                o["integ"].step_two()

            def outer(n, o=mts):
                o["integ"].kick(o["coulomb"].long, 0.5 * n)
                for _ in range(n):
                    o["integ"].step_one()
                    o["cavity"].compute()
                    o["mol"].compute()
                    o["coulomb"].compute(parts="short")
                    o["integ"].step_two()
                o["coulomb"].compute(parts="long")
                o["integ"].kick(o["coulomb"].long, 0.5 * n)

            graphs = {"plain": (capture(plain_step), 1)}
            for n in args.n:
                graphs[f"n{n}"] = (capture(lambda n=n: outer(n)), n)
            launches = max(3, min(50, 400 // B))
            samples = {name: [] for name in graphs}
            for _ in range(args.samples):
                for name, (g, _) in graphs.items():
                    samples[name].append(timed(g.replay, launches))
            line = {"B": B, "N": plain["coulomb"]._sizes[0], "K": plain["coulomb"].k_counts[0], "reciprocal": method,
                    "plain_library": "parent" if args.parent_lib else "this tree", "launches": launches, "samples": args.samples}
            for name, (_, steps) in graphs.items():
                line[name] = spread(samples[name], steps)
            if "n4" in line:
                line["n4_p90_below_plain_p10"] = line["n4"]["p90_us"] < line["plain"]["p10_us"]
                line["plain_over_n4"] = line["plain"]["median_us"] / line["n4"]["median_us"]
            state = mts["integ"].state()
            line["out_of_box"] = int(state["out_of_box"].sum())
            print(json.dumps(line), flush=True)
            lines.append(line)
            del graphs
            torch.cuda.synchronize()
            for o in (plain, mts):
                for name in ("integ", "coulomb", "mol", "cavity"):
                    o[name].close()
    if args.markdown:
        names = ["plain"] + [f"n{n}" for n in args.n]
        print("\n| B | reciprocal | " + " | ".join(f"{name}: median (p10 - p90)" for name in names) + " | n4 p90 < plain p10 |")
        print("|---|---|" + "---|" * (len(names) + 1))
        for line in lines:
            cells = [f"{line[name]['median_us']:.1f} ({line[name]['p10_us']:.1f} - {line[name]['p90_us']:.1f})" for name in names]
            print(f"| {line['B']} | {line['reciprocal']} | " + " | ".join(cells) + f" | {line.get('n4_p90_below_plain_p10', '')} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--samples", type=int, default=11)
    ap.add_argument("--n", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--markdown", action="store_true")
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
