"""The two reciprocal-space methods of the Coulomb force batch against each other (cavmd_ewald_set_reciprocal: "direct", one sincos
per particle and k-vector, and "factored", per-axis phase factors), on ONE batch of B systems in ONE process, the methods
alternating sample by sample so that clocks and caches treat them alike.  The systems are those of
scripts/coulomb_batch_throughput.py: diatomic lattices of 6 x 6 x 6 molecules plus the photon (N = 433, a 48-bohr box,
r_cut = 15, accuracy 1e-5: kappa = 0.226, about 3400 k-vectors), bonded pairs excluded.

    python scripts/ewald_reciprocal_throughput.py [--B 1 8 64 512] [--samples 15] [--step]

One JSON line per B.  Per sample, device events bracket `launches` back-to-back evaluations; per method the line gives the
median and the 10th and 90th percentile of the samples, in microseconds per evaluation.  --step times, the same way, the
captured MD step {step one, cavity, molecular, Coulomb, step two} with each method (a graph keeps the method it was captured
with) and without the Coulomb evaluation.  Before anything is timed the two methods' forces are compared: they agree to
rounding, not bit for bit (tests/coulomb_factored_mirror.py derives the bound; here the largest difference is printed)."""
import argparse
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

from coulomb_batch_throughput import ACCURACY, HARMONIC, LJ, R_CUT, timed  # noqa: E402  (the sibling script: same systems)

METHODS = ("direct", "factored")


def spread(samples):
    import numpy as np
    s = 1e3 * np.asarray(samples)
    return {"median_us": float(np.median(s)), "p10_us": float(np.percentile(s, 10)), "p90_us": float(np.percentile(s, 90))}


def alternating(calls, launches, samples):
    """calls: name -> callable; -> name -> the samples of `timed`, the names taking turns"""
    out = {name: [] for name in calls}
    for _ in range(samples):
        for name, fn in calls.items():
            out[name].append(timed(fn, launches))
    return out


def measure(args):
    import numpy as np
    import torch

    import cavitymd
    from cavitymd import synthetic
    for B in args.B:
        cfgs = [synthetic.diatomic_lattice(6, 8.0, seed=k + 1) for k in range(B)]
        sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                               c["types"], c["box"], device="cuda")) for c in cfgs]
        bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
        coulomb = cavitymd.CoulombForceBatch(sysdefs, [b[0] for b in bonds], r_cut=R_CUT, accuracy=ACCURACY)
        forces = {}
        for method in METHODS:
            coulomb.set_reciprocal(method)
            coulomb.compute()
            torch.cuda.synchronize()
            forces[method] = torch.stack([f.clone() for f in coulomb.forces]) if B <= 64 else coulomb.forces[0].clone()
        apart = float((forces["direct"] - forces["factored"]).abs().max())
        scale = float(forces["direct"].abs().max())

        def evaluate(method):
            def fn():
                coulomb.set_reciprocal(method)                # a host-side switch: no device work
                coulomb.compute()
            return fn

        launches = max(3, min(50, 400 // B))
        line = {"B": B, "N": len(cfgs[0]["charge"]), "K": coulomb.k_counts[0], "launches": launches, "samples": args.samples,
                "largest_force_difference": apart, "largest_force": scale}
        for method, samples in alternating({m: evaluate(m) for m in METHODS}, launches, args.samples).items():
            line[method] = spread(samples)
        line["factored_p90_below_direct_p10"] = line["factored"]["p90_us"] < line["direct"]["p10_us"]
        line["direct_over_factored"] = line["direct"]["median_us"] / line["factored"]["median_us"]
        if args.step:
            velocities = []
            rng = np.random.default_rng(0)
            for c in cfgs:
                n = len(c["charge"])
                mass = np.where(c["typeid"] == 2, 1.0, rng.uniform(2.5e4, 3.0e4, n))
                v = rng.normal(size=(n, 3)) * np.sqrt(3.167e-4 / mass)[:, None]
                velocities.append(torch.from_numpy(np.concatenate([v, mass[:, None]], axis=1)).cuda())
            cavity = cavitymd.CavityForceBatch(sysdefs, cfgs[0]["params"])
            mol = cavitymd.MolecularForceBatch(sysdefs, [b[0] for b in bonds], [b[1] for b in bonds], HARMONIC, LJ)
            integ = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(mol.forces, coulomb.forces)])
            integ.set_inputs(1.0)                             # a short step: the systems barely move while the step is timed
            cavity.compute()
            mol.compute()
            coulomb.compute()
            integ.prime()
            torch.cuda.synchronize()
            graphs = {}
            for name in METHODS + ("without",):
                if name != "without":
                    coulomb.set_reciprocal(name)              # before the capture: a captured launch keeps its kernels
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    integ.step_one()
                    cavity.compute()
                    mol.compute()
                    if name != "without":
                        coulomb.compute()
                    integ.step_two()
                graphs[name] = g
            step = alternating({name: g.replay for name, g in graphs.items()}, launches, args.samples)
            line["step"] = {name: spread(samples) for name, samples in step.items()}
            for method in METHODS:
                line["step"][method]["coulomb_share"] = 1.0 - line["step"]["without"]["median_us"] / line["step"][method]["median_us"]
            integ.close()
            mol.close()
            cavity.close()
        print(json.dumps(line), flush=True)
        coulomb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--step", action="store_true")
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
