"""Throughput of the Coulomb force evaluation (cavmd_coulomb_compute, two launches): ONE batch of B systems against B batches of
one system each, enqueued back to back on the same stream.  Both run the same two kernels, so what the ratio measures is the
batching.  The systems are diatomic lattices of 6 x 6 x 6 molecules plus the photon (N = 433, a 48-bohr box, r_cut = 15,
accuracy 1e-5: kappa = 0.226, about 3400 k-vectors), bonded pairs excluded.

    make -C cav-hoomd_amd/csrc coulomb_variants              # once, needs no GPU: the library with candidates of (S, T)
    python scripts/coulomb_batch_throughput.py [--variants] [--B 1 8 64] [--repeats 3] [--step]

Without --variants the product library is measured alone.  With it every build named in the Makefile's COULOMB_VARIANTS is
measured in a child process of its own (S = CAVMD_COULOMB_J_SPLIT and T = CAVMD_COULOMB_K_SPLIT are compile-time constants: one
library per candidate), one after the other.  One JSON line per (library, B): the median over the
repeats of the device time per evaluation (device events around `launches` back-to-back evaluations) for the one batch and for
the B single-system batches, and their ratio.  --step adds the share of a full captured MD step {step one, cavity, molecular,
Coulomb, step two} that the Coulomb evaluation takes (the same graph timed with and without it)."""
import argparse
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]
CSRC = os.path.join(ROOT, "cav-hoomd_amd", "csrc")

HARMONIC = {0: dict(k=2 * 0.36602, r0=2.281655158), 1: dict(k=2 * 0.71625, r0=2.0743522177)}
LJ = {("O", "O"): dict(epsilon=0.00016685201, sigma=6.230426584, r_cut=15.0),
      ("N", "N"): dict(epsilon=0.000083426, sigma=5.48277488, r_cut=15.0),
      ("N", "O"): dict(epsilon=0.00025027802, sigma=4.9832074319, r_cut=15.0)}
R_CUT, ACCURACY = 15.0, 1e-5


def timed(fn, launches):
    """milliseconds of device time per call of fn, `launches` calls between two events"""
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def measure(args):
    import numpy as np
    import torch

    import cavitymd
    from cavitymd import _capi, synthetic
    if args.library:
        _capi.LIB_PATH = args.library
    rows, S, k_rows, T = _capi.coulomb_order()
    for B in args.B:
        cfgs = [synthetic.diatomic_lattice(6, 8.0, seed=k + 1) for k in range(B)]
        sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                               c["types"], c["box"], device="cuda")) for c in cfgs]
        bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
        one = cavitymd.CoulombForceBatch(sysdefs, [b[0] for b in bonds], r_cut=R_CUT, accuracy=ACCURACY)
        singles = [cavitymd.CoulombForceBatch([sd], [b[0]], r_cut=R_CUT, accuracy=ACCURACY) for sd, b in zip(sysdefs, bonds)]
        one.compute()
        for s in singles:
            s.compute()
        torch.cuda.synchronize()
        for k, s in enumerate(singles):                       # the same kernels on the same input: the same bits
            assert torch.equal(s.forces[0], one.forces[k]), k

        def all_singles():
            for s in singles:
                s.compute()

        launches = max(3, min(200, int(2000 / B)))
        t_one = sorted(timed(one.compute, launches) for _ in range(args.repeats))[args.repeats // 2]
        t_singles = sorted(timed(all_singles, launches) for _ in range(args.repeats))[args.repeats // 2]
        line = {"library": os.path.basename(_capi.LIB_PATH), "S": S, "ROWS": rows, "T": T, "KROWS": k_rows, "B": B,
                "N": len(cfgs[0]["charge"]), "K": one.k_counts[0], "launches": launches, "one_batch_us": 1e3 * t_one,
                "single_batches_us": 1e3 * t_singles, "singles_over_batch": t_singles / t_one}
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
            integ = cavitymd.VerletBatch(cavity, velocities, extra_forces=[[m, c] for m, c in zip(mol.forces, one.forces)])
            integ.set_inputs(1.0)                             # a short step: the systems barely move while the step is timed
            cavity.compute()
            mol.compute()
            one.compute()
            integ.prime()
            torch.cuda.synchronize()
            graphs = {}
            for with_coulomb in (True, False):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    integ.step_one()
                    cavity.compute()
                    mol.compute()
                    if with_coulomb:
                        one.compute()
                    integ.step_two()
                graphs[with_coulomb] = g
            t_full = sorted(timed(graphs[True].replay, launches) for _ in range(args.repeats))[args.repeats // 2]
            t_rest = sorted(timed(graphs[False].replay, launches) for _ in range(args.repeats))[args.repeats // 2]
            line.update({"step_us": 1e3 * t_full, "step_without_coulomb_us": 1e3 * t_rest, "coulomb_share_of_step": 1.0 - t_rest / t_full})
            integ.close()
            mol.close()
            cavity.close()
        print(json.dumps(line), flush=True)
        one.close()
        for s in singles:
            s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--library", default=None, help="measure this build of the library (what --variants passes to its children)")
    args = ap.parse_args()
    if not args.variants:
        measure(args)
        return
    libs = sorted(glob.glob(os.path.join(CSRC, "libcavmd_coulomb_s*_t*.so")))
    if not libs:
        sys.exit("no candidate libraries: run `make -C cav-hoomd_amd/csrc coulomb_variants` first")
    for lib in libs:                                          # one fresh process per library: a process loads one libcavmd
        cmd = [sys.executable, os.path.abspath(__file__), "--library", lib, "--repeats", str(args.repeats), "--B"] + [str(b) for b in args.B]
        status = subprocess.run(cmd, timeout=300).returncode
        if status != 0:
            sys.exit(f"{os.path.basename(lib)} ended with status {status}: nothing more is started")


if __name__ == "__main__":
    main()
