"""Throughput of the molecular force launch (cavmd_molecular_compute) at the production size: B replicas of config 1 (N = 501,
a 40-bohr box, the driver's bond and Lennard-Jones constants, r_cut = 15), against the same forces computed with torch fp64
broadcasting on the same GPU.

    make -C cav-hoomd_amd/csrc molecular_variants            # once, needs no GPU: the library with S = 1, 4 and 16
    python scripts/molecular_batch_throughput.py [--variants] [--B 1 8 64 512] [--repeats 5]

Without --variants the product library is measured alone.  With it every build of CAVMD_MOLECULAR_J_SPLIT is measured in a
child process of its own (S is a compile-time constant: one library per candidate), the candidates alternating within each
repeat.  One JSON line per (library, B): the median over the repeats of the device time per launch (device events around
`launches` back-to-back launches), pair evaluations per second (B N (N - 1) per launch: what the kernel walks), the share of
the fp64 vector issue rate those evaluations account for, and the torch baseline's time with the ratio to it.  The kernel's
forces are compared with the baseline's before anything is timed."""
import argparse
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
# fp64 operations of one pair evaluation that contributes, counted from the contract in include/cavmd.h: 3 subtractions and 3
# image corrections, 5 for rsq, 1 division, 2 + 3 + 4 for r6inv, fdivr and e, 8 for the four accumulations
FLOPS_PER_PAIR = 29
PEAK_FP64_VECTOR = 78.6e12   # MI355X vector fp64, FMA counted as two: an FMA-free kernel can reach half of it


def torch_baseline(pos, typeid, box, tab, bonded, K, r0):
    """(B, N, 4): the same forces with torch fp64 broadcasting (its own summation order)."""
    import torch
    x = pos[:, :, :3]
    d = x[:, :, None, :] - x[:, None, :, :]
    L = box[:, None, None, :]
    d = torch.where(d >= 0.5 * L, d - L, torch.where(d < -0.5 * L, d + L, d))
    rsq = (d * d).sum(dim=3)
    ti, tj = typeid[:, :, None], typeid[:, None, :]
    n = pos.shape[1]
    eye = torch.eye(n, dtype=torch.bool, device=pos.device)[None]
    rc = tab["rcutsq"][ti, tj]
    ok = ~eye & ~(bonded >= 0) & (rsq < rc)
    safe = torch.where(ok, rsq, torch.ones_like(rsq))
    r2inv = 1.0 / safe
    r6inv = r2inv * r2inv * r2inv
    fdivr = torch.where(ok, r2inv * r6inv * (tab["lj1_12"][ti, tj] * r6inv - tab["lj2_6"][ti, tj]), torch.zeros_like(rsq))
    e = torch.where(ok, r6inv * (tab["lj1"][ti, tj] * r6inv - tab["lj2"][ti, tj]) - tab["eshift"][ti, tj], torch.zeros_like(rsq))
    is_bond = bonded >= 0
    r = torch.sqrt(torch.where(is_bond, rsq, torch.ones_like(rsq)))
    bt = bonded.clamp(min=0)
    fdivr = fdivr + torch.where(is_bond, K[bt] * (r0[bt] / r - 1.0), torch.zeros_like(rsq))
    e = e + torch.where(is_bond, 0.5 * K[bt] * (r0[bt] - r) ** 2, torch.zeros_like(rsq))
    out = torch.empty((pos.shape[0], n, 4), dtype=torch.float64, device=pos.device)
    out[:, :, :3] = (d * fdivr[:, :, :, None]).sum(dim=2)
    out[:, :, 3] = 0.5 * e.sum(dim=2)
    return out


def measure(args):
    import numpy as np
    import torch
    import cavitymd
    from cavitymd import _capi, synthetic
    if args.library:
        _capi.LIB_PATH = args.library
    assert torch.cuda.is_available(), "this measurement needs a GPU; nothing is timed without one"
    rows, split = _capi.molecular_order()

    def timed(fn, count):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(count):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3 / count

    for B in args.B:
        cfgs = [synthetic.config1(seed=k + 1) for k in range(B)]
        sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                                c["types"], c["box"], device="cuda")) for c in cfgs]
        bonds = [synthetic.diatomic_bonds(c) for c in cfgs]
        mol = cavitymd.MolecularForceBatch(sysdefs, [b[0] for b in bonds], [b[1] for b in bonds], HARMONIC, LJ)
        n = len(cfgs[0]["charge"])
        # the baseline's inputs, stacked
        pos = torch.stack([s.getParticleData().getPositions() for s in sysdefs])
        typeid = torch.from_numpy(np.stack([c["typeid"] for c in cfgs]).astype(np.int64)).cuda()
        box = torch.tensor([c["box"] for c in cfgs], dtype=torch.float64, device="cuda")
        prm = mol.params
        tab = {name: torch.tensor([[getattr(prm.pair[a][b], name) for b in range(3)] for a in range(3)], dtype=torch.float64,
                                  device="cuda") for name in ("lj1", "lj2", "lj1_12", "lj2_6", "rcutsq", "eshift")}
        bonded = torch.full((B, n, n), -1, dtype=torch.int64)
        for k, (b, t) in enumerate(bonds):
            bonded[k, b[:, 0], b[:, 1]] = torch.from_numpy(t.astype(np.int64))
            bonded[k, b[:, 1], b[:, 0]] = torch.from_numpy(t.astype(np.int64))
        bonded = bonded.cuda()
        K = torch.tensor([HARMONIC[0]["k"], HARMONIC[1]["k"]], dtype=torch.float64, device="cuda")
        r0 = torch.tensor([HARMONIC[0]["r0"], HARMONIC[1]["r0"]], dtype=torch.float64, device="cuda")
        chunk = min(B, 32)                               # the baseline's (chunk, N, N, 3) temporaries stay below 1 GiB

        def baseline():
            return torch.cat([torch_baseline(pos[i:i + chunk], typeid[i:i + chunk], box[i:i + chunk], tab, bonded[i:i + chunk], K, r0)
                              for i in range(0, B, chunk)])

        mol.compute()
        got = torch.stack(mol.forces)
        want = baseline()
        scale = float(want[:, :, :3].abs().max())
        error = float((got - want).abs().max()) / scale
        assert error <= 1e-11, f"the launch and the torch baseline disagree: {error:.3e} of the largest force"
        launches = max(20, min(2000, int(args.window / max(timed(mol.compute, 20), 1e-7))))
        base_calls = max(2, min(200, int(args.window / max(timed(baseline, 2), 1e-7))))
        t_launch, t_base = [], []
        for _ in range(args.repeats):
            t_launch.append(timed(mol.compute, launches))
            t_base.append(timed(baseline, base_calls))
        t, tb = float(np.median(t_launch)), float(np.median(t_base))
        pairs = B * n * (n - 1)
        print(json.dumps({"library": os.path.basename(_capi.LIB_PATH), "S": split, "ROWS": rows, "B": B, "N": n,
                          "launch_us": t * 1e6, "launch_us_min_max": [min(t_launch) * 1e6, max(t_launch) * 1e6],
                          "launches_per_sample": launches, "pair_evaluations_per_s": pairs / t,
                          "fp64_issue_fraction": pairs * FLOPS_PER_PAIR / t / (0.5 * PEAK_FP64_VECTOR),
                          "torch_us": tb * 1e6, "torch_over_launch": tb / t, "max_error_vs_torch": error}), flush=True)
        mol.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device work per timing sample")
    ap.add_argument("--library", default=None, help="measure this build of libcavmd.so")
    ap.add_argument("--variants", action="store_true", help="measure the builds of `make molecular_variants`, one child each")
    args = ap.parse_args()
    if not args.variants:
        return measure(args)
    libs = [os.path.join(CSRC, f"libcavmd_molecular_s{s}.so") for s in (1, 4, 16)]
    missing = [p for p in libs if not os.path.exists(p)]
    if missing:
        sys.exit(f"missing {missing}: run `make -C {CSRC} molecular_variants` first (it needs no GPU)")
    for _ in range(2):                                   # two rounds, the candidates alternating
        for lib in libs:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--library", lib, "--repeats", str(args.repeats), "--window",
                            str(args.window), "--B"] + [str(b) for b in args.B], check=True, timeout=600)


if __name__ == "__main__":
    main()
