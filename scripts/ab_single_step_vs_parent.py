"""The single-system thermostat step of this tree against a checkout of the parent commit.

usage: python scripts/ab_single_step_vs_parent.py --parent-tree DIR [--rounds 3]

Runs `bench.py --gpus 1 --full --no-cpu-baseline` of the parent tree (built beforehand) and of this tree alternately,
`--rounds` times each, every run a fresh child process, and prints extras.bussi_thermostat_step_1e6 of each run plus, per
figure, the parent's min..max and this tree's median.  A measurement path: it needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
KEYS = ("kinetic_energy_us", "full_step_us", "full_step_on_device_us")


def run(tree):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "10", "--full",
                          "--no-cpu-baseline"], cwd=tree, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    return line["extras"]["bussi_thermostat_step_1e6"], line["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    got = {"parent": [], "branch": []}
    for r in range(args.rounds):
        for name, tree in (("parent", args.parent_tree), ("branch", ROOT)):
            th, value = run(tree)
            got[name].append(th)
            print(f"round {r} {name:<6s} " + " ".join(f"{k}={th[k]:.2f}" for k in KEYS) + f"  flagship evals/s={value:.1f}",
                  flush=True)
    for k in KEYS:
        p = [x[k] for x in got["parent"]]
        b = statistics.median(x[k] for x in got["branch"])
        inside = min(p) <= b <= max(p)
        print(f"{k}: parent min..max {min(p):.2f} .. {max(p):.2f}, branch median {b:.2f} -> "
              f"{'inside' if inside else 'OUTSIDE'} the parent's own range")


if __name__ == "__main__":
    main()
