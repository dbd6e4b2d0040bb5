"""Writes tests/golden/rolling_tile_loop_parent.json, the yardstick of tests/test_gpu_rolling_tile_loop.py.

Run it on an MI355X from a checkout of the commit BEFORE the rolling tile loop (with this file and the test module copied into
its tests/ directory, and the library built):

    python tests/make_rolling_tile_loop_golden.py [OUTPUT.json]

For every case of the test it evaluates once with two launches and once with one launch, insists that the two agree bit for
bit (they did at that commit), and records the result block's doubles and the SHA-256 of the force array's bytes.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
for p in (HERE, ROOT, os.path.join(ROOT, "cav-hoomd_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_rolling_tile_loop as t  # noqa: E402
from parity_support import gpu_eval  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden", t.GOLDEN_NAME)
    cases = {}
    jobs = [(n, v, 2) for n in t.SIZES for v in t.VARIANTS] + [(70_001, "photon_last", 1)]
    for n, variant, unroll in jobs:
        cfg = t.make_cfg(n, variant)
        two = t.record(gpu_eval(cfg, dict(t.TWO, reduce_unroll=unroll)))
        one = t.record(gpu_eval(cfg, dict(t.ONE, reduce_unroll=unroll)))
        assert one == two, (n, variant, unroll)
        cases[t.case_key(n, variant, unroll)] = two
        print(t.case_key(n, variant, unroll), two["force_sha256"][:16], flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    doc = {"what": "cavity-force evaluation before the rolling tile loop: result doubles (dipole, q, Dq, energy, photon_force, "
                   "dipole_lo, total_dipole; little-endian hex), ints (photon_idx, n_photon_typed, n_particles, n_partials) "
                   "and SHA-256 of the (N, 4) float64 force array",
           "recorded_at_commit": commit or os.environ.get("CAVMD_GOLDEN_COMMIT", "unknown"),
           "cases": cases}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {out_path}: {len(cases)} cases")


if __name__ == "__main__":
    main()
