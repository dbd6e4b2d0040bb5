"""What a checkpoint of a batch run costs (profiles/checkpoint/README.md): the blob sizes of every object, the wall time of
``BatchCheckpoint.save`` and ``load``, and one captured step's time for scale, for B replicas of N = 501 particles
(synthetic.config1, one seed per replica) under the step and the ring sizes of
examples/checkpoint/batch_restart_in_one_graph.py.  Measurements to write down, not thresholds.

    python scripts/checkpoint_timing.py [B] [steps] [repeats]"""
import os
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd"), os.path.join(ROOT, "examples", "checkpoint")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from batch_restart_in_one_graph import FRAMES, LEDGER_ROWS, RECORDER_ROWS, Replicas  # noqa: E402
from cavitymd import synthetic  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    assert torch.cuda.is_available(), "this script needs a GPU"
    t0 = time.perf_counter()
    run = Replicas(B, config=lambda k: synthetic.config1(seed=k + 1))
    N = run.sysdefs[0].getParticleData().getN()
    print(f"B = {B}, N = {N}; rings: recorder {RECORDER_ROWS} rows, ledger {LEDGER_ROWS} rows, trajectory {FRAMES} frames (f64); "
          f"built in {time.perf_counter() - t0:.1f} s", flush=True)
    run.run(5)                                                             # capture and warm up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run.run(steps)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / steps * 1e3
    print(f"one captured step: {step_ms:.3f} ms (mean of {steps} replays, wall clock)", flush=True)
    print("blob sizes (bytes):")
    total = 0
    for name, obj in run.checkpoint._objects.items():
        size = obj._need().snapshot_bytes()
        total += size
        print(f"  {name:<12} {size:>12}")
    arrays = run.checkpoint.state()
    tensors = sum(a.nbytes for key, a in arrays.items() if not key.endswith(".snapshot"))
    print(f"  all blobs    {total:>12}\n  tensors      {tensors:>12}   (positions, images, velocities, accel, input rows, net forces)")
    path = os.path.join(tempfile.mkdtemp(), "checkpoint_timing.npz")
    save, load = [], []
    for _ in range(repeats):
        run.run(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run.checkpoint.save(path)
        save.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        run.checkpoint.load(path)
        load.append(time.perf_counter() - t0)
    print(f"file: {os.path.getsize(path)} bytes")
    print(f"BatchCheckpoint.save: median {np.median(save) * 1e3:.1f} ms, min {min(save) * 1e3:.1f}, max {max(save) * 1e3:.1f} "
          f"({repeats} runs, wall clock, fsync included)")
    print(f"BatchCheckpoint.load: median {np.median(load) * 1e3:.1f} ms, min {min(load) * 1e3:.1f}, max {max(load) * 1e3:.1f}")
    print(f"save / step = {np.median(save) * 1e3 / step_ms:.0f} steps' worth of time")
    run.close()
    os.remove(path)


if __name__ == "__main__":
    main()
