"""Time per evaluation of the shared cavity (cavmd_shared_cavity_compute, two launches) at the production size, B = 512 systems of
N = 433, grouped into cavities of 1, 8, 64 and 512 members, against cavmd_batch_compute (one launch) on the same arrays in the
same process.  That kernel is not touched by the shared cavity, so it is the parent's.

    python scripts/shared_cavity_throughput.py [--B 512] [--members 1 8 64 512] [--repeats 30] [--out profiles/shared_cavity/README.md]

Per object and mode (eager launches, replays of a captured graph holding one evaluation): `repeats` samples, each the device time
(events) of `per_sample` back-to-back evaluations divided by their number, the candidates alternating within every repeat;
p10, p50 and p90 of the samples.  Before anything is timed the cavities of one member are compared, bytes for bytes, with the
batch's forces.  With --out the table is written as Markdown under the heading the README carries; nothing is timed without a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--per-sample", type=int, default=200, help="evaluations per timing sample")
    ap.add_argument("--out", default=None, help="write the Markdown table here as well")
    args = ap.parse_args()

    import numpy as np
    import torch
    import cavitymd
    from cavitymd import _capi, synthetic
    assert torch.cuda.is_available(), "this measurement needs a GPU; nothing is timed without one"
    B = args.B
    cfgs = [synthetic.diatomic_lattice(6, 8.0, seed=k + 1) for k in range(B)]           # 216 molecules + the photon: N = 433
    n = len(cfgs[0]["charge"])
    prm = _capi.make_params(cfgs[0]["params"]["omegac"], cfgs[0]["params"]["couplstr"], cfgs[0]["params"]["phmass"])
    L_typeid = cfgs[0]["L_typeid"]
    tag = cavitymd.state.type_tag_as_double
    pos = [torch.from_numpy(np.concatenate([c["position"], tag(c["typeid"])[:, None]], axis=1)).cuda() for c in cfgs]
    chg = [torch.from_numpy(np.ascontiguousarray(c["charge"], dtype=np.float64)).cuda() for c in cfgs]
    img = [torch.from_numpy(np.ascontiguousarray(c["image"], dtype=np.int32)).cuda() for c in cfgs]
    force_batch = torch.zeros((B, n, 4), dtype=torch.float64, device="cuda")
    force_shared = torch.zeros((B, n, 4), dtype=torch.float64, device="cuda")
    ws = _capi.Workspace(1)
    batch = _capi.Batch(ws, [_capi.batch_item(n, pos[k].data_ptr(), chg[k].data_ptr(), img[k].data_ptr(), force_batch[k].data_ptr(),
                                              cfgs[k]["box"], L_typeid, prm) for k in range(B)])

    def shared_items(members):
        # the first system of every cavity is its carrier; the others keep their (uncoupled, charge 0) L-typed particle out of
        # the sum by naming no photon type
        return [_capi.shared_cavity_item(n, pos[k].data_ptr(), chg[k].data_ptr(), img[k].data_ptr(), force_shared[k].data_ptr(),
                                         cfgs[k]["box"], L_typeid if k % members == 0 else -1, prm, k // members) for k in range(B)]

    objects = {"batch (1 launch)": batch}
    for m in args.members:
        if B % m:
            sys.exit(f"--members {m} does not divide --B {B}")
        objects[f"shared, {m} per cavity"] = _capi.SharedCavity(ws, shared_items(m))
    stream = torch.cuda.current_stream().cuda_stream
    for obj in objects.values():                                                         # warm up every object
        obj.compute(stream)
    torch.cuda.synchronize()
    if 1 in args.members:
        batch.compute(stream)
        objects["shared, 1 per cavity"].compute(stream)
        torch.cuda.synchronize()
        assert force_batch.cpu().numpy().tobytes() == force_shared.cpu().numpy().tobytes(), "cavities of one member differ from the batch"

    graphs = {}
    for name, obj in objects.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            obj.compute(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()

    def timed(fn, count):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(count):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / count                                    # microseconds per evaluation

    samples = {(name, mode): [] for name in objects for mode in ("eager", "graph")}
    for _ in range(args.repeats):                                                        # the candidates alternate within a repeat
        for name, obj in objects.items():
            samples[(name, "eager")].append(timed(lambda: obj.compute(stream), args.per_sample))
            samples[(name, "graph")].append(timed(graphs[name].replay, args.per_sample))
    rows = []
    for (name, mode), s in samples.items():
        p10, p50, p90 = (float(x) for x in np.percentile(s, [10, 50, 90]))
        rows.append({"object": name, "mode": mode, "B": B, "N": n, "p10_us": p10, "p50_us": p50, "p90_us": p90,
                     "samples": len(s), "evaluations_per_sample": args.per_sample})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        base = {mode: next(r for r in rows if r["object"].startswith("batch") and r["mode"] == mode)["p50_us"] for mode in ("eager", "graph")}
        lines = ["| object | mode | p10 µs | p50 µs | p90 µs | p50 minus the batch's µs |", "|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['object']} | {r['mode']} | {r['p10_us']:.2f} | {r['p50_us']:.2f} | {r['p90_us']:.2f} | "
                         f"{r['p50_us'] - base[r['mode']]:+.2f} |")
        def p50(prefix, mode):
            return next((r["p50_us"] for r in rows if r["object"].startswith(prefix) and r["mode"] == mode), None)

        notes = []
        for mode in ("eager", "graph"):
            one, most = p50("shared, 1 per", mode), p50(f"shared, {max(args.members)} per", mode)
            if one is not None and most is not None:
                notes.append(f"- {mode}: cavities of 1 against the batch: {one - base[mode]:+.2f} µs at p50.  This does NOT isolate the "
                             "second launch and its boundary: the batch's kernel also publishes every item's result block to mapped "
                             "host memory behind a system-scope release, which the shared cavity does not do (its results are read "
                             f"behind a stream synchronisation).  The redundant fold at {max(args.members)} members against cavities "
                             f"of 1: {most - one:+.2f} µs at p50, to be held against the 1.5-1.9 µs expected of one kernel boundary "
                             "(the price a separate fold launch would pay instead).")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# The shared cavity against the batch: time per evaluation\n\n"
                    "Written by `python scripts/shared_cavity_throughput.py --out profiles/shared_cavity/README.md` on an MI355X.\n"
                    f"B = {B} systems of N = {n}; {args.repeats} samples of {args.per_sample} evaluations each, device events, the "
                    "candidates alternating within every repeat.  `batch` is cavmd_batch_compute on the same arrays in the same "
                    "process: its kernel is the parent commit's, instruction for instruction (device_code.txt).\n\n"
                    + "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n\n"
                    "Expected before measuring: one dependent kernel boundary more, about 1.5-1.9 µs.  A separate fold launch (one "
                    "workgroup per cavity instead of one fold per member) would be a later change; it is not built.\n")


if __name__ == "__main__":
    main()
