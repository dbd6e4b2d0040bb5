"""One field-recorder launch against the sequential sweep of per-system density fields it replaces, and what the field recorder
adds to a replay of the captured step.

usage: python scripts/field_recorder_throughput.py [--sizes 1,8,64,256,512,2048] [--sweeps 200] [--repeats 3] [--ragged]
                                                   [--refs 1,10] [--only recorded|sequential] [--parent-lib PATH] [--graph]
                                                   [--json PATH]

For every B: B independent systems of 501 particles (the reference's production size), 50 wavevectors (the reference tracker's
kmag * generate_fibonacci_sphere(50)).  Ways to observe rho(k) and F against `refs` stored references of all of them once
("a sweep"), alternated `--repeats` times in this one process:
  sequential         per system cavmd_density_field + cavmd_density_field_read on a workspace of its own (two launches, a
                     stream synchronisation and a copy each) and F = mean_k Re(rho_r conj rho) in numpy for every reference:
                     what a caller had before the field recorder existed;
  sequential@parent  the same calls through a libcavmd.so built from the parent commit (`--parent-lib`): the baseline;
  recorded           one cavmd_field_recorder_record (the references are already stored: the warm-up fills them).
Every sweep ends in a stream synchronise and is timed on the host clock around it (`--sweeps` sweeps per repeat, after a
warm-up of every shape).  Printed per B, refs and variant: median, p10 and p90 microseconds per sweep.  `--ragged` adds one
mixed batch (sizes 64..4096).  `--graph` measures instead the time per replay of the captured step {force batch, recorder,
thermostat batch} through the parent's library and through this one, and the same with the field recorder as fourth kernel.
`--only` runs one variant alone, for `rocprofv3 --kernel-trace --stats -- python scripts/field_recorder_throughput.py --only
recorded`.  A measurement path: it needs a GPU and has no fallback."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cavitymd import _capi, observables  # noqa: E402
import recorder_throughput as rt  # noqa: E402  (System, the alternating timer and the summary)

KVEC = np.ascontiguousarray(1.0 * observables.generate_fibonacci_sphere(50))
N_K = KVEC.shape[0]


def _parent(path):
    """The parent commit's library, declared by hand: it has the recorder but no field recorder."""
    lib = ctypes.CDLL(path)
    vp, sz, dbl, ci, u64, P = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER
    assert not hasattr(lib, "cavmd_field_recorder_record"), "--parent-lib must be the library of the parent commit"
    lib.cavmd_create.argtypes = [ci, sz, P(vp)]
    lib.cavmd_destroy.argtypes = [vp]
    lib.cavmd_set_wavevectors.argtypes = [vp, sz, vp]
    lib.cavmd_density_field.argtypes = [vp, vp, sz, vp, sz]
    lib.cavmd_density_field_read.argtypes = [vp, vp]
    lib.cavmd_batch_create.argtypes = [vp, sz, P(_capi.BatchItem), ci, P(vp)]
    lib.cavmd_batch_compute.argtypes = [vp, vp]
    lib.cavmd_batch_destroy.argtypes = [vp]
    lib.cavmd_batch_results_device_ptr.argtypes = [vp, P(vp)]
    lib.cavmd_bussi_batch_create.argtypes = [vp, sz, P(_capi.BussiBatchItem), P(vp)]
    lib.cavmd_bussi_batch_step.argtypes = [vp, vp, vp]
    lib.cavmd_bussi_batch_destroy.argtypes = [vp]
    lib.cavmd_recorder_create.argtypes = [vp, sz, P(_capi.RecorderItem), sz, u64, dbl, P(vp)]
    lib.cavmd_recorder_record.argtypes = [vp, vp]
    lib.cavmd_recorder_destroy.argtypes = [vp]
    return lib


def _field_items(systems):
    return [_capi.field_item(s.pos.data_ptr(), 32, s.n) for s in systems]


def measure(systems, refs, sweeps, repeats, only, parent):
    B = len(systems)
    lib = _capi.load()
    kp = ctypes.c_void_p(KVEC.ctypes.data)
    for s in systems:
        if s.ws is None:
            s.ws = _capi.Workspace(s.n)
            s.ws.set_wavevectors(KVEC)
        if parent is not None and s.parent_ws is None:
            s.parent_ws = ctypes.c_void_p()
            assert parent.cavmd_create(-1, s.n, ctypes.byref(s.parent_ws)) == 0
            assert parent.cavmd_set_wavevectors(s.parent_ws, N_K, kp) == 0
    holder = _capi.Workspace(1)
    rec = _capi.FieldRecorder(holder, _field_items(systems), KVEC, 64, 1, refs, 1)   # the warm-up stores the references
    torch.cuda.synchronize()
    out = np.zeros(2 * N_K)
    outp = ctypes.c_void_p(out.ctypes.data)
    ref_fields = [np.random.default_rng(k).normal(size=(refs, N_K)) + 1j * np.random.default_rng(k + 1).normal(size=(refs, N_K))
                  for k in range(B)]
    F = np.zeros((B, refs))

    def sweep_through(l, handles):
        field, read = l.cavmd_density_field, l.cavmd_density_field_read
        calls = [(h, s.pos.data_ptr(), s.n, ref_fields[k], F[k]) for k, (h, s) in enumerate(zip(handles, systems))]
        cur = out.view(np.complex128)

        def run():
            for h, pos, n, rf, f in calls:
                field(h, None, n, pos, 32)
                read(h, outp)
                for r in range(refs):                              # compute_field_autocorr, src/cavitymd/analysis.py:359-364
                    f[r] = np.mean(np.real(rf[r] * np.conj(cur)))
        return run

    variants = {"sequential": sweep_through(lib, [s.ws.handle for s in systems]), "recorded": lambda: rec.record(0)}
    if parent is not None:   # the baseline replaces this library's own sequential sweep (the same kernels, instruction for instruction)
        variants = {"sequential@parent": sweep_through(parent, [s.parent_ws for s in systems]), "recorded": variants["recorded"]}
    if only:
        variants = {only: variants[only]}
    res = rt._summary(rt._alternate(variants, sweeps, repeats), B)
    if "recorded" in variants:
        rows = rec.rows(0)
        assert len(set(rows.tolist())) == 1 and rows[0] > 0
        last = rec.read(0, 0, B, int(rows[0]) - 1, 1)[:, 0]
        assert (last["n_references"] == refs).all() and np.isfinite(last["F"]).all() and (last["rho2"] > 0).all()
    rec.close()
    holder.close()
    return res


def measure_graph(systems, refs, sweeps, repeats, parent):
    """Time per replay of the captured step, the field recorder in it or not."""
    B = len(systems)
    lib = _capi.load()
    fitems = (_capi.BatchItem * B)(*[s.force_item() for s in systems])
    titems = (_capi.BussiBatchItem * B)(*[_capi.bussi_batch_item(s.vel.data_ptr(), 0, s.n, s.dof) for s in systems])
    arr = (_capi.BussiBatchInput * B)(*[_capi.bussi_batch_input_make(rt.DT, s.kT, rt.TAU, rt.R, s.gamma) for s in systems])
    rows = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.float64).reshape(B, 8).copy()).cuda()
    gitems = (_capi.FieldItem * B)(*_field_items(systems))
    kp = ctypes.c_void_p(KVEC.ctypes.data)
    keep, graphs = [], {}

    def build(name, l, with_fields):
        ws, fb, tb, rec, frec = (ctypes.c_void_p() for _ in range(5))
        assert l.cavmd_create(-1, 1, ctypes.byref(ws)) == 0
        assert l.cavmd_batch_create(ws, B, fitems, 64, ctypes.byref(fb)) == 0
        assert l.cavmd_bussi_batch_create(ws, B, titems, ctypes.byref(tb)) == 0
        res = ctypes.c_void_p()
        assert l.cavmd_batch_results_device_ptr(fb, ctypes.byref(res)) == 0
        ritems = (_capi.RecorderItem * B)(*[_capi.recorder_item(res.value + 192 * k, s.vel.data_ptr(), s.frc.data_ptr(), 0,
                                                                 s.n, s.n) for k, s in enumerate(systems)])
        assert l.cavmd_recorder_create(ws, B, ritems, 64, 1, rt.KB, ctypes.byref(rec)) == 0
        if with_fields:
            assert l.cavmd_field_recorder_create(ws, B, gitems, N_K, kp, 64, 1, refs, 1, ctypes.byref(frec)) == 0

        def step(stream):
            assert l.cavmd_batch_compute(fb, stream) == 0
            assert l.cavmd_recorder_record(rec, stream) == 0
            if with_fields:
                assert l.cavmd_field_recorder_record(frec, stream, None) == 0
            assert l.cavmd_bussi_batch_step(tb, stream, rows.data_ptr()) == 0

        for _ in range(refs + 1):                          # every kernel has run, and the references are stored, before capture
            step(None)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        keep.append((l, ws, fb, tb, rec, frec if with_fields else None))
        graphs[name] = graph.replay

    if parent is not None:
        build("step@parent", parent, False)
    build("step", lib, False)
    build("step+fields", lib, True)
    out = rt._summary(rt._alternate(graphs, sweeps, repeats), B)
    torch.cuda.synchronize()
    for l, ws, fb, tb, rec, frec in keep:
        if frec is not None:
            l.cavmd_field_recorder_destroy(frec)
        l.cavmd_recorder_destroy(rec)
        l.cavmd_bussi_batch_destroy(tb)
        l.cavmd_batch_destroy(fb)
        l.cavmd_destroy(ws)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256,512,2048")
    ap.add_argument("--refs", default="1,10")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--only", choices=("recorded", "sequential"), default=None)
    ap.add_argument("--parent-lib", default=None, help="libcavmd.so built from the parent commit: the baseline")
    ap.add_argument("--graph", action="store_true", help="time per replay of the captured step instead")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "field_recorder_throughput.py measures on a GPU; there is no fallback"
    parent = _parent(args.parent_lib) if (args.parent_lib and not args.only) else None
    sizes = [int(x) for x in args.sizes.split(",") if x]
    refs_list = [int(x) for x in args.refs.split(",") if x]
    pool = [rt.System(501, seed) for seed in range(1, max(sizes) + 1)]
    out = {"n": 501, "n_k": N_K, "graph": args.graph, "rows": []}
    print(f"n=501 n_k={N_K} sweeps/repeat={args.sweeps} repeats={args.repeats} parent={'yes' if parent is not None else 'no'} "
          f"mode={'captured step, per replay' if args.graph else 'rho(k) and F of every system once'}")
    print(f"{'B':>6s} {'refs':>4s} {'variant':<18s} {'median us':>10s} {'p10':>9s} {'p90':>9s}")
    cases = [(f"{B}", pool[:B]) for B in sizes]
    if args.ragged:
        cases.append(("ragged", [rt.System(n, 1000 + k) for k, n in enumerate(rt.RAGGED)]))
    for label, systems in cases:
        for refs in refs_list:
            rows = measure_graph(systems, refs, args.sweeps, args.repeats, parent) if args.graph \
                else measure(systems, refs, args.sweeps, args.repeats, args.only, parent)
            for name, r in rows.items():
                r["case"], r["variant"], r["refs"] = label, name, refs
                out["rows"].append(r)
                print(f"{label:>6s} {refs:4d} {name:<18s} {r['median_us']:10.2f} {r['p10_us']:9.2f} {r['p90_us']:9.2f}", flush=True)
            if args.graph:
                ref = rows.get("step@parent", rows["step"])
                print(f"{label:>6s} {refs:4d} step+fields - {ref['variant']} = "
                      f"{rows['step+fields']['median_us'] - ref['median_us']:.2f} us per replay; step p10..p90 "
                      f"{rows['step']['p10_us']:.2f}..{rows['step']['p90_us']:.2f}", flush=True)
            else:
                ref = rows.get("sequential@parent", rows.get("sequential"))
                if ref is not None and "recorded" in rows:
                    b = rows["recorded"]
                    print(f"{label:>6s} {refs:4d} {ref['variant']}/recorded = {ref['median_us'] / b['median_us']:.2f}x; recorded p90 "
                          f"{b['p90_us']:.2f} {'<' if b['p90_us'] < ref['p10_us'] else '>='} {ref['variant']} p10 "
                          f"{ref['p10_us']:.2f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
