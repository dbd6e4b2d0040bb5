"""One recorder launch against the sequential sweep of per-system observables it replaces, and what the recorder adds to a
replay of the captured step.

usage: python scripts/recorder_throughput.py [--sizes 1,8,64,256,512,2048] [--sweeps 200] [--repeats 3] [--ragged]
                                             [--only recorded|sequential] [--parent-lib PATH] [--graph] [--json PATH]

For every B: B independent systems of 501 particles (the reference's production size), each evaluated once so that a result
block exists.  Ways to observe all of them once ("a sweep"), alternated `--repeats` times in this one process:
  sequential         per system cavmd_cavity_mode + cavmd_kinetic_energy + cavmd_force_mass_sum on a workspace of its own
                     (three launches and three host spins each): what a caller had before the recorder existed;
  sequential@parent  the same calls through a libcavmd.so built from the parent commit (`--parent-lib`): the baseline;
  recorded           one cavmd_recorder_record.
Every sweep ends in a stream synchronise and is timed on the host clock around it (`--sweeps` sweeps per repeat, after a
warm-up of every shape).  Printed per B and variant: median, p10 and p90 microseconds per sweep.  `--ragged` adds one mixed
batch (sizes 64..4096).  `--graph` measures instead the time per replay of the captured step: {force batch, thermostat batch}
through the parent's library and through this one, and {force batch, recorder, thermostat batch}; the thermostat's tau is
large and its variates fixed, so the velocities stay bounded over any number of replays.  `--only` runs one variant alone,
for `rocprofv3 --kernel-trace --stats -- python scripts/recorder_throughput.py --only recorded`.  A measurement path: it
needs a GPU and has no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cav-hoomd_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cavitymd  # noqa: E402
from cavitymd import _capi, synthetic  # noqa: E402

RAGGED = [64, 128, 256, 501, 501, 501, 501, 1024, 1024, 2048, 4096] * 6  # 66 systems
KB = cavitymd.PhysicalConstants.KB_HARTREE_PER_K
DT, TAU, R, GAMMA_OVER_SHAPE = 0.005, 50.0, 0.1, 1.0


class System:
    def __init__(self, n, seed):
        cfg = synthetic.config1(seed=seed) if n == 501 else synthetic.random_charged_box(n - 1, seed=seed)
        N = len(cfg["charge"])
        rng = np.random.default_rng(seed)
        tag = cavitymd.state.type_tag_as_double(cfg["typeid"])[:, None]
        self.n = N
        self.pos = torch.from_numpy(np.concatenate([cfg["position"], tag], axis=1).reshape(N, 4)).cuda()
        self.chg = torch.from_numpy(np.ascontiguousarray(cfg["charge"], dtype=np.float64)).cuda()
        self.img = torch.from_numpy(np.ascontiguousarray(cfg["image"], dtype=np.int32).reshape(N, 3)).cuda()
        self.frc = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        v = np.ones((N, 4))
        v[:, :3] = rng.normal(0.0, 1e-3, (N, 3))
        self.vel = torch.from_numpy(v).cuda()
        self.box = tuple(float(x) for x in cfg["box"])
        self.L_typeid = cfg["L_typeid"]
        p = cfg["params"]
        self.params = _capi.make_params(p["omegac"], p["couplstr"], p["phmass"])
        self.dof = 3.0 * N - 3.0
        self.kT = float((v[:, :3] ** 2).sum() / self.dof)
        self.gamma = GAMMA_OVER_SHAPE * (self.dof - 1.0) / 2.0
        self.ws = None
        self.parent_ws = None

    def force_item(self):
        return _capi.batch_item(self.n, self.pos.data_ptr(), self.chg.data_ptr(), self.img.data_ptr(), self.frc.data_ptr(),
                                self.box, self.L_typeid, self.params)

    def evaluate(self, lib, ws):
        st = lib.cavmd_compute_hoomd(ws, None, self.n, self.pos.data_ptr(), self.chg.data_ptr(), self.img.data_ptr(), *self.box,
                                     self.L_typeid, ctypes.byref(self.params), self.frc.data_ptr())
        assert st == 0, st


def _parent(path):
    """The parent commit's library, declared by hand: it has no recorder."""
    lib = ctypes.CDLL(path)
    vp, sz, dbl, ci, P = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int, ctypes.POINTER
    assert not hasattr(lib, "cavmd_recorder_record"), "--parent-lib must be the library of the parent commit"
    lib.cavmd_create.argtypes = [ci, sz, P(vp)]
    lib.cavmd_destroy.argtypes = [vp]
    lib.cavmd_compute_hoomd.argtypes = [vp, vp, sz, vp, vp, vp, dbl, dbl, dbl, ci, P(_capi.Params), vp]
    lib.cavmd_cavity_mode.argtypes = [vp, vp, vp, dbl, P(dbl * 4)]
    lib.cavmd_force_mass_sum.argtypes = [vp, vp, sz, vp, vp, P(dbl)]
    lib.cavmd_kinetic_energy.argtypes = [vp, vp, vp, vp, sz, P(dbl)]
    lib.cavmd_batch_create.argtypes = [vp, sz, P(_capi.BatchItem), ci, P(vp)]
    lib.cavmd_batch_compute.argtypes = [vp, vp]
    lib.cavmd_batch_destroy.argtypes = [vp]
    lib.cavmd_bussi_batch_create.argtypes = [vp, sz, P(_capi.BussiBatchItem), P(vp)]
    lib.cavmd_bussi_batch_step.argtypes = [vp, vp, vp]
    lib.cavmd_bussi_batch_destroy.argtypes = [vp]
    return lib


def _summary(times, B):
    out = {}
    for name, v in times.items():
        us = np.array(v) * 1e6
        out[name] = {"B": B, "sweeps": len(v), "median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)),
                     "p90_us": float(np.percentile(us, 90))}
    return out


def _alternate(variants, sweeps, repeats):
    sync = torch.cuda.synchronize
    for fn in variants.values():              # warm-up of every shape and code path
        for _ in range(10):
            fn()
        sync()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for name, fn in variants.items():     # alternated
            for _ in range(sweeps):
                t0 = time.perf_counter()
                fn()
                sync()
                times[name].append(time.perf_counter() - t0)
    return times


def measure(systems, sweeps, repeats, only, parent):
    B = len(systems)
    lib = _capi.load()
    for s in systems:
        if s.ws is None:
            s.ws = _capi.Workspace(s.n)
            s.evaluate(lib, s.ws.handle)
        if parent is not None and s.parent_ws is None:
            s.parent_ws = ctypes.c_void_p()
            assert parent.cavmd_create(-1, s.n, ctypes.byref(s.parent_ws)) == 0
            s.evaluate(parent, s.parent_ws)
    holder = _capi.Workspace(1)
    fb = _capi.Batch(holder, [s.force_item() for s in systems])
    fb.compute(0)
    res = fb.results_device_ptr()
    rec = _capi.Recorder(holder, [_capi.recorder_item(res + 192 * k, s.vel.data_ptr(), s.frc.data_ptr(), 0, s.n, s.n)
                                  for k, s in enumerate(systems)], 64, 1, KB)
    torch.cuda.synchronize()
    out4, out1 = (ctypes.c_double * 4)(), ctypes.c_double()

    def sweep_through(l, handles):
        mode, ke, fm = l.cavmd_cavity_mode, l.cavmd_kinetic_energy, l.cavmd_force_mass_sum
        p4, p1 = ctypes.byref(out4), ctypes.byref(out1)
        calls = [(h, s.vel.data_ptr(), s.frc.data_ptr(), s.n) for h, s in zip(handles, systems)]

        def run():
            for h, vel, frc, n in calls:
                mode(h, None, vel, KB, p4)
                ke(h, None, vel, None, n, p1)
                fm(h, None, n, frc, vel, p1)
        return run

    variants = {"sequential": sweep_through(lib, [s.ws.handle for s in systems]), "recorded": lambda: rec.record(0)}
    if parent is not None:
        variants = {"sequential@parent": sweep_through(parent, [s.parent_ws for s in systems]), **variants}
    if only:
        variants = {only: variants[only]}
    out = _summary(_alternate(variants, sweeps, repeats), B)
    if "recorded" in variants:
        rows = rec.rows(0)
        assert len(set(rows.tolist())) == 1 and rows[0] > 0
        last = rec.read(0, 0, B, int(rows[0]) - 1, 1)[:, 0]
        assert np.isfinite(last["kinetic_energy"]).all() and (last["force_mass_sum"] > 0).all()
    rec.close()
    fb.close()
    holder.close()
    return out


def measure_graph(systems, sweeps, repeats, parent):
    """Time per replay of the captured step, the recorder in it or not."""
    B = len(systems)
    lib = _capi.load()
    fitems = (_capi.BatchItem * B)(*[s.force_item() for s in systems])
    titems = (_capi.BussiBatchItem * B)(*[_capi.bussi_batch_item(s.vel.data_ptr(), 0, s.n, s.dof) for s in systems])
    arr = (_capi.BussiBatchInput * B)(*[_capi.bussi_batch_input_make(DT, s.kT, TAU, R, s.gamma) for s in systems])
    rows = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.float64).reshape(B, 8).copy()).cuda()
    keep, graphs = [], {}

    def build(name, l, with_recorder):
        ws, fb, tb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        assert l.cavmd_create(-1, 1, ctypes.byref(ws)) == 0
        assert l.cavmd_batch_create(ws, B, fitems, 64, ctypes.byref(fb)) == 0
        assert l.cavmd_bussi_batch_create(ws, B, titems, ctypes.byref(tb)) == 0
        rec = None
        if with_recorder:
            res = ctypes.c_void_p()
            assert l.cavmd_batch_results_device_ptr(fb, ctypes.byref(res)) == 0
            ritems = (_capi.RecorderItem * B)(*[_capi.recorder_item(res.value + 192 * k, s.vel.data_ptr(), s.frc.data_ptr(), 0,
                                                                     s.n, s.n) for k, s in enumerate(systems)])
            rec = ctypes.c_void_p()
            assert l.cavmd_recorder_create(ws, B, ritems, 64, 1, KB, ctypes.byref(rec)) == 0
        assert l.cavmd_batch_compute(fb, None) == 0      # every kernel has run once before it is captured
        if rec is not None:
            assert l.cavmd_recorder_record(rec, None) == 0
        assert l.cavmd_bussi_batch_step(tb, None, rows.data_ptr()) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert l.cavmd_batch_compute(fb, stream) == 0
            if rec is not None:
                assert l.cavmd_recorder_record(rec, stream) == 0
            assert l.cavmd_bussi_batch_step(tb, stream, rows.data_ptr()) == 0
        keep.append((l, ws, fb, tb, rec))
        graphs[name] = graph.replay

    if parent is not None:
        build("step@parent", parent, False)
    build("step", lib, False)
    build("step+recorder", lib, True)
    out = _summary(_alternate(graphs, sweeps, repeats), B)
    torch.cuda.synchronize()
    for l, ws, fb, tb, rec in keep:
        if rec is not None:
            l.cavmd_recorder_destroy(rec)
        l.cavmd_bussi_batch_destroy(tb)
        l.cavmd_batch_destroy(fb)
        l.cavmd_destroy(ws)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256,512,2048")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--only", choices=("recorded", "sequential"), default=None)
    ap.add_argument("--parent-lib", default=None, help="libcavmd.so built from the parent commit: the baseline")
    ap.add_argument("--graph", action="store_true", help="time per replay of the captured step instead")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "recorder_throughput.py measures on a GPU; there is no fallback"
    parent = _parent(args.parent_lib) if (args.parent_lib and not args.only) else None
    sizes = [int(x) for x in args.sizes.split(",") if x]
    pool = [System(501, seed) for seed in range(1, max(sizes) + 1)]
    out = {"n": 501, "graph": args.graph, "rows": []}
    print(f"n=501 sweeps/repeat={args.sweeps} repeats={args.repeats} parent={'yes' if parent is not None else 'no'} "
          f"mode={'captured step, per replay' if args.graph else 'observe every system once'}")
    print(f"{'B':>6s} {'variant':<18s} {'median us':>10s} {'p10':>9s} {'p90':>9s}")
    cases = [(f"{B}", pool[:B]) for B in sizes]
    if args.ragged:
        cases.append(("ragged", [System(n, 1000 + k) for k, n in enumerate(RAGGED)]))
    for label, systems in cases:
        rows = measure_graph(systems, args.sweeps, args.repeats, parent) if args.graph \
            else measure(systems, args.sweeps, args.repeats, args.only, parent)
        for name, r in rows.items():
            r["case"], r["variant"] = label, name
            out["rows"].append(r)
            print(f"{label:>6s} {name:<18s} {r['median_us']:10.2f} {r['p10_us']:9.2f} {r['p90_us']:9.2f}", flush=True)
        if args.graph:
            ref = rows.get("step@parent", rows["step"])
            print(f"{label:>6s} step+recorder - {ref['variant']} = {rows['step+recorder']['median_us'] - ref['median_us']:.2f} us "
                  f"per replay; step p10..p90 {rows['step']['p10_us']:.2f}..{rows['step']['p90_us']:.2f}", flush=True)
        else:
            ref = rows.get("sequential@parent", rows.get("sequential"))
            if ref is not None and "recorded" in rows:
                b = rows["recorded"]
                print(f"{label:>6s} {ref['variant']}/recorded = {ref['median_us'] / b['median_us']:.2f}x; recorded p90 "
                      f"{b['p90_us']:.2f} {'<' if b['p90_us'] < ref['p10_us'] else '>='} {ref['variant']} p10 {ref['p10_us']:.2f}",
                      flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
