"""cavmd_mts_verlet_kick on the GPU, bit for bit beside tests/verlet_kick_mirror.py.  Run with `-m gpu` on an MI355X.
  1. one ragged batch, N on every boundary of the kernel's tile of 512: the velocities equal the mirror's; a skipped row, a NULL
     force pointer and an empty item leave everything alone; vel.w, pos, image, d_accel, d_net_force and the states keep their bytes;
  2. 50 replays of a captured kick follow a dt row and a pointer table rewritten between them;
  3. the refusals that need a live integrator;  4. VerletBatch.kick."""
import math

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi, synthetic
from gpu_support import same as _same
from gpu_support import stream as _stream
from verlet_kick_mirror import mirror_kick

pytestmark = pytest.mark.gpu

INV = _capi.CAVMD_ERR_INVALID_VALUE
SIZES = (0, 1, 511, 512, 513, 1025, 40, 40)                     # the tile is 512 particles; the last two: skipped, NULL
SKIPPED, NULL = 6, 7


def _rows_array(rows) -> np.ndarray:
    arr = (_capi.VerletInput * len(rows))(*rows)
    return np.frombuffer(bytes(arr), dtype=np.float64).reshape(len(rows), 8).copy()


def _system(k, n, rng):
    m = max(n, 1)
    vel = np.zeros((m, 4))
    vel[:, :3] = rng.normal(0.0, 3.0, (m, 3))
    vel[:, 3] = rng.uniform(0.5, 20.0, m)
    return {"N": n, "box": (8.0, 10.0, 12.0), "pos": rng.uniform(-4.0, 4.0, (m, 4))[:n], "vel": vel[:n],
            "image": rng.integers(-3, 4, (m, 3)).astype(np.int32)[:n], "own": rng.normal(0.0, 5.0, (m, 4))[:n],
            "kick": [rng.normal(0.0, 5.0, (m, 4))[:n] for _ in range(2)], "accel": np.full((n, 3), -3.0), "net": np.full((n, 4), 7.0)}


def _to_device(s):
    d = {name: torch.from_numpy(np.ascontiguousarray(s[name])).cuda() for name in ("pos", "vel", "image", "accel", "net", "own")}
    d["kick"] = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in s["kick"]]
    return d


def _item(s, d):
    n = s["N"]
    return _capi.verlet_item(n, d["pos"].data_ptr() if n else 0, d["image"].data_ptr() if n else 0, d["vel"].data_ptr() if n else 0,
                             d["accel"].data_ptr() if n else 0, [d["own"].data_ptr() if n else 0], d["net"].data_ptr() if n else 0,
                             s["box"], -1)


def _others(d):
    """everything a kick must not write, as bytes (vel.w with it)"""
    out = [d[name].cpu().numpy().tobytes() for name in ("pos", "image", "accel", "net", "own")]
    return out + [f.cpu().numpy().tobytes() for f in d["kick"]] + [d["vel"].cpu().numpy()[:, 3].tobytes()]


def _table(dev, which, null=()):
    ptrs = [0 if (k in null or d["kick"][which].shape[0] == 0) else d["kick"][which].data_ptr() for k, d in enumerate(dev)]
    return torch.from_numpy(np.array(ptrs, dtype=np.uint64).view(np.int64).copy()).cuda()


def _batch(seed):
    rng = np.random.default_rng(seed)
    systems = [_system(k, n, rng) for k, n in enumerate(SIZES)]
    dev = [_to_device(s) for s in systems]
    ws = _capi.Workspace(1)
    batch = _capi.Verlet(ws, [_item(s, d) for s, d in zip(systems, dev)])
    torch.cuda.synchronize()
    return systems, dev, ws, batch


def _rows(dts):
    return [_capi.verlet_input_make(dt, 0.0, 0.0, (0.0, 0.0, 0.0)) for dt in dts]


# ---- 1. one ragged batch --------------------------------------------------------------------------------------------------------
def test_one_ragged_batch_equals_the_mirror_bit_for_bit():
    systems, dev, ws, batch = _batch(20261110)
    before = [_others(d) for d in dev]
    state0 = batch.read(_stream()).tobytes()
    for step, (weight, which) in enumerate(((2.0, 0), (0.5, 1), (-1.5, 0))):
        dts = [0.0 if k == SKIPPED else (0.5, 0.3, 10.0)[(k + step) % 3] for k in range(len(SIZES))]
        rows = _rows(dts)
        assert rows[SKIPPED].skip != 0 and sum(r.skip != 0 for r in rows) == 1
        d_rows = torch.from_numpy(_rows_array(rows)).cuda()
        table = _table(dev, which, null=(NULL,))
        batch.kick(_stream(), d_rows.data_ptr(), table.data_ptr(), weight)
        torch.cuda.synchronize()
        for k, (s, d) in enumerate(zip(systems, dev)):
            old = s["vel"].copy()
            mirror_kick(s, rows[k], None if k == NULL else s["kick"][which], weight)
            assert _same(d["vel"].cpu().numpy(), s["vel"]), (step, k)
            assert (k in (0, SKIPPED, NULL)) == _same(old, s["vel"]), (step, k)   # the kick moved every other item's velocities
            assert _others(d) == before[k], (step, k)                              # ... and wrote nothing else
        assert batch.read(_stream()).tobytes() == state0                           # steps, out_of_box, the reservoir: untouched
    assert state0 == bytes(32 * len(SIZES))
    batch.close()
    ws.close()


# ---- 2. capture -----------------------------------------------------------------------------------------------------------------
def test_fifty_replays_follow_the_dt_row_and_the_pointer_table():
    results = []
    for captured in (False, True):
        systems, dev, ws, batch = _batch(20261111)
        d_rows = torch.from_numpy(_rows_array(_rows([1.0] * len(SIZES)))).cuda()
        table = _table(dev, 0)
        tables = [_table(dev, 0, null=(NULL,)), _table(dev, 1)]
        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                batch.kick(_stream(), d_rows.data_ptr(), table.data_ptr(), 0.5)
            torch.cuda.synchronize()
            assert _same(dev[1]["vel"].cpu().numpy(), systems[1]["vel"])           # capturing ran nothing
        for step in range(50):
            dts = [0.0 if (k + step) % 5 == 0 else 0.25 * (1 + (k + step) % 4) for k in range(len(SIZES))]
            rows = _rows(dts)
            d_rows.copy_(torch.from_numpy(_rows_array(rows)).cuda())               # in stream order, between the replays
            table.copy_(tables[step % 2])
            if captured:
                graph.replay()
            else:
                batch.kick(_stream(), d_rows.data_ptr(), table.data_ptr(), 0.5)
            for k, s in enumerate(systems):
                mirror_kick(s, rows[k], None if (step % 2 == 0 and k == NULL) else s["kick"][step % 2], 0.5)
        torch.cuda.synchronize()
        for k, (s, d) in enumerate(zip(systems, dev)):
            assert _same(d["vel"].cpu().numpy(), s["vel"]), (captured, k)
        results.append([d["vel"].cpu().numpy().tobytes() for d in dev])
        batch.close()
        ws.close()
    assert results[0] == results[1]


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_live_integrator():
    systems, dev, ws, batch = _batch(20261112)
    d_rows = torch.from_numpy(_rows_array(_rows([1.0] * len(SIZES)))).cuda()
    table = _table(dev, 0)
    rows, forces = d_rows.data_ptr(), table.data_ptr()
    for args in ((0, forces, 0.5), (rows + 4, forces, 0.5), (rows, 0, 0.5), (rows, forces + 4, 0.5), (rows, forces, math.nan),
                 (rows, forces, math.inf), (rows, forces, -math.inf)):
        with pytest.raises(_capi.CavmdError) as e:
            batch.kick(_stream(), *args)
        assert e.value.status == INV, args
    torch.cuda.synchronize()
    for s, d in zip(systems, dev):
        assert _same(d["vel"].cpu().numpy(), s["vel"])                             # a refused call launched nothing
    batch.kick(_stream(), rows, forces, 0.0)                                       # weight 0 is a kick: v + (f / m) 0
    torch.cuda.synchronize()
    for s, d in zip(systems, dev):
        assert (d["vel"].cpu().numpy() == s["vel"]).all()
    batch.close()
    ws.close()


# ---- 4. the Python class ---------------------------------------------------------------------------------------------------------
def test_verlet_batch_kick_takes_tensors_or_an_object_with_forces():
    cfgs = [synthetic.config1(seed=3), synthetic.config1(seed=4)]
    sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                           c["types"], c["box"], device="cuda")) for c in cfgs]
    cavity = cavitymd.CavityForceBatch(sysdefs, [c["params"] for c in cfgs])
    rng = np.random.default_rng(20261113)
    host = []
    for c in cfgs:
        n = len(c["charge"])
        v = np.concatenate([rng.normal(0.0, 1e-3, (n, 3)), rng.uniform(1.0, 30.0, (n, 1))], axis=1)
        host.append({"N": n, "vel": v, "f": rng.normal(0.0, 1e-2, (n, 4))})
    velocities = [torch.from_numpy(h["vel"].copy()).cuda() for h in host]
    integrator = cavitymd.VerletBatch(cavity, velocities)
    integrator.set_inputs(7.0)

    class Part:
        forces = [torch.from_numpy(h["f"].copy()).cuda() for h in host]

    integrator.kick(Part, 2.0)                                                     # an object with .forces
    integrator.kick([Part.forces[0], None], 0.5)                                   # tensors; None: that system is left alone
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        integrator.kick(Part, 2.0)                                                 # the table exists: capturable
        with pytest.raises(RuntimeError, match="kick_table"):
            integrator.kick([None, Part.forces[1]], 1.0)                           # a new table is an upload: not in a capture
    graph.replay()
    torch.cuda.synchronize()
    row = _capi.verlet_input_make(7.0)
    for k, h in enumerate(host):
        mirror_kick(h, row, h["f"], 2.0)
        if k == 0:
            mirror_kick(h, row, h["f"], 0.5)
        mirror_kick(h, row, h["f"], 2.0)
        assert _same(velocities[k].cpu().numpy(), h["vel"]), k
    assert integrator.state()["steps"].tolist() == [0, 0]
    with pytest.raises(ValueError):
        integrator.kick([Part.forces[0]], 1.0)
    with pytest.raises(ValueError):
        integrator.kick([Part.forces[0][:, :3], Part.forces[1]], 1.0)
    integrator.close()
    cavity.close()
