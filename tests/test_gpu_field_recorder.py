"""The field recorder on the GPU: rho(k) of a batch of small systems, F(k,t) against each system's stored references and the
reference bookkeeping in ONE launch (cavmd_field_recorder_*, cavitymd.BatchFieldRecorder).

Tolerances -- none is new:
  rho(k) against the executed reference    <= 1e-12 N per component      (tests/test_gpu_reference_golden.py)
  F against the executed reference         <= 1e-12 N^2                  (tests/test_gpu_reference_golden.py)
  rho(k) against the exactly rounded sum   <= 1e-13 N per component      (tests/test_gpu_observables.py)
  rho(k) against cavmd_density_field       <= 2e-13 N                    (tests/test_gpu_observable_shapes.py, between mappings)
  F and rho2 given the fields              bit for bit: include/cavmd.h's expression in numpy float64 scalars
  items alone / shuffled / repeated / eager against replay: bit for bit.

Wall time on an MI355X: see DESIGN.md 3.7d (next to tests/test_gpu_recorder.py's)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi
from gpu_support import same_bits as _same_bits
from gpu_support import stream as _stream
from oracle import observables as obs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RAGGED_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 501, 1024, 4097, 65536)
NK_LIST = (1, 17, 50, 64, 65, 128, 256)
INV, EXPIRED, NOT_COMPUTED = _capi.CAVMD_ERR_INVALID_VALUE, _capi.CAVMD_ERR_EXPIRED, _capi.CAVMD_ERR_NOT_COMPUTED


def _wavevectors(n_k, kmag=1.0):
    return (obs.fibonacci_sphere(n_k) if n_k > 1 else np.array([[0.3, -0.4, 1.2]])) * kmag


def _device_positions(pos, stride):
    """(N, 3) packed for stride 24; (N, 4) with NaN in .w for stride 32 (the kernel must never read .w)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    if stride == 24:
        return torch.from_numpy(np.ascontiguousarray(pos)).cuda()
    p4 = np.full((pos.shape[0], 4), np.nan)
    p4[:, :3] = pos
    return torch.from_numpy(p4).cuda()


def _F(ref, cur):
    """include/cavmd.h, step 2: (sum over k ascending of (a_r a + b_r b)) / n_k, one rounding per operation, from +0."""
    acc = np.float64(0.0)
    for k in range(len(cur)):
        acc = acc + (np.float64(ref[k].real) * np.float64(cur[k].real) + np.float64(ref[k].imag) * np.float64(cur[k].imag))
    return acc / np.float64(len(cur))


def _expect_status(status, fn, *args):
    with pytest.raises(_capi.CavmdError) as e:
        fn(*args)
    assert e.value.status == status, (e.value.status, status)


# ---- 1. the executed reference -------------------------------------------------------------------------------------------
def test_old_fixtures_fields_and_F_match_the_executed_reference():
    gold = np.load(os.path.join(GOLDEN, "reference_python_golden.npz"))
    frames = gold["trajectory/frames"]
    n = frames.shape[1]
    for key in ("density/k1.0_n50", "density/k0.35_n17", "density/k2.5_n64"):
        pos = torch.from_numpy(np.ascontiguousarray(frames[0])).cuda()
        rec = cavitymd.BatchFieldRecorder([pos], wavevectors=gold[key + "/wavevectors"], capacity=8, max_references=1)
        for t in range(len(frames)):
            pos.copy_(torch.from_numpy(np.ascontiguousarray(frames[t])))
            rec.record()
            now, refs, ref_rows = rec.fields(0)
            err = np.abs(now - gold[key + "/rho_k"][t]).max()
            print(f"{key} frame {t}: |rho - reference| = {err:.3e} (bound {1e-12 * n:.3e})")
            assert err <= 1e-12 * n
            assert list(ref_rows) == [0] and refs.shape == (1, len(now))
        rows = rec.read()[0]
        assert list(rows["n_references"]) == [0, 1, 1, 1] and list(rows["took_reference"]) == [1, 0, 0, 0]
        for t in range(1, len(frames)):
            err = abs(rows["F"][t, 0] - gold[key + "/F_kt"][t])
            print(f"{key} row {t}: |F - reference| = {err:.3e} (bound {1e-12 * n * n:.3e})")
            assert err <= 1e-12 * n * n
        rec.close()


def test_new_fixture_when_references_are_taken_and_every_F():
    gold = np.load(os.path.join(GOLDEN, "reference_field_autocorr_golden.npz"))
    frames = gold["field_autocorr/frames"]
    T, n = frames.shape[0], frames.shape[1]
    assert T >= 12 and int(gold["field_autocorr/reference_interval_steps"]) == 3
    for run in gold["field_autocorr/runs"]:
        key = f"field_autocorr/{run}/"
        max_refs = int(gold[key + "max_references"])
        want_n, want_F = gold[key + "n_references"], gold[key + "F"]
        pos = torch.from_numpy(np.ascontiguousarray(frames[0])).cuda()
        rec = cavitymd.BatchFieldRecorder([pos], wavevectors=gold[key + "wavevectors"], capacity=T, max_references=max_refs,
                                          reference_interval=3)
        for t in range(T):
            pos.copy_(torch.from_numpy(np.ascontiguousarray(frames[t])))
            rec.record()
        rows = rec.read()[0]
        _, refs, ref_rows = rec.fields(0)
        # the reference's count AFTER step t is this row's count before it plus what it took
        assert list(rows["n_references"][1:]) == list(want_n[:-1]) and rows["n_references"][0] == 0
        assert list(rows["n_references"] + rows["took_reference"]) == list(want_n)
        assert list(ref_rows) == list(gold[key + "reference_timesteps"]) and len(refs) == min(max_refs, len(ref_rows))
        assert rows["took_reference"].sum() == max_refs                      # the cap bites in both runs
        worst = 0.0
        for t in range(T):
            for r in range(16):
                if r < max_refs and not np.isnan(want_F[t, r]):
                    assert r < rows["n_references"][t]
                    err = abs(rows["F"][t, r] - want_F[t, r])
                    worst = max(worst, err)
                    assert err <= 1e-12 * n * n, (run, t, r, err)
                else:
                    assert rows["F"][t, r] == 0.0 and r >= rows["n_references"][t], (run, t, r)
        print(f"{run}: references at rows {list(ref_rows)}; max |F - reference| = {worst:.3e} (bound {1e-12 * n * n:.3e})")
        rec.close()


# ---- 2. rho against the exact sum and the single path; independence; fixed order ---------------------------------------
def _ragged_systems(seed=7):
    rng = np.random.default_rng(seed)
    return [(n, (24, 32)[i % 2], rng.uniform(-20.0, 20.0, (n, 3))) for i, n in enumerate(RAGGED_SIZES)]


def _record_once(systems, k, calls=1, **kw):
    """One recorder over `systems` [(n, stride, pos)], `calls` record calls; rows (B, calls) and per-item fields."""
    tensors = [_device_positions(p, s) for _, s, p in systems]
    ws = _capi.Workspace(1)
    rec = _capi.FieldRecorder(ws, [_capi.field_item(t.data_ptr() if n else 0, s, n) for t, (n, s, _) in zip(tensors, systems)],
                              k, kw.get("capacity", 8), 1, kw.get("max_references", 2), kw.get("reference_interval", 1))
    for _ in range(calls):
        rec.record(_stream())
    rows = rec.read(_stream(), 0, len(systems), 0, calls)
    fields = [rec.read_fields(_stream(), i) for i in range(len(systems))]
    rec.close()
    ws.close()
    return rows, fields


@pytest.mark.parametrize("n_k", NK_LIST)
def test_ragged_batch_against_the_exact_sum_and_the_single_path(n_k):
    systems = _ragged_systems()
    k = _wavevectors(n_k)
    rows, fields = _record_once(systems, k)
    single = _capi.Workspace(max(RAGGED_SIZES))
    single.set_wavevectors(k)
    for i, (n, stride, pos) in enumerate(systems):
        now = fields[i][0]
        assert now.shape == (n_k,)
        if n == 0:
            assert not now.real.any() and not now.imag.any() and rows[i, 0]["rho2"] == 0.0
            continue
        exact = obs.density_field_exact(pos, k)
        err = max(np.abs(now.real - exact.real).max(), np.abs(now.imag - exact.imag).max())
        t = _device_positions(pos, stride)
        single.density_field(_stream(), n, t.data_ptr(), stride)
        one = single.density_field_read()
        err1 = max(np.abs(now.real - one.real).max(), np.abs(now.imag - one.imag).max())
        print(f"n_k={n_k} N={n} stride={stride}: |rho - exact| = {err:.3e} (bound {1e-13 * n:.3e}); "
              f"|rho - cavmd_density_field| = {err1:.3e} (bound {2e-13 * n:.3e})")
        assert err <= 1e-13 * n, (n, n_k)
        assert err1 <= 2e-13 * n, (n, n_k)
    single.close()


@pytest.mark.parametrize("n_k", (50, 65))
def test_items_are_independent_and_the_sum_order_is_fixed(n_k):
    systems = _ragged_systems()
    k = _wavevectors(n_k)
    rows, fields = _record_once(systems, k, calls=3)
    # repetition: the same positions give the same field bits on every call (rho2 sees every bit of it)
    for i in range(len(systems)):
        assert len({rows[i, c]["rho2"].tobytes() for c in range(3)}) == 1
        assert _same_bits(fields[i][1][0], fields[i][0])                     # reference 0 (call 1) = the field of call 3
    # alone in a batch of one
    for i, s in enumerate(systems):
        rows1, fields1 = _record_once([s], k, calls=3)
        assert _same_bits(rows1[0], rows[i]), s[0]
        assert _same_bits(fields1[0][0], fields[i][0]) and _same_bits(fields1[0][1], fields[i][1])
    # shuffled (and with it every item's place in the launch order and its block)
    perm = np.random.default_rng(3).permutation(len(systems))
    rows_p, fields_p = _record_once([systems[j] for j in perm], k, calls=3)
    for pos_in_batch, j in enumerate(perm):
        assert _same_bits(rows_p[pos_in_batch], rows[j]), systems[j][0]
        assert _same_bits(fields_p[pos_in_batch][0], fields[j][0])


# ---- 3. F is exact given rho -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_k", (50, 65, 256))
def test_F_and_rho2_are_the_stated_expression_bit_for_bit(n_k):
    rng = np.random.default_rng(11)
    sizes = (501, 64, 0, 130)
    tensors = [torch.from_numpy(rng.uniform(-20.0, 20.0, (n, 3))).cuda() for n in sizes]
    rec = cavitymd.BatchFieldRecorder(tensors, wavevectors=_wavevectors(n_k, 0.7), capacity=4, max_references=4,
                                      reference_interval=2)
    CALLS = 10
    for call in range(CALLS):
        for t in tensors:
            t.add_(0.01 * (call + 1))
        rec.record()
        last = rec.read(first=call, count=1)[:, 0]
        for i, n in enumerate(sizes):
            now, refs, ref_rows = rec.fields(i)
            row = last[i]
            want_refs = min(4, call // 2 + 1)                                 # taken at rows 0, 2, 4, 6
            assert len(refs) == want_refs and list(ref_rows) == [0, 2, 4, 6][:want_refs], (call, i)
            took = int(row["took_reference"])
            assert row["call"] == call + 1 and row["reserved"] == 0.0 and row["n_references"] + took == len(refs)
            assert took == (1 if call in (0, 2, 4, 6) else 0)
            for r in range(16):
                if r < row["n_references"]:
                    assert _same_bits(row["F"][r], _F(refs[r], now)), (call, i, r)
                else:
                    assert row["F"][r] == 0.0 and not np.signbit(row["F"][r])
            assert _same_bits(row["rho2"], _F(now, now)), (call, i)
            if took:
                assert _same_bits(refs[-1], now)                              # the reference taken now IS this call's field
            if n == 0:
                assert row["rho2"] == 0.0 and not now.real.any()
    _expect_status(EXPIRED, rec.read, 0, 1)                                    # capacity 4: rows 0 .. 5 are gone
    assert rec.read(first=None).shape == (len(sizes), 4)
    rec.close()


# ---- 4. replay --------------------------------------------------------------------------------------------------------------
def _replay_run(captured, replays, take_at=(), **kw):
    rng = np.random.default_rng(21)
    sizes = (501, 501, 64, 257)
    tensors = [torch.from_numpy(rng.uniform(-20.0, 20.0, (n, 3))).cuda() for n in sizes]
    deltas = [torch.from_numpy(rng.normal(0.0, 1e-3, (n, 3))).cuda() for n in sizes]
    take = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
    rec = cavitymd.BatchFieldRecorder(tensors, wavevectors=_wavevectors(50), **kw)

    def step():
        for t, d in zip(tensors, deltas):
            t.add_(d)
        rec.record(take_reference=take)

    torch.cuda.synchronize()
    graph = None
    if captured:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        assert list(rec.rows()) == [0] * len(sizes)                            # a capture runs nothing
    for r in range(replays):
        if r in take_at:
            take.fill_(1)                                                       # in stream order, before the step
        graph.replay() if captured else step()
        if r in take_at:
            take.zero_()
        if r == replays // 2:                                                   # a read between replays disturbs nothing
            assert len(set(rec.rows().tolist())) == 1
    rows = rec.rows()
    series = rec.read(first=None)
    fields = [rec.fields(i) for i in range(len(sizes))]
    first_held = max(int(rows.max()) - rec.capacity, 0)
    if first_held > 0:
        _expect_status(EXPIRED, rec.read, first_held - 1, 1)
    rec.close()
    return rows, series, fields, first_held


def test_a_replayed_graph_appends_and_takes_references_like_eager_calls():
    REPLAYS, kw = 200, dict(reference_interval=7, max_references=5, capacity=64, period=3)
    rows_e, eager, fields_e, _ = _replay_run(False, REPLAYS, **kw)
    rows_g, replayed, fields_g, first = _replay_run(True, REPLAYS, **kw)
    assert list(rows_e) == list(rows_g) == [REPLAYS // 3] * 4 and first == REPLAYS // 3 - 64 == 2
    assert eager.shape == replayed.shape == (4, 64)
    for i in range(4):
        assert list(replayed[i]["call"]) == [3 * (j + 1) for j in range(first, first + 64)]
        assert _same_bits(replayed[i], eager[i]), i
        assert list(fields_g[i][2]) == [0, 7, 14, 21, 28]                       # step 4 of the contract
        took = [first + j for j in range(64) if replayed[i]["took_reference"][j]]
        assert took == [7, 14, 21, 28]                                           # row 0 has left the ring
        assert set(replayed[i]["n_references"][27:]) == {5}
        assert _same_bits(fields_g[i][0], fields_e[i][0]) and _same_bits(fields_g[i][1], fields_e[i][1])
        assert len({r["rho2"].tobytes() for r in replayed[i]}) == 64            # a series: every replay saw other positions


def test_take_reference_words_refreshed_between_replays():
    kw = dict(reference_interval=0, max_references=3, capacity=64, period=1)
    asked = (5, 9, 12, 20)
    rows_e, eager, fields_e, _ = _replay_run(False, 30, take_at=asked, **kw)
    rows_g, replayed, fields_g, _ = _replay_run(True, 30, take_at=asked, **kw)
    assert list(rows_g) == [30] * 4
    for i in range(4):
        assert list(fields_g[i][2]) == [0, 5, 9]                                # never beyond max_references
        assert [j for j in range(30) if replayed[i]["took_reference"][j]] == [0, 5, 9]
        assert list(replayed[i]["n_references"]) == [0] + [1] * 5 + [2] * 4 + [3] * 20
        assert _same_bits(replayed[i], eager[i])
        assert _same_bits(fields_g[i][1], fields_e[i][1])


# ---- 5. slow path and non-finite input --------------------------------------------------------------------------------------
def test_huge_and_non_finite_coordinates_stay_in_their_item():
    rng = np.random.default_rng(31)
    sizes = (501, 300, 130, 64)
    k = _wavevectors(17, 1.3)
    base = [rng.uniform(-20.0, 20.0, (n, 3)) for n in sizes]
    second = [p + 0.01 for p in base]
    third = [p - 0.02 for p in base]
    dirty = [p.copy() for p in second]
    dirty[1][77, 1] = 1.0e12          # |k . r| ~ 1e12: that tile must take the device library's sincos
    dirty[2][129, 0] = np.nan

    def run(frames):
        tensors = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in frames[0]]
        rec = cavitymd.BatchFieldRecorder(tensors, wavevectors=k, capacity=8, max_references=2, reference_interval=0)
        fields = []
        for f in frames:
            for t, p in zip(tensors, f):
                t.copy_(torch.from_numpy(np.ascontiguousarray(p)))
            rec.record()
            fields.append([rec.fields(i)[0] for i in range(len(sizes))])
        rows = rec.read()
        rec.close()
        return rows, fields

    rows_d, fields_d = run([base, dirty, third])
    rows_c, fields_c = run([base, second, third])
    for i in (0, 3):                                                            # untouched items: the same bits throughout
        assert _same_bits(rows_d[i], rows_c[i])
    assert np.isnan(rows_d[2, 1]["rho2"]) and np.isnan(rows_d[2, 1]["F"][0]) and np.isnan(fields_d[1][2]).all()
    assert np.isfinite(rows_d[1, 1]["rho2"]) and np.isfinite(fields_d[1][1].real).all()
    # the huge coordinate: torch's CPU sin / cos on the phases formed as the kernel forms them, summed exactly
    p = dirty[1]
    got = fields_d[1][1]
    for j, kv in enumerate(k):
        kr = torch.from_numpy((p[:, 0] * kv[0] + p[:, 1] * kv[1]) + p[:, 2] * kv[2])
        want = complex(math.fsum(torch.cos(kr).tolist()), math.fsum(torch.sin(kr).tolist()))
        err = max(abs(got[j].real - want.real), abs(got[j].imag - want.imag))
        assert err <= 1e-13 * len(p), (j, err)
    # the next clean call equals a recorder's that never saw them: rows and fields of every item
    assert _same_bits(rows_d[:, 2], rows_c[:, 2])
    for i in range(len(sizes)):
        assert _same_bits(fields_d[2][i], fields_c[2][i])
    assert _same_bits(rows_d[:, 0], rows_c[:, 0])


# ---- 6. refusals, each followed by a correct call ------------------------------------------------------------------------
def test_refusals_and_lifetime():
    rng = np.random.default_rng(41)
    pos = torch.from_numpy(rng.uniform(-20.0, 20.0, (501, 3))).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.BatchFieldRecorder([pos.cpu()])
    for bad in (dict(wavevectors=np.zeros((0, 3))), dict(wavevectors=_wavevectors(257)), dict(max_references=0),
                dict(max_references=17), dict(capacity=0), dict(period=0)):
        _expect_status(INV, lambda kw=bad: cavitymd.BatchFieldRecorder([pos], **kw))
    ws = _capi.Workspace(1)
    item = _capi.field_item(pos.data_ptr(), 24, 501)
    rec = _capi.FieldRecorder(ws, [item], _wavevectors(50), 4, 1, 2, 0)
    assert ws._lib.cavmd_destroy(ws.handle) == INV                              # refused while the field recorder lives
    _expect_status(NOT_COMPUTED, rec.read, _stream(), 0, 1, 0, 1)
    _expect_status(NOT_COMPUTED, rec.read_fields, _stream(), 0)
    _expect_status(INV, rec.record, _stream(), pos.data_ptr() + 2)              # a misaligned take_reference array
    rec.record(_stream())
    assert list(rec.rows(_stream())) == [1]
    for first_row, count in ((1, 1), (0, 2), (0, 0)):
        _expect_status(INV, rec.read, _stream(), 0, 1, first_row, count)
    for first_item, n_items in ((1, 1), (0, 2), (0, 0)):
        _expect_status(INV, rec.read, _stream(), first_item, n_items, 0, 1)
    _expect_status(INV, rec.read_fields, _stream(), 1)
    _expect_status(_capi.CAVMD_ERR_INVALID_VALUE, rec.set_items, 0, [_capi.field_item(pos.data_ptr(), 28, 501)])
    _expect_status(_capi.CAVMD_ERR_CAPACITY, rec.set_items, 0, [_capi.field_item(pos.data_ptr(), 24, 65537)])
    _expect_status(INV, rec.set_items, 1, [item])
    first = rec.read(_stream(), 0, 1, 0, 1)
    # a capturing stream: record is captured, everything that would wait for the stream is refused
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = _stream()
        rec.record(s)
        _expect_status(INV, rec.rows, s)
        _expect_status(INV, rec.read, s, 0, 1, 0, 1)
        _expect_status(INV, rec.read_fields, s, 0)
        _expect_status(INV, rec.set_items, 0, [item])
    torch.cuda.synchronize()
    assert list(rec.rows(_stream())) == [1]
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert list(rec.rows(_stream())) == [3]
    got = rec.read(_stream(), 0, 1, 0, 3)
    assert _same_bits(got[0, 0], first[0, 0]) and list(got[0]["call"]) == [1, 2, 3]
    assert list(got[0]["n_references"]) == [0, 1, 1] and got[0, 1]["F"][0] == got[0, 0]["rho2"] == got[0, 2]["F"][0]
    # set_items: item 0 now follows other positions; counters, series and references are kept
    other = torch.from_numpy(rng.uniform(-20.0, 20.0, (64, 4))).cuda()
    rec.set_items(0, [_capi.field_item(other.data_ptr(), 32, 64)])
    rec.record(_stream())
    assert list(rec.rows(_stream())) == [4]
    assert _same_bits(rec.read(_stream(), 0, 1, 1, 3)[0, :2], got[0, 1:])
    now, refs, ref_rows = rec.read_fields(_stream(), 0)
    exact = obs.density_field_exact(other[:, :3].cpu().numpy(), _wavevectors(50))
    assert max(np.abs(now.real - exact.real).max(), np.abs(now.imag - exact.imag).max()) <= 1e-13 * 64
    assert list(ref_rows) == [0]
    # reset forgets rows, counters and references
    rec.reset(_stream())
    assert list(rec.rows(_stream())) == [0]
    _expect_status(NOT_COMPUTED, rec.read_fields, _stream(), 0)
    rec.record(_stream())
    row = rec.read(_stream(), 0, 1, 0, 1)[0, 0]
    assert row["call"] == 1 and row["n_references"] == 0 and row["took_reference"] == 1
    records_ptr, rows_ptr = rec.device_ptr()
    assert records_ptr and rows_ptr and records_ptr % 16 == 0
    del graph
    rec.close()
    assert ws._lib.cavmd_destroy(ctypes.c_void_p(0)) == 0
    ws.close()                                                                   # now it goes
