"""Save and restore of a batch run on the GPU (tests/checkpoint_runs.py builds the run): a run stopped after 11 replays, saved,
thrown away, rebuilt from the same constructors, loaded and replayed 13 more times holds the bytes of 24 uninterrupted
replays -- arrays, accelerations, every object's state, and every row the four series still hold; the same with a
LangevinBathBatch; a rewind inside live objects under the graph captured before it; saves that disturb nothing; the refusals;
and the example.  Every comparison is exact: the feature copies bytes and every kernel involved repeats bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_support import ROOT
from checkpoint_runs import Run
from gpu_support import stream as _stream

pytestmark = pytest.mark.gpu

TOTAL, STOP = 24, 11          # 11 lands in the middle of the field recorder's period of 2 and between two references


def _assert_same(got: dict, want: dict, what: str):
    assert got.keys() == want.keys(), (what, set(got) ^ set(want))
    differ = [key for key in want if got[key] != want[key]]
    assert not differ, (what, differ)


def _uninterrupted(with_bath: bool):
    run = Run(with_bath)
    run.capture()
    run.replay(STOP)
    at_stop = run.observe()
    run.replay(TOTAL - STOP)
    at_end = run.observe()
    rows = {name: np.frombuffer(at_end["rows." + name], dtype=np.uint64) for name in ("recorder", "ledger", "fields", "trajectory")}
    assert rows["recorder"].tolist() == [TOTAL] * 4 == rows["ledger"].tolist()     # the empty system takes part
    assert rows["fields"].tolist() == [TOTAL // 2] * 4                              # all three rings have wrapped (8, 8, 4 slots)
    assert differs(at_stop, at_end)
    run.close()
    return at_stop, at_end


def differs(a: dict, b: dict):
    return [key for key in a if a[key] != b[key]]


@pytest.fixture(scope="module")
def run_a():
    return _uninterrupted(False)


@pytest.fixture(scope="module")
def run_a_bath():
    return _uninterrupted(True)


def _stopped_and_resumed(with_bath: bool, reference, path):
    at_stop, at_end = reference
    run = Run(with_bath)
    run.capture()
    run.replay(STOP)
    _assert_same(run.observe(), at_stop, "the run before the save")
    run.checkpoint.save(path)
    run.close()                                                                   # every object and tensor goes
    del run
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    fresh = Run(with_bath)                                                        # the same constructors
    assert fresh.draw.state().tobytes() != at_stop["state.draw"]                  # nothing of the old run is left
    fresh.checkpoint.load(path)
    _assert_same(fresh.observe(), at_stop, "fresh objects after the load, before any launch")
    fresh.capture()                                                               # a new graph
    fresh.replay(TOTAL - STOP)
    got = fresh.observe()
    fresh.close()
    _assert_same(got, at_end, "fresh objects, 13 replays after the load")
    return got


def test_continuation_in_fresh_objects(run_a, tmp_path):
    got = _stopped_and_resumed(False, run_a, tmp_path / "run.npz")
    with np.load(tmp_path / "run.npz", allow_pickle=False) as f:                  # one .npz, numpy alone reads it
        assert "object.integrator.accel.3" in f.files and f["object.integrator.accel.3"].shape == (0, 3)
        assert f["object.integrator.accel.2"].shape == (433, 3) and f["system.2.position"].shape == (433, 4)
        assert f["object.thermostat.snapshot"].dtype == np.uint8
    states = np.frombuffer(got["state.thermostat"], dtype=np.float64).reshape(4, 6)
    assert (states[:3, 0] != 0.0).all()                                           # the Bussi reservoirs moved, and continued


def test_continuation_with_a_langevin_bath(run_a_bath, tmp_path):
    from cavitymd import _capi
    got = _stopped_and_resumed(True, run_a_bath, tmp_path / "run.npz")
    bath = np.frombuffer(got["state.bath"], dtype=_capi.bath_state_dtype())
    stop = np.frombuffer(run_a_bath[0]["state.bath"], dtype=_capi.bath_state_dtype())
    assert (bath["draws"][:3] > stop["draws"][:3]).all() and (stop["draws"][:3] > 0).all()    # the counters went on from the save
    assert (bath["reservoir"][:3] != stop["reservoir"][:3]).all()


def test_rewind_in_live_objects_under_the_same_graph(run_a):
    run = Run(False)
    run.capture()
    run.replay(STOP)
    saved = run.checkpoint.state()                                                # to memory
    run.replay(5)
    first = run.observe()
    assert differs(first, run_a[0])
    run.checkpoint.load_state(saved)
    _assert_same(run.observe(), run_a[0], "after the rewind")
    run.replay(5)                                                                 # the SAME graph: device addresses did not move
    second = run.observe()
    run.close()
    _assert_same(second, first, "5 replays after the rewind")


def test_saving_disturbs_nothing(run_a, tmp_path):
    run = Run(False)
    run.capture()
    for r in range(1, TOTAL + 1):
        run.replay(1)
        if r in (3, 11, 12):
            run.checkpoint.save(tmp_path / "run.npz")
    got = run.observe()
    run.close()
    _assert_same(got, run_a[1], "24 replays with three saves")
    assert sorted(os.listdir(tmp_path)) == ["run.npz"]


def test_refusals_on_the_device():
    from cavitymd import _capi
    INV = _capi.CAVMD_ERR_INVALID_VALUE

    def refused(call, *args):
        with pytest.raises(_capi.CavmdError) as e:
            call(*args)
        assert e.value.status == INV, e.value

    run = Run(False)
    run.capture()
    run.replay(3)
    other = Run(False, draw_seed=2025, recorder_capacity=16, n_k=6)                # each differs in one word of its shape
    other.capture()
    other.replay(3)
    fewer = Run(False, n_systems=3)
    before = run.observe()
    handles = {name: obj._need() for name, obj in run.objects.items()}
    blobs = {name: h.snapshot_save(_stream()) for name, h in handles.items()}
    assert {name: len(b) for name, b in blobs.items()} == {name: h.snapshot_bytes() for name, h in handles.items()}
    names = list(handles)
    for k, name in enumerate(names):
        h = handles[name]
        refused(h.snapshot_load, _stream(), blobs[names[(k + 1) % len(names)]])                   # a blob of another kind
        refused(h.snapshot_load, _stream(), fewer.objects[name]._need().snapshot_save(_stream()))  # of another n_items
        refused(h.snapshot_load, _stream(), blobs[name][:-1])                                     # truncated
        refused(h.snapshot_load, _stream(), blobs[name][:40])
        refused(h.snapshot_load, _stream(), np.concatenate([blobs[name], np.zeros(16, dtype=np.uint8)]))
        refused(h.snapshot_load, _stream(), np.zeros(0, dtype=np.uint8))                          # a null buffer
        fn = getattr(h._lib, "cavmd_snapshot_%s_save" % h._PREFIX[len("cavmd_"):])
        assert fn(h._h, None, None, len(blobs[name])) == INV
        small = np.zeros(len(blobs[name]) - 16, dtype=np.uint8)
        assert fn(h._h, None, small.ctypes.data, small.size) == INV                               # a buffer of another size
        assert not small.any()
    refused(handles["recorder"].snapshot_load, _stream(), other.recorder._need().snapshot_save(_stream()))   # another capacity
    refused(handles["fields"].snapshot_load, _stream(), other.fields._need().snapshot_save(_stream()))       # another n_k
    refused(handles["draw"].snapshot_load, _stream(), other.draw._need().snapshot_save(_stream()))           # another seed
    # ... which the blobs of the unchanged shapes are not: the ledger's would load
    assert _capi.snapshot_check(other.ledger._need().snapshot_save(_stream()),
                                _capi.SnapshotHeader.from_buffer_copy(blobs["ledger"][:64].tobytes())) == _capi.CAVMD_OK
    refused(run.draw.load_state_dict, other.draw.state_dict())                     # the library's word: the seed
    with pytest.raises(ValueError):                                                # the Python check: the names, before the library
        run.integrator.load_state_dict(fewer.integrator.state_dict())
    _assert_same(run.observe(), before, "after the refused loads")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                                # during a capture
        run.recorder.record()
        for name, h in handles.items():
            refused(h.snapshot_save, _stream())
            refused(h.snapshot_load, _stream(), blobs[name])
        with pytest.raises(RuntimeError, match="cannot be captured"):
            run.recorder.state_dict()
        with pytest.raises(RuntimeError, match="cannot be captured"):
            run.recorder.load_state_dict({"snapshot": blobs["recorder"]})
        with pytest.raises(RuntimeError, match="cannot be captured"):
            run.checkpoint.state()
    del graph                                                                                    # never replayed
    _assert_same(run.observe(), before, "after the refusals during a capture")
    for name, h in handles.items():                                                              # and the accepted one
        h.snapshot_load(_stream(), blobs[name])
    _assert_same(run.observe(), before, "after loading its own blobs")
    for r in (fewer, other, run):
        r.close()


def test_the_example_runs_and_prints_the_equality_line():
    example = os.path.join(ROOT, "examples", "checkpoint", "batch_restart_in_one_graph.py")
    done = subprocess.run([sys.executable, example, "3", "6"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "the restarted run equals the uninterrupted one: True" in done.stdout, done.stdout
