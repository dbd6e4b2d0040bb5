"""Save and restore of a batch run, what a machine WITHOUT a GPU can check: the 28 cavmd_snapshot_* names in the header and in
both libraries, the layout of cavmd_snapshot_header from C99, ctypes and numpy, null arguments, the refusal matrix of
cavmd_snapshot_check, and BatchCheckpoint's file handling on CPU tensors with objects that record the calls they receive."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_support as abi

OBJECTS = ("verlet", "bath", "draw", "thermalize", "bussi_batch", "recorder", "ledger", "trajectory", "field_recorder")
NAMES = ["cavmd_snapshot_check"] + ["cavmd_snapshot_%s_%s" % (obj, call) for obj in OBJECTS for call in ("bytes", "save", "load")]
HEADER_OFFSETS = dict(magic=0, version=8, kind=12, n_items=16, n_counters=20, capacity=24, record_bytes=32, word=40, bytes=48,
                      reserved=56)


# ---- the names -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_libraries_export_the_28_names(capi):
    assert len(NAMES) == 28
    assert abi.declared("cavmd_snapshot_") == sorted(NAMES)
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        assert {s for s in abi.exported(path) if s.startswith("cavmd_snapshot_")} == set(NAMES), path
    in_capi = [n for n in capi._PROTOTYPES if n.startswith("cavmd_snapshot_")]
    assert in_capi == NAMES                                                        # the header's order
    text = abi.header_text()
    at = [text.index("%s(" % n) for n in NAMES]
    assert at == sorted(at) and text.index("cavmd_profile_samples(") < at[0] and at[-1] < text.index("cavmd_set_tunable(")
    order = list(capi._PROTOTYPES)
    assert order.index("cavmd_profile_samples") + 1 == order.index(NAMES[0])
    assert order.index(NAMES[-1]) + 1 == order.index("cavmd_set_tunable")
    assert capi.SNAPSHOT_KINDS == {obj: k + 1 for k, obj in enumerate(OBJECTS)}
    for obj, kind in capi.SNAPSHOT_KINDS.items():
        assert "#define CAVMD_SNAPSHOT_%s %du" % (obj.upper(), kind) in text
    assert "#define CAVMD_SNAPSHOT_MAGIC 0x%016Xull" % capi.SNAPSHOT_MAGIC in text
    assert capi.SNAPSHOT_MAGIC.to_bytes(8, "little") == b"CAVSNAP1"


def test_the_nine_classes_have_state_dict_and_the_package_exports_the_checkpoint():
    import cavitymd
    for cls in ("VerletBatch", "LangevinBathBatch", "StepDraw", "BatchThermalizer", "BussiReservoirBatch", "BatchRecorder",
                "BatchEnergyLedger", "BatchFieldRecorder", "BatchTrajectoryRecorder"):
        for name in ("state_dict", "load_state_dict"):
            assert callable(getattr(getattr(cavitymd, cls), name)), (cls, name)
    assert "BatchCheckpoint" in cavitymd.__all__ and cavitymd.BatchCheckpoint is cavitymd.checkpoint.BatchCheckpoint
    for handle in ("Verlet", "Bath", "Draw", "Thermalize", "BussiBatch", "Recorder", "Ledger", "Trajectory", "FieldRecorder"):
        for name in ("snapshot_bytes", "snapshot_save", "snapshot_load"):
            assert callable(getattr(getattr(cavitymd._capi, handle), name)), (handle, name)
    for handle in ("Batch", "Molecular", "Coulomb"):                               # they keep nothing a later launch reads
        assert not hasattr(getattr(cavitymd._capi, handle), "snapshot_save"), handle


# ---- the layout ----------------------------------------------------------------------------------------------------------
def test_header_layout_from_c99_ctypes_and_numpy(capi, tmp_path):
    stdout = abi.run_c99("snapshot_abi_check", capi, tmp_path)
    assert "SNAPSHOT-ABI-OK" in stdout, stdout
    sizes, offsets = abi.c_layouts(stdout)
    assert sizes == {"header": 64} and offsets["header"] == HEADER_OFFSETS
    S = capi.SnapshotHeader
    assert ctypes.sizeof(S) == 64 and {name: getattr(S, name).offset for name, *_ in S._fields_} == HEADER_OFFSETS
    dt = capi.snapshot_header_dtype()
    assert dt.itemsize == 64 and {name: dt.fields[name][1] for name in dt.names} == HEADER_OFFSETS
    for name in dt.names:
        assert dt.fields[name][0].itemsize == getattr(S, name).size, name


# ---- null arguments ------------------------------------------------------------------------------------------------------
def test_null_object_or_buffer_is_refused(capi):
    INV = capi.CAVMD_ERR_INVALID_VALUE
    for lib in (capi.load(), capi.load_hooks_build()):
        buf = np.zeros(256, dtype=np.uint8)
        p = ctypes.c_void_p(buf.ctypes.data)
        for obj in OBJECTS:
            n = ctypes.c_size_t(7)
            assert getattr(lib, "cavmd_snapshot_%s_bytes" % obj)(None, ctypes.byref(n)) == INV and n.value == 7, obj
            assert getattr(lib, "cavmd_snapshot_%s_bytes" % obj)(None, None) == INV, obj
            for call in ("save", "load"):
                fn = getattr(lib, "cavmd_snapshot_%s_%s" % (obj, call))
                assert fn(None, None, p, buf.size) == INV, (obj, call)
                assert fn(None, None, None, buf.size) == INV, (obj, call)
                assert fn(None, None, None, 0) == INV, (obj, call)
        assert not buf.any()


# ---- cavmd_snapshot_check --------------------------------------------------------------------------------------------------
def _header(capi, kind=6, n_items=3, n_counters=4, capacity=8, record_bytes=128, word=(0, 0), nbytes=64 + 96 + 3072):
    h = capi.SnapshotHeader()
    h.magic, h.version, h.kind, h.n_items, h.n_counters = capi.SNAPSHOT_MAGIC, capi.SNAPSHOT_VERSION, kind, n_items, n_counters
    h.capacity, h.record_bytes, h.bytes = capacity, record_bytes, nbytes
    h.word[0], h.word[1] = word
    return h


def _blob(h, length=None):
    length = int(h.bytes) if length is None else length
    raw = bytes(h)[:length]
    return np.frombuffer(raw + b"\xA5" * (length - len(raw)), dtype=np.uint8).copy()


ALTERED = [("magic", lambda h: setattr(h, "magic", h.magic ^ 1)), ("version", lambda h: setattr(h, "version", 2)),
           ("kind", lambda h: setattr(h, "kind", 7)), ("n_items", lambda h: setattr(h, "n_items", 4)),
           ("n_counters", lambda h: setattr(h, "n_counters", 5)), ("capacity", lambda h: setattr(h, "capacity", 9)),
           ("record_bytes", lambda h: setattr(h, "record_bytes", 192)), ("word0", lambda h: h.word.__setitem__(0, 1)),
           ("word1", lambda h: h.word.__setitem__(1, 1)), ("bytes", lambda h: setattr(h, "bytes", h.bytes + 16)),
           ("reserved0", lambda h: h.reserved.__setitem__(0, 1)), ("reserved1", lambda h: h.reserved.__setitem__(1, 1))]


def test_check_accepts_one_blob_and_refuses_the_matrix(capi):
    INV = capi.CAVMD_ERR_INVALID_VALUE
    good = _header(capi)
    total = int(good.bytes)
    assert capi.snapshot_check(_blob(good), good) == capi.CAVMD_OK
    assert capi.snapshot_check(bytes(_blob(good)), good) == capi.CAVMD_OK
    for name, alter in ALTERED:                                                   # each field, one at a time
        h = _header(capi)
        alter(h)
        assert bytes(h) != bytes(good), name
        assert capi.snapshot_check(_blob(h, total), good) == INV, name
        if name not in ("magic", "version", "reserved0", "reserved1"):            # and on the side of what is expected
            assert capi.snapshot_check(_blob(good), h) == INV, name
    for length in range(0, 65):                                                   # every truncation
        assert capi.snapshot_check(_blob(good, length), good) == INV, length
    for length in (total - 1, total + 1):                                         # bytes off by one
        assert capi.snapshot_check(_blob(good, length), good) == INV, length
    lib = capi.load()
    b = _blob(good)
    assert lib.cavmd_snapshot_check(None, total, ctypes.byref(good)) == INV
    assert lib.cavmd_snapshot_check(ctypes.c_void_p(b.ctypes.data), total, None) == INV
    odd = np.zeros(total + 1, dtype=np.uint8)                                     # a blob need not be aligned
    odd[1:] = b
    assert lib.cavmd_snapshot_check(ctypes.c_void_p(odd.ctypes.data + 1), total, ctypes.byref(good)) == capi.CAVMD_OK


# ---- BatchCheckpoint on CPU tensors ----------------------------------------------------------------------------------------
class Recording:
    """stands in for a batch object: hands out a state and records the calls it receives"""

    def __init__(self, value):
        self.value, self.calls = value, []

    def state_dict(self, stream=None):
        self.calls.append("state_dict")
        return {"snapshot": np.full(80, self.value, dtype=np.uint8), "inputs": np.full((2, 8), float(self.value))}

    def check_state_dict(self, d):
        self.calls.append("check_state_dict")
        if set(d) != {"snapshot", "inputs"}:
            raise ValueError("names")

    def load_state_dict(self, d, stream=None):
        self.calls.append(("load_state_dict", int(d["snapshot"][0]), float(d["inputs"][0, 0])))


def _run(sizes=(17, 0, 5), seed=0):
    import cavitymd
    rng = np.random.default_rng(seed)
    sysdefs, velocities = [], []
    for n in sizes:
        pd = cavitymd.ParticleData.from_arrays(rng.normal(size=(n, 3)), np.zeros(n, dtype=np.int32), rng.normal(size=n),
                                               rng.integers(-3, 4, size=(n, 3)).astype(np.int32), ["O"], [9.0, 10.0, 11.0],
                                               device="cpu")
        sysdefs.append(cavitymd.SystemDefinition(pd))
        velocities.append(torch.from_numpy(rng.normal(size=(n, 4))))
    objects = {"integrator": Recording(3), "draw": Recording(4)}
    return cavitymd.BatchCheckpoint(sysdefs, velocities, objects), sysdefs, velocities, objects


def _tensors(sysdefs, velocities):
    out = []
    for s, v in zip(sysdefs, velocities):
        pd = s.getParticleData()
        out += [pd.getPositions().clone(), pd.getImages().clone(), v.clone()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_checkpoint_round_trip_on_cpu(tmp_path):
    path = tmp_path / "run.npz"
    ckpt, sysdefs, velocities, objects = _run(seed=1)
    saved = _tensors(sysdefs, velocities)
    ckpt.save(path)
    assert sorted(os.listdir(tmp_path)) == ["run.npz"]
    assert objects["integrator"].calls == ["state_dict"]
    other, sysdefs2, velocities2, objects2 = _run(seed=2)
    assert not _same(_tensors(sysdefs2, velocities2), saved)
    other.load(path)
    assert _same(_tensors(sysdefs2, velocities2), saved)                            # all four columns, images, velocities
    assert objects2["integrator"].calls == ["check_state_dict", ("load_state_dict", 3, 3.0)]
    assert objects2["draw"].calls == ["check_state_dict", ("load_state_dict", 4, 4.0)]


@pytest.mark.parametrize("case", ["missing system array", "missing object array", "unknown name", "system count", "N", "dtype",
                                  "format"])
def test_checkpoint_load_refuses_before_it_writes(tmp_path, case):
    path = tmp_path / "run.npz"
    if case == "system count":
        _run(sizes=(17, 0), seed=1)[0].save(path)
    elif case == "N":
        _run(sizes=(17, 0, 6), seed=1)[0].save(path)
    else:
        ckpt = _run(seed=1)[0]
        arrays = ckpt.state()
        if case == "missing system array":
            del arrays["system.2.image"]
        elif case == "missing object array":
            del arrays["object.draw.inputs"]
        elif case == "unknown name":
            arrays["system.3.position"] = np.zeros((1, 4))
        elif case == "dtype":
            arrays["system.0.velocity"] = arrays["system.0.velocity"].astype(np.float32)
        elif case == "format":
            arrays["format"] = np.array([2], dtype=np.int64)
        np.savez(path, **arrays)
    other, sysdefs, velocities, objects = _run(seed=2)
    before = _tensors(sysdefs, velocities)
    with pytest.raises(ValueError):
        other.load(path)
    assert _same(_tensors(sysdefs, velocities), before)
    assert not any(isinstance(c, tuple) for obj in objects.values() for c in obj.calls)   # no load_state_dict was reached


def test_save_leaves_the_old_file_or_the_new_one(tmp_path, monkeypatch):
    from cavitymd import checkpoint
    path = tmp_path / "run.npz"
    first, *_ = _run(seed=1)
    first.save(path)
    old = open(path, "rb").read()
    second, *_ = _run(seed=2)

    def dies_half_way(file, arrays):
        file.write(b"PK half a file")
        raise OSError("disk full")

    monkeypatch.setattr(checkpoint, "_write_npz", dies_half_way)
    with pytest.raises(OSError, match="disk full"):
        second.save(path)
    assert sorted(os.listdir(tmp_path)) == ["run.npz"] and open(path, "rb").read() == old
    monkeypatch.undo()
    second.save(path)
    assert sorted(os.listdir(tmp_path)) == ["run.npz"] and open(path, "rb").read() != old
    third, sysdefs, velocities, _ = _run(seed=3)
    third.load(path)
    assert _same(_tensors(sysdefs, velocities), _tensors(*_run(seed=2)[1:3]))
