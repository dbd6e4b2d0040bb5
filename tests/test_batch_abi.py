"""The batch of independent small systems (cavmd_batch_*) on a machine WITHOUT a GPU: the header declares and the library
exports the ten entry points and nothing stray, the item layout agrees between C and ctypes, a C99 caller compiles against
the extended header, the per-item validation of cavmd_batch_create works without a device (cavmd_batch_item_check), the
launch order is a stable descending sort, and the batch history bookkeeping holds against a fake batch object."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "cavmd.h")
BATCH = ("cavmd_batch_item_check", "cavmd_batch_create", "cavmd_batch_destroy", "cavmd_batch_set_items",
         "cavmd_batch_compute", "cavmd_batch_last_sequence", "cavmd_batch_results_read", "cavmd_batch_results_at",
         "cavmd_batch_energies_at", "cavmd_batch_results_device_ptr")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_ten_entry_points_and_keeps_the_version():
    text = _header_text()
    declared = sorted(set(re.findall(r"CAVMD_API\s+[\w\s\*]+?\b(cavmd_batch_\w+)\s*\(", text)))
    assert declared == sorted(BATCH)
    assert re.search(r"#define\s+CAVMD_VERSION_MINOR\s+2\b", text)
    assert re.search(r"#define\s+CAVMD_BATCH_MAX_ITEMS\s+65536\b", text)
    assert re.search(r"#define\s+CAVMD_BATCH_MAX_ITEM_N\s+65536\b", text)
    assert "typedef struct cavmd_batch cavmd_batch;" in text


def test_library_exports_them_and_nothing_stray(capi):
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in BATCH:
            assert hasattr(lib, name), (path, name)
    for name in BATCH:
        assert name in capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("cavmd_batch")} == set(BATCH)
    assert {s for s in exported if s.startswith("cavmd_")} == set(capi.EXPORTED_SYMBOLS)
    assert not {s for s in exported if not s.startswith("cavmd_") and not s.startswith("_")}
    assert capi.load().cavmd_version() == 2
    assert b"cavity_batch_kernel" in open(capi.LIB_PATH, "rb").read()


def test_item_layout_matches_the_ctypes_structure(capi):
    B = capi.BatchItem
    assert ctypes.sizeof(B) == 128
    assert (B.d_pos.offset, B.d_charge.offset, B.d_image.offset, B.d_force.offset) == (0, 8, 16, 24)
    assert (B.Lx.offset, B.Ly.offset, B.Lz.offset) == (32, 40, 48)
    assert B.params.offset == 56 and ctypes.sizeof(capi.Params) == 32
    assert (B.N.offset, B.L_typeid.offset, B.reserved.offset) == (88, 92, 96)
    assert capi.BATCH_MAX_ITEMS == 65536 and capi.BATCH_MAX_ITEM_N == 65536


def test_a_c99_caller_compiles_links_and_runs(capi, tmp_path):
    """tests/c_abi/batch_abi_check.c: the same offsets seen from C, the refusals of cavmd_batch_item_check, null handles."""
    src = os.path.join(ROOT, "tests", "c_abi", "batch_abi_check.c")
    exe = str(tmp_path / "batch_abi_check")
    libdir = os.path.dirname(capi.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                         "-o", exe, "-L", libdir, "-lcavmd", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "BATCH-ABI-OK" in out.stdout, (out.returncode, out.stdout, out.stderr[-2000:])
    if not torch.cuda.is_available():
        assert "no device: no workspace, hence no batch" in out.stdout


def _good(capi, n=501):
    return capi.batch_item(n, 0x10000, 0x20000, 0x30000, 0x40000, (40.0, 40.0, 40.0), 2, capi.make_params(0.0091, 1e-3, 1.0))


def test_item_check_refuses_what_compute_hoomd_refuses(capi):
    lib = capi.load()
    INV, CAP, BAD = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY, capi.CAVMD_ERR_BAD_PARAMS
    assert lib.cavmd_batch_item_check(None) == INV
    assert capi.batch_item_check(_good(capi)) == 0
    assert capi.batch_item_check(_good(capi, 1)) == 0 and capi.batch_item_check(_good(capi, 65536)) == 0
    # null arrays
    for field in ("d_pos", "d_charge", "d_image", "d_force"):
        it = _good(capi)
        setattr(it, field, None)
        assert capi.batch_item_check(it) == INV, field
    # alignments 16 / 8 / 4 / 16
    for field, off, ok_off in (("d_pos", 8, 16), ("d_force", 8, 16), ("d_charge", 4, 8), ("d_image", 2, 4)):
        it = _good(capi)
        base = getattr(it, field)
        setattr(it, field, base + off)
        assert capi.batch_item_check(it) == INV, field
        setattr(it, field, base + ok_off)
        assert capi.batch_item_check(it) == 0, field
    # size
    assert capi.batch_item_check(_good(capi, 65537)) == CAP
    assert capi.batch_item_check(_good(capi, 2**32 - 1)) == CAP
    # parameters
    for prm in (capi.Params(0.1, 0.1, 0.0, 1.0), capi.Params(float("nan"), 0.1, 1.0, 1.0), capi.Params(0.1, float("inf"), 1.0, 1.0),
                capi.Params(0.1, 0.1, float("inf"), 1.0), capi.Params(0.1, 0.1, 1.0, float("nan"))):
        it = _good(capi)
        it.params = prm
        assert capi.batch_item_check(it) == BAD
    # reserved words
    for k in range(4):
        it = _good(capi)
        it.reserved[k] = 1 << (7 * k)
        assert capi.batch_item_check(it) == INV, k


def test_an_empty_item_is_legal_and_may_leave_its_arrays_out(capi):
    it = capi.batch_item(0, 0, 0, 0, 0, (1.0, 1.0, 1.0), 2, capi.Params(0.0, 0.0, 0.0, 0.0))
    assert it.d_pos is None and it.d_force is None
    assert capi.batch_item_check(it) == 0
    it.reserved[0] = 5                                         # ... but not its reserved words
    assert capi.batch_item_check(it) == capi.CAVMD_ERR_INVALID_VALUE
    it = capi.batch_item(0, 0x10008, 0, 0, 0, (1.0, 1.0, 1.0), 2, capi.Params(0.0, 0.0, 0.0, 0.0))
    assert capi.batch_item_check(it) == capi.CAVMD_ERR_INVALID_VALUE       # an array that is given is aligned
    it = capi.batch_item(1, 0, 0, 0, 0, (1.0, 1.0, 1.0), 2, capi.make_params(0.1, 0.1, 1.0))
    assert capi.batch_item_check(it) == capi.CAVMD_ERR_INVALID_VALUE       # only N == 0 may


def test_null_handles_are_refused_without_a_device(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    it = _good(capi)
    out = ctypes.c_void_p(123)
    r = capi.Result()
    seq = ctypes.c_uint64()
    assert lib.cavmd_batch_create(None, 1, ctypes.byref(it), 4, ctypes.byref(out)) == INV and not out.value
    assert lib.cavmd_batch_create(None, 1, ctypes.byref(it), 4, None) == INV
    assert lib.cavmd_batch_destroy(None) == 0
    assert lib.cavmd_batch_set_items(None, 0, 1, ctypes.byref(it)) == INV
    assert lib.cavmd_batch_compute(None, None) == INV
    assert lib.cavmd_batch_last_sequence(None, ctypes.byref(seq)) == INV
    assert lib.cavmd_batch_results_read(None, ctypes.byref(r)) == INV
    assert lib.cavmd_batch_results_at(None, 1, ctypes.byref(r)) == INV
    assert lib.cavmd_batch_energies_at(None, 1, None) == INV
    assert lib.cavmd_batch_results_device_ptr(None, ctypes.byref(out)) == INV


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_batch_no_fallback(capi):
    import cavitymd
    from cavitymd import synthetic
    with pytest.raises(capi.CavmdError) as e:
        capi.Workspace(1)
    assert e.value.status == capi.CAVMD_ERR_NO_DEVICE
    cfg = synthetic.config1()
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                           cfg["box"], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.CavityForceBatch([cavitymd.SystemDefinition(pd)], cfg["params"])
    from cavitymd import _cavitymd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _cavitymd.Batch([(0x1000, 0x2000, 0x3000, 0x4000, 1.0, 1.0, 1.0, 0.0091, 1e-3, 1.0, 10, 2)])


def test_launch_order_is_a_stable_descending_sort(capi):
    rng = random.Random(5)
    for trial in range(50):
        sizes = [rng.choice([0, 1, 64, 501, 501, 501, 1024, 4096, 20001]) for _ in range(rng.randrange(1, 200))]
        want = sorted(range(len(sizes)), key=lambda i: -sizes[i])           # sorted() is stable: ties stay in item order
        assert capi.batch_launch_order(sizes) == want
    assert capi.batch_launch_order([5, 0, 7, 5, 7]) == [2, 4, 0, 3, 1]
    assert capi.batch_launch_order([501] * 8) == list(range(8))


def test_pybind_module_and_package_expose_the_batch(capi):
    import cavitymd
    from cavitymd import _cavitymd, replicas
    for name in ("compute", "lastSequence", "results", "resultsAt", "energiesAt", "setItems", "resultsDevicePtr"):
        assert hasattr(_cavitymd.Batch, name), name
    good = (0x1000, 0x2000, 0x3000, 0x4000, 1.0, 1.0, 1.0, 0.0091, 1e-3, 1.0, 10, 2)
    assert _cavitymd.batch_item_check(good) == 0
    assert _cavitymd.batch_item_check((0x1008,) + good[1:]) == capi.CAVMD_ERR_INVALID_VALUE
    assert _cavitymd.batch_item_check(good[:10] + (70000, 2)) == capi.CAVMD_ERR_CAPACITY
    for name in ("compute", "forces", "energies", "energies_at", "history", "refresh", "last_sequence"):
        assert hasattr(cavitymd.CavityForceBatch, name), name
    assert "CavityForceBatch" in cavitymd.__all__ and callable(replicas.local_batch)
    for name in ("compute", "last_sequence", "results", "results_at", "energies_at", "set_items", "close"):
        assert callable(getattr(capi.Batch, name)), name


def test_deferred_destroy_takes_batches_before_workspaces(capi, monkeypatch):
    order = []

    class Lib:
        def cavmd_destroy(self, h):
            order.append(("ws", h.value))
            return 0

        def cavmd_batch_destroy(self, h):
            order.append(("batch", h.value))
            return 0

    ws = object.__new__(capi.Workspace)
    ws._lib, ws._h = Lib(), ctypes.c_void_p(0x10)
    b = object.__new__(capi.Batch)
    b._lib, b._h, b._ws = ws._lib, ctypes.c_void_p(0x20), ws
    monkeypatch.setattr(capi, "_capturing", lambda: True)
    ws.close()
    b.close()
    assert order == [] and not b._h.value and not ws._h.value
    monkeypatch.setattr(capi, "_capturing", lambda: False)
    capi._destroy_deferred()
    assert order == [("batch", 0x20), ("ws", 0x10)]
    assert not capi._deferred and not capi._deferred_children


# ---- BatchEnergyHistory against a fake batch object ---------------------------------------------------------------------
class FakeBatch:
    """Sequences and (B, 3) energies as a batch would hand them out; `status` maps a sequence to the error its read gives."""

    def __init__(self, n_items=3):
        self.n_items = n_items
        self.seq = 0
        self.reads = []
        self.status = {}

    def compute(self):
        self.seq += 1

    def last_sequence(self):
        return self.seq

    def energies_at(self, sequence):
        from cavitymd._capi import CavmdError
        self.reads.append(sequence)
        if sequence in self.status:
            raise CavmdError(self.status[sequence], "fake", "cavmd_batch_energies_at")
        if sequence == 0:
            raise CavmdError(-5, "fake", "cavmd_batch_energies_at")
        assert 1 <= sequence <= self.seq
        return np.arange(self.n_items * 3, dtype=np.float64).reshape(self.n_items, 3) + 100.0 * sequence


def _rows_equal(got, want):
    assert [t for t, _ in got] == [t for t, _ in want]
    for (_, a), (_, b) in zip(got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _row(ts, seq, n_items=3):
    return (ts, np.arange(n_items * 3, dtype=np.float64).reshape(n_items, 3) + 100.0 * seq)


def test_batch_history_keeps_the_newest_and_reads_each_step_once():
    from cavitymd import BatchEnergyHistory
    b = FakeBatch()
    h = BatchEnergyHistory(b)
    assert h.drain() == [] and h.flush() == []
    rows = []
    for ts in range(100, 110):
        b.compute()
        h.record(ts)
        rows += h.drain()
        assert len(h) == 1                                     # the newest is kept back
    _rows_equal(rows, [_row(100 + k, k + 1) for k in range(9)])
    assert rows[0][1].shape == (3, 3)
    assert b.reads == list(range(1, 10))                       # oldest first, nothing read twice, the newest not yet
    _rows_equal(h.flush(), [_row(109, 10)])
    assert len(h) == 0 and h.flush() == [] and h.drain() == []
    assert b.reads == list(range(1, 11))


@pytest.mark.parametrize("status", [-7, 719], ids=["expired", "launch_failure"])
def test_batch_history_raises_once_for_a_step_it_cannot_read(status):
    from cavitymd import BatchEnergyHistory
    from cavitymd._capi import CavmdError
    b = FakeBatch()
    b.status[3] = status
    h = BatchEnergyHistory(b)
    for ts in range(6):
        b.compute()
        h.record(ts)
    with pytest.raises(CavmdError) as e:
        h.drain()
    assert e.value.status == status
    _rows_equal(h.drain(), [_row(0, 1), _row(1, 2), _row(3, 4), _row(4, 5)])
    _rows_equal(h.flush(), [_row(5, 6)])
    assert b.reads == [1, 2, 3, 4, 5, 6]


def test_batch_history_before_any_evaluation_reports_not_computed():
    from cavitymd import BatchEnergyHistory
    from cavitymd._capi import CavmdError
    b = FakeBatch()
    h = BatchEnergyHistory(b)
    h.record(0)
    with pytest.raises(CavmdError) as e:
        h.flush()
    assert e.value.status == -5 and len(h) == 0
