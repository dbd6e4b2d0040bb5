"""What is specific to the batch of independent small systems (cavmd_batch_*) on a machine WITHOUT a GPU: the limits the header
states, the per-item validation of cavmd_batch_create (cavmd_batch_item_check is host arithmetic), the pybind11 module's view
of the batch, and the batch history bookkeeping against a fake batch object.  Header, exports, layouts, null arguments, launch
order, Python surface and deferred destroy are the shared checks of tests/batch_objects.py, called here with this object's
row."""
import re

import numpy as np
import pytest
import torch

import batch_objects as checks
from abi_support import good_batch as _good
from abi_support import header_text

ROW = checks.ROWS["batch"]


def test_header_declares_the_ten_entry_points_and_keeps_the_version(capi):
    checks.header_declares_exactly_the_entry_points(ROW)
    text = header_text()
    assert re.search(r"#define\s+CAVMD_BATCH_MAX_ITEMS\s+65536\b", text)
    assert re.search(r"#define\s+CAVMD_BATCH_MAX_ITEM_N\s+65536\b", text)
    assert capi.BATCH_MAX_ITEMS == 65536 and capi.BATCH_MAX_ITEM_N == 65536


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


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_batch_no_fallback(capi):
    """the pybind11 class; capi.Workspace and cavitymd.CavityForceBatch are checks f and h of tests/test_batch_objects_abi.py"""
    from cavitymd import _cavitymd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _cavitymd.Batch([(0x1000, 0x2000, 0x3000, 0x4000, 1.0, 1.0, 1.0, 0.0091, 1e-3, 1.0, 10, 2)])


def test_pybind_module_and_package_expose_the_batch(capi):
    from cavitymd import _cavitymd, replicas
    for name in ("compute", "lastSequence", "results", "resultsAt", "energiesAt", "setItems", "resultsDevicePtr"):
        assert hasattr(_cavitymd.Batch, name), name
    good = (0x1000, 0x2000, 0x3000, 0x4000, 1.0, 1.0, 1.0, 0.0091, 1e-3, 1.0, 10, 2)
    assert _cavitymd.batch_item_check(good) == 0
    assert _cavitymd.batch_item_check((0x1008,) + good[1:]) == capi.CAVMD_ERR_INVALID_VALUE
    assert _cavitymd.batch_item_check(good[:10] + (70000, 2)) == capi.CAVMD_ERR_CAPACITY
    assert callable(replicas.local_batch)


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


# ---- the checks every batch object gets (tests/batch_objects.py), on this object's row ---------------------------------------
def test_library_exports_them_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)


def test_a_c99_caller_compiles_links_and_runs(capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)


def test_launch_order_is_a_stable_descending_sort(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)
