"""What is specific to the field recorder (cavmd_field_recorder_*) on a machine WITHOUT a GPU: the contract and the limits the
header states, the per-item validation and the refusals of create's scalar arguments (host arithmetic).  Header, exports,
layouts, null arguments, launch order, Python surface and deferred destroy are the shared checks of tests/batch_objects.py,
called here with this object's row."""
import ctypes
import re

import numpy as np

import batch_objects as checks
from abi_support import HEADER, header_text

ROW = checks.ROWS["field_recorder"]


def test_header_declares_the_entry_points_and_states_the_contract():
    checks.header_declares_exactly_the_entry_points(ROW)
    raw, text = open(HEADER).read(), header_text()
    assert re.search(r"#define\s+CAVMD_FIELD_MAX_WAVEVECTORS\s+256\b", text)
    assert re.search(r"#define\s+CAVMD_FIELD_MAX_REFERENCES\s+16\b", text)
    start = raw.index("density field and F(k,t) of a batch, recorded on the device")
    section = " ".join(raw[start:raw.index("cavmd_field_recorder_device_ptr(")].replace("*", " ").split())
    for phrase in ("analysis.py:260-418", ":380-414", "bit for bit", "no FMA", "AFTER step 2", "depends on (N, n_k) ONLY",
                   "1e-13", "reference_interval_ps"):
        assert phrase in section, phrase
    assert "FieldAutocorrelationTracker" in raw[:raw.index("#ifndef CAVMD_H_")]   # the reference-interface table at the top


def test_layouts_match_between_c_ctypes_and_numpy(capi, tmp_path):
    """... and the limits as a C99 compiler sees them (tests/c_abi/field_recorder_abi_check.c) are the ones Python restates"""
    stdout = checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)
    limits = re.search(r"^limits (\d+) (\d+)$", stdout, flags=re.M)
    assert [int(x) for x in limits.groups()] == [capi.FIELD_MAX_WAVEVECTORS, capi.FIELD_MAX_REFERENCES] == [256, 16]


def test_item_check_verdicts(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    check = capi.field_item_check
    assert lib.cavmd_field_recorder_item_check(None) == INV
    assert check(capi.field_item(0x10000, 24, 501)) == 0 and check(capi.field_item(0x10000, 32, 501)) == 0
    assert check(capi.field_item(0x10000, 40, 65536)) == 0 and check(capi.field_item(0x10000, 1 << 20, 1)) == 0
    assert check(capi.field_item(0, 24, 0)) == 0                    # N = 0 with a null pointer is legal
    assert check(capi.field_item(0, 24, 1)) == INV                  # null with particles
    for off, status in ((1, INV), (2, INV), (4, INV), (8, 0), (24, 0)):
        assert check(capi.field_item(0x10000 + off, 24, 501)) == status, off
    for stride in (0, 8, 16, 23, 28, 25, 36, 2**63 + 4):
        assert check(capi.field_item(0x10000, stride, 501)) == INV, stride
    assert check(capi.field_item(0x10000, 24, 65537)) == CAP and check(capi.field_item(0x10000, 24, 2**32 - 1)) == CAP
    it = capi.field_item(0x10000, 24, 501)
    it.reserved0 = 1
    assert check(it) == INV
    for k in range(5):
        it = capi.field_item(0x10000, 24, 501)
        it.reserved[k] = 1 << (7 * k)
        assert check(it) == INV, k


def test_create_refuses_its_scalar_arguments_before_it_touches_a_device(capi):
    """create validates everything it is given before it looks into the workspace, so its refusals can be checked with a
    workspace handle that is never dereferenced (a zeroed buffer; every call below must be refused)."""
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    fake_ws = ctypes.create_string_buffer(1 << 16)
    ws = ctypes.cast(fake_ws, ctypes.c_void_p)
    it = capi.field_item(0x10000, 24, 501)
    kv = np.ascontiguousarray(np.random.default_rng(1).normal(size=(256, 3)))
    kp = ctypes.c_void_p(kv.ctypes.data)

    def create(n_items, items, n_k, k, capacity, period, max_refs, interval=0):
        out = ctypes.c_void_p(123)
        st = lib.cavmd_field_recorder_create(ws, n_items, items, n_k, k, capacity, period, max_refs, interval, ctypes.byref(out))
        assert not out.value
        return st

    one = ctypes.byref(it)
    assert create(0, one, 50, kp, 8, 1, 1) == INV
    assert create(capi.BATCH_MAX_ITEMS + 1, one, 50, kp, 8, 1, 1) == INV
    assert create(1, None, 50, kp, 8, 1, 1) == INV
    assert create(1, one, 50, None, 8, 1, 1) == INV
    assert create(1, one, 0, kp, 8, 1, 1) == INV and create(1, one, 257, kp, 8, 1, 1) == INV
    assert create(1, one, 50, kp, 0, 1, 1) == INV and create(1, one, 50, kp, 8, 0, 1) == INV
    assert create(1, one, 50, kp, 8, 1, 0) == INV and create(1, one, 50, kp, 8, 1, 17) == INV
    bad = kv.copy()
    bad[49, 2] = np.nan
    assert create(1, one, 50, ctypes.c_void_p(bad.ctypes.data), 8, 1, 1) == INV
    bad[49, 2] = np.inf
    assert create(1, one, 50, ctypes.c_void_p(bad.ctypes.data), 8, 1, 1) == INV
    # series + fields may take 1 GiB at the most: 160 B a row, 16 n_k (max_references + 1) B of fields per item
    assert create(1, one, 50, kp, (1 << 30) // 160 + 1, 1, 1) == CAP
    assert create(1, one, 256, kp, ((1 << 30) - 17 * 4096) // 160 + 1, 1, 16) == CAP
    assert create(1, one, 50, kp, 2**63, 1, 1) == CAP
    many = (capi.FieldItem * 65536)(*([it] * 65536))
    assert create(65536, many, 256, kp, 1, 1, 16) == CAP            # 65536 x 17 x 4 KiB of fields alone
    bad_row = (capi.FieldItem * 2)(it, capi.field_item(0x10000, 24, 65537))
    assert create(2, bad_row, 50, kp, 8, 1, 1) == CAP
    bad_row[1] = capi.field_item(0x10000, 28, 5)
    assert create(2, bad_row, 50, kp, 8, 1, 1) == INV


# ---- the checks every batch object gets (tests/batch_objects.py), on this object's row ---------------------------------------
def test_libraries_export_them_and_carry_the_kernel(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
