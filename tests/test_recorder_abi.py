"""What is specific to the recorder (cavmd_recorder_*) on a machine WITHOUT a GPU: the equivalences the header states, the
per-item validation and the refusals of create's scalar arguments (host arithmetic).  Header, exports, layouts, null
arguments, launch order, Python surface and deferred destroy are the shared checks of tests/batch_objects.py, called here with
this object's row."""
import ctypes

import batch_objects as checks
from abi_support import HEADER
from abi_support import good_recorder as _good

ROW = checks.ROWS["recorder"]


# ---- 1. the header ------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_keeps_the_version():
    checks.header_declares_exactly_the_entry_points(ROW)
    # the equivalences and their condition are stated where a C caller reads them
    raw = open(HEADER).read()
    start = raw.index("per-step observables of a batch, recorded on the device")
    section = " ".join(raw[start:raw.index("cavmd_recorder_device_ptr(")].replace("*", " ").split())
    assert "at least 64 compute units" in section and "2 ulp" in section and "bit for bit" in section
    for name in ("CavityModeTracker", "EnergyTracker", "DipoleAutocorrelation", "AdaptiveTimestepUpdater"):
        assert name in raw[:raw.index("#ifndef CAVMD_H_")], name      # the reference-interface table at the top


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    assert lib.cavmd_recorder_item_check(None) == INV
    assert capi.recorder_item_check(_good(capi)) == 0
    assert capi.recorder_item_check(_good(capi, 0, 0)) == 0 and capi.recorder_item_check(_good(capi, 65536, 65536)) == 0
    # only the result block is required
    assert capi.recorder_item_check(capi.recorder_item(0x10000, 0, 0, 0, 501, 501)) == 0
    assert capi.recorder_item_check(capi.recorder_item(0, 0x20000, 0x30000, 0x40000, 501, 501)) == INV
    # alignments: 16 / 16 / 16 / 4 bytes
    for field in range(3):
        for off, status in ((8, INV), (4, INV), (1, INV), (16, 0)):
            ptrs = [0x10000, 0x20000, 0x30000, 0x40000]
            ptrs[field] += off
            assert capi.recorder_item_check(capi.recorder_item(*ptrs, 501, 501)) == status, (field, off)
    for off, status in ((1, INV), (2, INV), (4, 0)):
        assert capi.recorder_item_check(capi.recorder_item(0x10000, 0x20000, 0x30000, 0x40000 + off, 501, 501)) == status, off
    # sizes
    assert capi.recorder_item_check(_good(capi, 65537, 1)) == CAP
    assert capi.recorder_item_check(_good(capi, 1, 65537)) == CAP
    assert capi.recorder_item_check(_good(capi, 2**32 - 1, 2**32 - 1)) == CAP
    # reserved words
    for k in range(3):
        it = _good(capi)
        it.reserved[k] = 1 << (9 * k)
        assert capi.recorder_item_check(it) == INV, k


def test_create_refuses_its_scalar_arguments_before_it_touches_a_device(capi):
    """create validates everything it is given before it looks into the workspace, so its refusals can be checked with a
    workspace handle that is never dereferenced (a zeroed buffer; every call below must be refused)."""
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    fake_ws = ctypes.create_string_buffer(1 << 16)
    ws = ctypes.cast(fake_ws, ctypes.c_void_p)
    it = _good(capi)
    kB = 3.167e-6

    def create(n_items, items, capacity, period, kB_):
        out = ctypes.c_void_p(123)
        st = lib.cavmd_recorder_create(ws, n_items, items, capacity, period, kB_, ctypes.byref(out))
        assert not out.value
        return st

    one = ctypes.byref(it)
    assert create(0, one, 8, 1, kB) == INV
    assert create(capi.BATCH_MAX_ITEMS + 1, one, 8, 1, kB) == INV
    assert create(1, None, 8, 1, kB) == INV
    assert create(1, one, 0, 1, kB) == INV
    assert create(1, one, 8, 0, kB) == INV
    for bad in (0.0, -0.0, -3.167e-6, float("nan"), float("inf"), float("-inf")):
        assert create(1, one, 8, 1, bad) == INV, bad
    # the series may take 1 GiB at the most: 2^23 records in all
    assert create(1, one, (1 << 23) + 1, 1, kB) == CAP
    two = (capi.RecorderItem * 2)(_good(capi), _good(capi))
    assert create(2, two, (1 << 22) + 1, 1, kB) == CAP
    assert create(1, one, 2**63, 1, kB) == CAP
    # a refused row is reported with its own status
    bad_row = (capi.RecorderItem * 2)(_good(capi), _good(capi, 65537, 1))
    assert create(2, bad_row, 8, 1, kB) == CAP
    bad_row[1] = capi.recorder_item(0, 0, 0, 0, 1, 1)
    assert create(2, bad_row, 8, 1, kB) == INV


# ---- the checks every batch object gets (tests/batch_objects.py), on this object's row ---------------------------------------
def test_libraries_export_them_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)


def test_a_c99_caller_compiles_links_and_runs(capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)


def test_launch_order_is_a_stable_descending_sort(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
