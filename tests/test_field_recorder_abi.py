"""The field recorder (cavmd_field_recorder_*) on a machine WITHOUT a GPU: the header declares and both libraries export the
ten entry points, the record and item layouts agree between the header as a C compiler reads it, ctypes and numpy, the
per-item validation and the refusals of create's scalar arguments work without a device, nothing can be created without one,
and the Python class refuses CPU tensors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "cavmd.h")
FIELD = ("cavmd_field_recorder_item_check", "cavmd_field_recorder_create", "cavmd_field_recorder_destroy",
         "cavmd_field_recorder_set_items", "cavmd_field_recorder_record", "cavmd_field_recorder_rows",
         "cavmd_field_recorder_read", "cavmd_field_recorder_read_fields", "cavmd_field_recorder_reset",
         "cavmd_field_recorder_device_ptr")


def test_header_declares_the_entry_points_and_states_the_contract():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"CAVMD_API\s+[\w\s\*]+?\b(cavmd_field_recorder_\w+)\s*\(", text)))
    assert declared == sorted(FIELD)
    assert re.search(r"#define\s+CAVMD_FIELD_MAX_WAVEVECTORS\s+256\b", text)
    assert re.search(r"#define\s+CAVMD_FIELD_MAX_REFERENCES\s+16\b", text)
    assert "typedef struct cavmd_field_recorder cavmd_field_recorder;" in text
    start = raw.index("density field and F(k,t) of a batch, recorded on the device")
    section = " ".join(raw[start:raw.index("cavmd_field_recorder_device_ptr(")].replace("*", " ").split())
    for phrase in ("analysis.py:260-418", ":380-414", "bit for bit", "no FMA", "AFTER step 2", "depends on (N, n_k) ONLY",
                   "1e-13", "reference_interval_ps"):
        assert phrase in section, phrase
    assert "FieldAutocorrelationTracker" in raw[:raw.index("#ifndef CAVMD_H_")]   # the reference-interface table at the top


def test_libraries_export_them_and_carry_the_kernel(capi):
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in FIELD:
            assert hasattr(lib, name), (path, name)
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("cavmd_field_recorder")} == set(FIELD), path
    assert set(FIELD) <= set(capi.EXPORTED_SYMBOLS)
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"field_recorder_batch_kernel" in blob and b"gfx950" in blob


def test_layouts_match_between_c_ctypes_and_numpy(capi, tmp_path):
    """tests/c_abi/field_recorder_abi_check.c prints sizes and offsets as a C99 compiler sees the header."""
    src = os.path.join(ROOT, "tests", "c_abi", "field_recorder_abi_check.c")
    exe = str(tmp_path / "field_recorder_abi_check")
    libdir = os.path.dirname(capi.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                         "-o", exe, "-L", libdir, "-lcavmd", "-lm", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FIELD-RECORDER-ABI-OK" in out.stdout, (out.returncode, out.stdout, out.stderr[-2000:])
    if not torch.cuda.is_available():
        assert "no device: no workspace, hence no field recorder" in out.stdout
    lines = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.stdout.splitlines() if l.split()[0] in
             ("record", "item", "limits")}
    R, I = capi.FieldRecord, capi.FieldItem
    assert lines["record"] == [160, 0, 8, 12, 16, 24, 32]
    assert lines["record"] == [ctypes.sizeof(R), R.call.offset, R.n_references.offset, R.took_reference.offset, R.rho2.offset,
                               R.reserved.offset, R.F.offset]
    assert lines["item"] == [64, 0, 8, 16, 20, 24]
    assert lines["item"] == [ctypes.sizeof(I), I.d_position.offset, I.position_stride.offset, I.N.offset, I.reserved0.offset,
                             I.reserved.offset]
    assert lines["limits"] == [capi.FIELD_MAX_WAVEVECTORS, capi.FIELD_MAX_REFERENCES] == [256, 16]
    dt = capi.field_record_dtype()
    assert dt.itemsize == 160 and dt["F"].shape == (16,)
    for name, _ in R._fields_:
        assert dt.fields[name][1] == getattr(R, name).offset, name


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


def test_null_handles_are_refused_without_a_device(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    it = capi.field_item(0x10000, 24, 501)
    kv = np.zeros((1, 3))
    out = ctypes.c_void_p(123)
    rows, n = ctypes.c_uint64(), ctypes.c_uint32()
    rec = capi.FieldRecord()
    args = (1, ctypes.byref(it), 1, ctypes.c_void_p(kv.ctypes.data), 8, 1, 1, 0)
    assert lib.cavmd_field_recorder_create(None, *args, ctypes.byref(out)) == INV and not out.value
    assert lib.cavmd_field_recorder_create(None, *args, None) == INV
    assert lib.cavmd_field_recorder_destroy(None) == 0
    assert lib.cavmd_field_recorder_set_items(None, 0, 1, ctypes.byref(it)) == INV
    assert lib.cavmd_field_recorder_record(None, None, None) == INV
    assert lib.cavmd_field_recorder_rows(None, None, ctypes.byref(rows)) == INV
    assert lib.cavmd_field_recorder_read(None, None, 0, 1, 0, 1, ctypes.byref(rec)) == INV
    assert lib.cavmd_field_recorder_read_fields(None, None, 0, None, None, None, ctypes.byref(n)) == INV
    assert lib.cavmd_field_recorder_reset(None, None) == INV
    assert lib.cavmd_field_recorder_device_ptr(None, ctypes.byref(out), ctypes.byref(out)) == INV


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_workspace_no_field_recorder(capi):
    with pytest.raises(capi.CavmdError) as e:
        capi.Workspace(1)
    assert e.value.status == capi.CAVMD_ERR_NO_DEVICE


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    import cavitymd
    assert "BatchFieldRecorder" in cavitymd.__all__
    assert cavitymd.BatchFieldRecorder is cavitymd.field_recorder.BatchFieldRecorder
    for name in ("record", "rows", "read", "fields", "reset", "close"):
        assert callable(getattr(cavitymd.BatchFieldRecorder, name)), name
    for name in ("record", "rows", "read", "read_fields", "reset", "set_items", "device_ptr", "close"):
        assert callable(getattr(capi.FieldRecorder, name)), name
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.BatchFieldRecorder([torch.zeros((10, 3), dtype=torch.float64)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.BatchFieldRecorder([np.zeros((10, 4))])


def test_deferred_destroy_takes_field_recorders_before_workspaces(capi, monkeypatch):
    order = []

    class Lib:
        def cavmd_destroy(self, h):
            order.append(("ws", h.value))
            return 0

        def cavmd_field_recorder_destroy(self, h):
            order.append(("field_recorder", h.value))
            return 0

    ws = object.__new__(capi.Workspace)
    ws._lib, ws._h = Lib(), ctypes.c_void_p(0x10)
    r = object.__new__(capi.FieldRecorder)
    r._lib, r._h, r._ws = ws._lib, ctypes.c_void_p(0x20), ws
    monkeypatch.setattr(capi, "_capturing", lambda: True)
    ws.close()
    r.close()
    assert order == [] and not r._h.value and not ws._h.value
    monkeypatch.setattr(capi, "_capturing", lambda: False)
    capi._destroy_deferred()
    assert order == [("field_recorder", 0x20), ("ws", 0x10)]
    assert not capi._deferred and not capi._deferred_children
