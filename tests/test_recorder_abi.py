"""The recorder (cavmd_recorder_*) on a machine WITHOUT a GPU: the header declares and both libraries export the nine entry
points and nothing stray, the record and item layouts agree between C and ctypes, a C99 caller compiles against the header,
the per-item validation and the refusals of create's scalar arguments work without a device, the launch order is a stable
descending sort, the deferred-destroy order takes recorders before workspaces, and the Python class refuses CPU tensors."""
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
RECORDER = ("cavmd_recorder_item_check", "cavmd_recorder_create", "cavmd_recorder_destroy", "cavmd_recorder_set_items",
            "cavmd_recorder_record", "cavmd_recorder_rows", "cavmd_recorder_read", "cavmd_recorder_reset",
            "cavmd_recorder_device_ptr")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- 1. header, libraries, binary -------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_keeps_the_version():
    text = _header_text()
    declared = sorted(set(re.findall(r"CAVMD_API\s+[\w\s\*]+?\b(cavmd_recorder_\w+)\s*\(", text)))
    assert declared == sorted(RECORDER)
    assert re.search(r"#define\s+CAVMD_VERSION_MINOR\s+2\b", text)
    assert "typedef struct cavmd_recorder cavmd_recorder;" in text
    # the equivalences and their condition are stated where a C caller reads them
    raw = open(HEADER).read()
    start = raw.index("per-step observables of a batch, recorded on the device")
    section = " ".join(raw[start:raw.index("cavmd_recorder_device_ptr(")].replace("*", " ").split())
    assert "at least 64 compute units" in section and "2 ulp" in section and "bit for bit" in section
    for name in ("CavityModeTracker", "EnergyTracker", "DipoleAutocorrelation", "AdaptiveTimestepUpdater"):
        assert name in raw[:raw.index("#ifndef CAVMD_H_")], name      # the reference-interface table at the top


def test_libraries_export_them_and_nothing_stray(capi):
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in RECORDER:
            assert hasattr(lib, name), (path, name)
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("cavmd_recorder")} == set(RECORDER), path
        assert not {s for s in exported if not s.startswith("cavmd_") and not s.startswith("_")}, path
        assert {s for s in exported if s.startswith("cavmd_")} == set(capi.EXPORTED_SYMBOLS), path
    assert capi.load().cavmd_version() == 2
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"recorder_batch_kernel" in blob and b"gfx950" in blob


# ---- 2. layouts ---------------------------------------------------------------------------------------------------------
def test_layouts_match_the_ctypes_structures(capi):
    R, I = capi.Record, capi.RecorderItem
    assert ctypes.sizeof(R) == 128 and ctypes.sizeof(I) == 64
    assert (R.call.offset, R.eval_sequence.offset, R.energy.offset, R.total_dipole.offset, R.q.offset, R.cavity_kinetic.offset,
            R.cavity_temperature.offset, R.kinetic_energy.offset, R.force_mass_sum.offset, R.reserved.offset) \
        == (0, 8, 16, 40, 64, 88, 96, 104, 112, 120)
    assert (I.d_result.offset, I.d_vel.offset, I.d_net_force.offset, I.d_members.offset, I.N.offset, I.n_members.offset,
            I.reserved.offset) == (0, 8, 16, 24, 32, 36, 40)
    dt = capi.record_dtype()
    assert dt.itemsize == 128
    for name, _ in R._fields_:
        assert dt.fields[name][1] == getattr(R, name).offset, name


def test_a_c99_caller_compiles_links_and_runs(capi, tmp_path):
    """tests/c_abi/recorder_abi_check.c: the same offsets seen from C, the refusals, null handles."""
    src = os.path.join(ROOT, "tests", "c_abi", "recorder_abi_check.c")
    exe = str(tmp_path / "recorder_abi_check")
    libdir = os.path.dirname(capi.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                         "-o", exe, "-L", libdir, "-lcavmd", "-lm", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "RECORDER-ABI-OK" in out.stdout, (out.returncode, out.stdout, out.stderr[-2000:])
    if not torch.cuda.is_available():
        assert "no device: no workspace, hence no recorder" in out.stdout


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def _good(capi, N=501, n_members=501):
    return capi.recorder_item(0x10000, 0x20000, 0x30000, 0x40000, N, n_members)


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


def test_null_handles_are_refused_without_a_device(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    it = _good(capi)
    out = ctypes.c_void_p(123)
    rows = ctypes.c_uint64()
    rec = capi.Record()
    assert lib.cavmd_recorder_create(None, 1, ctypes.byref(it), 8, 1, 3.167e-6, ctypes.byref(out)) == INV and not out.value
    assert lib.cavmd_recorder_create(None, 1, ctypes.byref(it), 8, 1, 3.167e-6, None) == INV
    assert lib.cavmd_recorder_destroy(None) == 0
    assert lib.cavmd_recorder_set_items(None, 0, 1, ctypes.byref(it)) == INV
    assert lib.cavmd_recorder_record(None, None) == INV
    assert lib.cavmd_recorder_rows(None, None, ctypes.byref(rows)) == INV
    assert lib.cavmd_recorder_read(None, None, 0, 1, 0, 1, ctypes.byref(rec)) == INV
    assert lib.cavmd_recorder_reset(None, None) == INV
    assert lib.cavmd_recorder_device_ptr(None, ctypes.byref(out), ctypes.byref(out)) == INV


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_workspace_no_recorder(capi):
    with pytest.raises(capi.CavmdError) as e:
        capi.Workspace(1)
    assert e.value.status == capi.CAVMD_ERR_NO_DEVICE


# ---- 4. launch order, the Python surface -------------------------------------------------------------------------------
def test_launch_order_is_a_stable_descending_sort(capi):
    rng = random.Random(12)
    for _ in range(50):
        sizes = [rng.choice([0, 1, 64, 501, 501, 501, 1024, 4097, 65536]) for _ in range(rng.randrange(1, 200))]
        want = sorted(range(len(sizes)), key=lambda i: -sizes[i])
        r = object.__new__(capi.Recorder)
        r.sizes = sizes
        assert r.launch_order == want
    for name in ("record", "rows", "read", "reset", "set_items", "device_ptr", "close"):
        assert callable(getattr(capi.Recorder, name)), name


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    import cavitymd
    assert "BatchRecorder" in cavitymd.__all__ and cavitymd.BatchRecorder is cavitymd.recorder.BatchRecorder
    for name in ("record", "rows", "read", "reset", "close"):
        assert callable(getattr(cavitymd.BatchRecorder, name)), name

    class NoBatch:   # never reached: CPU tensors are refused first
        def __len__(self):
            return 1

    vel = torch.zeros((10, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.BatchRecorder(NoBatch(), [vel])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.BatchRecorder(NoBatch(), [None], net_forces=[vel])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.BatchRecorder(NoBatch(), [np.zeros((10, 4))])


def test_deferred_destroy_takes_recorders_before_workspaces(capi, monkeypatch):
    order = []

    class Lib:
        def cavmd_destroy(self, h):
            order.append(("ws", h.value))
            return 0

        def cavmd_recorder_destroy(self, h):
            order.append(("recorder", h.value))
            return 0

    ws = object.__new__(capi.Workspace)
    ws._lib, ws._h = Lib(), ctypes.c_void_p(0x10)
    r = object.__new__(capi.Recorder)
    r._lib, r._h, r._ws = ws._lib, ctypes.c_void_p(0x20), ws
    monkeypatch.setattr(capi, "_capturing", lambda: True)
    ws.close()
    r.close()
    assert order == [] and not r._h.value and not ws._h.value
    monkeypatch.setattr(capi, "_capturing", lambda: False)
    capi._destroy_deferred()
    assert order == [("recorder", 0x20), ("ws", 0x10)]
    assert not capi._deferred and not capi._deferred_children
