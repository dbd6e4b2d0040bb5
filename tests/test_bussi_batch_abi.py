"""The thermostat batch (cavmd_bussi_batch_*) on a machine WITHOUT a GPU: the header declares and both libraries export the
ten entry points and nothing stray, the item and input layouts agree between C and ctypes, a C99 caller compiles against the
header, the per-item validation and the input-row maker work without a device, the row maker's c is the c the reference's
executed C++ recorded (tests/golden/bussi_reference_golden.npz), the launch order is a stable descending sort, and the Python
class refuses CPU tensors."""
import ctypes
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "cavmd.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bussi_reference_golden.npz")
BUSSI_BATCH = ("cavmd_bussi_batch_item_check", "cavmd_bussi_batch_input_make", "cavmd_bussi_batch_create",
               "cavmd_bussi_batch_destroy", "cavmd_bussi_batch_set_items", "cavmd_bussi_batch_step",
               "cavmd_bussi_batch_last_sequence", "cavmd_bussi_batch_read", "cavmd_bussi_batch_reset",
               "cavmd_bussi_batch_state_device_ptr")


def _bits(x) -> int:
    return int(np.float64(x).view(np.uint64))


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- 1. header, libraries, binary -------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_keeps_the_version():
    text = _header_text()
    declared = sorted(set(re.findall(r"CAVMD_API\s+[\w\s\*]+?\b(cavmd_bussi_batch_\w+)\s*\(", text)))
    assert declared == sorted(BUSSI_BATCH)
    assert re.search(r"#define\s+CAVMD_VERSION_MINOR\s+2\b", text)
    assert "typedef struct cavmd_bussi_batch cavmd_bussi_batch;" in text
    # the equivalence and its condition are stated where a C caller reads them
    raw = open(HEADER).read()
    assert "at least 64 compute units" in raw and "2 ulp" in raw


def test_libraries_export_them_and_nothing_stray(capi):
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in BUSSI_BATCH:
            assert hasattr(lib, name), (path, name)
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("cavmd_bussi_batch")} == set(BUSSI_BATCH), path
        assert not {s for s in exported if not s.startswith("cavmd_") and not s.startswith("_")}, path
    for name in BUSSI_BATCH:
        assert name in capi.EXPORTED_SYMBOLS
    assert capi.load().cavmd_version() == 2
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"bussi_batch_kernel" in blob and b"gfx950" in blob


# ---- 2. layouts ---------------------------------------------------------------------------------------------------------
def test_layouts_match_the_ctypes_structures(capi):
    I, R = capi.BussiBatchItem, capi.BussiBatchInput
    assert ctypes.sizeof(I) == 64 and ctypes.sizeof(R) == 64 and ctypes.sizeof(capi.BussiDeviceState) == 48
    assert (I.d_vel.offset, I.d_members.offset, I.n_members.offset, I.reserved0.offset, I.dof_translational.offset,
            I.reserved.offset) == (0, 8, 16, 20, 24, 32)
    assert (R.normal_variate.offset, R.gamma_variate.offset, R.c.offset, R.set_T.offset, R.skip.offset,
            R.reserved.offset) == (0, 8, 16, 24, 32, 40)


def test_a_c99_caller_compiles_links_and_runs(capi, tmp_path):
    """tests/c_abi/bussi_batch_abi_check.c: the same offsets seen from C, the refusals, the row maker, null handles."""
    src = os.path.join(ROOT, "tests", "c_abi", "bussi_batch_abi_check.c")
    exe = str(tmp_path / "bussi_batch_abi_check")
    libdir = os.path.dirname(capi.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                         "-o", exe, "-L", libdir, "-lcavmd", "-lm", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "BUSSI-BATCH-ABI-OK" in out.stdout, (out.returncode, out.stdout, out.stderr[-2000:])
    if not torch.cuda.is_available():
        assert "no device: no workspace, hence no batch" in out.stdout


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def _good(capi, n=501, dof=1500.0):
    return capi.bussi_batch_item(0x10000, 0x20000, n, dof)


def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    assert lib.cavmd_bussi_batch_item_check(None) == INV
    assert capi.bussi_batch_item_check(_good(capi)) == 0
    assert capi.bussi_batch_item_check(_good(capi, 1)) == 0 and capi.bussi_batch_item_check(_good(capi, 65536)) == 0
    assert capi.bussi_batch_item_check(capi.bussi_batch_item(0x10000, 0, 501, 3.0)) == 0      # no member list: 0 .. n-1
    assert capi.bussi_batch_item_check(_good(capi, dof=0.0)) == 0
    # null / misaligned velocities, misaligned members
    assert capi.bussi_batch_item_check(capi.bussi_batch_item(0, 0x20000, 501, 3.0)) == INV
    for off, status in ((8, INV), (4, INV), (16, 0)):
        assert capi.bussi_batch_item_check(capi.bussi_batch_item(0x10000 + off, 0x20000, 501, 3.0)) == status, off
    for off, status in ((1, INV), (2, INV), (4, 0)):
        assert capi.bussi_batch_item_check(capi.bussi_batch_item(0x10000, 0x20000 + off, 501, 3.0)) == status, off
    # an empty item may leave its velocities out, but what it gives is aligned and its reserved words are 0
    assert capi.bussi_batch_item_check(capi.bussi_batch_item(0, 0, 0, 0.0)) == 0
    assert capi.bussi_batch_item_check(capi.bussi_batch_item(0x10008, 0, 0, 0.0)) == INV
    # size
    assert capi.bussi_batch_item_check(_good(capi, 65537)) == CAP
    assert capi.bussi_batch_item_check(_good(capi, 2**32 - 1)) == CAP
    # degrees of freedom
    for dof in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert capi.bussi_batch_item_check(_good(capi, dof=dof)) == INV, dof
    # reserved words
    it = _good(capi)
    it.reserved0 = 1
    assert capi.bussi_batch_item_check(it) == INV
    for k in range(4):
        it = _good(capi)
        it.reserved[k] = 1 << (9 * k)
        assert capi.bussi_batch_item_check(it) == INV, k
        it = capi.bussi_batch_item(0, 0, 0, 0.0)
        it.reserved[k] = 1
        assert capi.bussi_batch_item_check(it) == INV, k


def test_null_handles_are_refused_without_a_device(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    it = _good(capi)
    out = ctypes.c_void_p(123)
    st = capi.BussiDeviceState()
    seq = ctypes.c_uint64()
    assert lib.cavmd_bussi_batch_create(None, 1, ctypes.byref(it), ctypes.byref(out)) == INV and not out.value
    assert lib.cavmd_bussi_batch_create(None, 1, ctypes.byref(it), None) == INV
    assert lib.cavmd_bussi_batch_destroy(None) == 0
    assert lib.cavmd_bussi_batch_set_items(None, 0, 1, ctypes.byref(it)) == INV
    assert lib.cavmd_bussi_batch_step(None, None, ctypes.c_void_p(0x1000)) == INV
    assert lib.cavmd_bussi_batch_last_sequence(None, ctypes.byref(seq)) == INV
    assert lib.cavmd_bussi_batch_read(None, ctypes.byref(st)) == INV
    assert lib.cavmd_bussi_batch_reset(None, None) == INV
    assert lib.cavmd_bussi_batch_state_device_ptr(None, ctypes.byref(out)) == INV
    assert lib.cavmd_bussi_batch_input_make(0.1, 1.0, 1.0, 0.0, 0.0, None) == INV


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_workspace_no_batch(capi):
    with pytest.raises(capi.CavmdError) as e:
        capi.Workspace(1)
    assert e.value.status == capi.CAVMD_ERR_NO_DEVICE


# ---- 4. the input row ---------------------------------------------------------------------------------------------------
def test_input_make_sets_skip_iff_dt_is_zero_and_c_zero_for_tau_zero(capi):
    for dt in (0.0, -0.0):
        row = capi.bussi_batch_input_make(dt, 1.5, 0.5, 0.25, 3.0)
        assert row.skip != 0
    for dt in (5e-324, 1e-300, 0.005, 1.0, 1e300, -0.005):
        row = capi.bussi_batch_input_make(dt, 1.5, 0.5, 0.25, 3.0)
        assert row.skip == 0, dt
        assert _bits(row.c) == _bits(math.exp(-dt / 0.5))                 # the same libm call as cavmd_bussi_step_device
        assert (row.normal_variate, row.gamma_variate, row.set_T) == (0.25, 3.0, 1.5) and list(row.reserved) == [0, 0, 0]
        row = capi.bussi_batch_input_make(dt, 1.5, 0.0, 0.25, 3.0)
        assert _bits(row.c) == _bits(0.0) and row.skip == 0


def test_input_make_gives_the_c_the_executed_reference_recorded(capi):
    """Bit for bit on every recorded call where this machine's exp reproduces the recorded c (the c_agrees notion of
    tests/test_bussi_reference_golden.py: libm may differ from the fixture's build); at least 99 % of the calls must agree,
    and on ALL calls the row's c is this machine's exp(-dt / tau), the expression cavmd_bussi_step_device uses."""
    with np.load(GOLDEN) as z:
        cols = {name: i for i, name in enumerate(z["in_cols"].tolist())}
        ocol = {name: i for i, name in enumerate(z["out_cols"].tolist())}
        rows_in = np.concatenate([z["case_in"], z["seq_in"].reshape(-1, z["seq_in"].shape[-1])])
        rows_out = np.concatenate([z["case_out"], z["seq_out"].reshape(-1, z["seq_out"].shape[-1])])
    agree = []
    for rin, rout in zip(rows_in, rows_out):
        dt, tau, set_T = float(rin[cols["dt"]]), float(rin[cols["tau"]]), float(rin[cols["set_T"]])
        recorded = float(rout[ocol["c"]]) if "c" in ocol else float(rin[cols["c"]])
        row = capi.bussi_batch_input_make(dt, set_T, tau, 0.5, 1.0)
        here = math.exp(-dt / tau) if tau != 0.0 else 0.0
        assert _bits(row.c) == _bits(here)
        assert (row.skip != 0) == (dt == 0.0)
        if rout[ocol["throws"]] != 0.0 or dt == 0.0:
            continue
        agree.append(_bits(here) == _bits(recorded))
        if agree[-1]:
            assert _bits(row.c) == _bits(recorded)
    assert len(agree) > 2000 and sum(agree) >= 0.99 * len(agree)


# ---- 5. launch order, the Python surface -------------------------------------------------------------------------------
def test_launch_order_is_a_stable_descending_sort(capi):
    rng = random.Random(11)
    for _ in range(50):
        sizes = [rng.choice([0, 1, 64, 501, 501, 501, 1024, 4097, 65536]) for _ in range(rng.randrange(1, 200))]
        want = sorted(range(len(sizes)), key=lambda i: -sizes[i])
        assert capi.batch_launch_order(sizes) == want
        b = object.__new__(capi.BussiBatch)
        b.sizes = sizes
        assert b.launch_order == want
    for name in ("step", "read", "reset", "set_items", "last_sequence", "state_device_ptr", "close"):
        assert callable(getattr(capi.BussiBatch, name)), name


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    import cavitymd
    assert "BussiReservoirBatch" in cavitymd.__all__
    for name in ("attach", "set_inputs", "draw_inputs", "step_async", "device_state", "reset_reservoir_energy",
                 "reservoir_energy_translational", "reservoir_energy_rotational", "total_reservoir_energy",
                 "instantaneous_reservoir_translational", "instantaneous_reservoir_rotational",
                 "instantaneous_reservoir_total"):
        assert hasattr(cavitymd.BussiReservoirBatch, name), name
    t = cavitymd.BussiReservoirBatch(kT=1.0, tau=0.5)
    vel = torch.zeros((10, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.attach([vel], 27.0)
    with pytest.raises(RuntimeError, match="before attach"):
        t.step_async()
    with pytest.raises(ValueError):
        cavitymd.BussiReservoirBatch(kT=[1.0, 2.0]).attach([], 3.0)


def test_deferred_destroy_takes_thermostat_batches_before_workspaces(capi, monkeypatch):
    order = []

    class Lib:
        def cavmd_destroy(self, h):
            order.append(("ws", h.value))
            return 0

        def cavmd_bussi_batch_destroy(self, h):
            order.append(("bussi_batch", h.value))
            return 0

    ws = object.__new__(capi.Workspace)
    ws._lib, ws._h = Lib(), ctypes.c_void_p(0x10)
    b = object.__new__(capi.BussiBatch)
    b._lib, b._h, b._ws = ws._lib, ctypes.c_void_p(0x20), ws
    monkeypatch.setattr(capi, "_capturing", lambda: True)
    ws.close()
    b.close()
    assert order == [] and not b._h.value and not ws._h.value
    monkeypatch.setattr(capi, "_capturing", lambda: False)
    capi._destroy_deferred()
    assert order == [("bussi_batch", 0x20), ("ws", 0x10)]
    assert not capi._deferred and not capi._deferred_children
