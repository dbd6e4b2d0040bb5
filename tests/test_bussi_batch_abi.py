"""What is specific to the thermostat batch (cavmd_bussi_batch_*) on a machine WITHOUT a GPU: the equivalence the header states,
the per-item validation and the input-row maker (host arithmetic), the row maker's c against the c the reference's executed
C++ recorded (tests/golden/bussi_reference_golden.npz), and what the Python class refuses besides CPU tensors.  Header,
exports, layouts, null arguments, launch order, Python surface and deferred destroy are the shared checks of
tests/batch_objects.py, called here with this object's row."""
import math
import os

import numpy as np
import pytest
import torch

import batch_objects as checks
from abi_support import HEADER, ROOT
from abi_support import bits as _bits
from abi_support import good_bussi_batch as _good

GOLDEN = os.path.join(ROOT, "tests", "golden", "bussi_reference_golden.npz")
ROW = checks.ROWS["bussi_batch"]


# ---- 1. the header ------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_keeps_the_version():
    checks.header_declares_exactly_the_entry_points(ROW)
    # the equivalence and its condition are stated where a C caller reads them
    raw = open(HEADER).read()
    assert "at least 64 compute units" in raw and "2 ulp" in raw


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------
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


# ---- 3. the input row ---------------------------------------------------------------------------------------------------
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
    assert capi.load().cavmd_bussi_batch_input_make(0.1, 1.0, 1.0, 0.0, 0.0, None) == capi.CAVMD_ERR_INVALID_VALUE


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


# ---- 4. the Python class ---------------------------------------------------------------------------------------------
def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
    import cavitymd
    t = cavitymd.BussiReservoirBatch(kT=1.0, tau=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.attach([torch.zeros((10, 4), dtype=torch.float64)], 27.0)
    with pytest.raises(RuntimeError, match="before attach"):                  # a refused attach attaches nothing
        t.step_async()
    with pytest.raises(ValueError):
        cavitymd.BussiReservoirBatch(kT=[1.0, 2.0]).attach([], 3.0)


# ---- the checks every batch object gets (tests/batch_objects.py), on this object's row ---------------------------------------
def test_libraries_export_them_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)


def test_a_c99_caller_compiles_links_and_runs(capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)


def test_launch_order_is_a_stable_descending_sort(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)
