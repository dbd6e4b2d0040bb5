"""What is specific to the energy ledger (cavmd_ledger_*) on a machine WITHOUT a GPU (tests/test_batch_objects_abi.py runs the
shared checks a to i on its row of tests/batch_objects.py; none is skipped): the header's prose, every refusal of its item check with its status and the precedence among them, and
the literal layouts of the two structures."""
import ctypes

import numpy as np
import pytest
import torch

import batch_objects as checks
from abi_support import HEADER
from abi_support import good_ledger as _good

ROW = checks.ROWS["ledger"]
ROW_FIELDS, ITEM_FIELDS = ROW.structs["row"][2], ROW.structs["item"][2]          # {field: offset}, pinned as literals in the row


# ---- what this object adds to the checks every batch object gets (tests/batch_objects.py a to i) ------------------------------
def test_header_declares_the_nine_entry_points_and_the_contract():
    checks.header_declares_exactly_the_entry_points(ROW)
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for words in ("(cavity[0] + cavity[1]) + cavity[2]",
                  "(((potential[0] + potential[1]) + potential[2]) + potential[3]) + cavity_potential",
                  "kinetic_group + kinetic_cavity if add_cavity_kinetic, else kinetic_group", "kinetic_total + potential_total",
                  "((reservoir[0] + reservoir[1]) + reservoir[2]) + reservoir[3]", "system_total + reservoir_total",
                  "(2.0 kinetic_group) / (dof kB), or 0 where dof == 0", "dof = 9 n", "[CONSERVED]", "within 2 ulp",
                  "src/cavitymd/analysis.py:425-1046"):
        assert words in text, words
    # the section stands after the bath's and before the draws'
    raw = open(HEADER).read()
    assert raw.index("cavmd_bath_state_device_ptr(") < raw.index("typedef struct cavmd_ledger_row") < raw.index("cavmd_draw_item_check(")


def test_libraries_export_them_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)
    names = [n for n in capi._PROTOTYPES if n.startswith("cavmd_ledger_")]
    assert names == ["cavmd_ledger_" + s for s in ROW.entry_points]                 # the header's order
    order = list(capi._PROTOTYPES)
    assert order.index("cavmd_bath_state_device_ptr") + 1 == order.index("cavmd_ledger_item_check")


def test_the_version_is_still_2(capi):
    checks.the_version_is_still_2(capi)                                    # not a check on a row: it stays with each object


def test_c_layouts_equal_the_ctypes_ones_and_the_numpy_dtype(capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)
    assert ctypes.sizeof(capi.LedgerItem) == 128 and ctypes.sizeof(capi.LedgerRow) == 192
    for S, fields in ((capi.LedgerRow, ROW_FIELDS), (capi.LedgerItem, ITEM_FIELDS)):
        assert {name: getattr(S, name).offset for name, *_ in S._fields_} == fields
    dt = capi.ledger_row_dtype()
    assert dt.itemsize == 192 and {n: dt.fields[n][1] for n in dt.names} == ROW_FIELDS


def test_launch_order_is_a_stable_descending_sort(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)
    assert capi.Ledger._size(_good(capi, N=77, n_members=5)) == 77 and capi.Ledger._size(_good(capi, N=7, n_members=50)) == 50


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
    import cavitymd
    doc = cavitymd.ledger.__doc__
    step = doc[doc.index("with torch.cuda.graph(graph):"):]
    order = [step.index(call) for call in ("integrator.step_one()", "cavity.compute()", "integrator.step_two()", "ledger.record()",
                                          "thermostat.step_async()")]
    assert order == sorted(order)                        # the captured step, in its launch order
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.ledger._reservoir_addresses(torch.zeros(3, dtype=torch.float64), 3)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    chk = capi.ledger_item_check
    assert lib.cavmd_ledger_item_check(None) == INV
    assert chk(_good(capi)) == 0
    assert chk(capi.LedgerItem()) == 0                                     # nothing is required
    # every pointer may be absent on its own; d_energy[0] non-NULL with N == 0 is fine
    for kw in (dict(result_ptr=0), dict(vel_ptr=0), dict(members_ptr=0), dict(time_ptr=0), dict(energy_ptrs=()),
               dict(reservoir_ptrs=()), dict(N=0), dict(n_members=0), dict(N=0, n_members=0)):
        assert chk(_good(capi, **kw)) == 0, kw
    # misaligned pointers: 16 bytes for arrays, 8 for doubles, 4 for members
    for off in (1, 2, 4, 8):
        assert chk(_good(capi, result_ptr=0x10000 + off)) == INV, off
        assert chk(_good(capi, vel_ptr=0x20000 + off)) == INV, off
        for k in range(4):
            ptrs = [0x40000 + 0x1000 * j for j in range(4)]
            ptrs[k] += off
            assert chk(_good(capi, energy_ptrs=ptrs)) == INV, (k, off)
    for off, status in ((1, INV), (2, INV), (4, INV), (8, 0)):
        assert chk(_good(capi, time_ptr=0x90000 + off)) == status, off
        for k in range(4):
            ptrs = [0x60000 + 0x1000 * j for j in range(4)]
            ptrs[k] += off
            assert chk(_good(capi, reservoir_ptrs=ptrs)) == status, (k, off)
    for off, status in ((1, INV), (2, INV), (3, INV), (4, 0), (8, 0)):
        assert chk(_good(capi, members_ptr=0x30000 + off)) == status, off
    # a gap in either pointer list; full lists are fine
    full_e, full_r = [0x40000 + 0x1000 * j for j in range(4)], [0x60000 + 0x1000 * j for j in range(4)]
    assert chk(_good(capi, energy_ptrs=full_e, reservoir_ptrs=full_r)) == 0
    for n in range(4):                                                     # a prefix of n entries passes ...
        assert chk(_good(capi, energy_ptrs=full_e[:n], reservoir_ptrs=full_r[:n])) == 0, n
    for hole in range(3):                                                  # ... a hole before a later entry does not
        for later in range(hole + 1, 4):
            e, r = [0] * 4, [0] * 4
            e[:hole], r[:hole] = full_e[:hole], full_r[:hole]
            e[later], r[later] = full_e[later], full_r[later]
            assert chk(_good(capi, energy_ptrs=e)) == INV and chk(_good(capi, reservoir_ptrs=r)) == INV, (hole, later)
    # dof: finite and >= 0; 0 is legal
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert chk(_good(capi, dof=bad)) == INV, bad
    assert chk(_good(capi, dof=0.0)) == 0 and chk(_good(capi, dof=1e300)) == 0
    # add_cavity_kinetic: 0 or 1
    assert chk(_good(capi, add_cavity_kinetic=0)) == 0
    for bad in (2, 3, 2 ** 32 - 1):
        assert chk(_good(capi, add_cavity_kinetic=bad)) == INV, bad
    # the cap
    M = capi.BATCH_MAX_ITEM_N
    assert chk(_good(capi, N=M, n_members=M)) == 0
    assert chk(_good(capi, N=M + 1)) == CAP and chk(_good(capi, n_members=M + 1)) == CAP
    # reserved words
    for name, value in (("reserved0", 1), ("reserved0", 2 ** 31), ("reserved", 1), ("reserved", 2 ** 63)):
        it = _good(capi)
        setattr(it, name, value)
        assert chk(it) == INV, (name, value)
    # precedence, as the recorder's: reserved words, pointers and values before the capacity
    it = _good(capi, N=M + 1)
    it.reserved = 1
    assert chk(it) == INV
    assert chk(_good(capi, N=M + 1, vel_ptr=0x20008)) == INV
    assert chk(_good(capi, N=M + 1, dof=-1.0)) == INV and chk(_good(capi, n_members=M + 1, add_cavity_kinetic=2)) == INV


def test_the_named_columns_alias_the_rows_own(capi):
    """BatchEnergyLedger.read() views the row with one more field per named term and reservoir, at that column's offset"""
    import cavitymd
    led = object.__new__(cavitymd.BatchEnergyLedger)
    led.term_names, led.reservoir_names = ("molecular", "coulomb"), ("bussi", "langevin", "bath")
    dt = led._dtype_with_names()
    assert dt.itemsize == 192 and dt.names[:len(ROW_FIELDS)] == capi.ledger_row_dtype().names
    assert [dt.fields[n][1] for n in led.term_names] == [24, 32] and [dt.fields[n][1] for n in led.reservoir_names] == [128, 136, 144]
    rows = np.zeros(2, dtype=capi.ledger_row_dtype())
    rows["potential"][:, 1] = (3.0, 4.0)
    rows["reservoir"][:, 2] = (5.0, 6.0)
    named = rows.view(dt)
    assert named["coulomb"].tolist() == [3.0, 4.0] and named["bath"].tolist() == [5.0, 6.0]
    led.term_names = ("time",)
    with pytest.raises(ValueError, match="a column of the row already"):
        led._dtype_with_names()
