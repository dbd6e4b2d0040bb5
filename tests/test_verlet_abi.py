"""What is specific to the integrator batch (cavmd_verlet_*) on a machine WITHOUT a GPU: where the header says its expressions
come from, the per-item validation and the input-row maker (host arithmetic).  Header, exports, layouts, null arguments,
launch order, Python surface and deferred destroy are the shared checks of tests/batch_objects.py, called here with this
object's row."""
import ctypes

import numpy as np

import batch_objects as checks
from abi_support import HEADER
from abi_support import bits as _bits
from abi_support import good_verlet as _good

ROW = checks.ROWS["verlet"]


# ---- 1. the header ------------------------------------------------------------------------------------------------------
def test_header_declares_the_eleven_entry_points_and_keeps_the_version():
    checks.header_declares_exactly_the_entry_points(ROW)
    assert "[HOOMD upstream, not in checkout]" in open(HEADER).read()      # where a C caller reads it


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    chk = capi.verlet_item_check
    assert lib.cavmd_verlet_item_check(None) == INV
    assert chk(_good(capi)) == 0 and chk(_good(capi, 1)) == 0 and chk(_good(capi, 65536)) == 0
    assert chk(_good(capi, forces=(0x50000, 0x60000, 0x70000, 0x80000), net=0x90000, langevin=500)) == 0
    # an empty item may leave every array out, but what it gives is aligned and its reserved words are 0
    empty = capi.verlet_item(0, 0, 0, 0, 0, (), 0, (1.0, 1.0, 1.0))
    assert chk(empty) == 0
    # a null array
    for field in ("d_pos", "d_image", "d_vel", "d_accel"):
        it = _good(capi)
        setattr(it, field, None)
        assert chk(it) == INV, field
    assert chk(_good(capi, forces=())) == INV                                  # the first force array is required
    # a misaligned array
    for field, bad, ok in (("d_pos", 8, 16), ("d_vel", 8, 16), ("d_net_force", 8, 16), ("d_accel", 4, 8), ("d_image", 2, 4)):
        for off, status in ((bad, INV), (1, INV), (ok, 0)):
            it = _good(capi, net=0x90000)
            setattr(it, field, getattr(it, field) + off)
            assert chk(it) == status, (field, off)
    for k in range(4):
        forces = [0x50000, 0x60000, 0x70000, 0x80000]
        forces[k] += 8
        assert chk(_good(capi, forces=forces)) == INV, k
    it = capi.verlet_item(0, 0x10008, 0, 0, 0, (), 0, (1.0, 1.0, 1.0))
    assert chk(it) == INV
    # a non-NULL force pointer after a NULL one
    for forces in ((0x50000, 0, 0x70000), (0x50000, 0, 0, 0x80000), (0, 0x60000), (0x50000, 0x60000, 0, 0x80000)):
        assert chk(_good(capi, forces=forces)) == INV, forces
    it = capi.verlet_item(0, 0, 0, 0, 0, (0, 0x60000), 0, (1.0, 1.0, 1.0))
    assert chk(it) == INV
    # size
    assert chk(_good(capi, 65537)) == CAP and chk(_good(capi, 2**32 - 1)) == CAP
    # the Langevin index
    for n, idx, status in ((501, 500, 0), (501, 0, 0), (501, -1, 0), (501, 501, INV), (501, -2, INV), (501, 2**31 - 1, INV),
                           (0, 0, INV), (1, 0, 0), (1, 1, INV)):
        it = _good(capi, n, langevin=idx) if n else capi.verlet_item(0, 0, 0, 0, 0, (), 0, (1.0, 1.0, 1.0), idx)
        assert chk(it) == status, (n, idx)
    # reserved words
    for k in range(3):
        it = _good(capi)
        it.reserved[k] = 1 << (20 * k)
        assert chk(it) == INV, k
        it = capi.verlet_item(0, 0, 0, 0, 0, (), 0, (1.0, 1.0, 1.0))
        it.reserved[k] = 1
        assert chk(it) == INV, k


# ---- 3. the input row ---------------------------------------------------------------------------------------------------
def test_input_make_takes_the_coefficient_on_the_host(capi):
    rng = np.random.default_rng(17)
    cases = [(5.0, 0.01, 3.167e-4), (0.005, 1.0, 1.0), (1e-300, 1e-3, 1e-3), (41.341, 2.5e-5, 9.5e-4), (1.0, 1e300, 1e-300)]
    cases += [tuple(float(x) for x in 10.0 ** rng.uniform(-6, 3, 3)) for _ in range(200)]
    for dt, gamma, kT in cases:
        u = rng.uniform(-1, 1, 3)
        row = capi.verlet_input_make(dt, gamma, kT, u)
        assert _bits(row.langevin_coeff) == _bits(np.sqrt(6 * gamma * kT / dt)), (dt, gamma, kT)
        assert (row.dt, row.langevin_gamma, list(row.uniform), row.skip, row.reserved) == (dt, gamma, list(u), 0, 0)
        row = capi.verlet_input_make(dt, 0.0, kT, u)
        assert _bits(row.langevin_coeff) == _bits(0.0) and row.skip == 0            # no bath: coefficient 0
    for dt in (0.0, -0.0):
        row = capi.verlet_input_make(dt, 0.01, 1.0, (0.1, 0.2, 0.3))
        assert row.skip != 0 and row.langevin_coeff == 0.0
    lib = capi.load()
    u = (ctypes.c_double * 3)()
    assert lib.cavmd_verlet_input_make(1.0, 0.0, 0.0, ctypes.byref(u), None) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_verlet_input_make(1.0, 0.0, 0.0, None, ctypes.byref(capi.VerletInput())) == capi.CAVMD_ERR_INVALID_VALUE


# ---- the checks every batch object gets (tests/batch_objects.py), on this object's row ---------------------------------------
def test_libraries_export_them_and_nothing_stray(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)


def test_c_layouts_equal_the_ctypes_ones(capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)


def test_null_handles_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)
