"""The integrator batch (cavmd_verlet_*) on a machine WITHOUT a GPU: the header declares and both libraries export the eleven
entry points and nothing stray, the version is still 2, the item, input and state layouts agree between C and ctypes, the
per-item validation and the input-row maker work without a device, and the Python class refuses CPU tensors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "cavmd.h")
VERLET = ("cavmd_verlet_item_check", "cavmd_verlet_input_make", "cavmd_verlet_create", "cavmd_verlet_destroy",
          "cavmd_verlet_set_items", "cavmd_verlet_accelerations", "cavmd_verlet_step_one", "cavmd_verlet_step_two",
          "cavmd_verlet_read", "cavmd_verlet_reset", "cavmd_verlet_state_device_ptr")


def _bits(x) -> int:
    return int(np.float64(x).view(np.uint64))


# ---- 1. header, libraries, binary -------------------------------------------------------------------------------------
def test_header_declares_the_eleven_entry_points_and_keeps_the_version():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"CAVMD_API\s+[\w\s\*]+?\b(cavmd_verlet_\w+)\s*\(", text)))
    assert len(VERLET) == 11 and declared == sorted(VERLET)
    assert re.search(r"#define\s+CAVMD_VERSION_MINOR\s+2\b", text)
    assert "typedef struct cavmd_verlet cavmd_verlet;" in text
    assert "[HOOMD upstream, not in checkout]" in raw        # where the expressions come from is said where a C caller reads


def test_libraries_export_them_and_nothing_stray(capi):
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in VERLET:
            assert hasattr(lib, name), (path, name)
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert {s for s in exported if s.startswith("cavmd_verlet")} == set(VERLET), path
        assert not {s for s in exported if not s.startswith("cavmd_") and not s.startswith("_")}, path
    for name in VERLET:
        assert name in capi.EXPORTED_SYMBOLS
    assert capi.load().cavmd_version() == 2
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"verlet_step_one_kernel" in blob and b"verlet_step_two_kernel" in blob and b"gfx950" in blob


# ---- 2. layouts ---------------------------------------------------------------------------------------------------------
def test_c_layouts_equal_the_ctypes_ones(capi, tmp_path):
    """tests/c_abi/verlet_abi_check.c, built as C99 with -pedantic -Werror, prints sizeof and offsetof of every field as the C
    compiler sees them; they equal the ctypes structures field by field.  It also runs the refusals seen from C."""
    src = os.path.join(ROOT, "tests", "c_abi", "verlet_abi_check.c")
    exe = str(tmp_path / "verlet_abi_check")
    libdir = os.path.dirname(capi.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                         "-o", exe, "-L", libdir, "-lcavmd", "-lm", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "VERLET-ABI-OK" in out.stdout, (out.returncode, out.stdout, out.stderr[-2000:])
    structs = {"item": capi.VerletItem, "input": capi.VerletInput, "state": capi.VerletState}
    sizes = re.search(r"sizeof item (\d+) input (\d+) state (\d+)", out.stdout)
    assert tuple(int(x) for x in sizes.groups()) == (128, 64, 32)
    assert tuple(ctypes.sizeof(structs[k]) for k in ("item", "input", "state")) == (128, 64, 32)
    seen = {k: {} for k in structs}
    for which, field, off in re.findall(r"^(item|input|state)\.(\w+) (\d+)$", out.stdout, flags=re.M):
        seen[which][field] = int(off)
    for which, S in structs.items():
        assert seen[which] == {name: getattr(S, name).offset for name, *_ in S._fields_}, which
    assert seen["item"]["d_force"] == 32 and seen["item"]["N"] == 96 and seen["input"]["skip"] == 48
    assert capi.verlet_state_dtype().itemsize == 32
    assert [capi.verlet_state_dtype().fields[n][1] for n, _ in capi.VERLET_STATE_DTYPE_FIELDS] == \
        [seen["state"][n] for n, _ in capi.VERLET_STATE_DTYPE_FIELDS]


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def _good(capi, n=501, forces=(0x50000,), net=0, langevin=-1):
    return capi.verlet_item(n, 0x10000, 0x20004, 0x30000, 0x40008, forces, net, (10.0, 11.0, 12.0), langevin)


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


def test_null_handles_are_refused_without_a_device(capi):
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    it = _good(capi)
    out = ctypes.c_void_p(123)
    st = capi.VerletState()
    assert lib.cavmd_verlet_create(None, 1, ctypes.byref(it), ctypes.byref(out)) == INV and not out.value
    assert lib.cavmd_verlet_create(None, 1, ctypes.byref(it), None) == INV
    assert lib.cavmd_verlet_destroy(None) == 0
    assert lib.cavmd_verlet_set_items(None, 0, 1, ctypes.byref(it)) == INV
    assert lib.cavmd_verlet_accelerations(None, None) == INV
    assert lib.cavmd_verlet_step_one(None, None, ctypes.c_void_p(0x1000)) == INV
    assert lib.cavmd_verlet_step_two(None, None, ctypes.c_void_p(0x1000)) == INV
    assert lib.cavmd_verlet_read(None, None, ctypes.byref(st)) == INV
    assert lib.cavmd_verlet_reset(None, None) == INV
    assert lib.cavmd_verlet_state_device_ptr(None, ctypes.byref(out)) == INV


# ---- 4. the input row ---------------------------------------------------------------------------------------------------
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


# ---- 5. the Python surface ----------------------------------------------------------------------------------------------
def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    import cavitymd
    assert "VerletBatch" in cavitymd.__all__ and cavitymd.VerletBatch is cavitymd.integrator_batch.VerletBatch
    for name in ("set_inputs", "draw_inputs", "prime", "step_one", "step_two", "state", "reset", "close"):
        assert callable(getattr(cavitymd.VerletBatch, name)), name
    for name in ("accelerations", "step_one", "step_two", "read", "reset", "set_items", "state_device_ptr", "close"):
        assert callable(getattr(capi.Verlet, name)), name
    b = object.__new__(capi.Verlet)
    b.sizes = [501, 0, 2049, 501]
    assert b.launch_order == [2, 0, 3, 1]

    class NoBatch:                                     # never looked at: the CPU tensor is refused first
        def __len__(self):
            return 1

    vel = torch.zeros((10, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.VerletBatch(NoBatch(), [vel])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cavitymd.VerletBatch(NoBatch(), [np.zeros((10, 4))])
