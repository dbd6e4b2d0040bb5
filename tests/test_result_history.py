"""Result history without a GPU: the C ABI declares and exports cavmd_last_sequence / cavmd_result_at / cavmd_energies_at and
CAVMD_ERR_EXPIRED, a C99 caller compiles against them, argument validation needs no device, the pybind11 module and the
HOOMD shim (stand-ins) expose lastSequence / getResultAt / getEnergiesAt, and cavitymd.EnergyHistory's bookkeeping holds
against a fake compute object."""
import ctypes
import glob
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "cavmd.h")
NEW = ("cavmd_last_sequence", "cavmd_result_at", "cavmd_energies_at")

C_CALLER = r"""
#include <stdio.h>
#include "cavmd.h"

int main(void)
{
    cavmd_workspace* ws = NULL;
    uint64_t last = 0;
    cavmd_result r;
    double e[3];
    int st = cavmd_last_sequence(ws, &last);
    if (st != CAVMD_ERR_INVALID_VALUE)
        return 1;
    if (cavmd_result_at(ws, (uint64_t)1, &r) != CAVMD_ERR_INVALID_VALUE)
        return 2;
    if (cavmd_energies_at(ws, (uint64_t)1, e) != CAVMD_ERR_INVALID_VALUE)
        return 3;
    if (CAVMD_ERR_EXPIRED != -7)
        return 4;
    printf("HISTORY-ABI-OK %s\n", cavmd_error_string(CAVMD_ERR_EXPIRED));
    return 0;
}
"""


def test_header_declares_the_history_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"CAVMD_API\s+int\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+CAVMD_ERR_EXPIRED\s+\(-7\)", text)
    assert re.search(r"#define\s+CAVMD_VERSION_MINOR\s+2\b", text)


def test_a_c99_caller_compiles_links_and_runs(capi, tmp_path):
    src = tmp_path / "history_caller.c"
    src.write_text(C_CALLER)
    exe = str(tmp_path / "history_caller")
    libdir = os.path.dirname(capi.LIB_PATH)
    cc = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                         "-L", libdir, "-lcavmd", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "HISTORY-ABI-OK" in out.stdout, (out.returncode, out.stdout, out.stderr[-2000:])


def test_library_exports_and_names_the_new_code(capi):
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS
    assert capi.CAVMD_ERR_EXPIRED == -7
    s = capi.error_string(capi.CAVMD_ERR_EXPIRED)
    assert s and s != capi.error_string(-99) and "result_history" in s
    assert capi.load().cavmd_version() == 2


def test_null_arguments_are_refused_without_a_device(capi):
    lib = capi.load()
    r = capi.Result()
    e = (ctypes.c_double * 3)()
    last = ctypes.c_uint64(123)
    assert lib.cavmd_result_at(None, 1, ctypes.byref(r)) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_result_at(None, 1, None) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_energies_at(None, 1, ctypes.byref(e)) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_energies_at(None, 1, None) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_last_sequence(None, ctypes.byref(last)) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_last_sequence(None, None) == capi.CAVMD_ERR_INVALID_VALUE
    assert lib.cavmd_set_tunable(None, b"result_history", 8) == capi.CAVMD_ERR_INVALID_VALUE


def test_pybind_module_exposes_the_history_methods(capi):
    from cavitymd import _cavitymd
    for name in ("lastSequence", "getResultAt", "getEnergiesAt"):
        assert hasattr(_cavitymd.CavityForceComputeHIP, name), name
    import cavitymd
    for name in ("lastSequence", "getResultAt", "getEnergiesAt"):
        assert callable(getattr(cavitymd.CavityForceComputeHIP, name)), name
    assert cavitymd.EnergyHistory is cavitymd.history.EnergyHistory
    assert "EnergyHistory" in cavitymd.__all__


def test_hoomd_shim_exposes_the_history_methods(capi):
    standin = os.path.join(ROOT, "tests", "stubs", "hoomd_cpp")
    subprocess.run(["make", "-C", standin, "-s", "syntax"], check=True)
    subprocess.run(["make", "-C", standin, "-s", "all"], check=True)
    path = glob.glob(os.path.join(standin, "_cavitymd_hip_standin*.so"))[0]
    spec = importlib.util.spec_from_file_location("_cavitymd_hip_standin", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("lastSequence", "getResultAt", "getEnergiesAt"):
        assert hasattr(mod.CavityForceComputeHIP, name), name


# ---- EnergyHistory against a fake compute object ----------------------------------------------------------------------
class FakeCompute:
    """Sequences and energies as a workspace would hand them out; `status` maps a sequence to the error its read gives."""

    def __init__(self):
        self.seq = 0
        self.reads = []
        self.status = {}

    def compute(self, timestep, n=1):
        if n:
            self.seq += 1

    def lastSequence(self):
        return self.seq

    def getEnergiesAt(self, sequence):
        from cavitymd._capi import CavmdError
        self.reads.append(sequence)
        if sequence in self.status:
            raise CavmdError(self.status[sequence], "fake", "cavmd_energies_at")
        assert 1 <= sequence <= self.seq
        return (1.0 * sequence, 2.0 * sequence, 3.0 * sequence)


def _row(ts, seq):
    return (ts, 1.0 * seq, 2.0 * seq, 3.0 * seq)


def test_energy_history_keeps_the_newest_and_reads_each_step_once():
    from cavitymd import EnergyHistory
    c = FakeCompute()
    h = EnergyHistory(c)
    assert h.drain() == [] and h.flush() == []
    rows = []
    for ts in range(100, 110):
        c.compute(ts)
        h.record(ts)
        got = h.drain()
        assert len(h) == 1                                     # the newest is kept back
        rows += got
    assert rows == [_row(100 + k, k + 1) for k in range(9)]
    assert c.reads == list(range(1, 10))                       # oldest first, nothing read twice, the newest not yet
    assert h.flush() == [_row(109, 10)]
    assert len(h) == 0 and h.flush() == [] and h.drain() == []
    assert c.reads == list(range(1, 11))


def test_energy_history_batches_and_empty_steps():
    from cavitymd import EnergyHistory
    c = FakeCompute()
    h = EnergyHistory(c)
    h.record(0)                                                # before any evaluation: the getters' zeros
    for ts in (1, 2, 3):
        c.compute(ts)
        h.record(ts)
    c.compute(4, n=0)                                          # N = 0 consumes no sequence: same energies as step 3
    h.record(4)
    assert h.drain() == [(0, 0.0, 0.0, 0.0), _row(1, 1), _row(2, 2), _row(3, 3)]
    assert h.flush() == [_row(4, 3)]
    assert 0 not in c.reads


@pytest.mark.parametrize("status", [-7, -6, 719], ids=["expired", "sync_timeout", "launch_failure"])
def test_energy_history_raises_for_a_step_it_cannot_read(status):
    from cavitymd import EnergyHistory
    from cavitymd._capi import CavmdError
    c = FakeCompute()
    c.status[3] = status
    h = EnergyHistory(c)
    for ts in range(6):
        c.compute(ts)
        h.record(ts)
    with pytest.raises(CavmdError) as e:
        h.drain()
    assert e.value.status == status
    # the rows read before it are not lost, the failed step is reported once, the rest follows
    assert h.drain() == [_row(0, 1), _row(1, 2), _row(3, 4), _row(4, 5)]
    assert h.flush() == [_row(5, 6)]
    assert c.reads == [1, 2, 3, 4, 5, 6]
