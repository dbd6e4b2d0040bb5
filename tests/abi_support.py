"""What the no-GPU checks of include/cavmd.h and the libraries share (tests/batch_objects.py, the per-object
tests/test_*_abi.py, tests/test_capi_abi.py): reading the header, listing a library's exports, building and running a C99
caller, parsing the layouts it prints -- and one good item per batch object, which the refusal tests start from."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "include", "cavmd.h")


def header_text() -> str:
    """include/cavmd.h with its comments stripped"""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared(prefix: str = "cavmd_"):
    """the entry points the header declares under `prefix`, sorted"""
    return sorted(set(re.findall(r"CAVMD_API\s+[\w\s\*]+?\b(%s\w*)\s*\(" % re.escape(prefix), header_text())))


def exported(path: str):
    """the text symbols `nm -D --defined-only` lists for the library at `path`"""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


_C99_OUTPUT = {}


def run_c99(name: str, capi, tmp_path) -> str:
    """Builds tests/c_abi/<name>.c as C99 with -pedantic -Wall -Wextra -Werror against include/cavmd.h, links it with
    libcavmd.so and runs it; the exit status must be 0.  Returns what it printed.  A program is built and run once per session:
    a second caller gets the first run's output."""
    if name in _C99_OUTPUT:
        return _C99_OUTPUT[name]
    src = os.path.join(ROOT, "tests", "c_abi", name + ".c")
    exe = str(tmp_path / name)
    libdir = os.path.dirname(capi.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                         "-o", exe, "-L", libdir, "-lcavmd", "-lm", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (name, out.returncode, out.stdout, out.stderr[-2000:])
    _C99_OUTPUT[name] = out.stdout
    return out.stdout


def c_layouts(stdout: str):
    """(sizes, offsets) from the lines tests/c_abi/abi_print.h writes: `sizeof <which> <n>` gives sizes[which] and
    `<which>.<field> <offset>` gives offsets[which][field]."""
    sizes = {which: int(n) for which, n in re.findall(r"^sizeof (\w+) (\d+)$", stdout, flags=re.M)}
    offsets = {which: {} for which in sizes}
    for which, field, off in re.findall(r"^(\w+)\.(\w+) (\d+)$", stdout, flags=re.M):
        offsets[which][field] = int(off)
    return sizes, offsets


def bits(x) -> int:
    return int(np.float64(x).view(np.uint64))


# ---- one good item per batch object: the `good` of its row in batch_objects.OBJECTS, and what the refusal matrices
# of the per-object modules vary ----------------------------------------------------------------------------------------------
def good_batch(capi, n=501):
    return capi.batch_item(n, 0x10000, 0x20000, 0x30000, 0x40000, (40.0, 40.0, 40.0), 2, capi.make_params(0.0091, 1e-3, 1.0))


def good_bussi_batch(capi, n=501, dof=1500.0):
    return capi.bussi_batch_item(0x10000, 0x20000, n, dof)


def good_recorder(capi, N=501, n_members=501):
    return capi.recorder_item(0x10000, 0x20000, 0x30000, 0x40000, N, n_members)


def good_field_recorder(capi):
    return capi.field_item(0x10000, 24, 501)


def good_verlet(capi, n=501, forces=(0x50000,), net=0, langevin=-1):
    return capi.verlet_item(n, 0x10000, 0x20004, 0x30000, 0x40008, forces, net, (10.0, 11.0, 12.0), langevin)


def good_bath(capi, **kw):
    args = dict(gamma_ptr=0x10008, N=501, kT=9.5e-4, seed=0x9E3779B97F4A7C15)
    args.update(kw)
    return capi.bath_item(**args)


def good_ledger(capi, **kw):
    args = dict(result_ptr=0x10000, vel_ptr=0x20000, members_ptr=0x30004, n_members=500, N=501, energy_ptrs=(0x40000, 0x50000),
                reservoir_ptrs=(0x60008, 0x70008, 0x80008), time_ptr=0x90008, dof=1500.0, add_cavity_kinetic=1)
    args.update(kw)
    return capi.ledger_item(**args)


def good_thermalize(capi, **kw):
    args = dict(vel_ptr=0x10000, N=501, kT=9.5e-4, seed=0x9E3779B97F4A7C15, members_ptr=0x50004, n_members=500,
                flags=capi.THERMALIZE_ZERO_MOMENTUM | capi.THERMALIZE_PLACE_PHOTON | capi.THERMALIZE_FINITE_Q
                | capi.THERMALIZE_PHOTON_VELOCITY, pos_ptr=0x20000, image_ptr=0x30004, result_ptr=0x40008,
                box_L=(40.0, 41.0, 42.0), params=capi.make_params(0.0091, 1e-3, 1.0))
    args.update(kw)
    return capi.thermalize_item(**args)


def good_draw(capi, **kw):
    args = dict(verlet_row_ptr=0x10000, bussi_row_ptr=0x20008, gamma=0.01, kT=9.5e-4, set_T=9.5e-4, tau=100.0, dof=1293.0,
                dt=5.0, records_ptr=0x30000, rows_ptr=0x40008, capacity=64, tolerance=1e-3, tolerance_initial=1e-4,
                tolerance_time_constant=1e4, dt_min=0.1, dt_max=50.0)
    args.update(kw)
    return capi.draw_item(**args)


def molecular_params(capi, r_cut=3.0):
    return capi.molecular_params(3, {0: (0.7, 2.2), 1: (1.4, 2.0)},
                                 {(0, 0): (1e-3, 2.0, r_cut), (0, 1): (2e-3, 1.5, r_cut), (1, 1): (5e-4, 1.0, 0.5 * r_cut)})


def good_molecular(capi, n=501, bonds=((0, 1, 0), (2, 3, 1)), box=(8.0, 9.0, 10.0)):
    return capi.molecular_item(n, 0x10000, 0x20000, box, np.array(bonds, dtype=np.uint32).reshape(-1, 3))


COULOMB_BOX = (8.0, 9.0, 10.0)


def good_coulomb(capi, n=501, exclusions=((0, 1), (2, 3)), box=COULOMB_BOX, kappa=0.9, r_cut=4.0, k_cut=3.0):
    return capi.coulomb_item(n, 0x10000, 0x30000, 0x20000, box, kappa, r_cut, k_cut, np.array(exclusions, dtype=np.uint32).reshape(-1, 2))
