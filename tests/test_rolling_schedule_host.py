"""The rolling tile loop's schedule (csrc/cavmd_tile_schedule.hpp), enumerated on the host.

tests/rolling_schedule_host.cpp is a stand-alone program: it drives the very function template the kernels run
(cavmd::rolling_rows) with recording callbacks over all N in [1, 6000] x G in {1, 5, 16, 17, 256} x UNROLL = 2 and checks that
every index loaded is < N and belongs to the block, that every owned full-tile particle is loaded exactly once, and that the
per-lane order is (tile, u) ascending with never more than UNROLL rows in flight.  Built with AddressSanitizer and UBSan on that
program alone; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join(ROOT, "cav-hoomd_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "rolling_schedule_host.cpp")


def test_rolling_schedule_enumerated_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rolling_schedule_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("rolling schedule ok:"), run.stdout
    # 5 grids x 6000 sizes, UNROLL rows per full tile: sum over N of 2 * (N // 512) rows per grid
    rows = 5 * sum(2 * (n // 512) for n in range(1, 6001))
    assert run.stdout.split()[3] == str(rows), (run.stdout, rows)


def test_the_kernels_use_the_enumerated_schedule():
    """The program checks the function the kernels call, not a copy: both call sites go through accumulate_full_tiles, which
    drives rolling_rows, and neither keeps a tile loop of its own."""
    force = open(os.path.join(CSRC, "cavmd_force_kernels.hpp")).read()
    persistent = open(os.path.join(CSRC, "cavmd_persistent_kernel.hpp")).read()
    assert force.count("rolling_rows<UNROLL>(") == 1 and '#include "cavmd_tile_schedule.hpp"' in force
    assert force.count("accumulate_full_tiles<Input, BLOCK, UNROLL>(") == 1     # dipole_partials_kernel
    assert persistent.count("accumulate_full_tiles<AosInputT<2>, BLOCK, UNROLL>(") == 1
    assert "tile_load<" not in persistent and "strided_tiles(N, G, b, TILE)" in persistent
