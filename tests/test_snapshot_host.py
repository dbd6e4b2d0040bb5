"""The host-only half of save and restore (csrc/cavmd_snapshot.hpp), driven by a stand-alone program.

tests/snapshot_check_host.cpp includes the very header the library's cavmd_snapshot_check and load go through and feeds
cavmd::snapshot_check, for one shape of each of the nine kinds, the accepted blob, each header field altered, every truncation,
`bytes` off by one and blobs of every length up to header + 64, each in a heap block of exactly its length.  Built with
AddressSanitizer and UBSan on that program alone; nothing is loaded into Python; no GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join(ROOT, "cav-hoomd_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "snapshot_check_host.cpp")


def test_snapshot_check_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "snapshot_check_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("snapshot check ok:"), run.stdout
    # per kind: 1 accepted + 12 + 7 altered + 65 truncations + 2 off by one + 2 x 129 lengths (less the accepted length, where
    # it lies within header + 64) + 2 null pointers
    assert int(run.stdout.split()[3]) >= 9 * (1 + 19 + 65 + 2 + 2 * 129 - 2 + 2), run.stdout


def test_the_library_uses_the_checked_header():
    """cavmd_snapshot_check and every load go through the function the program drives, and the header has no HIP in it."""
    header = open(os.path.join(CSRC, "cavmd_snapshot.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", header).lower()
    table = open(os.path.join(CSRC, "cavmd_item_table.hpp")).read()
    assert '#include "cavmd_snapshot.hpp"' in table and table.count("cavmd::snapshot_check(h_in, bytes, &h)") == 1
    verlet = open(os.path.join(CSRC, "cavmd_verlet.hip")).read()
    assert "return snapshot_check(blob, bytes, expected);" in verlet
