"""How the library is laid out and built, on a machine WITHOUT a GPU ('Translation units and the build graph'): nine
translation units that csrc/Makefile and csrc/hoomd_shim/CMakeLists.txt both list, headers that do not lean on include order,
libraries linked from shared objects so that a variant recompiles only the units whose flags differ, and batch units that
cannot see inside the workspace."""
import collections
import glob
import os
import re
import shlex
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

from abi_support import ROOT

CSRC = os.path.join(ROOT, "cav-hoomd_amd", "csrc")
BATCH_UNITS = ("cavmd_batch", "cavmd_bussi_batch", "cavmd_recorder", "cavmd_field_recorder", "cavmd_verlet", "cavmd_molecular",
               "cavmd_coulomb")


def _makefile_sources():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    return re.search(r"^SOURCES\s*=\s*(.*)$", text, flags=re.M).group(1).split()


def test_source_lists_agree():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")) if not os.path.basename(p).startswith("microbench"))
    listed = _makefile_sources()
    assert len(listed) == len(set(listed)) == 9 and sorted(listed) == on_disk
    assert {unit + ".hip" for unit in BATCH_UNITS} < set(listed)
    cmake = open(os.path.join(CSRC, "hoomd_shim", "CMakeLists.txt")).read()
    in_cmake = re.search(r"set\(CAVMD_SOURCES\s+([^)]*)\)", cmake).group(1).split()
    assert in_cmake == listed
    assert "add_library(cavmd SHARED ${CAVMD_SOURCES})" in cmake


def _compile_command(target):
    """the tokens of the command `make` would compile `target` with"""
    out = subprocess.run(["make", "-C", CSRC, "-n", "-B", target], capture_output=True, text=True, check=True).stdout
    lines = [line for line in out.splitlines() if " -c " in line]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


def test_headers_stand_alone(tmp_path):
    """Each csrc/*.hpp as the first include of an otherwise empty HIP file, syntax-checked with the library's flags (host side:
    the device side reads the same text).  cavmd_small_system_body.hpp is the body of two kernels, shared as text, and says so."""
    tokens = _compile_command("build/product/cavmd_batch.o")
    flags, skip = [], False
    for tok in tokens[1:-1]:                                # between the compiler and the source
        if skip or tok in ("-MMD", "-MP", "-c"):
            skip = False
        elif tok == "-o":
            skip = True
        else:
            flags.append(tok)
    assert any(f.startswith("--offload-arch=") for f in flags) and "-ffp-contract=off" in flags
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp")))
    assert "NOT a stand-alone header" in open(os.path.join(CSRC, "cavmd_small_system_body.hpp")).read()
    headers.remove("cavmd_small_system_body.hpp")
    assert len(headers) >= 16

    def check(header):
        src = tmp_path / (header[:-4] + "_alone.hip")
        src.write_text('#include "%s"\n' % header)
        return header, subprocess.run([tokens[0]] + flags + ["-I", CSRC, "-fsyntax-only", "--cuda-host-only", "-x", "hip", str(src)],
                                      capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for header, done in pool.map(check, headers):
            assert done.returncode == 0, (header, done.stderr[-3000:])


def test_variants_share_what_they_should(tmp_path):
    """With the product up to date, the hooks build compiles cavmd_capi alone and each lane-split build cavmd_molecular and
    cavmd_coulomb alone; every other object is the product's.  A dry run in a copy of csrc/, nothing is compiled."""
    csrc = tmp_path / "pkg" / "csrc"
    os.makedirs(csrc / "build" / "product")
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")) + [os.path.join(CSRC, "Makefile")]:
        shutil.copy(path, csrc)
    subprocess.run(["make", "-C", str(csrc), "-s", "-t", "libcavmd.so"], check=True, capture_output=True)
    assert subprocess.run(["make", "-C", str(csrc), "-q", "libcavmd.so"]).returncode == 0
    out = subprocess.run(["make", "-C", str(csrc), "-n", "libcavmd_hooks.so", "split_variants"], capture_output=True, text=True,
                         check=True).stdout
    compiled = collections.Counter(os.path.basename(shlex.split(line)[-1]) for line in out.splitlines() if " -c " in line)
    assert compiled == {"cavmd_capi.hip": 1, "cavmd_molecular.hip": 3, "cavmd_coulomb.hip": 3}, out
    links = [line for line in out.splitlines() if " -shared " in line]
    assert len(links) == 4 and all(len(re.findall(r"\S+\.o\b", line)) == 9 for line in links), links
    hooks = next(line for line in links if "libcavmd_hooks.so" in line)
    assert "build/hooks/cavmd_capi.o" in hooks and hooks.count("build/product/") == 8
    for name in "abc":
        line = next(line for line in links if f"libcavmd_split_{name}.so" in line)
        assert f"build/split_{name}/cavmd_molecular.o" in line and f"build/split_{name}/cavmd_coulomb.o" in line
        assert line.count("build/product/") == 7


def test_batch_units_cannot_see_the_workspace():
    """The ten batch objects and the table layer they share reach a workspace through its WorkspaceTie alone; the switches
    of the variants are each read by one unit."""
    for name in [unit + ".hip" for unit in BATCH_UNITS] + ["cavmd_item_table.hpp"]:
        text = open(os.path.join(CSRC, name)).read()
        assert "cavmd_workspace.hpp" not in text and "cavmd_kernels.hpp" not in text, name
    readers = collections.defaultdict(set)
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        if os.path.basename(path).startswith("microbench"):
            continue
        code = re.sub(r"//.*", "", open(path).read())
        for switch in ("CAVMD_TEST_HOOKS", "CAVMD_MOLECULAR_J_SPLIT", "CAVMD_COULOMB_J_SPLIT", "CAVMD_COULOMB_K_SPLIT"):
            if switch in code:
                readers[switch].add(os.path.basename(path))
    assert readers == {"CAVMD_TEST_HOOKS": {"cavmd_capi.hip"}, "CAVMD_MOLECULAR_J_SPLIT": {"cavmd_molecular.hip"},
                       "CAVMD_COULOMB_J_SPLIT": {"cavmd_coulomb.hip"}, "CAVMD_COULOMB_K_SPLIT": {"cavmd_coulomb.hip"}}


def _conditional_names(path):
    """every CAVMD_* name a preprocessor conditional of `path` tests (#if, #ifdef, #ifndef, #elif, defined(...))"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S).replace("\\\n", " ")
    names = set()
    for line in text.splitlines():
        line = re.sub(r"//.*", "", line)
        if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
            names |= set(re.findall(r"\bCAVMD_\w+", line))
    return names


def test_compile_time_switches_are_the_ones_meant():
    """The library's sources branch on six names and no more: the test hooks, the two stamp hooks of the micro-benchmarks
    (empty in the product) and, in the public header the units compile against, the three lane splits.  A rejected variant or a
    diagnostic behind a -D (fault injection, a cheaper accumulate, protocol constants) has no place in them: it would be one
    flag away from the product."""
    sources = [p for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))
               if not os.path.basename(p).startswith("microbench")]
    assert len(sources) >= 26
    in_csrc = set().union(*[_conditional_names(p) for p in sources])
    assert in_csrc == {"CAVMD_TEST_HOOKS", "CAVMD_STAMP", "CAVMD_PSTAMP"}
    in_header = _conditional_names(os.path.join(ROOT, "include", "cavmd.h")) - {"CAVMD_H_"}
    assert in_header == {"CAVMD_MOLECULAR_J_SPLIT", "CAVMD_COULOMB_J_SPLIT", "CAVMD_COULOMB_K_SPLIT"}
    for name in in_csrc | in_header:
        assert not any(word in name for word in ("FAULT", "DIAG", "GROUP_COPIES", "POLL_SLEEP")), name
