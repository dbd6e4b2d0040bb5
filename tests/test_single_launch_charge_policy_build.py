"""The load policy of the single-launch kernel, read from `make asm` (no GPU): every product instantiation of
cavity_persistent_kernel takes the default NT_LOAD = 1 (csrc/cavmd_persistent_kernel.hpp) -- pos and image non-temporal, the
charges temporal, so that they can be found in the Infinity Cache by the next evaluation, and within one evaluation by the
tiles beyond the LDS budget that phase 2 reads a second time.

In the ISA the three streams are told apart by their width: pos is read as two 16-byte loads (global_load_dwordx4), the image
as one 12-byte load (dwordx3), a charge as one 8-byte load (dwordx2).  The only other 8-byte loads of the kernel are the polls
of the hand-off's granules, which carry `sc1` (agent-scope atomics), never `nt`.
"""
import os
import re
import subprocess

PRODUCT_INSTANTIATIONS = 6  # UNROLL 1, 2 x store policy 0, 1, 2 (tests/test_launch_arguments_build.py counts the same)


def kernel_bodies(capi):
    """mangled kernel name -> its instructions, from the label to the function's end"""
    csrc = os.path.dirname(capi.LIB_PATH)
    subprocess.run(["make", "-C", csrc, "-s", "asm"], check=True, capture_output=True)
    text = open(os.path.join(csrc, "cavmd_capi.s")).read()
    # (to the function's end label, not to the first s_endpgm: blocks of the function may stand behind that)
    return {name: body for name, body in re.findall(r"^(_ZN5cavmd\w+):.*?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)}


def loads(body, width, hint=None):
    """the global loads of `width` (e.g. "dwordx2") in `body`; with `hint`, those that carry it as a cache-policy modifier"""
    found = re.findall(r"^\s*global_load_%s\s+(.*)$" % width, body, re.M)
    if hint is None:
        return found
    return [line for line in found if re.search(r"\b%s\b" % hint, line.split("//")[0].split(";")[0])]


def test_product_single_launch_kernels_read_charges_temporal_and_the_rest_non_temporal(capi):
    bodies = kernel_bodies(capi)
    mine = {n: b for n, b in bodies.items() if re.match(r"_ZN5cavmd\d+cavity_persistent_kernelI", n)}
    assert len(mine) == PRODUCT_INSTANTIATIONS, sorted(mine)
    for name, body in mine.items():
        # <256, UNROLL, NT_STORE, FAULT = false, NT_LOAD = 1>
        assert re.match(r"_ZN5cavmd\d+cavity_persistent_kernelILi256ELi[12]ELi[012]ELb0ELi1EE", name), name
        x2, x2_nt = loads(body, "dwordx2"), loads(body, "dwordx2", "nt")
        x3_nt, x4_nt = loads(body, "dwordx3", "nt"), loads(body, "dwordx4", "nt")
        print(f"{name}: dwordx2 loads {len(x2)} (nt {len(x2_nt)}, sc1 {len(loads(body, 'dwordx2', 'sc1'))}), "
              f"dwordx3 nt {len(x3_nt)}, dwordx4 nt {len(x4_nt)}")
        assert x2, name                      # the charge loads are there to be judged
        assert not x2_nt, (name, x2_nt)      # charges (and polls) never non-temporal
        assert x4_nt, name                   # pos
        assert x3_nt, name                   # image


def test_the_check_sees_a_non_temporal_charge_load_where_there_is_one(capi):
    """dipole_partials_aos_kernel<NT, 256, UNROLL> is built with all three policies: 2 reads the charges non-temporal, 1 not."""
    bodies = kernel_bodies(capi)
    for policy, expect_nt in ((2, True), (1, False)):
        mine = {n: b for n, b in bodies.items()
                if re.match(r"_ZN5cavmd\d+dipole_partials_aos_kernelILi%dELi256ELi[12]EE" % policy, n)}
        assert len(mine) == 2, (policy, sorted(mine))
        for name, body in mine.items():
            x2_nt = loads(body, "dwordx2", "nt")
            print(f"{name}: dwordx2 nt loads {len(x2_nt)} of {len(loads(body, 'dwordx2'))}")
            assert loads(body, "dwordx2"), name
            assert bool(x2_nt) == expect_nt, (name, x2_nt)
            assert loads(body, "dwordx4", "nt") and loads(body, "dwordx3", "nt"), name
