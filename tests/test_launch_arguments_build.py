"""The kernel descriptors of the four kernels an AoS evaluation can launch, read from `make asm` (no GPU): each takes its leading
arguments in user SGPRs at wave start (kernel-argument preload: csrc/Makefile, UNITFLAGS_cavmd_capi), at least as many dwords
as its prologue was laid out for, and none of them uses scratch memory.

Planned dwords (csrc/cavmd_persistent_kernel.hpp, csrc/cavmd_force_kernels.hpp):
  cavity_persistent_kernel     12   pos2, charge, image, epoch (8), N, G, L_typeid, lds_slots
  dipole_partials_aos_kernel    9   pos2, charge, image (6), N, G, L_typeid
  force_map_aos_fused_kernel   14   pos2, charge, image, part_d, part_i (10), N, G, reverse, nparts
  cavity_small_system_kernel    8   pos2, charge, image (6), N, L_typeid
"""
import os
import re
import subprocess

PLANNED = {"cavity_persistent_kernel": (12, 6),      # kernel -> (dwords, instantiations in the product)
           "dipole_partials_aos_kernel": (9, 6),
           "force_map_aos_fused_kernel": (14, 3),
           "cavity_small_system_kernel": (8, 1)}


def descriptors(capi):
    csrc = os.path.dirname(capi.LIB_PATH)
    subprocess.run(["make", "-C", csrc, "-s", "asm"], check=True, capture_output=True)
    text = open(os.path.join(csrc, "cavmd_capi.s")).read()
    out = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        out[name] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\n", body)}
    return out


def test_leading_arguments_are_preloaded_and_nothing_uses_scratch(capi):
    desc = descriptors(capi)
    for kernel, (dwords, instantiations) in PLANNED.items():
        mine = {name: d for name, d in desc.items() if re.match(r"_ZN5cavmd\d+%sI" % kernel, name)}
        assert len(mine) == instantiations, (kernel, sorted(mine))
        for name, d in mine.items():
            print(f"{name}: preload {d['user_sgpr_kernarg_preload_length']} of {d['user_sgpr_count']} user SGPRs, "
                  f"scratch {d['private_segment_fixed_size']}")
            assert d["user_sgpr_kernarg_preload_length"] >= dwords, (name, d["user_sgpr_kernarg_preload_length"], dwords)
            assert d["user_sgpr_kernarg_preload_offset"] == 0, name
            assert d["private_segment_fixed_size"] == 0 and d["enable_private_segment"] == 0, name
            assert d["uses_dynamic_stack"] == 0, name


def test_only_the_evaluation_unit_is_built_with_the_preload_option(capi):
    """Every other unit is compiled as before: none of its kernels preloads."""
    csrc = os.path.dirname(capi.LIB_PATH)
    subprocess.run(["make", "-C", csrc, "-s", "asm"], check=True, capture_output=True)
    for unit in os.listdir(os.path.join(csrc, "build", "asm")):
        if not unit.endswith(".s") or unit == "cavmd_capi.s":
            continue
        text = open(os.path.join(csrc, "build", "asm", unit)).read()
        lengths = {int(v) for v in re.findall(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", text)}
        assert lengths <= {0}, (unit, lengths)
