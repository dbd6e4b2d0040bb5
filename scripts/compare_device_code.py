"""Device code of two builds of csrc/, kernel by kernel (the method of profiles/batch_object_layers/device_code.txt).

From every object file build/<flavour>/<unit>.o of both trees the gfx950 code object is taken out of its .hip_fatbin section
(llvm-objcopy, clang-offload-bundler); per kernel, `code` compares the disassembly of the kernel's symbol (llvm-objdump -d,
addresses dropped), `descriptor` the 64 bytes of its .kd symbol and the resource figures of its metadata note (`moved`: the
figures and every byte but kernel_code_entry_byte_offset, bytes 16..23, agree -- where the code lies in a unit that gained a
kernel; `new`: a kernel the parent has not).  Needs no GPU.

    python scripts/compare_device_code.py PARENT_CSRC THIS_CSRC > table.txt"""
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FLAVOURS = ("product", "hooks", "split_a", "split_b", "split_c")
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def code_object(obj: str, tmp: str) -> str:
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, obj, os.path.join(tmp, "copy.o")],
                   check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fatbin,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    return co


def descriptors(co: str) -> dict:
    """kernel -> the 64 bytes of its .kd symbol, read from the ELF"""
    data = open(co, "rb").read()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for sec in sections:
        if sec[1] != 2:                                                          # SHT_SYMTAB
            continue
        strtab = sections[sec[6]]
        for k in range(sec[5] // sec[9]):
            name_off, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", data, sec[4] + k * sec[9])
            end = data.index(b"\0", strtab[4] + name_off)
            name = data[strtab[4] + name_off:end].decode()
            if name.endswith(".kd") and 0 < shndx < shnum:
                home = sections[shndx]
                at = home[4] + value - home[3]
                out[name[:-3]] = data[at:at + 64]
    return out


def disassembly(co: str) -> dict:
    """kernel symbol -> its instructions, addresses dropped"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                          check=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def figures(co: str) -> dict:
    """kernel symbol -> the resource figures of the metadata note"""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + text)[1:]:
        block = "  - .agpr_count:" + block
        name = re.search(r"\.symbol:\s+'?([^'\s]+)\.kd'?", block).group(1)
        out[name] = tuple(int(re.search(re.escape(f) + r":\s+(\d+)", block).group(1)) for f in FIGURES)
    return out


def demangled(names):
    filt = os.path.join(LLVM, "llvm-cxxfilt")
    text = subprocess.run([filt if os.path.exists(filt) else "c++filt"] + list(names), capture_output=True, text=True, check=True).stdout
    return {n: re.sub(r"^void |\(.*$", "", d).replace(", ", ",").replace("(cavmd::", "").replace("bool)", "")
            for n, d in zip(names, text.splitlines())}


def main():
    parent, this = sys.argv[1], sys.argv[2]
    rows, counts, new, moved = [], {}, 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for flavour in FLAVOURS:
            for obj in sorted(glob.glob(os.path.join(this, "build", flavour, "*.o"))):
                unit = os.path.basename(obj)[:-2]
                old = os.path.join(parent, "build", flavour, unit + ".o")
                sides = []
                for k, path in enumerate((old, obj)):
                    sub = os.path.join(tmp, f"{flavour}_{unit}_{k}")
                    os.makedirs(sub)
                    co = code_object(path, sub)
                    sides.append((descriptors(co), disassembly(co), figures(co)))
                (kd0, dis0, fig0), (kd1, dis1, fig1) = sides
                kernels = sorted(set(kd0) | set(kd1))
                names = demangled(kernels)
                for kern in kernels:
                    code = "identical" if kern in dis0 and kern in dis1 and dis0[kern] == dis1[kern] and dis1[kern] else \
                        ("only parent" if kern not in dis1 else "only this" if kern not in dis0 else "DIFFERS")
                    desc = "identical" if kd0.get(kern) == kd1.get(kern) and fig0.get(kern) == fig1.get(kern) and kern in kd1 else "DIFFERS"
                    if desc == "DIFFERS" and kern in kd0 and kern in kd1 and fig0.get(kern) == fig1.get(kern) \
                            and kd0[kern][:16] + kd0[kern][24:] == kd1[kern][:16] + kd1[kern][24:]:
                        desc = "moved"           # kernel_code_entry_byte_offset alone: a kernel was added to the unit
                        moved += code == "identical"
                    if code == "only this":
                        desc = "new"
                        new += 1
                    rows.append((f"{flavour}/{unit}", names[kern], code, desc) + tuple(str(x) for x in fig1.get(kern, fig0.get(kern))))
                    c = counts.setdefault(flavour.split("_")[0], [0, 0])
                    c[0] += 1
                    c[1] += code == "identical" and desc in ("identical", "moved")
    head = ("flavour/unit", "kernel", "code", "descriptor", "vgpr", "agpr", "sgpr", "lds_bytes", "scratch_bytes")
    widths = [max(len(r[i]) for r in rows + [head]) for i in range(len(head))]
    for r in [head] + rows:
        print("  ".join(x.ljust(w) for x, w in zip(r, widths)).rstrip())
    print()
    total = sum(c[0] for c in counts.values())
    same = sum(c[1] for c in counts.values())
    print(f"product kernels: {counts['product'][0]}, of them with the parent's code, resource figures and descriptor "
          f"(its code entry offset aside): {counts['product'][1]}")
    print(f"descriptors byte-identical: {same - moved}; differing in kernel_code_entry_byte_offset alone (`moved`): {moved}; "
          f"kernels the parent has not (`new`): {new}")
    print(f"all {total} rows ({counts['product'][0]} product, {counts['hooks'][0]} hooks, {counts['split'][0]} split variants): "
          + (f"{new} new, " if new else "") + ("the rest identical" if new and same + new == total else
                                                "identical" if same == total else f"{total - same - new} DIFFER"))
    return 0 if same + new == total else 1


if __name__ == "__main__":
    sys.exit(main())
