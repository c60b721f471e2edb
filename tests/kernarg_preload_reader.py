"""Reads, from a host object or shared library hipcc made, the kernel descriptors of its gfx950 code object: kernel name -> the number of
kernel-argument dwords the command processor preloads into user SGPRs (amd_kernel_code kernel descriptor, bytes 58..59:
kernarg_preload_spec_length in bits 0..6). Pure Python: the clang offload bundle (uncompressed) and the ELF64 symbol table."""
import struct
import subprocess

_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(blob, arch="gfx950"):
    out, i = [], blob.find(_MAGIC)
    while i >= 0:
        n, o = struct.unpack_from("<Q", blob, i + 24)[0], i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, o)
            triple = blob[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if size and triple.endswith(arch) and "amdgcn" in triple:
                out.append(blob[i + off:i + off + size])
        i = blob.find(_MAGIC, i + len(_MAGIC))
    return out


def preload_lengths(elf):
    """{mangled kernel name: preloaded dwords} of one AMDGPU ELF64 code object"""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2, "ELF64 expected"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]   # name, type, flags, addr, offset, size, link, info, align, entsize
    out = {}
    for s in secs:
        if s[1] != 2:        # SHT_SYMTAB
            continue
        strtab = secs[s[6]]
        for k in range(s[5] // 24):
            name_off, info, other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, s[4] + k * 24)
            end = elf.index(b"\0", strtab[4] + name_off)
            name = elf[strtab[4] + name_off:end].decode()
            if not name.endswith(".kd") or shndx == 0 or shndx >= shnum or size != 64:
                continue
            sec = secs[shndx]
            kd = elf[sec[4] + (value - sec[3]):sec[4] + (value - sec[3]) + 64]
            out[name[:-3]] = struct.unpack_from("<H", kd, 58)[0] & 0x7F
    return out


def file_preload_lengths(path):
    blob = open(path, "rb").read()
    out = {}
    for co in code_objects(blob):
        out.update(preload_lengths(co))
    return out


def demangle(names):
    names = list(names)
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))
