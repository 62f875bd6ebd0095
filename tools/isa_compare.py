"""Compare the gfx950 kernels of two builds of libaz_hip.so / libaz_hip_tuning.so byte for byte.

    python tools/isa_compare.py PARENT_DIR CHANGE_DIR [> profiles/gemm_split/isa_compare.txt]

Each directory holds the two libraries of one build (tools/ab_lib.sh or a checkout of the other
revision builds the second pair).  For every kernel (a FUNC symbol with a `.kd` kernel
descriptor) the machine code and the 64-byte descriptor (LDS, scratch, kernarg size, the
compute_pgm_rsrc words: VGPRs, SGPRs, occupancy-relevant fields) are compared; the descriptor's
code-entry offset (bytes 16..23) is a displacement and is left out.  A kernel whose mangled name
changed (a template parameter removed) is matched to a parent kernel of the same template with
identical bytes and reported as renamed.  Code that differs only in the literal of an
s_add_u32 / s_addc_u32 (a pc-relative displacement to another symbol) is reported as such.
The tuning library's kernels are also held against the parent's product library: the compiler's
output for one kernel can depend on the other instantiations in its translation unit, so a
parent whose two libraries disagree on a kernel is reported, with which of the two the change
matches.
Kernels of the parent that the change no longer has are listed; why each could go is for the
change's own record to say.  Exit status 1 if a kernel of the change has no identical parent
kernel."""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def code_objects(so_path):
    """The gfx950 code objects of a HIP shared library (tests/test_lib_abi.py)."""
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([LLVM + "llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", so_path,
                        os.devnull], check=True, capture_output=True)
        blob = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = [], blob.find(magic)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + 24)[0]
        p = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(magic, pos + 32)
    return out


def kernels_of(co):
    """{mangled name: (code bytes, descriptor bytes)} and the names of the other device functions
    of one ELF64 code object."""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]
    symtab = next((s for s in secs if s[1] == 2), None) or next(s for s in secs if s[1] == 11)
    strtab = secs[symtab[6]]

    def at(addr, size):
        for s in secs:
            if s[1] != 8 and s[3] <= addr and addr + size <= s[3] + s[5] and (s[2] & 2):
                return co[s[4] + addr - s[3]:s[4] + addr - s[3] + size]
        raise ValueError("address %#x not in a section" % addr)

    syms = {}
    for i in range(symtab[5] // 24):
        name, info, _, _, value, size = struct.unpack_from("<IBBHQQ", co, symtab[4] + i * 24)
        end = co.index(b"\0", strtab[4] + name)
        syms[co[strtab[4] + name:end].decode()] = (info & 15, value, size)
    kernels, others = {}, []
    for n, (typ, value, size) in syms.items():
        if typ != 2:
            continue
        if n + ".kd" in syms:
            kd = bytearray(at(syms[n + ".kd"][1], 64))
            kd[16:24] = bytes(8)
            kernels[n] = (at(value, size), bytes(kd))
        else:
            others.append(n)
    return kernels, others


def library(path):
    kernels, others = {}, []
    for co in code_objects(path):
        k, o = kernels_of(co)
        assert not set(k) & set(kernels), "a kernel in two code objects"
        kernels.update(k)
        others += o
    return kernels, others


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    if not filt:
        raise SystemExit("isa_compare: needs c++filt or llvm-cxxfilt")
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def base(dem):
    d = dem[5:] if dem.startswith("void ") else dem
    return d.split("<")[0].split("(")[0]


def displacement_only(a, b):
    """Same length, and every differing dword is the literal of an s_add_u32 / s_addc_u32."""
    if len(a) != len(b):
        return False
    for i in range(0, len(a), 4):
        if a[i:i + 4] == b[i:i + 4]:
            continue
        if i < 4:
            return False
        w, = struct.unpack_from("<I", a, i - 4)
        sop2_add = (w >> 30) == 2 and ((w >> 23) & 0x7F) in (0, 4)
        if not (sop2_add and ((w & 0xFF) == 255 or ((w >> 8) & 0xFF) == 255) and
                a[i - 4:i] == b[i - 4:i]):
            return False
    return True


def kd_fields(kd):
    lds, scratch, kernarg = struct.unpack_from("<III", kd, 0)
    rsrc3, rsrc1, rsrc2 = struct.unpack_from("<III", kd, 44)
    return "lds=%d scratch=%d kernarg=%d rsrc1=%#x rsrc2=%#x rsrc3=%#x" % (
        lds, scratch, kernarg, rsrc1, rsrc2, rsrc3)


def compare(name, old_path, new_path, alt_path=None):
    """alt_path: the parent's product library, as a second reference for the tuning library."""
    old, old_other = library(old_path)
    new, new_other = library(new_path)
    alt = library(alt_path)[0] if alt_path else {}
    dem = demangle(sorted(set(old) | set(new) | set(alt)))
    dem_alt = dem.__getitem__
    as_product = 0
    print("== %s: parent %d kernels, change %d kernels" % (name, len(old), len(new)))
    if old_other or new_other:
        print("   device functions that are not kernels: parent %d, change %d" %
              (len(old_other), len(new_other)))
    bad = 0
    same = renamed = disp = 0
    used = set()
    for n in sorted(new, key=lambda x: dem[x]):
        cands = [n] if n in old else [o for o in old if o not in new and base(dem[o]) == base(dem[n])]
        hit = next((o for o in cands if old[o] == new[n]), None)
        if hit is not None:
            used.add(hit)
            if hit == n:
                same += 1
            else:
                renamed += 1
                print("   renamed, identical: %s\n        was %s" % (dem[n], dem[hit]))
            continue
        if n in old and old[n][1] == new[n][1] and displacement_only(old[n][0], new[n][0]):
            used.add(n)
            disp += 1
            print("   displacement to another symbol only: %s" % dem[n])
            continue
        alt_hit = next((o for o in alt if base(dem_alt(o)) == base(dem[n]) and alt[o] == new[n]),
                       None)
        if alt_hit is not None and (n in old or alt_hit in old):
            # the parent's two libraries already disagreed on this kernel (its tuning copy was
            # compiled beside variants that are gone now); the change's copy is the product's
            used.add(n if n in old else alt_hit)
            as_product += 1
            print("   identical to the parent's PRODUCT-library kernel, not to its tuning copy: %s"
                  % dem[n])
            continue
        bad += 1
        if n in old:
            used.add(n)
            print("   DIFFERS: %s\n        code %d -> %d bytes%s\n        parent %s\n        change %s" % (
                dem[n], len(old[n][0]), len(new[n][0]),
                "" if old[n][0] != new[n][0] else " (identical code, descriptor differs)",
                kd_fields(old[n][1]), kd_fields(new[n][1])))
        else:
            print("   NOT IN PARENT (no identical kernel of that template): %s" % dem[n])
    gone = sorted((o for o in old if o not in used), key=lambda x: dem[x])
    print("   identical %d, renamed but identical %d, displacement only %d, identical to the "
          "parent's product copy only %d, different %d, gone %d" %
          (same, renamed, disp, as_product, bad, len(gone)))
    for o in gone:
        print("   gone: %s" % dem[o])
    return bad


def main():
    parent, change = sys.argv[1:3]
    bad = 0
    for lib in ("libaz_hip.so", "libaz_hip_tuning.so"):
        product = lib == "libaz_hip.so"
        bad += compare(lib, os.path.join(parent, lib), os.path.join(change, lib),
                       None if product else os.path.join(parent, "libaz_hip.so"))
    print("RESULT: %s" % ("every kernel of the change is a parent kernel, byte for byte"
                          if bad == 0 else "%d problems" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
