#!/usr/bin/env python3
"""Per-kernel code hashes and resource usage of the library's kernel objects, for "did this change touch a kernel that exists" questions.

    python tools/kernel_code_hashes.py [build-dir] > hashes.txt          # one line per kernel of every object that holds device code
    python tools/kernel_code_hashes.py --diff before.txt after.txt       # kernels whose code changed / disappeared / appeared

For every object in the build directory (default easyhybrid.jl_amd/csrc/build) the gfx950 code object is taken out of the .hip_fatbin
section (llvm-objcopy, clang-offload-bundler) and every kernel -- the FUNC symbols that have a kernel descriptor `<name>.kd` -- is hashed
over the bytes of its code in .text (md5), which is position independent.  Next to the hash: code bytes, VGPRs, AGPRs, SGPRs, scratch
bytes, static LDS bytes and the waves per SIMD the register count allows (512 VGPRs per SIMD lane on gfx950, accumulation registers
included, allocated in blocks of 8) from the code object's metadata.  Dynamic LDS is chosen at launch and is not in the object.  Runs
without a GPU."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("EH_LLVM_BIN", "/opt/rocm/llvm/bin")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stdout


def code_object(obj, tmp):
    fb, co = os.path.join(tmp, "fb.bin"), os.path.join(tmp, "co.elf")
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb)
    if not os.path.exists(fb) or os.path.getsize(fb) == 0:
        return None
    targets = run(f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fb}", "--list").decode().split()
    dev = [t for t in targets if "amdgcn" in t]
    if not dev:
        return None
    run(f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fb}", f"--output={co}", f"--targets={dev[0]}", "--unbundle")
    return co


def kernels_of(co):
    """[(demangled name, md5 of the code, code bytes, resources...)] of one code object"""
    elf = open(co, "rb").read()
    sec = run(f"{LLVM}/llvm-readelf", "-S", "-W", co).decode()
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    if not m:
        return []
    addr, off = int(m.group(1), 16), int(m.group(2), 16)
    syms = run(f"{LLVM}/llvm-readelf", "-s", "-W", co).decode().splitlines()
    funcs, kds = {}, set()
    for ln in syms:
        p = ln.split()
        if len(p) < 8:
            continue
        if p[3] == "FUNC":
            funcs[p[7]] = (int(p[1], 16), int(p[2]))
        elif p[3] == "OBJECT" and p[7].endswith(".kd"):
            kds.add(p[7][:-3])
    notes = run(f"{LLVM}/llvm-readelf", "--notes", co).decode()
    meta = {}
    for blk in re.split(r"\n\s*- \.", "\n" + notes):
        nm = re.search(r"\.name:\s+(\S+)", "." + blk)
        if not nm:
            continue
        get = lambda k: (re.search(r"\." + k + r":\s+(\d+)", "." + blk) or [None, "-1"])[1]
        meta[nm.group(1).strip("'\"")] = tuple(int(get(k)) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    names = sorted(kds & set(funcs))
    filt = next((f for f in (f"{LLVM}/llvm-cxxfilt", shutil.which("c++filt") or "") if f and os.path.exists(f)), None)
    dem = subprocess.run([filt], input="\n".join(names).encode(), check=True, stdout=subprocess.PIPE).stdout.decode().splitlines() if names and filt else names
    out = []
    for n, d in zip(names, dem):
        a, size = funcs[n]
        body = elf[off + a - addr: off + a - addr + size]
        v, ag, s, scr, lds = meta.get(n, (-1,) * 5)
        regs = max(v, 0) + max(ag, 0)
        waves = min(8, 512 // max(8, (regs + 7) // 8 * 8)) if v >= 0 else -1
        out.append((re.sub(r"^void ", "", d).replace("(EhNet, EhStepArgs)", ""), hashlib.md5(body).hexdigest(), size, v, ag, s, scr, lds, waves))
    return out


def dump(build):
    print("# object | kernel | md5 of the code | code bytes | VGPRs AGPRs SGPRs | scratch bytes | static LDS bytes | waves per SIMD")
    with tempfile.TemporaryDirectory() as tmp:
        for fn in sorted(os.listdir(build)):
            if not fn.endswith(".o"):
                continue
            co = code_object(os.path.join(build, fn), tmp)
            if co is None:
                continue
            for k in kernels_of(co):
                print(f"{fn} | {k[0]} | {k[1]} | {k[2]} | {k[3]} {k[4]} {k[5]} | {k[6]} | {k[7]} | {k[8]}")
            os.remove(co)


def diff(a, b):
    def load(p):
        d = {}
        for ln in open(p):
            if ln.startswith("#") or "|" not in ln:
                continue
            f = [x.strip() for x in ln.split("|")]
            d[(f[0], f[1])] = f[2]
        return d
    A, B = load(a), load(b)
    changed = sorted(k for k in A if k in B and A[k] != B[k])
    gone, new = sorted(k for k in A if k not in B), sorted(k for k in B if k not in A)
    print(f"{len(A)} kernels before, {len(B)} after: {len(A) - len(changed) - len(gone)} with identical code, {len(changed)} changed, {len(gone)} gone, {len(new)} new")
    for tag, ks in (("changed", changed), ("gone", gone), ("new", new)):
        for k in ks:
            print(f"  {tag}: {k[0]} | {k[1]}")
    return 1 if changed or gone else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "easyhybrid.jl_amd", "csrc", "build"))
