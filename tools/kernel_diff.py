#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the same translation unit, kernel by kernel: the code-object metadata
(registers, spills, scratch, LDS, kernel-argument size) and the disassembly.  Only reads object files.

usage: kernel_diff.py [-v] [--rename REGEX REPL]... BEFORE.o AFTER.o [more pairs ...]

--rename REGEX REPL: re.sub applied to the mangled kernel names of AFTER before pairing, for kernels that gained a
template parameter (e.g. a trailing `false`: --rename 'Lb0E(EEvNS_\d+\w+ParamsE)$' '\1') or moved to a shared name; may be
given several times, each applied in turn; kernels of AFTER that then have no partner in BEFORE are counted as new, not as
a difference.

Per kernel, one of
  identical   the instruction text is the same (addresses and encodings stripped)
  renamed     the same mnemonics in the same order with operands of the same kinds; what differs is register numbers
              and / or the literal offsets of scalar loads (s_load_*: kernel arguments that moved inside their struct).
              Renaming is not checked for consistency: read the printed diff of a kernel you care about.
  changed     anything else: its registers, LDS and instruction count in both builds are printed, with -v its unified
              diff too
and a line for every metadata note that differs."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
NOTES = ["vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
         "group_segment_fixed_size", "kernarg_segment_size"]


def code_object(obj, td, tag):
    fat, co = os.path.join(td, tag + ".fat"), os.path.join(td, tag + ".co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    return co


def notes_of(co):
    text = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in NOTES}
    return out


def kernels_of(co):
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                          text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip() or line.strip() == "...":      # "...": zero padding up to the next kernel's alignment
            continue
        cur.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())
    return out


REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")


def shape(ins):
    def reg(m):
        r = m.group(2)
        n = 1 if r[0] != "[" else int(r[1:-1].split(":")[1]) - int(r[1:-1].split(":")[0]) + 1
        return f"{m.group(1)}#{n}"
    s = REG.sub(reg, ins)
    if s.startswith("s_load_"):
        s = re.sub(r"(0x[0-9a-f]+|\b\d+)$", "OFF", s)
        s = re.sub(r"offset:\S+", "OFF", s)
    return s


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"\(anonymous namespace\)::|^void ", "", d) for n, d in zip(names, out)}


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    rename = []
    while "--rename" in args:
        k = args.index("--rename")
        rename.append((re.compile(args[k + 1]), args[k + 2]))
        del args[k:k + 3]
    if not args or len(args) % 2:
        sys.exit(__doc__)
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        for before, after in zip(args[::2], args[1::2]):
            ca, cb = code_object(before, td, "a"), code_object(after, td, "b")
            na, nb = notes_of(ca), notes_of(cb)
            ka, kb = kernels_of(ca), kernels_of(cb)
            if rename:
                paired = {}
                for n in nb:
                    r = n
                    for rx, repl in rename:
                        r = rx.sub(repl, r)
                    paired[r] = n
                new = sorted(n for r, n in paired.items() if r not in na)
                nb = {r: nb[n] for r, n in paired.items() if r in na}
                kb = {r: kb[n] for r, n in paired.items() if r in na}
            names = sorted(na)
            dem = demangle(names)
            tally = {"identical": [], "renamed": [], "changed": []}
            print(f"== {os.path.basename(after)}: {len(na)} kernels before, {len(nb)} after")
            if rename:
                print(f"   new in the second build: {len(new)} kernels")
            for n in sorted(set(na) ^ set(nb)):
                print(f"   only in one build: {n}")
                bad += 1
            for n in names:
                if n not in nb:
                    continue
                for k in NOTES:
                    if na[n][k] != nb[n][k]:
                        print(f"   {dem[n]}: {k} {na[n][k]} -> {nb[n][k]}")
                        bad += k != "kernarg_segment_size"
                a, b = ka[n], kb[n]
                kind = "identical" if a == b else "renamed" if [shape(i) for i in a] == [shape(i) for i in b] else "changed"
                tally[kind].append(dem[n])
                if kind == "changed":
                    print(f"   {dem[n]}: vgpr {na[n]['vgpr_count']} -> {nb[n]['vgpr_count']}, sgpr {na[n]['sgpr_count']} -> "
                          f"{nb[n]['sgpr_count']}, LDS {na[n]['group_segment_fixed_size']} -> {nb[n]['group_segment_fixed_size']}, "
                          f"scratch {na[n]['private_segment_fixed_size']} -> {nb[n]['private_segment_fixed_size']}, "
                          f"instructions {len(a)} -> {len(b)}")
                if kind == "changed" and verbose:
                    print("\n".join(difflib.unified_diff(a, b, "before", "after", lineterm="", n=2)))
            print("   " + ", ".join(f"{k} {len(v)}" for k, v in tally.items()))
            for d in tally["changed"]:
                print(f"   changed: {d}")
            bad += len(tally["changed"])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
