#!/usr/bin/env python3
"""Compare two `hipcc -S --cuda-device-only` outputs of one translation unit, kernel by kernel (CPU only).

    python tools/isa_diff.py parent/gemv_mfma.s branch/gemv_mfma.s

Per kernel (matched by mangled name) it prints EQUAL, or what differs among
  * VGPR / AGPR / SGPR counts, scratch and LDS bytes, occupancy, the number of MFMA instructions;
  * the ordered mnemonics (with the `nt` flag) of every global_*, ds_*, scratch_*, buffer_*, s_load* instruction and s_barrier;
  * the ordered s_waitcnt instructions with their operands.
Code length, register names and commuted operands are not compared. Exit status 1 when any kernel differs or exists on one side only.
These are the criteria of profiles/seg_gemv_refactor_ab.md."""
import re
import sys

META = (("vgpr", r"\.vgpr_count:\s+(\d+)"), ("agpr", r"\.agpr_count:\s+(\d+)"), ("sgpr", r"\.sgpr_count:\s+(\d+)"),
        ("scratch", r"\.private_segment_fixed_size:\s+(\d+)"), ("lds", r"\.group_segment_fixed_size:\s+(\d+)"))
MEMOP = re.compile(r"^\s+((?:global_|ds_|scratch_|buffer_|s_load)\w+|s_barrier)\b([^\n;]*)", re.M)
WAIT = re.compile(r"^\s+(s_waitcnt[^\n;]*)", re.M)


def kernels(path):
    """mangled name -> {'meta': {...}, 'mem': [...], 'wait': [...]}"""
    asm = open(path).read()
    out = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", asm, re.S | re.M):   # one metadata entry per kernel
        name = re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)
        out[name] = {"meta": {k: int(re.search(rx, m.group(0)).group(1)) for k, rx in META}}
    if not out:
        sys.exit(f"{path}: no kernel metadata (.agpr_count entries): is it the output of hipcc -S --cuda-device-only?")
    for name, k in out.items():
        start = asm.find("\n" + name + ":")
        end = asm.find(".Lfunc_end", start)
        occ = re.compile(r"; Occupancy:\s+(\d+)").search(asm, end)                 # the kernel info behind the body
        if start < 0 or end < 0 or not occ:
            sys.exit(f"{path}: kernel {name}: no body, .Lfunc_end or '; Occupancy:' line found (another assembly layout?)")
        body = asm[start:end]
        k["meta"]["occupancy"] = int(occ.group(1))
        k["meta"]["mfma"] = len(re.findall(r"^\s+v_mfma_", body, re.M))
        k["mem"] = [op + (" nt" if re.search(r"\bnt\b", rest) else "") for op, rest in MEMOP.findall(body)]
        k["wait"] = [" ".join(w.split()) for w in WAIT.findall(body)]
    return out


def first_diff(a, b):
    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"{len(a)} -> {len(b)} entries, first difference at {i}: {a[i] if i < len(a) else '-'} | {b[i] if i < len(b) else '-'}"


def compare(p, b):
    diffs = [f"{k} {p['meta'][k]} -> {b['meta'][k]}" for k in p["meta"] if p["meta"][k] != b["meta"][k]]
    for what in ("mem", "wait"):
        if p[what] != b[what]:
            diffs.append(f"{what} sequence {first_diff(p[what], b[what])}")
    return diffs


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    P, B = kernels(argv[0]), kernels(argv[1])
    bad = 0
    for name in sorted(set(P) | set(B)):
        if name not in P or name not in B:
            print(f"{name}: only in {'the second' if name not in P else 'the first'} file")
            bad += 1
            continue
        diffs = compare(P[name], B[name])
        bad += bool(diffs)
        print(f"{name}: " + ("EQUAL" if not diffs else "; ".join(diffs)))
    print(f"{len(set(P) | set(B))} kernels, {bad} not equal")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
