"""Static check of the hand-counted inline-asm load rings (csrc/token_block.hip tb_gemm, csrc/wgrad_planes.hip): in the compiler's assembly, no
instruction may touch the destination registers of an inline-asm global_load between the load and the inline-asm `s_waitcnt vmcnt(N)` that
guarantees it has landed (vector memory operations retire in order: after vmcnt(N) only the N youngest may be outstanding, so a load with at
least N operations issued after it is complete) -- the compiler believes an asm output is valid immediately, so a spill or copy of an in-flight
register would silently read stale data.

What counts as "issued after it", conservatively (an undercount only makes a wait look too weak, never too strong):
  * every inline-asm global_load_dword* (the fragment loads, and the dwordx2 row requests of the forward's S4);
  * every other vector memory instruction -- stores count in vmcnt on CDNA, and so do the compiler's own loads and the LDS-DMA copies -- but
    ONLY where it is issued unconditionally on the path from the load to the wait: an instruction behind a forward branch that has not yet
    reached its target (a store under `if (!(dbg & 1))`, a null-pointer test, a tile-range test) may be skipped and counts as zero.  A backward
    branch or a label that was not announced by a forward branch (a loop, a join from elsewhere) ends the counting of such instructions for
    good: from there on only the inline-asm loads count.
usage: python tools/check_asm_ring.py file.s"""
import re
import sys

VMEM = ("global_load", "global_store", "global_atomic", "buffer_load", "buffer_store", "buffer_atomic", "scratch_load", "scratch_store",
        "flat_load", "flat_store", "flat_atomic")


def regs_of(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        if m.group(1) is not None:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.add(int(m.group(3)))
    return out


def check(path):
    lines = open(path).read().split("\n")
    ins = []            # (line no, text, in_asm)
    in_asm, kernel = False, None
    bad = 0
    for no, l in enumerate(lines, 1):
        s = l.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if re.match(r"^_Z\w+:", s):
            kernel = s[:-1]
            ins.append((no, "@kernel " + kernel, False))
            continue
        m = re.match(r"^(\.?\w+):", s)
        if m and not in_asm:
            ins.append((no, "@label " + m.group(1), False))
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        ins.append((no, s.split(";")[0].strip(), in_asm))
    label_at = {t[7:]: k for k, (_, t, _) in enumerate(ins) if t.startswith("@label")}
    n_loads = 0
    for i, (no, text, asm) in enumerate(ins):
        if text.startswith("@kernel"):
            kernel = text[8:]
        if not (asm and text.startswith("global_load_dword")):
            continue
        n_loads += 1
        dest = regs_of(text.split(",")[0])
        younger = 0
        pending = set()         # targets of forward branches passed and not yet reached: inside, an instruction may be skipped
        straight = True         # False once control flow was met that the above does not describe
        for no2, t2, asm2 in ins[i + 1:]:
            if t2.startswith("@kernel") or t2.startswith("s_endpgm"):
                print(f"{path}:{no}: load {text.split(',')[0]} never guarded before the end of {kernel}")
                bad += 1
                break
            if t2.startswith("@label"):
                if t2[7:] in pending:
                    pending.discard(t2[7:])
                else:
                    straight = False
                continue
            if asm2 and t2.startswith("global_load_dword"):
                if regs_of(t2.split(",")[0]) & dest:
                    print(f"{path}:{no2}: ring register reloaded before its previous load was guarded (issued at line {no})")
                    bad += 1
                    break
                younger += 1
                continue
            m = re.match(r"s_waitcnt vmcnt\((\d+)\)", t2)
            if asm2 and m:
                if younger >= int(m.group(1)):
                    break
                continue
            if regs_of(t2) & dest:
                print(f"{path}:{no2}: `{t2}` touches {sorted(regs_of(t2) & dest)} of the in-flight load at line {no} ({kernel})")
                bad += 1
                break
            m = re.match(r"s_c?branch\w*\s+(\.?\w+)", t2)
            if m:
                # (a target at or before the load is a backward branch; one ahead is remembered until its label)
                if label_at.get(m.group(1), len(ins)) <= i:
                    straight = False
                else:
                    pending.add(m.group(1))
                continue
            if t2.startswith(("s_setpc", "s_swappc", "s_call")):
                straight = False
                continue
            if t2.startswith(VMEM) and straight and not pending:
                younger += 1
    print(f"{path}: {n_loads} inline-asm loads checked, {bad} violations")
    return bad


if __name__ == "__main__":
    sys.exit(1 if sum(check(p) for p in sys.argv[1:]) else 0)
