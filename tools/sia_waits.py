"""Diagnostic (no GPU needed): where a kernel of sia.hip waits for vector memory, read from the gfx950 assembly that
`hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -save-temps -c sia.hip` leaves
(sia-hip-amdgcn-amd-amdhsa-gfx950.s). Per basic block of the kernel, in program order: runs of global loads (`16L`),
global stores (`2S`) and every `s_waitcnt vmcnt(k)` (`W0`, `W3`, ...). A wait that follows loads whose addresses
needed an earlier wait's data is a dependent round trip; a block's `L` runs between two `W` are in flight together.
Usage: sia_waits.py file.s [waves mode]      (default: 1 2, the batched one-wave shape)"""
import re
import sys

path = sys.argv[1]
waves, mode = (sys.argv[2], sys.argv[3]) if len(sys.argv) > 3 else ("1", "2")
kernel = f"_ZN3svo13sia_gn_kernelILi{waves}ELi{mode}EEEvPKNS_7SiaArgsEii"
lines = open(path).read().splitlines()
start = next(k for k, ln in enumerate(lines) if ln.startswith(kernel + ":"))
blocks, cur = [], ["entry", []]
for ln in lines[start + 1:]:
    t = ln.strip()
    if t.startswith(".Lfunc_end"):
        break
    t = t.split(";")[0].strip()
    m = re.match(r"(\.LBB\d+_\d+):", t)
    if m:
        blocks.append(cur)
        cur = [m.group(1), []]
        continue
    op = t.split()[0] if t else ""
    if op.startswith("global_load"):
        cur[1].append("L")
    elif op.startswith("global_store"):
        cur[1].append("S")
    elif op == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", t)
        if m:
            cur[1].append("W" + m.group(1))
    elif op == "s_cbranch_execz" or op == "s_cbranch_scc0" or op == "s_cbranch_scc1" or op == "s_cbranch_vccnz" \
            or op == "s_cbranch_vccz" or op == "s_cbranch_execnz" or op == "s_branch":
        cur[1].append("->" + t.split()[1])
blocks.append(cur)
n_load = n_wait = 0
for name, ev in blocks:
    if not any(e[0] in "LSW" for e in ev):
        continue
    out, k = [], 0
    while k < len(ev):
        e = ev[k]
        if e in ("L", "S"):
            j = k
            while j < len(ev) and ev[j] == e:
                j += 1
            out.append(f"{j - k}{e}")
            n_load += (j - k) if e == "L" else 0
            k = j
        else:
            n_wait += e[0] == "W"
            out.append(e)
            k += 1
    print(f"{name:12s} {' '.join(out)}")
print(f"{kernel}: {n_load} global loads, {n_wait} s_waitcnt vmcnt in the code")
