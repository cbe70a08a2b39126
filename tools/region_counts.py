#!/usr/bin/env python3
"""Instruction-class counts per region of one kernel in a tools/disasm.sh listing.

    tools/disasm.sh reed-solomon-simd_amd/build/rs_mono.hip.o /tmp/mono.s
    python tools/region_counts.py /tmp/mono.s k_mono_denseILi10ELi1ELi0ELb0ELi2E

The symbol is chosen by substring of its mangled name (exactly one must match).  The
kernel's instruction stream, in listing order, is cut at markers the listing itself
shows:
  - the first plain global load (the row loads begin),
  - the first and the last global_load_lds of every run of LDS-DMAs (a run ends at the
    next wait on vmcnt or the next barrier),
  - every s_barrier,
  - the first global store (the epilogue begins).
Per region it prints the number of instructions by opcode prefix -- VALU (v_), SALU
(s_), LDS (ds_), VMEM (global_) -- and, of the VALU, the GF multiply's own opcodes
(v_perm_b32, v_bitop3_b32, v_lshrrev_b64, v_alignbit_b32).  Nothing else is looked for.
"""
import re
import sys

MULT = ("v_perm_b32", "v_bitop3_b32", "v_lshrrev_b64", "v_alignbit_b32")


def kernel_body(path, sub):
    bodies, name = {}, None
    for line in open(path):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif name and line.startswith("\t"):
            ins = line.partition("//")[0].strip()
            if ins:
                bodies[name].append(ins)
    hits = [k for k in bodies if sub in k]
    if len(hits) != 1:
        sys.exit("%d symbols match %r: %s" % (len(hits), sub, hits[:8]))
    return hits[0], bodies[hits[0]]


def cuts(body):
    """[(index, label)]: a region runs from its index to the next one's."""
    out = [(0, "entry")]
    op = [i.split()[0] for i in body]
    plain = next((k for k, o in enumerate(op) if o.startswith("global_load") and "lds" not in o), None)
    if plain is not None:
        out.append((plain, "row loads"))
    k, run, barriers = 0, 0, 0
    store = next((k for k, o in enumerate(op) if o.startswith("global_store")), len(op))
    while k < len(op):
        if "global_load_lds" in op[k]:
            run += 1
            last = k
            j = k + 1
            while j < len(op) and op[j] != "s_barrier" and not (op[j] == "s_waitcnt" and "vmcnt" in body[j]):
                if "global_load_lds" in op[j]:
                    last = j
                j += 1
            out.append((k, "LDS-DMA run %d" % run))
            out.append((last + 1, "after LDS-DMA run %d" % run))
            k = last + 1
            continue
        if op[k] == "s_barrier":
            barriers += 1
            out.append((k, "barrier %d" % barriers))
        if k == store:
            out.append((k, "stores"))
        k += 1
    return sorted(set(out))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    name, body = kernel_body(sys.argv[1], sys.argv[2])
    print(name)
    print("%d instructions" % len(body))
    print("%-26s %6s %6s %9s %6s %6s %6s" % ("region (from)", "insts", "VALU", "GF mult.", "SALU", "LDS", "VMEM"))
    c = cuts(body) + [(len(body), "end")]
    tot = [0] * 6
    for (a, label), (b, _) in zip(c, c[1:]):
        ops = [i.split()[0] for i in body[a:b]]
        row = [len(ops), sum(o.startswith("v_") for o in ops), sum(o in MULT for o in ops),
               sum(o.startswith("s_") for o in ops), sum(o.startswith("ds_") for o in ops),
               sum(o.startswith("global_") for o in ops)]
        tot = [x + y for x, y in zip(tot, row)]
        print("%-26s %6d %6d %9d %6d %6d %6d" % ((label,) + tuple(row)))
    print("%-26s %6d %6d %9d %6d %6d %6d" % (("total",) + tuple(tot)))


if __name__ == "__main__":
    main()
