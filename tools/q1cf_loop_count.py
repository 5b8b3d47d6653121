#!/usr/bin/env python3
"""Instruction counts of the closed-form 2-D Q1 kernel's main loop, from the assembly of poisson2d_q1_cf.hip:

    hipcc <FLAGS of diffnet_amd/build.py> --cuda-device-only -S diffnet_amd/csrc/poisson2d_q1_cf.hip -o cf.s
    python tools/q1cf_loop_count.py cf.s [substring of the mangled kernel name ...]

Per kernel: VGPRs, scratch bytes, and for the two-row march (the natural loop, by the compiler's "Loop Header" annotations, that both
loads node rows and stores result rows) the number of VALU instructions, loads, stores and barriers in the loop's text."""
import re
import sys


def kernels(lines):
    name, start = None, 0
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w*poisson2d_q1_cf_kernel\w*):", ln)
        if m:
            name, start = m.group(1), i
        elif name and ln.startswith(".Lfunc_end"):
            yield name, start, i
            name = None


def meta(lines, name):
    out = {}
    for i, ln in enumerate(lines):
        if ln.startswith("\t.amdhsa_kernel " + name):
            for l2 in lines[i:i + 80]:
                m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size|accum_offset)\s+(\d+)", l2)
                if m:
                    out[m.group(1)] = int(m.group(2))
            break
    return out


def main():
    lines = open(sys.argv[1]).read().split("\n")
    want = sys.argv[2:]
    for name, a, b in kernels(lines):
        if want and not any(w in name for w in want):
            continue
        labels, back = {}, []               # label -> (line, its comment); branches to a label at or above them (line, target)
        for i in range(a, b):
            m = re.match(r"^(\.LBB\d+_\d+):(.*)", lines[i])
            if m:
                labels[m.group(1)] = (i, m.group(2))
                continue
            m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[i])
            if m and m.group(1) in labels:
                back.append((i, m.group(1)))
        best = None
        for h, (hl, note) in labels.items():
            if "Loop Header" not in note:
                continue
            # the loop's blocks by the compiler's annotations (the latch may be laid out above the header), closed by its last backward branch;
            # scalar-only blocks directly above it that a backward branch from inside reaches (the rotated priority switch) belong to it as well
            tag = h[2:]                       # "BBn_m"
            member = {l for l, (_, c) in labels.items() if l == h or ("Header=" + tag) in c or ("Parent Loop " + tag) in c}
            # a block = its label's line up to the next label; the loop's text = its blocks, wherever the compiler laid them out
            order = sorted(v[0] for v in labels.values()) + [b]
            nxt = {order[i]: order[i + 1] for i in range(len(order) - 1)}
            spans = sorted((labels[l][0], nxt[labels[l][0]]) for l in member)
            start = spans[0][0]
            inside = lambda i: any(lo <= i < hi for lo, hi in spans)
            for t in sorted({labels[t][0] for i, t in back if inside(i) and labels[t][0] < start}):
                between = [l.strip() for l in lines[t:start] if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;")]
                if all(l.startswith("s_") and not l.startswith("s_barrier") for l in between):      # scalar control only: the rotated priority switch
                    spans.insert(0, (t, start))
                    break
            body = [l.strip() for lo, hi in spans for l in lines[lo:hi] if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;")]
            # the march is the kernel's one loop that loads node rows AND stores result rows (the hand-over polls of the chained strips and
            # the loops of the final reduction do at most one of the two); the largest, should the compiler ever split it
            ld = any(re.match(r"(global|buffer|flat)_load", l) for l in body)
            st = any(re.match(r"(global|buffer|flat)_store", l) for l in body)
            if ld and st and (best is None or len(body) > len(best)):
                best = body
        md = meta(lines, name)
        m = re.search(r"kernelILi(\d)ELb(\d)ELi(\d+)ELi(\d)E", name)
        if m:
            name = "E=%s vec=%s FL=%s W=%s" % m.groups()
        if best is None:
            print(f"{name}: vgpr {md.get('next_free_vgpr')} scratch {md.get('private_segment_fixed_size')} | march loop not identified")
            continue
        valu = sum(1 for l in best if l.startswith("v_") and not l.startswith("v_nop"))
        ld = sum(1 for l in best if re.match(r"(global|buffer|flat)_load", l))
        ld4 = sum(1 for l in best if re.match(r"(global|buffer|flat)_load_dwordx4", l))
        st = sum(1 for l in best if re.match(r"(global|buffer|flat)_store", l))
        bar = sum(1 for l in best if l.startswith("s_barrier"))
        salu = sum(1 for l in best if l.startswith("s_"))
        print(f"{name}: vgpr {md.get('next_free_vgpr')} scratch {md.get('private_segment_fixed_size')} | loop: {len(best)} instr, VALU {valu}, "
              f"loads {ld} ({ld4} x4), stores {st}, barriers {bar}, SALU {salu}")


if __name__ == "__main__":
    main()
