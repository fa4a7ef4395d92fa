#!/usr/bin/env python3
"""Instructions EXECUTED on one path through a kernel's hot loop, from hipcc's -S output (see tools/kernel_resources.py for the
compile line) -- what tools/isa_mix.py cannot say of a loop that holds several wave-uniform cases side by side.

    python tools/isa_path.py /tmp/epiekf.s 'eks_bwd_lane6<0, 40, 1>' [DECISIONS] [--all-in]

Walks the largest inner loop from its header until it branches back (or leaves).  A branch on the exec mask behind a NaN test
(v_cmp_u) is followed as "some lane is active", behind any other compare (the slope interval) as "no lane is" (--all-in: "some lane
is").  Every other conditional branch takes the next letter of DECISIONS, T (taken) or N; when the letters run out the walk stops
and prints the branches it asked about with the three instructions ahead of each, so that the string can be extended by reading
what each one tests.  The paths quoted in DESIGN.md 4.2 (steady state: results pending, n_npi = 12, k > k_to, rank word >= 0):
    this commit   historic NTNTTNTNTNNNNNTTTN   horizon NTNTNTNNNNNTTTN
    its parent    historic NTNTTNNNNNNTN        horizon NTNTNNTNNNNNN"""
import re
import subprocess
import sys

CLASSES = [("fp64 arith", ("v_fma_f64", "v_mul_f64", "v_add_f64")), ("agpr move", ("v_accvgpr",)), ("cmp/select", ("v_cmp", "v_cndmask")),
           ("valu other", ("v_",)), ("branch", ("s_cbranch", "s_branch")), ("s_waitcnt", ("s_waitcnt",)), ("s_nop", ("s_nop",)),
           ("salu", ("s_",)), ("lds", ("ds_",)), ("vmem", ("buffer_", "global_", "flat_", "scratch_"))]


def main():
    path, want = sys.argv[1], sys.argv[2]
    dec = list(sys.argv[3]) if len(sys.argv) > 3 and not sys.argv[3].startswith("--") else []
    all_in = "--all-in" in sys.argv
    lines = open(path).read().split("\n")
    starts = [(i, m.group(1)) for i, l in enumerate(lines) if (m := re.match(r"^(_Z\w+):", l))]
    names = subprocess.run(["c++filt"] + [s[1] for s in starts], capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=60).stdout.split("\n")
    sel = [s for s, n in zip(starts, names) if want in n.replace("epi::", "")]
    if not sel:
        sys.exit("no kernel matches " + want)
    i0 = sel[0][0]
    body = lines[i0:next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))]
    blocks, cur = [], ("entry", [], "")
    for k, l in enumerate(body[1:], 1):
        if m := re.match(r"^(\.LBB\d+_\d+):(.*)", l):
            blocks.append(cur)
            cur = (m.group(1), [], m.group(2) + body[k + 1])
        elif l.startswith("\t") and not l.strip().startswith((".", ";")):
            cur[1].append(l.strip())
    blocks.append(cur)
    idx = {b[0]: k for k, b in enumerate(blocks)}
    # the inner loop with the most blocks: its header, and the last block that names it
    heads = [b[0] for b in blocks if "Inner Loop Header" in b[2]]
    extent = {h: [k for k, b in enumerate(blocks) if "Header=" + h[2:] + " " in b[2] + " "] for h in heads}
    head = max(heads, key=lambda h: len(extent[h]))
    lo, hi = idx[head], max(extent[head])
    k, hist, asked, cnt, total = lo, [], [], {}, 0
    while True:
        nxt = k + 1
        for i in blocks[k][1]:
            total += 1
            hist.append(i)
            op = i.split()[0]
            c = next(c for c, pre in CLASSES + [("other", ("",))] if op.startswith(pre))
            cnt[c] = cnt.get(c, 0) + 1
            if op == "s_branch":
                nxt = idx[i.split()[1]]
                break
            if op.startswith("s_cbranch"):
                cmps = [h for h in hist[-12:-1] if h.startswith("v_cmp")]
                if op in ("s_cbranch_execz", "s_cbranch_execnz") and cmps:
                    take = (cmps[-1].startswith("v_cmp_u_") or all_in) == (op == "s_cbranch_execnz")
                else:
                    asked.append((blocks[k][0], i, hist[-4:-1]))
                    if not dec:
                        print("out of decisions after %d instructions; asked so far:" % total)
                        for a in asked:
                            print("  %-12s %-28s after  %s" % (a[0], a[1], " ; ".join(a[2])))
                        sys.exit(1)
                    take = dec.pop(0) == "T"
                if take:
                    nxt = idx.get(i.split()[1], -1)
                    break
        if nxt <= lo or nxt > hi:
            break
        k = nxt
    print("%s: %d instructions executed from %s until the loop %s" % (want, total, head, "branches back" if nxt == lo else "is left"))
    for c, n in sorted(cnt.items(), key=lambda x: -x[1]):
        print("  %-12s %5d" % (c, n))


if __name__ == "__main__":
    main()
