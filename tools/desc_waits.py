#!/usr/bin/env python3
"""Where k_describe_fused's key-point loop waits, read from its ISA (a reading aid like tools/fast_issue.py, no test).

    python tools/desc_waits.py [--source orb_extractor.hip] [--asm file.s] [--all]

Compiles vieo_slam_amd/csrc/orb_extractor.hip (or --source, e.g. the parent's copy) with build.py's flags plus
--cuda-device-only -S, or reads an assembly file made that way (--asm), and isolates the key-point loop of
k_describe_fused: the largest loop that holds patch loads, the blur's stores and the wave reduction.  It
prints the loop's s_waitcnt, global_load, s_load, ds_read and ds_write lines in layout order under their block labels
(--all: every instruction), then:

  * the vmcnt waits between the issue of the next key point's patch loads (the last global_load_dword in front of the
    horizontal pass's ds_write_b128) and the back edge -- the blocks of the border path (those with global_load_ubyte, which must
    wait to assemble their dwords; one line each in the listing unless --all) are counted apart;
  * the scalar-load waits: s_waitcnt lgkmcnt(..) with at least one s_load issued since the previous one, in the loop and
    in the prologue (entry to loop head);
  * the disc section (IC_Angle): from the end of the horizontal pass (the back edge of the inner loop that holds a
    ds_write_b128, or the last ds_write_b128 if the pass is unrolled) to the first v_add_u32_dpp / swizzle instruction
    of the wave reduction -- its LDS reads, the batches of reads it waits for and its branches.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNEL = "_ZN4vieo16k_describe_fusedE"
SHOWN = ("s_waitcnt", "global_load", "s_load", "ds_read", "ds_write")


def kernel_isa(source):
    from vieo_slam_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "x.s")
        subprocess.check_call([build.HIPCC] + build.FLAGS + ["--cuda-device-only", "-S", source, "-o", out],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def function_lines(text):
    s = text.split("\n")
    a = next(i for i, l in enumerate(s) if "Begin function " + KERNEL in l)
    b = next(i for i in range(a, len(s)) if "End function" in s[i])
    out = []  # (label or None, opcode, text)
    for l in s[a:b]:
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            out.append((m.group(1), None, t))
        elif t and not t.startswith(".") and not t.endswith(":"):
            out.append((None, t.split()[0], t))
    return out


def outer_loop(fn):
    pos = {lab: i for i, (lab, _, _) in enumerate(fn) if lab}
    back = []  # (head, branch) of every backward branch
    for i, (_, op, t) in enumerate(fn):
        if op and (op.startswith("s_cbranch") or op == "s_branch"):
            tgt = t.split()[-1]
            if tgt in pos and pos[tgt] < i:
                back.append((pos[tgt], i))
    # the key-point loop: the largest loop that holds patch loads, the horizontal pass's stores and the wave reduction
    def whole(b):
        ops = [(x[1] or "", x[2]) for x in fn[b[0]:b[1] + 1]]
        return (any(op == "global_load_dword" for op, _ in ops) and any(op == "ds_write_b128" for op, _ in ops)
                and any("row_bcast" in t for _, t in ops))
    head, tail = max((b for b in back if whole(b)), key=lambda b: b[1] - b[0])
    inner = sorted(b for b in back if head < b[0] and b[1] < tail)
    # blocks of the loop that the compiler laid out behind the back edge: they end with a branch back into the loop
    end, i = tail, tail + 1
    while i < len(fn) and fn[i][0]:
        j = i + 1
        while j < len(fn) and not fn[j][0]:
            j += 1
        last = fn[j - 1]
        if last[1] and last[1].startswith(("s_branch", "s_cbranch")) and head <= pos.get(last[2].split()[-1], -1) <= tail:
            end, i = j - 1, j
        else:
            break
    return head, tail, end, inner


def blocks(fn, a, b):
    out, cur = [], ["(entry)", []]
    for i in range(a, b + 1):
        lab, op, t = fn[i]
        if lab:
            if cur[1]:
                out.append(cur)
            cur = [lab, []]
        else:
            cur[1].append((i, op, t))
    if cur[1]:
        out.append(cur)
    return out


def smem_waits(fn, a, b):
    n, pending, where = 0, 0, []
    for i in range(a, b + 1):
        _, op, t = fn[i]
        if not op:
            continue
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            pending += 1
        elif op == "s_waitcnt" and "lgkmcnt" in t and pending:
            n, pending = n + 1, 0
            where.append(i)
    return n, where


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(ROOT, "vieo_slam_amd", "csrc", "orb_extractor.hip"))
    ap.add_argument("--asm")
    ap.add_argument("--all", action="store_true")
    args = ap.parse_args()
    fn = function_lines(open(args.asm).read() if args.asm else kernel_isa(args.source))
    head, tail, end, inner = outer_loop(fn)
    print("key-point loop: %s .. back edge `%s` (%d instructions, %d inner loops)"
          % (fn[head][0], fn[tail][2], sum(1 for x in fn[head:tail + 1] if x[1]), len(inner)))
    bl = blocks(fn, head, end)
    for lab, ins in bl:
        rows = [t for _, op, t in ins if args.all or op.startswith(SHOWN)]
        nb = sum(1 for _, op, _ in ins if op.startswith("global_load_ubyte"))
        if nb and not args.all:
            print("%s: (border path: %d global_load_ubyte, %d s_waitcnt vmcnt)" % (lab, nb, sum(1 for _, op, t in ins if op == "s_waitcnt" and "vmcnt" in t)))
        elif rows:
            print(lab + ":")
            for t in rows:
                print("    " + " ".join(t.split()))
    # ---- the next patch's loads, and the vector-memory waits behind them
    # (the last global_load_dword in front of the horizontal pass: a rotated loop holds the loads twice, for the first
    # key point and for the next one; blocks laid out behind the back edge belong to the run)
    issue = None
    for i in range(head, tail + 1):
        op = fn[i][1]
        if op == "global_load_dword":
            issue = i
        elif op == "ds_write_b128" and issue is not None:
            break
    border = [lab for lab, ins in bl if any(op.startswith("global_load_ubyte") for _, op, _ in ins)]
    vm, vm_border = [], []
    for lab, ins in bl:
        for i, op, t in ins:
            if issue is not None and issue < i <= tail and op == "s_waitcnt" and "vmcnt" in t:
                (vm_border if lab in border else vm).append("%s: %s" % (lab, " ".join(t.split())))
    print("\nsummary")
    print("  patch loads issued: %s" % ("not found" if issue is None else "last global_load_dword of the run is instruction %d of the loop" % (issue - head)))
    print("  vmcnt waits from there to the back edge: %d%s" % (len(vm), "".join("\n      " + x for x in vm)))
    print("  (in the border path's blocks %s: %d)" % (", ".join(border) or "-", len(vm_border)))
    later = [" ".join(t.split()) for lab, ins in bl for i, op, t in ins if issue is not None and issue < i <= tail and op.startswith("global_load") and lab not in border]
    print("  other vector loads behind them: %d%s" % (len(later), "".join("\n      " + x for x in later)))
    n_loop, _ = smem_waits(fn, head, end)
    n_pro, _ = smem_waits(fn, 0, head)
    n_sl = sum(1 for _, op, _ in fn[head:end + 1] if op and op.startswith("s_load"))
    print("  scalar loads in the loop: %d, waits with a scalar load outstanding: %d per trip (prologue: %d)" % (n_sl, n_loop, n_pro))
    # ---- the disc section
    w128 = [i for i in range(head, tail) if fn[i][1] == "ds_write_b128"]
    if w128:
        a = min(((b - h, b) for h, b in inner if h < w128[-1] < b and not any(x[1] == "global_load_dword" for x in fn[h:b])), default=(0, w128[-1]))[1]
        red = next((i for i in range(a, tail) if fn[i][1] and fn[i][1].startswith(("v_add_u32_dpp", "v_add_nc_u32_dpp", "ds_swizzle", "ds_bpermute", "v_permlane"))), tail)
        sec = [x for x in fn[a + 1:red] if x[1]]
        groups, fresh = 0, False  # a wait group = the waits that follow one batch of reads (lgkmcnt(2), (1), (0) drain ONE batch)
        for _, op, t in sec:
            if op.startswith("ds_read"):
                fresh = True
            elif op == "s_waitcnt" and "lgkmcnt" in t and fresh:
                groups, fresh = groups + 1, False
        print("  disc section (%d instructions): %d LDS reads, %d batches of reads waited for (%d lgkmcnt waits), %d branches"
              % (len(sec), sum(1 for _, op, _ in sec if op.startswith("ds_read")), groups,
                 sum(1 for _, op, t in sec if op == "s_waitcnt" and "lgkmcnt" in t),
                 sum(1 for _, op, _ in sec if op.startswith(("s_cbranch", "s_branch")))))


if __name__ == "__main__":
    main()
