"""Per-basic-block instruction counts of one kernel's step loop (static, from the device assembly).

  python tools/loop_regions.py [--kernel SUBSTR] [--src FILE.hip] [--asm FILE.s] [--json OUT]

Compiles SRC to device assembly with the build's flags (hipcc -S --cuda-device-only, ~30 s for one rollout translation unit)
unless --asm names an existing .s, finds the kernel whose mangled name contains SUBSTR and takes its step loop: the backward-branch
region holding the most instructions.  Every basic block of it is printed with its VALU, LDS, 32-bit multiply (v_mul_lo_u32 /
v_mul_hi_u32 / v_mad_*) and DPP counts.  A block is tagged `search` when it lies between the loop's first `s_setprio 2` and its
last `s_setprio 0` (d3_search's priority raise and drop, ewn_step_d3.hpp), else `step`.  The step blocks are what the env step
costs outside the opponent's search; blocks a wave takes only rarely (auto-reset, a rejected Lemire draw) are counted there too,
so the `step` total is an upper bound of what an iteration issues outside the search.  Blocks laid out behind the loop's latch that
jump back into it (a branch marked unlikely, e.g. the one cold block of LaneRng::step_dice) are tagged `cold` and totalled apart.
A block with >= 10 32-bit multiplies is a Philox-4x32-10 block (ten rounds of one 64-bit multiply in the pair form, of two in the one-lane form; sources that still issue
the high and low halves separately have 20 and 40): the first one in the loop is prime() at step start (noted `prime`), every later one (noted `refill`) is
reached only when a Lemire draw is rejected, with probability <= 6 / 2^32 per draw.  `step_common` is the step total without the
refills.  These are static counts, not measurements.

The default kernel is the benchmark's: k_rollout_slots<5, 2, 0, 1, false, 1>."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_mix import MUL32, kernel_body  # noqa: E402

DEFAULT_KERNEL = "_Z15k_rollout_slotsILi5ELi2ELi0ELi1ELb0ELi1EEv7RollCfg7RollBuf"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-S", "--cuda-device-only"]
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


def blocks_of(body):
    """[(label, [(op, text)])] in layout order; the kernel's entry block is labelled 'entry'"""
    out = [["entry", []]]
    for l in body:
        s = l.strip()
        m = LABEL.match(s)
        if m:
            out.append([m.group(1), []])
            continue
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        out[-1][1].append((op, s))
        if op.startswith("s_cbranch") or op == "s_branch":  # a branch ends a block; the fall-through is <label>+n
            base = out[-1][0].split("+")[0]
            n = int(out[-1][0].split("+")[1]) + 1 if "+" in out[-1][0] else 1
            out.append(["%s+%d" % (base, n), []])
    return [b for b in out if b[1]]


def counts(insts):
    c = {"valu": 0, "lds": 0, "mul": 0, "dpp": 0, "salu": 0, "vmem": 0, "all": len(insts)}
    for op, text in insts:
        if op.startswith("v_"):
            c["valu"] += 1
            base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
            if base in MUL32:
                c["mul"] += 1
            if op.endswith("_dpp") or " quad_perm:" in text or " row_" in text:
                c["dpp"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
    return c


def step_loop(blocks):
    """(first, last, hot_last) block index: the largest backward-branch region, widened by every backward-branch region that
    overlaps it.  Out-of-line blocks that the compiler lays out behind the loop's latch and that jump back into the loop (a branch
    marked unlikely) are such an overlapping region: hot_last is the latch, the last block of the region that starts first, and
    the blocks behind it are the loop's cold tail.  Without such blocks hot_last == last."""
    where = {lab: i for i, (lab, _) in enumerate(blocks)}
    size = [len(b[1]) for b in blocks]
    regions = []
    for i, (_, insts) in enumerate(blocks):
        for op, text in insts:
            if op.startswith("s_cbranch") or op == "s_branch":
                tgt = text.split()[-1]
                if tgt in where and where[tgt] <= i:
                    regions.append((sum(size[where[tgt]:i + 1]), where[tgt], i))
    if not regions:
        raise SystemExit("no loop in this kernel")
    _, lo, hi = max(regions)
    grown = True
    while grown:
        grown = False
        for _, a, b in regions:
            if a <= hi and b >= lo and (a < lo or b > hi):
                lo, hi, grown = min(lo, a), max(hi, b), True
    return lo, hi, max(b for _, a, b in regions if a == lo)


def analyse(blocks):
    lo, hi, hot = step_loop(blocks)
    loop = blocks[lo:hi + 1]
    # the search: from the block of the first priority raise to the block of the last priority drop
    raise_at = [i for i, (_, ins) in enumerate(loop) if any(t.startswith("s_setprio 2") for _, t in ins)]
    drop_at = [i for i, (_, ins) in enumerate(loop) if any(t.startswith("s_setprio 0") for _, t in ins)]
    s0 = raise_at[0] if raise_at else len(loop)
    s1 = drop_at[-1] if drop_at else -1
    rows = []
    seen_philox = False
    for i, (lab, ins) in enumerate(loop):
        c = counts(ins)
        c["label"] = lab
        c["region"] = "search" if s0 <= i <= s1 else "cold" if lo + i > hot else "step"
        c["note"] = ""
        if c["region"] == "cold" and c["mul"] >= 10:
            c["note"] = "refill"
        if c["region"] == "step" and c["mul"] >= 10:    # a Philox-4x32-10 block: 10 64-bit multiplies (pair form) or 20
            c["note"] = "refill" if seen_philox else "prime"
            seen_philox = True
        rows.append(c)
    keys = ("valu", "lds", "mul", "dpp", "salu", "vmem", "all")
    tot = {reg: {k: sum(r[k] for r in rows if r["region"] == reg) for k in keys} for reg in ("search", "step", "cold")}
    tot["step_common"] = {k: sum(r[k] for r in rows if r["region"] == "step" and r["note"] != "refill") for k in keys}
    return rows, tot


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel", default=DEFAULT_KERNEL, help="substring of the mangled kernel name")
    ap.add_argument("--src", default=os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_rollout_s5.hip"))
    ap.add_argument("--asm", default=None, help="an existing device assembly file (skips the compile)")
    ap.add_argument("--json", default=None, help="also write the per-block table and the totals here")
    a = ap.parse_args()
    asm = a.asm
    if asm is None:
        asm = os.path.join("/tmp", "ewn_loop_regions_%d.s" % os.getpid())
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-o", asm, a.src])
    lines = open(asm).read().split("\n")
    name, body = kernel_body(lines, a.kernel)
    rows, tot = analyse(blocks_of(body))
    print("kernel %s: %d blocks in the step loop" % (name, len(rows)))
    fmt = "%-14s %-11s %5s %5s %4s %4s %5s %5s  %s"
    print(fmt % ("block", "region", "valu", "lds", "mul", "dpp", "salu", "vmem", ""))
    for r in rows:
        print(fmt % (r["label"], r["region"], r["valu"], r["lds"], r["mul"], r["dpp"], r["salu"], r["vmem"], r["note"]))
    for reg in ("search", "step", "step_common", "cold"):
        t = tot[reg]
        print(fmt % ("total", reg, t["valu"], t["lds"], t["mul"], t["dpp"], t["salu"], t["vmem"], ""))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"kernel": name, "blocks": rows, "totals": tot}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
