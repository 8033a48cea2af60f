"""Which device symbols differ between two builds of libewn_hip.so (static, from the disassembly).

  python tools/kernel_symbol_diff.py OLD.so NEW.so [--allow SUBSTR] [--list]

Takes the gfx950 code objects out of both libraries (llvm-objdump --offloading), disassembles them (llvm-objdump -d) and compares
the instruction text symbol by symbol (addresses and encodings left out: a function that only moved compares equal).  Prints the
symbols that differ or exist on one side only, demangled, and a verdict: with --allow, every such symbol has to contain SUBSTR
(a change meant for one kernel family must leave every other kernel's code as it was).  Exit status 1 if it does not hold."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
HEAD = re.compile(r"^[0-9a-f]* ?<(.+)>:$")


def symbols(lib):
    """symbol -> digest of its instruction text, over every gfx950 code object of the library"""
    d = tempfile.mkdtemp()
    try:
        copy = os.path.join(d, "lib.so")   # the code objects are written next to the library
        shutil.copy(lib, copy)
        subprocess.check_call([OBJDUMP, "--offloading", copy], stdout=subprocess.DEVNULL)
        text = {}
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            out = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", os.path.join(d, f)]).decode()
            cur = None
            for line in out.splitlines():
                m = HEAD.match(line)
                if m:
                    cur = m.group(1)
                    text.setdefault(cur, [])
                elif cur is not None and line.strip():
                    text[cur].append(re.sub(r"\s*//.*$", "", line.strip()))   # the trailing address comment goes
        return {k: (hashlib.sha1("\n".join(v).encode()).hexdigest(), len(v)) for k, v in text.items()}
    finally:
        shutil.rmtree(d)


def demangle(names):
    if not names:
        return []
    return subprocess.run(["c++filt"], input="\n".join(names).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", default=None, help="substring every changed symbol must contain")
    ap.add_argument("--list", action="store_true", help="also list the identical symbols")
    a = ap.parse_args()
    o, n = symbols(a.old), symbols(a.new)
    same = sorted(k for k in o if k in n and o[k] == n[k])
    diff = sorted(k for k in o if k in n and o[k] != n[k])
    only = sorted(set(o) ^ set(n))
    print("%d symbols identical, %d differ, %d on one side only" % (len(same), len(diff), len(only)))
    for k, name in zip(diff, demangle(diff)):
        print("differs   %6d -> %6d instructions  %s" % (o[k][1], n[k][1], name))
    for k, name in zip(only, demangle(only)):
        print("only in %s  %s" % ("old" if k in o else "new", name))
    if a.list:
        for k, name in zip(same, demangle(same)):
            print("identical %6d instructions  %s" % (o[k][1], name))
    ok = True
    if a.allow is not None:
        bad = [k for k in diff + only if a.allow not in k]
        ok = not bad
        print("verdict: every symbol without '%s' in its name is identical" % a.allow if ok else
              "verdict: %d symbols without '%s' in their name changed" % (len(bad), a.allow))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
