"""Per-symbol comparison of two builds' gfx950 code objects (no GPU needed).

  python tools/symbol_diff.py PARENT.so NEW.so [> profiles/<name>_symbol_diff.txt]

Both libraries are unbundled and disassembled with llvm-objdump -d; every symbol's instruction stream (mnemonics and operands, without
addresses and encodings - a kernel that moved in the file is still the same kernel) is compared.  Branch targets are written relative to
the symbol by llvm-objdump (<symbol+0x..>), so they survive a move as well.  Prints the symbol counts of both, the identical and differing
counts, and the lists of differing, removed and added symbols.  Exit status 1 if a symbol of the parent differs or is gone: a pull request
that carries profiles/*.json measurements forward across a source change has to show that the measured kernels did not change."""
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def streams(lib: str) -> dict:
    d = tempfile.mkdtemp(prefix="symdiff")
    subprocess.run(["cp", lib, os.path.join(d, "lib.so")], check=True)
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    objs = [f for f in os.listdir(d) if "gfx950" in f]
    assert len(objs) == 1, os.listdir(d)
    out = subprocess.run([OBJDUMP, "-d", objs[0]], cwd=d, check=True, stdout=subprocess.PIPE, text=True).stdout
    funcs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur is not None and line.strip() and not line.startswith("Disassembly"):
            ins = line.split("//")[0].strip()
            if ins and ins != "...":              # ("...": llvm-objdump's elision of the zero padding behind a symbol - where the next one starts, not code)
                funcs[cur].append(ins)
    return funcs


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = streams(argv[1]), streams(argv[2])
    same = sorted(n for n in a if n in b and a[n] == b[n])
    differ = sorted(n for n in a if n in b and a[n] != b[n])
    gone = sorted(n for n in a if n not in b)
    added = sorted(n for n in b if n not in a)
    print("symbols: parent %d, new %d" % (len(a), len(b)))
    print("parent symbols identical in the new build (instruction stream, per symbol): %d" % len(same))
    print("parent symbols that differ: %d" % len(differ))
    for n in differ:
        print("  DIFFERS %s (%d -> %d instructions)" % (n, len(a[n]), len(b[n])))
    print("parent symbols missing from the new build: %d" % len(gone))
    for n in gone:
        print("  MISSING %s" % n)
    print("added symbols: %d" % len(added))
    for n in added:
        print("  + %s (%d instructions)" % (n, len(b[n])))
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
