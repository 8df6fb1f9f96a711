"""Compare the kernel-resource-usage remarks of two builds of csrc/api.hip (hipcc -Rpass-analysis=kernel-resource-usage, stderr
kept in a file each): every k_rec_mfma instantiation of the first file must appear in the second, without the trailing RAG = false
template argument that file may lack, with the same registers, scratch, occupancy, LDS and code size.  Prints the ragged
instantiations of the second file as well.

    python profiles/ragged/resource_usage.py parent_usage.txt branch_usage.txt [parent_symbols.txt branch_symbols.txt]

The optional pair holds `llvm-readelf -sW` of the two device code objects (hipcc --cuda-device-only --no-gpu-bundle-output -c):
code bytes per kernel.
"""
import re
import sys


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*): (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def add_code_sizes(table, symbols_path):
    """`llvm-readelf -sW` of the device code object (Num, Value, Size, Type, Bind, Vis, Ndx, Name): bytes of every kernel's code"""
    for line in open(symbols_path):
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in table:
            table[f[7]]["code bytes"] = int(f[2])


def key(mangled):
    """template arguments of a k_rec_mfma instantiation (PF, NQ, XIN, HP, CELL, ABL, DS, RAG) from its mangled name; a name
    without the last one (the parent's) reads as RAG = 0"""
    m = re.search(r"k_rec_mfmaI((?:L[ib]\d+E)+)E", mangled)
    if not m:
        return None
    args = re.findall(r"L[ib](\d+)E", m.group(1))
    return tuple(args + ["0"] * (8 - len(args)))


def main(parent, branch, parent_symbols=None, branch_symbols=None):
    a, b = parse(parent), parse(branch)
    if parent_symbols and branch_symbols:
        add_code_sizes(a, parent_symbols)
        add_code_sizes(b, branch_symbols)
    kb = {key(n): n for n in b if key(n)}
    bad = 0
    for n in a:
        k = key(n)
        if not k:
            continue
        twin = kb.get(k)
        same = twin is not None and a[n] == b[twin]
        bad += not same
        print(("same     " if same else "DIFFERENT"), "k_rec_mfma<%s>" % ", ".join(k[:7]), a[n], "" if same else b.get(twin))
    print("ragged instantiations of the second build:")
    for k, n in sorted(kb.items()):
        if k[7] == "1":
            print("   k_rec_mfma<%s>" % ", ".join(k), b[n])
    print("existing instantiations that differ:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
