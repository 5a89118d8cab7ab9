#!/usr/bin/env python3
"""`python tools/isa_compare.py A.so B.so`: every gfx950 kernel of two builds of the library, disassembled (llvm-objdump of the code objects inside),
addresses and encodings stripped, compared instruction for instruction -- which kernels a change of the sources touched.  Per side: the number of
instructions, and how many of them are not scalar (their mnemonic does not begin with `s_`).
`--by-name`: kernels are paired by demangled name without the parameter list (a renamed parameter type changes the mangled name and nothing else).
`--map OLD=NEW` (repeatable, with --by-name): A's kernel OLD is paired with B's kernel NEW, both named that way -- a kernel and its renamed successor.
`--pc-relative`: the displacement of a program-counter-relative address -- the literal of the `s_add_u32` (and, where it is one, of the `s_addc_u32`) that
follows an `s_getpc_b64` on the same register pair -- is left out of the comparison.  It is the distance from the instruction to a constant table of the
code object, and moves for EVERY kernel of a translation unit when the unit gains or loses a kernel; nothing else of an instruction is left out."""
import subprocess, sys, os, re, tempfile, shutil, hashlib
def kernels(lib):
    tmp = tempfile.mkdtemp()
    shutil.copy(lib, tmp)
    subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", os.path.basename(lib)], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f: continue
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d"] + (["--demangle"] if BY_NAME else []) + [f], cwd=tmp, check=True, capture_output=True, text=True).stdout
        cur = None; pc_pair = None; pc_left = 0
        for line in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m: cur = m.group(1); out[cur] = []; continue
            if cur and "//" in line:
                ins = line.split("//")[0].strip()
                ins = re.sub(r"<[^>]+>", "", ins)
                if PC_RELATIVE:
                    m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
                    if m: pc_pair = (m.group(1), m.group(2)); pc_left = 2
                    elif pc_left and re.match(r"s_add_u32 s%s, s%s, " % (pc_pair[0], pc_pair[0]), ins): ins = re.sub(r", [^,]+$", ", pc-relative", ins); pc_left -= 1
                    elif pc_left and re.match(r"s_addc_u32 s%s, s%s, " % (pc_pair[1], pc_pair[1]), ins): ins = re.sub(r", [^,]+$", ", pc-relative", ins); pc_left = 0
                    else: pc_left = 0
                out[cur].append(ins)
    shutil.rmtree(tmp)
    return out
def by_name(ks):
    """--by-name: keyed by the demangled name without its parameter list (template arguments kept), so that a kernel whose mangled name changed only
    because a parameter's TYPE was renamed is compared with itself.  Kernels that then share a key (overloads) keep their full names."""
    short = {n: re.sub(r"^void ", "", re.sub(r"\((?:[^()]|\([^()]*\))*\)( \[clone [^\]]*\])?$", "", n)) for n in ks}
    seen = list(short.values())
    return {(s if seen.count(s) == 1 else n): ks[n] for n, s in short.items()}
def counts(ins):
    return "%6s %6s" % (len(ins), sum(1 for i in ins if not i.startswith("s_")))
args, renamed = [], {}
argv = sys.argv[1:]
while argv:
    v = argv.pop(0)
    if v == "--map":
        old, new = argv.pop(0).split("=", 1)
        renamed[old] = new
    elif v not in ("--by-name", "--pc-relative"): args.append(v)
BY_NAME = "--by-name" in sys.argv[1:]
PC_RELATIVE = "--pc-relative" in sys.argv[1:]
a = kernels(args[0]); b = kernels(args[1])
if BY_NAME: a, b = by_name(a), by_name(b)
for old, new in renamed.items():
    if old not in a or new not in b: sys.exit("--map %s=%s: %s" % (old, new, "A holds no such kernel" if old not in a else "B holds no such kernel"))
    a[old + " -> " + new] = a.pop(old); b[old + " -> " + new] = b.pop(new)
for k in sorted(set(a) | set(b)):
    ha = hashlib.md5("\n".join(a.get(k, [])).encode()).hexdigest()[:8] if k in a else None
    hb = hashlib.md5("\n".join(b.get(k, [])).encode()).hexdigest()[:8] if k in b else None
    print("%-60s %s %s %s" % (k if " -> " in k else k[:60], counts(a.get(k, [])), counts(b.get(k, [])), "same" if ha == hb else "DIFFERENT"))
