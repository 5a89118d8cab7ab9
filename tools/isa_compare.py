#!/usr/bin/env python3
"""`python tools/isa_compare.py A.so B.so`: every gfx950 kernel of two builds of the library, disassembled (llvm-objdump of the code objects inside),
addresses and encodings stripped, compared instruction for instruction -- which kernels a change of the sources touched.
`--by-name`: kernels are paired by demangled name without the parameter list (a renamed parameter type changes the mangled name and nothing else)."""
import subprocess, sys, os, re, tempfile, shutil, hashlib
def kernels(lib):
    tmp = tempfile.mkdtemp()
    shutil.copy(lib, tmp)
    subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", os.path.basename(lib)], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f: continue
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d"] + (["--demangle"] if BY_NAME else []) + [f], cwd=tmp, check=True, capture_output=True, text=True).stdout
        cur = None
        for line in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m: cur = m.group(1); out[cur] = []; continue
            if cur and "//" in line:
                ins = line.split("//")[0].strip()
                ins = re.sub(r"<[^>]+>", "", ins)
                out[cur].append(ins)
    shutil.rmtree(tmp)
    return out
def by_name(ks):
    """--by-name: keyed by the demangled name without its parameter list (template arguments kept), so that a kernel whose mangled name changed only
    because a parameter's TYPE was renamed is compared with itself.  Kernels that then share a key (overloads) keep their full names."""
    short = {n: re.sub(r"^void ", "", re.sub(r"\((?:[^()]|\([^()]*\))*\)( \[clone [^\]]*\])?$", "", n)) for n in ks}
    seen = list(short.values())
    return {(s if seen.count(s) == 1 else n): ks[n] for n, s in short.items()}
args = [v for v in sys.argv[1:] if v != "--by-name"]
BY_NAME = len(args) < len(sys.argv) - 1
a = kernels(args[0]); b = kernels(args[1])
if BY_NAME: a, b = by_name(a), by_name(b)
for k in sorted(set(a) | set(b)):
    ha = hashlib.md5("\n".join(a.get(k, [])).encode()).hexdigest()[:8] if k in a else None
    hb = hashlib.md5("\n".join(b.get(k, [])).encode()).hexdigest()[:8] if k in b else None
    print("%-60s %6s %6s %s" % (k[:60], len(a.get(k, [])), len(b.get(k, [])), "same" if ha == hb else "DIFFERENT"))
