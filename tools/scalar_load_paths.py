#!/usr/bin/env python3
"""Every path from each `s_load_dwordx16` of a kernel to the `s_waitcnt lgkmcnt(0)` that makes its sixteen registers valid.

rt_trace_{parity,fast}_g (rt_trace.inc.h request_four_uniform / arrived) issue the scalar load in one asm statement and wait for it in
another; the compiler sees the destination registers as defined right after the request.  Nothing but the instruction order of the
build keeps it from reading, copying (s_mov, v_writelane) or reusing them before the wait -- which would test stale records.  This
walks the disassembly: from each load, along the fall-through and both sides of every conditional branch, forward and backward, and
reports any path that names a register of the destination range (as source or destination), ends the program, reaches the load again
or leaves by an indirect branch before an `s_waitcnt` whose lgkmcnt is 0.

    python tools/scalar_load_paths.py [LIBRARY] [KERNEL ...]      (default: the product library, rt_trace_parity_g rt_trace_fast_g)

tests/test_abi.py holds both shipped kernels to it."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
LOAD = "s_load_dwordx16"

_ADDR = re.compile(r"//\s*([0-9A-Fa-f]+):")
_HEAD = re.compile(r"^([0-9a-f]+) <(.+)>:\s*$")
# registers the scalar file aliases under names (gfx9): vcc = s[106:107]
_ALIAS = {"vcc": (106, 107), "vcc_lo": (106, 106), "vcc_hi": (107, 107)}


def disassemble(lib):
    """{kernel symbol: listing lines} of every gfx950 code object inside a built library: `llvm-objdump --offloading` in a scratch
    directory (as raytracing_simple_amd/_build.kernel_metadata does), then `llvm-objdump -d --mcpu=gfx950` of each code object."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], check=True, cwd=tmp, stdout=subprocess.DEVNULL)
        for name in sorted(os.listdir(tmp)):
            if "amdgcn" not in name:
                continue
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", os.path.join(tmp, name)], check=True,
                                  capture_output=True, text=True).stdout
            out.update(split_kernels(text))
    return out


def split_kernels(text):
    """A disassembly listing cut into {symbol: lines}, the header line `<address> <symbol>:` included."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _HEAD.match(line)
        if m:
            cur = m.group(2)
            out[cur] = [line]
        elif cur is not None:
            out[cur].append(line)
    return out


def parse(lines):
    """[(address, mnemonic, operand text, comment)] of the instructions of one kernel's listing, in address order."""
    insns = []
    for line in lines:
        if _HEAD.match(line) or "//" not in line:
            continue
        code, comment = line.split("//", 1)
        m = _ADDR.match("//" + comment)
        code = code.strip()
        if not m or not code:
            continue
        mnem, _, ops = code.partition(" ")
        insns.append((int(m.group(1), 16), mnem, ops.strip(), comment))
    insns.sort(key=lambda t: t[0])
    return insns


def registers(ops):
    """Scalar registers an operand text names: sN, s[a:b] and the vcc aliases, as a set of indices."""
    regs = set()
    for a, b in re.findall(r"\bs\[(\d+):(\d+)\]", ops):
        regs.update(range(int(a), int(b) + 1))
    for a in re.findall(r"\bs(\d+)\b", ops):
        regs.add(int(a))
    for name, (a, b) in _ALIAS.items():
        if re.search(r"\b%s\b" % name, ops):
            regs.update(range(a, b + 1))
    return regs


def waits_for_scalar_loads(mnem, ops):
    """An s_waitcnt that leaves no scalar-memory access outstanding: lgkmcnt(0), or a raw immediate whose lgkmcnt field (bits 11:8) is 0."""
    if mnem != "s_waitcnt":
        return False
    m = re.search(r"lgkmcnt\((\d+)\)", ops)
    if m:
        return int(m.group(1)) == 0
    if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", ops):
        return (int(ops, 0) >> 8) & 0xF == 0
    return False            # (only vmcnt / expcnt named: lgkmcnt is left as it is)


def branch_offset(ops):
    """The signed 16-bit dword offset of a branch: llvm-objdump prints it unsigned (65432 = -104)."""
    v = int(ops.split()[0].rstrip(","), 0) & 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def check_kernel(lines):
    """Every s_load_dwordx16 of one kernel's listing, every path from it.  Returns (number of such loads, list of complaints)."""
    insns = parse(lines)
    at = {a: k for k, (a, _, _, _) in enumerate(insns)}
    bad, n_loads = [], 0
    for k0, (a0, mnem0, ops0, _) in enumerate(insns):
        if mnem0 != LOAD:
            continue
        n_loads += 1
        m = re.match(r"s\[(\d+):(\d+)\]", ops0)
        if not m:
            bad.append("0x%x: %s %s: no destination range" % (a0, mnem0, ops0))
            continue
        dest = set(range(int(m.group(1)), int(m.group(2)) + 1))
        seen, todo = set(), [k0 + 1]
        while todo:
            k = todo.pop()
            if k in seen:
                continue
            seen.add(k)
            if k >= len(insns):
                bad.append("0x%x: a path runs off the end of the kernel before the wait" % a0)
                continue
            a, mnem, ops, comment = insns[k]
            where = "0x%x -> 0x%x %s %s" % (a0, a, mnem, ops)
            if k == k0:
                bad.append("%s: the load is reached again before its wait" % where)
                continue
            if waits_for_scalar_loads(mnem, ops):
                continue
            if registers(ops) & dest:
                bad.append("%s: names a register of s[%d:%d] before the wait" % (where, min(dest), max(dest)))
                continue
            if mnem == "s_endpgm":
                bad.append("%s: the program ends before the wait" % where)
                continue
            if mnem in ("s_setpc_b64", "s_swappc_b64", "s_cbranch_join"):
                bad.append("%s: an indirect branch before the wait" % where)
                continue
            if mnem == "s_branch" or mnem.startswith("s_cbranch_"):
                target = a + 4 + 4 * branch_offset(ops)
                if target not in at:
                    bad.append("%s: branch to 0x%x, which is not an instruction" % (where, target))
                    continue
                todo.append(at[target])
                if mnem == "s_branch":
                    continue
            todo.append(k + 1)
    return n_loads, bad


def main():
    args = sys.argv[1:]
    lib = args[0] if args and args[0].endswith(".so") else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                         "raytracing_simple_amd", "librt_hip.so")
    names = [a for a in args if not a.endswith(".so")] or ["rt_trace_parity_g", "rt_trace_fast_g"]
    kernels = disassemble(lib)
    rc = 0
    for name in names:
        n, bad = check_kernel(kernels[name])
        print("%s: %d x %s, %s" % (name, n, LOAD, "every path waits" if not bad else "%d complaints" % len(bad)))
        for b in bad:
            print("  " + b)
        rc |= 1 if bad or n == 0 else 0
    return rc


if __name__ == "__main__":
    sys.exit(main())
