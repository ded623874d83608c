#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libmolkgnn_hip.so, kernel by kernel (no GPU needed).

    python tools/compare_device_code.py OLD/libmolkgnn_hip.so NEW/libmolkgnn_hip.so [--show N]

For a refactor that moves kernels between translation units without touching them: the set of kernel names must be the same,
and every kernel must have the same instruction sequence and the same kernel descriptor.  Per kernel (by mangled name):

  * the disassembly (llvm-objdump -d) of its function, with addresses, encodings and the symbolic branch-target comments
    removed.  Branch operands are relative and stay.  The one operand that depends on where the linker put things -- the
    literal of the s_add_u32 behind an s_getpc_b64, a pc-relative address -- is replaced by the symbol + offset it points at
    (its s_addc_u32 carries the sign of the same distance and is masked);
  * the facts of its descriptor from the code object's metadata note: VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, spills,
    kernarg bytes, wavefront size, workgroup-size bound;
  * the 64 descriptor bytes themselves (the .kd symbol), less the entry-point offset.

Exit status 0 iff everything is equal.  The last line is the summary.
"""
import argparse
import bisect
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FACTS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
         ".vgpr_spill_count", ".sgpr_spill_count", ".kernarg_segment_size", ".wavefront_size", ".max_flat_workgroup_size",
         ".uses_dynamic_stack")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, work):
    """Every gfx950 code object bundled into `lib`, extracted under `work`."""
    local = os.path.join(work, "lib.so")
    os.symlink(os.path.abspath(lib), local)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so", cwd=work)
    return sorted(os.path.join(work, f) for f in os.listdir(work) if f.endswith("gfx950"))


def symbols(co):
    """[(address, name)] of the functions and objects of a code object, sorted; and {name: (address, size, section)}."""
    by_name = {}
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND":
            by_name[f[7]] = (int(f[1], 16), int(f[2]), f[6])
    return sorted((v[0], k) for k, v in by_name.items()), by_name


def metadata(co):
    """{kernel name: {fact: value}} from the AMDGPU metadata note."""
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        s = line.strip()
        if s.startswith("- "):                               # a new list entry: of amdhsa.kernels (indent 2) or of .args (deeper)
            if len(line) - len(line.lstrip()) == 2:
                cur = {}
            s = s[2:].strip()
        if cur is None or ":" not in s:
            continue
        key, val = (t.strip() for t in s.split(":", 1))
        if key == ".name" and len(line) - len(line.lstrip(" -")) <= 4 and ".symbol" not in cur:
            cur[".name"] = val
        elif key == ".symbol":
            cur[".symbol"] = val
            out[val[:-3]] = cur
        elif key in FACTS:
            cur[key] = val
    return out


INSN = re.compile(r"^\t(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")


def functions(co, addr_names, by_name):
    """{function name: [normalised instruction]} of a code object."""
    addrs = [a for a, _ in addr_names]

    def where(target):
        i = bisect.bisect_right(addrs, target) - 1
        if i < 0:
            return "<?>"
        a, n = addr_names[i]
        return f"<{n}+{target - a:#x}>"

    size_of = {n: by_name[n][1] for n in by_name}
    out, cur, end, pc_lo, pc_hi, pc_val = {}, None, 0, None, None, 0
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", co).splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(2), [])
            end = int(m.group(1), 16) + size_of.get(m.group(2), 0)      # (behind it: the section's padding, not the function)
            pc_lo = None
            continue
        m = INSN.match(line)
        if not m or cur is None:
            continue
        op, args, addr = m.group(1), m.group(2), int(m.group(3), 16)
        if addr >= end:
            continue
        if op == "s_getpc_b64":
            r = re.match(r"s\[(\d+):(\d+)\]", args)
            pc_lo, pc_hi, pc_val = (f"s{r.group(1)}", f"s{r.group(2)}", addr + 4) if r else (None, None, 0)
        elif pc_lo and op == "s_add_u32" and args.startswith(f"{pc_lo}, {pc_lo}, "):
            lit = int(args.split(", ")[2], 0)
            lit -= (1 << 32) if lit >= 1 << 31 else 0
            args = f"{pc_lo}, {pc_lo}, {where(pc_val + lit)}"
        elif pc_lo and op == "s_addc_u32" and args.startswith(f"{pc_hi}, {pc_hi}, "):
            args = f"{pc_hi}, {pc_hi}, <hi>"
            pc_lo = None
        cur.append(f"{op} {args}".strip())
    return out


def kernels(lib):
    """{kernel name: (instructions, facts, descriptor bytes)} over all code objects of a library."""
    out = {}
    with tempfile.TemporaryDirectory() as work:
        for co in code_objects(lib, work):
            addr_names, by_name = symbols(co)
            meta = metadata(co)
            funcs = functions(co, addr_names, by_name)
            blob = open(co, "rb").read()
            sections = {}
            for line in run(os.path.join(LLVM, "llvm-readelf"), "-SW", co).splitlines():
                m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", line)
                if m:
                    sections[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16))
            for name, facts in meta.items():
                if name in out:
                    raise SystemExit(f"{lib}: kernel {name} is defined in two code objects")
                if name not in funcs:
                    raise SystemExit(f"{lib}: kernel {name} has metadata and no code")
                a, size, sec = by_name[name + ".kd"]
                sa, so = sections[sec]
                kd = bytearray(blob[so + a - sa: so + a - sa + size])
                kd[16:24] = bytes(8)                          # kernel_code_entry_byte_offset: where the linker put the code
                out[name] = (funcs[name], {k: facts.get(k) for k in FACTS}, bytes(kd))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", type=int, default=40, help="lines of the instruction diff to print per kernel")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for n in only_old:
        print("only in old:", n)
    for n in only_new:
        print("only in new:", n)
    differ, insns = [], 0
    for n in sorted(set(old) & set(new)):
        (io, fo, ko), (inw, fn, kn) = old[n], new[n]
        insns += len(inw)
        why = []
        if io != inw:
            why.append(f"instructions ({len(io)} -> {len(inw)})")
        if fo != fn:
            why.append("facts " + ", ".join(f"{k} {fo[k]} -> {fn[k]}" for k in FACTS if fo[k] != fn[k]))
        if ko != kn:
            why.append("descriptor bytes")
        if why:
            differ.append(n)
            print("DIFFERS:", n, "--", "; ".join(why))
            for line in list(difflib.unified_diff(io, inw, "old", "new", n=1, lineterm=""))[:a.show]:
                print("    " + line)
    same = not (only_old or only_new or differ)
    print(f"device code: {len(old)} kernels old, {len(new)} new, {len(only_old)} only old, {len(only_new)} only new, "
          f"{len(differ)} differ, {insns} instructions compared: {'IDENTICAL' if same else 'DIFFERENT'}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
