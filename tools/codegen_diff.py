#!/usr/bin/env python3
"""tools/codegen_diff.py <a> <b> [--arch gfx950] [--llvm DIR] -- are the device kernels of two builds the same code?

<a>, <b>: a libweasal_hip.so, one object file, or a directory of object files (csrc/build).  Runs on the build machine, no GPU:
  * copies the inputs to a temporary directory and extracts their code objects for the architecture (llvm-objdump --offloading);
  * disassembles them (llvm-objdump -d) and keys every function by its symbol; an instruction is its text with the address and
    encoding columns stripped (a symbol an operand comment names is kept without its offset);
  * reads the per-kernel resource notes (llvm-readelf --notes): VGPR, AGPR and SGPR counts, LDS bytes, private segment size,
    kernarg size, workgroup size limit, wavefront size;
  * prints the symbols missing from <b>, added in <b>, defined a different number of times, and differing (first differing
    instruction, or the notes that differ); exit status 1 if there is any of them, 0 otherwise.
A plain differ: it knows nothing about particular instructions and normalises no symbol name.
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

NOTE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def run(cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout


def code_objects(path, arch, llvm, tmp):
    """The extracted code objects of `path` for `arch` (llvm-objdump writes them beside its input: work on copies)."""
    os.makedirs(tmp)
    if os.path.isdir(path):
        srcs = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith((".o", ".so")))
    else:
        srcs = [path]
    if not srcs:
        sys.exit(f"codegen_diff: nothing to read in {path}")
    for s in srcs:
        shutil.copy(s, tmp)
        run([os.path.join(llvm, "llvm-objdump"), "--offloading", os.path.basename(s)], cwd=tmp)
    out = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith("--" + arch))
    if not out:
        sys.exit(f"codegen_diff: no {arch} code object in {path}")
    return out


SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")
ADDRESS = re.compile(r"\s*([0-9A-Fa-f]+):")
TARGET = re.compile(r"<([^>+]+)(\+0x[0-9a-f]+)?>\s*$")


def functions(obj, llvm):
    """{symbol: [instruction text]} of one code object: the bytes of the symbol's own size (what the disassembler prints after
    them, up to the next symbol, is alignment fill and depends on the neighbour)."""
    end = {}
    for line in run([os.path.join(llvm, "llvm-readelf"), "-sW", obj]).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            end[f[7]] = int(f[1], 16) + int(f[2])
    funcs, cur, stop = {}, None, 0
    for line in run([os.path.join(llvm, "llvm-objdump"), "-d", obj]).splitlines():
        m = SYM.match(line)
        if m:
            cur, stop = funcs.setdefault(m.group(1), []), end.get(m.group(1), 1 << 62)
            continue
        text, _, comment = line.partition("//")
        a = ADDRESS.match(comment)
        if cur is None or not a or int(a.group(1), 16) >= stop:
            continue
        t = TARGET.search(comment)
        cur.append(" ".join(text.split()) + (f" <{t.group(1)}>" if t else ""))
    return funcs


def notes(obj, llvm):
    """{kernel symbol: {note key: value}} of one code object."""
    out, cur = {}, None
    for line in run([os.path.join(llvm, "llvm-readelf"), "--notes", obj]).splitlines():
        if line.startswith("  - "):                 # a new entry of amdhsa.kernels
            cur = {}
            line = "    " + line[4:]
        if cur is None or not line.startswith("    .") or ":" not in line:
            continue
        key, _, val = line.strip().partition(":")
        val = val.strip().strip("'")
        if key == ".name":
            out[val] = cur
        elif key in NOTE_KEYS:
            cur[key] = val
    return out


def build(path, arch, llvm, tmp):
    """{symbol: [(instructions, notes or None), ...]} over all code objects of a build (a list: a symbol may be defined twice)."""
    syms = collections.defaultdict(list)
    for obj in code_objects(path, arch, llvm, tmp):
        nt = notes(obj, llvm)
        for name, ins in functions(obj, llvm).items():
            syms[name].append((ins, nt.get(name)))
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--llvm", default=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a = build(args.a, args.arch, args.llvm, os.path.join(tmp, "a"))
        b = build(args.b, args.arch, args.llvm, os.path.join(tmp, "b"))
    missing = sorted(set(a) - set(b))
    added = sorted(set(b) - set(a))
    common = sorted(set(a) & set(b))
    # a symbol of internal linkage may be defined in several units: the same number of times in both builds, or it is reported
    twice = [f"{n}: {len(a[n])} / {len(b[n])} definitions" for n in common if len(a[n]) != len(b[n])]
    differing = []
    for name in common:
        if len(a[name]) != len(b[name]):
            continue
        key = lambda d: (d[0], sorted((d[1] or {}).items()))
        pairs = list(zip(sorted(a[name], key=key), sorted(b[name], key=key)))
        (ia, na), (ib, nb) = next((p for p in pairs if p[0] != p[1]), pairs[0])
        if ia != ib:
            at = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            differing.append(f"{name}: {len(ia)} / {len(ib)} instructions, first difference at {at}: "
                             f"{ia[at] if at < len(ia) else '(end)'} | {ib[at] if at < len(ib) else '(end)'}")
        elif na != nb:
            keys = sorted(k for k in set(na or {}) | set(nb or {}) if (na or {}).get(k) != (nb or {}).get(k))
            differing.append(f"{name}: notes " + ", ".join(f"{k} {(na or {}).get(k)} / {(nb or {}).get(k)}" for k in keys))

    def kernels(s):
        return sum(1 for v in s.values() for _, n in v if n is not None)

    print(f"a: {args.a}: {sum(len(v) for v in a.values())} functions, {kernels(a)} kernels, "
          f"{sum(len(i) for v in a.values() for i, _ in v)} instructions")
    print(f"b: {args.b}: {sum(len(v) for v in b.values())} functions, {kernels(b)} kernels, "
          f"{sum(len(i) for v in b.values() for i, _ in v)} instructions")
    for title, rows in (("missing from b", missing), ("added in b", added), ("defined a different number of times", twice),
                        ("differing", differing)):
        print(f"{title}: {len(rows)}")
        for r in rows:
            print("  " + r)
    print(f"identical (instructions and notes): {len(common) - len(twice) - len(differing)} symbols")
    return 1 if missing or added or twice or differing else 0


if __name__ == "__main__":
    sys.exit(main())
