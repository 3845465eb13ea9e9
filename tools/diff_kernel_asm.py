"""Compare the gfx950 kernels that one .hip file compiles to in two source trees (a refactor must leave them alone).

    python tools/diff_kernel_asm.py OLD_TREE NEW_TREE gemm.hip [--ablation] [--by-name]

Each tree's copy of the file is compiled to device assembly (``hipcc -S --cuda-device-only``: no GPU needed) with the flags
of ``cryovit_amd/build.py`` of the NEW tree, the output is cut into one piece per kernel -- its instruction stream and its
kernel descriptor (register counts, LDS and scratch size) -- and the kernels that differ or exist in one tree only are
printed.  Comments, label numbers and ``__hip_cuid`` are ignored.  Exit status 1 if anything differs.

Kernels are paired by their mangled name, which encodes the parameter types: after ``PickDims`` became ``BitDims`` every kernel that
takes one is MISSING on both sides.  ``--by-name`` pairs them by the demangled qualified name with its template arguments and
without the parameter list (``cvx::k_mask_round<26, false>``; needs ``c++filt``), and compares the bodies with the kernel's own
symbol replaced by that name.  Overloads, which would share such a name within one tree, are reported as AMBIGUOUS and not compared.
"""

from __future__ import annotations

import argparse
import difflib
import importlib.util
import re
import subprocess
import sys
from pathlib import Path


def load_build(tree: Path):
    spec = importlib.util.spec_from_file_location("cvx_build", tree / "cryovit_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(build, tree: Path, name: str, ablation: bool) -> str:
    cmd = [build.hipcc_path(), *build.FLAGS, *(["-DCVX_ABLATION"] if ablation else []), *build.FILE_FLAGS.get(name, []),
           "-I", str(tree / "include"), "-S", "--cuda-device-only", str(tree / "cryovit_amd" / "csrc" / name), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed in {tree}:\n{r.stderr}")
    return r.stdout


def kernels(asm: str) -> dict[str, list[str]]:
    """kernel name -> normalised lines of its body and of its .amdhsa_kernel block"""
    out: dict[str, list[str]] = {}
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    cur = None
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].rstrip()
        m = re.match(r"^(\w+):$", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not s or "__hip_cuid" in s or re.match(r"^\.L\w+:$", s):  # (labels of their own are skipped)
            continue
        cur.append(re.sub(r"\.L(BB|tmp)\d+(_\d+)?", lambda t: ".L" + t.group(1) + (t.group(2) or ""), s))
        if s.startswith(".end_amdhsa_kernel"):
            cur = None
    return out


def qualified(mangled: list[str]) -> list[str]:
    """the demangled names without return type and parameter list: ``void cvx::k<6, true>(int const*, cvx::A)`` -> ``cvx::k<6, true>``"""
    r = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True)
    out = []
    for full in r.stdout.splitlines():
        depth, cut = 0, len(full)
        for i in range(len(full) - 1, -1, -1):  # the "(" that closes last: the parameter list
            depth += (full[i] == ")") - (full[i] == "(")
            if depth == 0 and full[i] == "(":
                cut = i
                break
        head, depth, start = full[:cut], 0, 0
        for i, c in enumerate(head):  # the last blank outside <>: the end of a template kernel's return type
            depth += (c == "<") - (c == ">")
            if c == " " and depth == 0:
                start = i + 1
        out.append(head[start:])
    return out


def by_name(ks: dict[str, list[str]], side: str) -> tuple[dict[str, list[str]], int]:
    """ks keyed by qualified name, the kernel's own symbol replaced in its lines; and the number of names that collide"""
    names = dict(zip(ks, qualified(list(ks))))
    out: dict[str, list[str]] = {}
    clash = {q for q in names.values() if list(names.values()).count(q) > 1}
    for q in sorted(clash):
        print(f"AMBIGUOUS in {side}: {q} is {', '.join(m for m in ks if names[m] == q)}")
    for m, lines in ks.items():
        if names[m] not in clash:
            out[names[m]] = [ln.replace(m, names[m]) for ln in lines]
    return out, len(clash)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("file", help="name of a file under cryovit_amd/csrc, e.g. gemm.hip")
    ap.add_argument("--ablation", action="store_true", help="compile with -DCVX_ABLATION")
    ap.add_argument("--by-name", action="store_true", help="pair kernels by qualified name and template arguments, not by parameter types")
    a = ap.parse_args()
    build = load_build(a.new)
    old, new = (kernels(device_asm(build, t.resolve(), a.file, a.ablation)) for t in (a.old, a.new))
    bad = 0
    if a.by_name:
        (old, n_old), (new, n_new) = by_name(old, "old"), by_name(new, "new")
        bad = n_old + n_new
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print(f"MISSING in {'old' if k not in old else 'new'}: {k}")
        elif old[k] != new[k]:
            d = list(difflib.unified_diff(old[k], new[k], lineterm="", n=0))
            print(f"DIFFERS ({len(old[k])} -> {len(new[k])} lines, {sum(x[0] in '+-' for x in d) - 2} changed): {k}")
        else:
            continue
        bad += 1
    print(f"{a.file}{' (ablation)' if a.ablation else ''}: {len(set(old) | set(new))} kernels compared, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
