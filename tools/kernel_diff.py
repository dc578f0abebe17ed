"""Kernel text and resources of two source trees, side by side: the acceptance test of a refactor.

  python tools/kernel_diff.py OLD_TREE NEW_TREE --units pf_ba,pf_decode [--summary]
  python tools/kernel_diff.py OLD_TREE NEW_TREE --old-units pf_pages --new-units pf_flat,pf_flat_null [--show-diff]

Each unit (a csrc/*.hip name without its suffix) of each tree is compiled to gfx950 assembly, device side only, once per
build flavour (prod: no define; diag: -DPF_DIAG; stamps: -DPF_DIAG -DPF_STAMPS):
  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage
Nothing is linked and nothing runs. Per function, matched by symbol across all the units of a side (so a kernel may
move between units; a static device function of a header has one copy per unit that calls it, and every new copy is
compared with the old copy of the same unit, else with the first old one): the text from its label to its last instruction, with comments, directives and the function
index of block labels stripped, and VGPR / SGPR / scratch bytes per lane / LDS bytes per block from the compiler's
remarks (kernels only: a device function that is called has text and no remark). The output is tab-separated.
This is a diff, nothing else: it knows nothing about what a kernel should contain."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAVOURS = {"prod": [], "diag": ["-DPF_DIAG"], "stamps": ["-DPF_DIAG", "-DPF_STAMPS"]}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_unit(tree, unit, flavour, out_dir):
    """-> (assembly text, remarks text) of one unit in one flavour."""
    pkg = os.path.join(tree, "parquet-floor_amd")
    asm = os.path.join(out_dir, f"{unit}.{flavour}.s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", "-I" + os.path.join(tree, "include"), "-Icsrc",
           *FLAVOURS[flavour], os.path.join("csrc", unit + ".hip"), "-o", asm]
    r = subprocess.run(cmd, cwd=pkg, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}\n{r.stderr}")
    with open(asm) as f:
        return f.read(), r.stderr


LABEL_IDX = re.compile(r"(\.L[A-Za-z_]+)\d+_")


def functions(asm):
    """symbol -> normalised instruction lines, for every function of an assembly file."""
    out, name, body = {}, None, []
    pending = None
    for line in asm.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            pending = m.group(1)
            continue
        if pending and line.startswith(pending + ":"):
            name, body, pending = pending, [], None
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";", 1)[0].strip()
        if not s:
            continue
        if s.startswith(".") and not s.endswith(":"):   # a directive (block labels end in ':')
            continue
        body.append(LABEL_IDX.sub(r"\1_", s))
    return out


def resources(remarks):
    """kernel symbol -> 'VGPR/SGPR/scratch/LDS' from -Rpass-analysis=kernel-resource-usage."""
    out, name, cur = {}, None, {}
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|([A-Za-z][A-Za-z \[\]/]*): (\S+)) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            cur = out.setdefault(name, {})
        elif name:
            cur[m.group(2).strip()] = m.group(3)
    return {k: "/".join(v.get(f, "?") for f in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"))
            for k, v in out.items()}


def short_names(symbols):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(symbols), stdout=subprocess.PIPE, text=True, check=True)
        full = r.stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        full = list(symbols)
    out = {}
    for sym, f in zip(symbols, full):
        f = re.sub(r"^void ", "", f)
        depth, cut = 0, len(f)
        for i, c in enumerate(f):   # the argument list: the first '(' outside template brackets
            if c == "<":
                depth += 1
            elif c == ">":
                depth -= 1
            elif c == "(" and depth == 0:
                cut = i
                break
        out[sym] = f[:cut].replace("pf::", "")
    return out


def side(tree, units, flavours, jobs, tmp):
    """flavour -> symbol -> [(unit, lines, resources or '-')]: one entry per unit that holds the symbol (a static
    device function of a header is compiled in every unit that calls it)."""
    work = [(u, fl) for fl in flavours for u in units]
    with ThreadPoolExecutor(jobs) as ex:
        built = list(ex.map(lambda w: compile_unit(tree, w[0], w[1], tmp), work))
    out = {fl: {} for fl in flavours}
    for (u, fl), (asm, rem) in zip(work, built):
        res = resources(rem)
        for sym, lines in functions(asm).items():
            out[fl].setdefault(sym, []).append((u, lines, res.get(sym, "-")))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--units", default="", help="units compiled on both sides (comma-separated)")
    ap.add_argument("--old-units", default="", help="units of the old tree only")
    ap.add_argument("--new-units", default="", help="units of the new tree only")
    ap.add_argument("--flavours", default="prod,diag,stamps")
    ap.add_argument("--summary", action="store_true", help="one line per unit and flavour instead of one per function")
    ap.add_argument("--show-diff", action="store_true", help="print the differing lines of every function that differs")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    both = [u for u in a.units.split(",") if u]
    old_units = both + [u for u in a.old_units.split(",") if u]
    new_units = both + [u for u in a.new_units.split(",") if u]
    flavours = a.flavours.split(",")
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old = side(os.path.abspath(a.old_tree), old_units, flavours, a.j, t_old)
        new = side(os.path.abspath(a.new_tree), new_units, flavours, a.j, t_new)
    if a.summary:
        print("unit\tflavour\tfunctions\tidentical text\tidentical resources")
    else:
        print("unit\tfunction\tflavour\ttext\tinstructions\told\tnew")
    diffs = []
    for fl in flavours:
        syms = list(dict.fromkeys(list(old[fl]) + list(new[fl])))
        names = short_names(syms)
        per_unit = {}
        pairs = []   # every new copy against the old copy of its own unit, else against the first old copy
        for sym in syms:
            olds, news = old[fl].get(sym, []), new[fl].get(sym, [])
            used = set()
            for n in news:
                o = next((x for x in olds if x[0] == n[0]), olds[0] if olds else None)
                used.add(id(o))
                pairs.append((sym, o, n))
            pairs += [(sym, o, None) for o in olds if id(o) not in used]
        for sym, o, n in pairs:
            unit = (o or n)[0] if not (o and n) or o[0] == n[0] else f"{o[0]}->{n[0]}"
            if not (o and n):
                text, same_text, same_res = ("only old" if o else "only new"), False, False
            else:
                same_text, same_res = o[1] == n[1], o[2] == n[2]
                if same_text:
                    text = "identical"
                else:
                    d = [x for x in difflib.unified_diff(o[1], n[1], "old", "new", lineterm="", n=0)]
                    nd = sum(1 for x in d if x[:1] in "+-" and x[:3] not in ("+++", "---"))
                    text = f"DIFF {nd} lines ({len(o[1])} vs {len(n[1])})"
                    diffs.append((names[sym], fl, d))
            c = per_unit.setdefault(unit, [0, 0, 0])
            c[0] += 1
            c[1] += same_text
            c[2] += same_res
            if not a.summary:
                print(f"{unit}\t{names[sym]}\t{fl}\t{text}\t{len((o or n)[1])}\t{o[2] if o else ''}\t{n[2] if n else ''}")
        if a.summary:
            for unit, c in per_unit.items():
                print(f"{unit}\t{fl}\t{c[0]}\t{c[1]}\t{c[2]}")
    if a.show_diff:
        for name, fl, d in diffs:
            print(f"\n==== {name} ({fl})")
            print("\n".join(d))


if __name__ == "__main__":
    main()
