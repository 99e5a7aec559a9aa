#!/usr/bin/env python3
"""Compares the gfx950 code of the measure / relate kernels of two source trees, symbol by symbol.

    python tools/compare_kernel_isa.py OLD_TREE NEW_TREE [--all | --only FILE ...] [-o profiles/measure_kernels_isa.txt]

Every measure source of a tree (csrc/measure.hip, region_*.hip, label_*.hip, nucleus.hip), with --all every source of the
tree, is compiled to device-only assembly with _build.py's flags.  A kernel's text is its instructions and labels: comment and
directive lines are dropped, and the number of the function inside its file is taken out of the local labels, so a kernel
that moved to another file compares equal.  A kernel whose symbol changed with the name of a parameter's type is paired by
its own name (with its template arguments), where one symbol of that name left and one came; several instantiations or
overloads that change symbol together stay unpaired and are listed as "only in" one tree.  Per kernel the table says
"identical", or gives both trees' VGPRs, SGPRs, LDS bytes, scratch bytes and instruction count from the assembly's metadata.
Needs hipcc, no GPU.
"""

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_clx_build", os.path.join(tree, "cellulus_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def measure_sources(build):
    return [f for f in build.sources() if f in ("measure.hip", "nucleus.hip") or f.startswith(("region_", "label_"))]


def assembly(build, name, tmp):
    flags = [f for f in build.COMMON_FLAGS if f != "-Wall"] + build.PER_FILE_FLAGS.get(name, [])
    out = os.path.join(tmp, name + ".s")
    cmd = [build._hipcc(), *flags, "--offload-device-only", "-S", os.path.join(build.CSRC, name), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed for {name}:\n{res.stderr}")
    with open(out) as f:
        return f.read()


LOCAL_LABEL = re.compile(r"\.L(BB|JTI|tmp|func_begin|func_end)\d+(_\d+)?")


def kernels_of(text):
    """{symbol: (lines, metadata)} of the kernels in one assembly file"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        block = "  - .agpr_count:" + block
        sym = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        get = lambda key: int(re.search(r"^\s+\." + key + r":\s+(\d+)", block, re.M).group(1))
        meta[sym] = {"vgpr": get("vgpr_count"), "sgpr": get("sgpr_count"), "lds": get("group_segment_fixed_size"),
                     "scratch": get("private_segment_fixed_size")}
    out = {}
    lines = [line.split(";")[0].strip() for line in text.splitlines()]
    for sym in names:
        start = lines.index(sym + ":")
        body = []
        for s in lines[start + 1:]:
            if s.startswith(".Lfunc_end"):
                break
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue
            body.append(LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), s))
        m = dict(meta[sym])
        m["insts"] = sum(1 for s in body if not s.endswith(":"))
        out[sym] = (body, m)
    return out


def tree_kernels(tree, only, every):
    build = load_build(tree)
    names = [n for n in (build.sources() if every or only else measure_sources(build)) if not only or n in only]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as pool:
        texts = list(pool.map(lambda n: assembly(build, n, tmp), names))
    out = {}
    for name, text in zip(names, texts):
        for sym, v in kernels_of(text).items():
            out[sym] = (name,) + v
    return out


def demangle(syms):
    try:
        res = subprocess.run(["c++filt", *syms], capture_output=True, text=True, check=True)
        short = [s.replace("(anonymous namespace)::", "").replace("void ", "") for s in res.stdout.splitlines()]
        return dict(zip(syms, (re.sub(r"\((?!.*>).*", "", s) for s in short)))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def waves(vgpr):
    return min(8, 512 // max(8, -(-vgpr // 8) * 8))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-o", "--output")
    ap.add_argument("--only", nargs="*", help="source files to compare (default: all measure sources)")
    ap.add_argument("--all", action="store_true", help="compare every source of the trees")
    args = ap.parse_args()
    old, new = tree_kernels(args.old, args.only, args.all), tree_kernels(args.new, args.only, args.all)
    nice = demangle(sorted(set(old) | set(new)))
    # a kernel whose parameter types were renamed has another symbol: it is paired by its name where that is unambiguous
    gone, come = [s for s in old if s not in new], [s for s in new if s not in old]
    for sym in come:
        twins = [s for s in gone if nice[s] == nice[sym]]
        if len(twins) == 1 and sum(nice[s] == nice[sym] for s in come) == 1:
            name, body, meta = new.pop(sym)
            new[twins[0]] = (name, [line.replace(sym, twins[0]) for line in body], meta)
    rows = ["# kernel [file old -> new]: identical | old / new vgpr sgpr lds scratch insts (waves per SIMD)"]
    differ = worse = 0
    for sym in sorted(set(old) | set(new), key=lambda s: nice[s]):
        if sym not in old or sym not in new:
            rows.append(f"{nice[sym]}: only in the {'new' if sym in new else 'old'} tree")
            differ += 1
            continue
        (fo, bo, mo), (fn, bn, mn) = old[sym], new[sym]
        where = fo if fo == fn else f"{fo} -> {fn}"
        if bo == bn and mo == mn:
            rows.append(f"{nice[sym]} [{where}]: identical")
            continue
        differ += 1
        fmt = lambda m: f"vgpr {m['vgpr']} sgpr {m['sgpr']} lds {m['lds']} scratch {m['scratch']} insts {m['insts']} ({waves(m['vgpr'])} waves)"
        bad = mn["scratch"] > mo["scratch"] or mn["lds"] != mo["lds"] or waves(mn["vgpr"]) != waves(mo["vgpr"])
        worse += bad
        rows.append(f"{nice[sym]} [{where}]: old {fmt(mo)} / new {fmt(mn)}{'  DISQUALIFIED' if bad else ''}")
    rows.append(f"# {len(set(old) | set(new))} kernels, {differ} not identical, {worse} disqualified")
    text = "\n".join(rows) + "\n"
    if args.output:
        with open(args.output, "w") as f:
            f.write(text)
    sys.stdout.write(text)
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
