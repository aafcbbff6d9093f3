#!/usr/bin/env python3
"""Is the device code of two trees the same, kernel by kernel?  (CPU only: compiles, runs nothing.)

    python scripts/isa_equal.py A B [--only batchnorm.hip ...] [--jobs 8] [--keep DIR]

A and B are source trees, or git revisions of this repository (exported under a scratch directory).
Every ``csrc/kernels/*.hip`` is compiled for the device only to assembly, with the command line of
that tree's own ``fluxmpi_amd/_build.py`` (``EXTRA_FLAGS`` included). Per function symbol the
instruction stream and, for kernels, the descriptor (``.amdhsa_kernel`` block: VGPRs, SGPRs, LDS,
scratch, ...) are compared. Symbols are compared as a set, so their order in the file does not
matter; comments are dropped and local labels renumbered by first appearance. A file whose text and
every header under ``csrc/`` are byte-identical on both sides is not compiled.

Prints one line per file with the kernel count, lists every symbol that differs or exists on one
side only, and exits 1 if there is any.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tree_of(arg: str, scratch: str) -> str:
    if os.path.isdir(os.path.join(arg, "csrc")):
        return os.path.abspath(arg)
    dst = os.path.join(scratch, "rev_" + re.sub(r"\W", "_", arg))
    os.makedirs(dst)
    ar = subprocess.run(["git", "-C", HERE, "archive", arg, "csrc", "fluxmpi_amd/_build.py"], check=True,
                        capture_output=True)
    subprocess.run(["tar", "-x", "-C", dst], input=ar.stdout, check=True)
    return dst


def build_module(tree: str):
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(tree))),
                                                  os.path.join(tree, "fluxmpi_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(mod, src: str, out: str) -> str:
    cmd = mod._compile_cmd(src, out)
    cmd[cmd.index("-c")] = "-S"
    cmd.append("--cuda-device-only")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr}")
    with open(out) as f:
        return f.read()


LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def normalise(lines: list[str]) -> list[str]:
    names: dict[str, str] = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln or ln.startswith((".p2align", ".loc", ".file", ".cfi_")):
            continue
        ln = LABEL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), ln)
        out.append(re.sub(r"\s+", " ", ln))
    return out


def symbols(asm: str) -> dict[str, dict]:
    """{symbol: {"kernel": bool, "text": [...], "desc": [...]}} of one assembly file."""
    lines = asm.splitlines()
    funcs = [m.group(1) for ln in lines if (m := re.match(r"\s*\.type\s+([^,\s]+),@function", ln))]
    out = {}
    for sym in funcs:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        # a kernel's descriptor (.section .rodata ... .amdhsa_kernel) sits between its code and .Lfunc_end
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end") or ".section" in lines[i])
        out[sym] = {"kernel": False, "text": normalise(lines[start + 1:end]), "desc": []}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
            out[m.group(1)]["kernel"] = True
            out[m.group(1)]["desc"] = normalise(lines[i + 1:j])
            i = j
        i += 1
    return out


def same_inputs(a: str, b: str, rel: str) -> bool:
    def read(p):
        with open(p, "rb") as f:
            return f.read()

    ha = sorted(os.path.relpath(p, a) for p in glob.glob(os.path.join(a, "csrc", "**", "*.h"), recursive=True))
    hb = sorted(os.path.relpath(p, b) for p in glob.glob(os.path.join(b, "csrc", "**", "*.h"), recursive=True))
    return ha == hb and all(read(os.path.join(a, r)) == read(os.path.join(b, r)) for r in [rel, *ha])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--only", nargs="*", default=None, help="file names under csrc/kernels to compare")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 4))
    ap.add_argument("--keep", default=None, help="directory for the exported trees and assembly (default: temporary)")
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        scratch = args.keep or tmp
        os.makedirs(scratch, exist_ok=True)
        trees = [tree_of(args.a, scratch), tree_of(args.b, scratch)]
        mods = [build_module(t) for t in trees]
        names = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(t, "csrc", "kernels", "*.hip")))
                 for t in trees]
        bad = [f"{n}: file on one side only" for n in sorted(set(names[0]) ^ set(names[1]))]
        todo = [n for n in names[0] if n in names[1] and (args.only is None or n in args.only)]
        skipped = [n for n in todo if same_inputs(trees[0], trees[1], os.path.join("csrc", "kernels", n))]
        todo = [n for n in todo if n not in skipped]
        for n in skipped:
            print(f"{n}: text and headers identical, not compiled")

        def one(job):
            side, n = job
            out = os.path.join(scratch, f"{'ab'[side]}_{n}.s")
            return job, symbols(assemble(mods[side], os.path.join(trees[side], "csrc", "kernels", n), out))

        with cf.ThreadPoolExecutor(max_workers=args.jobs) as ex:
            got = dict(ex.map(one, [(s, n) for n in todo for s in (0, 1)]))
        for n in todo:
            sa, sb = got[0, n], got[1, n]
            diffs = []
            for sym in sorted(set(sa) | set(sb)):
                if sym not in sa or sym not in sb:
                    diffs.append(f"{sym}: only in {'B' if sym not in sa else 'A'}")
                elif sa[sym]["text"] != sb[sym]["text"]:
                    diffs.append(f"{sym}: instructions differ")
                elif sa[sym]["desc"] != sb[sym]["desc"]:
                    diffs.append(f"{sym}: descriptor differs")
            kernels = sum(1 for v in sa.values() if v["kernel"])
            print(f"{n}: {kernels} kernels, {len(sa)} symbols: {'equal' if not diffs else f'{len(diffs)} DIFFER'}")
            bad += [f"{n}: {d}" for d in diffs]
    for b in bad:
        print(b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
