#!/usr/bin/env python
"""Refresh the ``wgrad`` rows of a shipped kernel-choice table from a ``bench.py --choices measure
--dump-choices`` dump: every other row, the order of the rows and the pinned rows (``--keep KEY``,
default the 28x28 512 -> 256 1x1 that tests/test_common.py pins) stay byte-identical.

usage: python scripts/merge_wgrad_choices.py <shipped.jsonl> <dump.jsonl> [--keep KEY ...] > <new.jsonl>
"""
import json
import sys

PINNED = ["('1x1', (256, 512, 28, 28), 256)"]


def main():
    args = sys.argv[1:]
    keep = list(PINNED)
    while "--keep" in args:
        i = args.index("--keep")
        keep.append(args[i + 1])
        del args[i:i + 2]
    shipped, dump = args
    fresh = {}
    for line in open(dump):
        if line.strip():
            rec = json.loads(line)
            if rec["kind"] == "wgrad":
                fresh[rec["key"]] = line.rstrip("\n")
    for line in open(shipped):
        rec = json.loads(line) if line.strip() else None
        if rec is not None and rec["kind"] == "wgrad" and rec["key"] not in keep and rec["key"] in fresh:
            line = fresh[rec["key"]] + "\n"
        sys.stdout.write(line)


if __name__ == "__main__":
    main()
