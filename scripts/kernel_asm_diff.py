#!/usr/bin/env python3
"""Instruction streams of every device kernel that stores Y, two checkouts
compared function by function.

Cross-compiles (no GPU needed) the compilations scripts/kernel_resources.py
lists, for both packages, to assembly (-S), cuts each file into functions,
drops directives and comments and renumbers the labels, and prints one
markdown row per function:

  identical                      the same instructions in the same order
  same opcodes, registers differ the streams are equal once register numbers
                                 are masked (another allocation, nothing else)
  n equal, +a -d ~r              a difflib alignment of the masked streams:
                                 lines kept, inserted, deleted, replaced; and
                                 where the insertions lie (first and last
                                 inserted line as a share of the function)

    scripts/kernel_asm_diff.py --before PKG_A --after PKG_B [--units tsg_jit64_w128,...]
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402


def functions(pkg, name, src, defs, tmp):
    out = os.path.join(tmp, name + ".s")
    r = subprocess.run([KR.HIPCC, *KR.FLAGS, *defs, "--cuda-device-only", "--no-gpu-bundle-output", "-S",
                        os.path.join(pkg, "csrc", src), "-o", out], capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{name}: {r.stderr[-2000:]}")
    funcs, cur, body = {}, None, []
    for line in open(out):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur, body = m.group(1), []
            funcs[cur] = body
            continue
        if cur is None or not line.strip():
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if s.startswith(".") and not s.startswith(".L"):
            continue
        body.append(s)
    out = {}
    for f, lines in funcs.items():
        labels = {}
        norm = []
        for s in lines:
            s = re.sub(r"\.L[\w$]+", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), s)
            norm.append(re.sub(r"\s+", " ", s))
        if any(not x.endswith(":") for x in norm):
            out[KR.short(f)] = norm
    return out


def mask(lines):
    return [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", s) for s in lines]


def segments(lines):
    """The function cut after every s_endpgm: the first piece is the stream
    from the entry to the first exit -- the likely path, which the compiler lays
    out in line (the dispatchers' fp32 path) -- the others are the blocks placed
    out of line after it (their 16-bit and scaled branches)."""
    out, cur = [], []
    for s in lines:
        cur.append(s)
        if s.startswith("s_endpgm"):
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def by_segment(a, b):
    """Every piece of the function before, looked up in the function after."""
    sa, sb = segments(a), segments(b)
    mb = [mask(x) for x in sb]
    notes = []
    for i, seg in enumerate(sa):
        what = "entry to first exit" if i == 0 else f"out-of-line block {i}"
        if seg in sb:
            notes.append(f"{what} ({len(seg)}): identical")
        elif mask(seg) in mb:
            notes.append(f"{what} ({len(seg)}): same opcodes, registers differ")
        else:
            ms = mask(seg)
            best = max(mb, key=lambda x: difflib.SequenceMatcher(None, ms, x, autojunk=False).quick_ratio())
            sm = difflib.SequenceMatcher(None, ms, best, autojunk=False)
            eq = sum(i2 - i1 for t, i1, i2, _, _ in sm.get_opcodes() if t == "equal")
            note = f"{what} ({len(seg)}): closest block after has {len(best)}, {eq} lines aligned"
            if len(seg) - eq <= 40 and len(best) - eq <= 40:  # few enough to list
                diff = [f"-{x}" for t, i1, i2, _, _ in sm.get_opcodes() if t in ("delete", "replace") for x in ms[i1:i2]]
                diff += [f"+{x}" for t, _, _, j1, j2 in sm.get_opcodes() if t in ("insert", "replace") for x in best[j1:j2]]
                note += " [" + " / ".join(diff) + "]"
            notes.append(note)
    notes.append(f"{len(sb) - len(sa):+d} blocks")
    return "; ".join(notes)


def compare(a, b):
    if a == b:
        return "identical"
    if sum(s.startswith("s_endpgm") for s in a) > 1:
        return by_segment(a, b)
    ma, mb = mask(a), mask(b)
    if ma == mb:
        return "same opcodes, registers differ"
    sm = difflib.SequenceMatcher(None, ma, mb, autojunk=False)
    eq = ins = dele = rep = 0
    first = last = None
    for tag, i1, i2, j1, j2 in sm.get_opcodes():
        if tag == "equal":
            eq += i2 - i1
        elif tag == "insert":
            ins += j2 - j1
        elif tag == "delete":
            dele += i2 - i1
        else:
            rep += max(i2 - i1, j2 - j1)
        if tag != "equal":
            first = j1 if first is None else first
            last = j2
    return f"{eq} equal, +{ins} -{dele} ~{rep}; changes within {100 * first // len(b)}-{100 * last // len(b)} % of the function"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", required=True)
    ap.add_argument("--after", required=True)
    ap.add_argument("--units", help="comma-separated unit names (default: all)")
    a = ap.parse_args()
    want = set(a.units.split(",")) if a.units else None
    print("| unit | function | instructions before | after | streams |")
    print("|---|---|---|---|---|")
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for name, src, defs in KR.units():
            if want and name not in want:
                continue
            A, B = functions(a.before, name, src, defs, ta), functions(a.after, name, src, defs, tb)
            for f in sorted(set(A) | set(B)):
                if f not in A or f not in B:
                    print(f"| {name} | `{f}` | {len(A.get(f, [])) or ''} | {len(B.get(f, [])) or ''} | {'new' if f in B else 'gone'} |")
                else:
                    print(f"| {name} | `{f}` | {len(A[f])} | {len(B[f])} | {compare(A[f], B[f])} |", flush=True)


if __name__ == "__main__":
    main()
