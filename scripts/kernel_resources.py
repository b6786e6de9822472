#!/usr/bin/env python3
"""Register, scratch and occupancy figures of every device kernel that stores Y.

Cross-compiles (no GPU needed) each of the Makefile's dispatcher variants
(CO_ALL) and tsg_ell.hip / tcsc_kernels.hip with the Makefile's flags plus
-Rpass-analysis=kernel-resource-usage, and prints one JSON line per kernel:
  {"unit": ..., "kernel": ..., "vgprs": ..., "agprs": ..., "sgprs": ...,
   "sgpr_spill": ..., "vgpr_spill": ..., "scratch": ..., "occupancy": ..., "lds": ...}
Two runs (two checkouts, --pkg) diff into a before/after table:
  scripts/kernel_resources.py --pkg A > a.jsonl; ... --pkg B > b.jsonl
  scripts/kernel_resources.py --diff a.jsonl b.jsonl
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", "-ffp-contract=off"]


def units():
    """(name, source, defines) of every compilation the Makefile does for a Y-storing kernel."""
    out = [("tsg_jit", "tsg_jit_kernel.hip", [])]
    for w in (32, 16, 8):
        out.append((f"tsg_jit_w{w}", "tsg_jit_kernel.hip", [f"-DTSG_JIT_NW={w}"]))
    for w in (32, 16, 8):
        out.append((f"tsg_jit_w{w}_4w", "tsg_jit_kernel.hip", [f"-DTSG_JIT_NW={w}", "-DTSG_JIT_WAVES=4"]))
    r64 = ["-DTSG_JIT_ROWS64=1"]
    for w in (128, 64, 32, 16, 8):
        out.append((f"tsg_jit64_w{w}", "tsg_jit_kernel.hip", r64 + [f"-DTSG_JIT_NW={w}"]))
    for tag, extra in (("_4w", []), ("h", ["-DTSG_JIT_HALF=1"]), ("p", ["-DTSG_JIT_PAIR=1"])):
        for w in (32, 16, 8):
            name = f"tsg_jit64_w{w}_4w" if tag == "_4w" else f"tsg_jit64{tag}_w{w}"
            out.append((name, "tsg_jit_kernel.hip", r64 + [f"-DTSG_JIT_NW={w}", "-DTSG_JIT_WAVES=4"] + extra))
    out.append(("tsg_ell", "tsg_ell.hip", []))
    out.append(("tcsc_kernels", "tcsc_kernels.hip", []))
    return out


FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def measure(pkg):
    csrc = os.path.join(pkg, "csrc")
    if not os.path.exists(os.path.join(csrc, "tsg_rx_asm.inc")):
        subprocess.run([sys.executable, os.path.join(csrc, "gen_rx_asm.py"), os.path.join(csrc, "tsg_rx_asm.inc")], check=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, src, defs in units():
            r = subprocess.run([HIPCC, *FLAGS, *defs, "--cuda-device-only", "--no-gpu-bundle-output",
                                "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, src),
                                "-o", os.path.join(tmp, name + ".co")], capture_output=True, text=True)
            if r.returncode:
                sys.exit(f"{name}: {r.stderr[-2000:]}")
            cur = None
            for line in r.stderr.splitlines():
                m = re.search(r"remark: (?:\S+: )?\s*(.+?):\s*(\S+)\s*\[-Rpass-analysis", line)
                if not m:
                    continue
                key, val = m.group(1).strip(), m.group(2)
                if key == "Function Name":
                    if cur:
                        print(json.dumps(cur))
                    cur = {"unit": name, "kernel": short(val)}
                elif cur is not None and key in FIELDS:
                    cur[FIELDS[key]] = int(val)
            if cur:
                print(json.dumps(cur))


def short(k):
    # demangled without the parameter list: the same key before and after a signature change
    try:
        return subprocess.run(["c++filt", "-p", k], capture_output=True, text=True).stdout.strip() or k
    except OSError:
        return k


def diff(a, b):
    def load(p):
        return {(r["unit"], r["kernel"]): r for r in map(json.loads, open(p))}
    A, B = load(a), load(b)
    bad = 0
    print("| unit | kernel | VGPRs | SGPRs | SGPR spills (to VGPR lanes) | scratch | occupancy |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(set(A) | set(B)):
        x, y = A.get(k), B.get(k)
        if not x or not y:
            print(f"| {k[0]} | {k[1]} | {'new' if y else 'gone'} | | | | |")
            continue
        cell = lambda f: str(x[f]) if x[f] == y[f] else f"{x[f]} -> {y[f]}"
        print(f"| {k[0]} | {k[1]} | {cell('vgprs')} | {cell('sgprs')} | {cell('sgpr_spill')} | {cell('scratch')} | {cell('occupancy')} |")
        if (x["scratch"] == 0 and y["scratch"] != 0) or y["occupancy"] < x["occupancy"] or y["vgpr_spill"] > x["vgpr_spill"]:
            bad += 1
    print(f"\n{bad} kernel(s) gained scratch or VGPR spills, or lost occupancy")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(HERE, "..", "ternary-spgemm_amd"))
    ap.add_argument("--diff", nargs=2, metavar=("BEFORE", "AFTER"))
    a = ap.parse_args()
    sys.exit(diff(*a.diff) if a.diff else measure(a.pkg))
