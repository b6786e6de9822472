#!/usr/bin/env python3
"""A/B of the narrow-X calls: what does handing a bf16 or int8 X to
gemm_torch_x buy over widening it first?

Needs one MI355X.  Two legs per (shape, X type), alternated --rounds times on
the same card, each leg in a fresh child process:
  (a) the way before the narrow-X calls: Xf = X.float(), then gemm_torch(Xf).
      The cast is inside the timed window and its traffic (s M K bytes read,
      4 M K written, s the element size) is recorded.  With --parent DIR the
      leg imports tspgemm from DIR/ternary-spgemm_amd, a built checkout of the
      commit before the narrow-X calls; without it the leg runs this
      checkout's fp32 path, which is the same code.
  (b) gemm_torch_x(X) on this checkout.
Shapes: BASELINE configs[2] (M = 4096, K = 4096, N = 16384, s = 4) and M = 64
and M = 16 on the same W.  Per child and (shape, type): warm-up, then
--windows windows of --steps calls between two device events; a record holds
every window's ms per step.  Leg (b) also checks once per (shape, type) that
its Y equals gemm_torch(X.float()) bit for bit.

Every measurement is one JSON line of --out (default profiles/xtype_ab.jsonl);
the last line holds, per (shape, type), both legs' medians over all windows
and rounds, their max - min spreads, and the ratio b / a.  No pass / fail: the
expectation is (b) no slower than (a) beyond (a)'s spread.

    scripts/xtype_ab.py [--parent DIR] [--rounds 3] [--steps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, S, SEED = 4096, 16384, 4, 42
SHAPES_M = (4096, 64, 16)
TYPES = ("bfloat16", "int8")


def leg(which, pkg, steps, windows, warmup):
    """Runs inside a child process: the legs of the checkout whose package is `pkg`."""
    sys.path.insert(0, pkg)
    import torch
    import tspgemm as T
    h = T.TCSCDevice(*T.gen_tcsc(K, N, S, SEED), K, N)
    b = torch.linspace(-1, 1, N, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(12345)
    for M in SHAPES_M:
        Y = torch.empty((M, N), device="cuda")
        for name in TYPES:
            if name == "int8":
                X = torch.randint(-127, 128, (M, K), generator=g, device="cuda", dtype=torch.int32).to(torch.int8)
            else:
                X = torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16)
            if which == "a":
                def step():
                    h.gemm_torch(X.float(), b, Y)
            else:
                def step():
                    h.gemm_torch_x(X, b, Y)
                want = h.gemm_torch(X.float(), b)
                step()
                torch.cuda.synchronize()
                assert torch.equal(Y.view(torch.int32), want.view(torch.int32)), (M, name, "narrow != widened")
                del want
            for _ in range(warmup):
                step()
            torch.cuda.synchronize()
            ms = []
            for _ in range(windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    step()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / steps)
            es = X.element_size()
            rec = {"leg": which, "M": M, "K": K, "N": N, "s": S, "xtype": name, "kernel": h.call_kernel(M),
                   "steps": steps, "ms_per_step": ms,
                   "cast_bytes_per_step": (es + 4) * M * K if which == "a" else 0,
                   "x_bytes_resident": (es + 4) * M * K if which == "a" else es * M * K}
            print("LEG " + json.dumps(rec), flush=True)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the commit before the narrow-X calls (leg a)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "xtype_ab.jsonl"))
    ap.add_argument("--leg", nargs=2, metavar=("LEG", "PKG"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg[0], a.leg[1], a.steps, a.windows, a.warmup)
    me = os.path.abspath(__file__)
    series = {}
    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        for rnd in range(a.rounds):
            for which in ("a", "b"):
                env = dict(os.environ)
                env.pop("TSG_LIB", None)
                commit, tree = "branch", REPO
                if which == "a" and a.parent:
                    commit, tree = "parent", os.path.abspath(a.parent)
                r = subprocess.run([sys.executable, me, "--leg", which, os.path.join(tree, "ternary-spgemm_amd"),
                                    "--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup)],
                                   env=env, capture_output=True, text=True, timeout=900)
                if r.returncode:
                    sys.exit(f"leg {which} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                for ln in r.stdout.splitlines():
                    if ln.startswith("LEG "):
                        rec = json.loads(ln[4:])
                        emit({"what": "leg", "round": rnd, "commit": commit, **rec})
                        series.setdefault((rec["M"], rec["xtype"], which), []).extend(rec["ms_per_step"])
        summary = {"what": "summary", "rule": "expected: b_median <= a_median + a_spread (spread = max - min)",
                   "cases": []}
        for M in SHAPES_M:
            for name in TYPES:
                xa, xb = series[(M, name, "a")], series[(M, name, "b")]
                ma, mb = statistics.median(xa), statistics.median(xb)
                summary["cases"].append({"M": M, "xtype": name, "a_median_ms": ma, "b_median_ms": mb,
                                         "a_spread_ms": max(xa) - min(xa), "b_spread_ms": max(xb) - min(xb),
                                         "b_over_a": mb / ma, "as_expected": mb <= ma + (max(xa) - min(xa))})
        emit(summary)
    return 0


if __name__ == "__main__":
    sys.exit(main())
