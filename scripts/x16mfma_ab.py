#!/usr/bin/env python3
"""A/B of the 16-bit matrix-core kernel (tcsc_hip_set_x16_mfma) against the add
streams, the table of DESIGN.md 4.8.  Nothing is routed automatically, so no
threshold comes out of it: losing cells are reported like winning ones.

Needs one MI355X and two built checkouts: this one (the branch) and the commit
before the kernel (--parent DIR, built with its own `python __graft_entry__.py`).
Everything alternates parent / branch on the same card, each run in a fresh
child process.

  1. The untouched path: plain `python bench.py` (fp32 X) of each checkout,
     --rounds times each.  Rule: the branch's median ms_per_step is at most the
     parent's median plus the parent's own max - min spread.
  2. The 16-bit call, gemm_torch_scaled with bf16 X, bf16 Y and a column scale,
     at K = 4096, N = 16384 for M in 64, 512, 4096 on W at s = 2, 4, 16 and on
     one dense W drawn two-thirds nonzero (from_dense), --leg-rounds times each:
       (a) parent: the call as it is (the staging pass and the add streams);
       (b) branch: the same call with set_x16_mfma(1); once per shape it checks
           that its Y is the mode-0 call's, byte for byte (X is integer-valued,
           |x| <= 8: every partial sum is exact, the contract's exact case).
     Per child and shape: warm-up, then --windows windows of --steps calls
     between two device events.

Every measurement is one JSON line of --out (default profiles/x16mfma_ab.jsonl);
the last line is the verdict: per (W, M) the medians, the spreads and whether
(b) wins by more than (a)'s spread.  Exit status 1 when the untouched path
misses its rule.

    scripts/x16mfma_ab.py --parent ../parent-checkout [--rounds 5] [--leg-rounds 3] [--weights s2,s4,s16,dense]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, SEED = 4096, 16384, 42
SHAPES_M = (64, 512, 4096)


def handle(T, w):
    """The handle of weight set `w`: s2 / s4 / s16 (gen_tcsc) or dense (two thirds nonzero)."""
    if w != "dense":
        return T.TCSCDevice(*T.gen_tcsc(K, N, int(w[1:]), SEED), K, N)
    import numpy as np
    return T.TCSCDevice.from_dense(np.random.default_rng(SEED).integers(-1, 2, size=(K, N)).astype(np.int32))


def leg(which, pkg, weights, steps, windows, warmup):
    """Runs inside a child process: one leg on the checkout whose package is `pkg`."""
    sys.path.insert(0, pkg)
    import torch
    import tspgemm as T
    b = torch.linspace(-1, 1, N, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(12345)
    for w in weights:
        h = handle(T, w)
        nnz = h.info()["nnz_pos"] + h.info()["nnz_neg"]
        for M in SHAPES_M:
            X = torch.randint(-8, 9, (M, K), generator=g, device="cuda", dtype=torch.int32).to(torch.bfloat16)
            cs = torch.rand(N, generator=g, device="cuda") * 1.5 + 0.5
            Y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")

            def step():
                h.gemm_torch_scaled(X, b, Y, col_scale=cs)
            if which == "b":
                step()
                want = Y.clone()
                h.set_x16_mfma(1)
                assert h.call_x16_mfma(M, T.TSG_X_BF16) == 1
                Y.zero_()
                step()
                torch.cuda.synchronize()
                assert torch.equal(Y.view(torch.int16), want.view(torch.int16)), (w, M, "matrix cores != add streams")
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
            rec = {"leg": which, "W": w, "M": M, "K": K, "N": N, "density": nnz / (K * N), "xtype": "bfloat16",
                   "ytype": "bfloat16", "kernel": "tsg_x16mfma_kernel" if which == "b" else h.call_kernel(M),
                   "steps": steps, "ms_per_step": ms}
            print("LEG " + json.dumps(rec), flush=True)
        h.close()


def child(args, cwd):
    env = dict(os.environ)
    env.pop("TSG_LIB", None)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=1100)
    if r.returncode:
        sys.exit(f"{args} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the commit before the kernel")
    ap.add_argument("--rounds", type=int, default=5, help="bench.py runs per checkout")
    ap.add_argument("--leg-rounds", type=int, default=3)
    ap.add_argument("--weights", default="s2,s4,s16,dense")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "x16mfma_ab.jsonl"))
    ap.add_argument("--leg", nargs=2, metavar=("LEG", "PKG"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    weights = a.weights.split(",")
    if a.leg:
        return leg(a.leg[0], a.leg[1], weights, a.steps, a.windows, a.warmup)
    if not a.parent:
        ap.error("--parent is required")
    trees = {"parent": os.path.abspath(a.parent), "branch": REPO}
    me = os.path.abspath(__file__)
    bench, legs, dens = {}, {}, {}
    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        for rnd in range(a.rounds):
            for name, tree in trees.items():
                line = [ln for ln in child(["bench.py"], tree).splitlines() if ln.startswith("{")][-1]
                r = json.loads(line)
                emit({"what": "bench fp32 X", "commit": name, "round": rnd, "ms_per_step": r["ms_per_step"],
                      "value": r["value"], "unit": r.get("unit")})
                bench.setdefault(name, []).append(r["ms_per_step"])
        for rnd in range(a.leg_rounds):
            for which, name in (("a", "parent"), ("b", "branch")):
                out = child([me, "--leg", which, os.path.join(trees[name], "ternary-spgemm_amd"), "--weights", a.weights,
                             "--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup)], trees[name])
                for ln in out.splitlines():
                    if ln.startswith("LEG "):
                        rec = json.loads(ln[4:])
                        emit({"what": "leg", "round": rnd, "commit": name, **rec})
                        legs.setdefault((rec["W"], rec["M"], which), []).extend(rec["ms_per_step"])
                        dens[rec["W"]] = rec["density"]
        verdict = {"what": "verdict", "cases": []}
        if bench:
            p, b = bench["parent"], bench["branch"]
            pm, bm, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
            verdict["untouched_path"] = {"rule": "branch median <= parent median + (parent max - parent min)",
                                         "parent_median_ms": pm, "branch_median_ms": bm, "parent_spread_ms": spread,
                                         "branch_spread_ms": max(b) - min(b), "ok": bm <= pm + spread}
        for w in weights if a.leg_rounds else ():
            for M in SHAPES_M:
                xa, xb = legs[(w, M, "a")], legs[(w, M, "b")]
                ma, mb = statistics.median(xa), statistics.median(xb)
                verdict["cases"].append({"W": w, "density": dens[w], "M": M, "a_median_ms": ma, "b_median_ms": mb,
                                         "a_spread_ms": max(xa) - min(xa), "b_spread_ms": max(xb) - min(xb),
                                         "a_over_b": ma / mb, "b_wins_past_spread": mb < ma - (max(xa) - min(xa))})
        emit(verdict)
    return 0 if verdict.get("untouched_path", {"ok": True})["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
