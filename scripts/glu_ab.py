#!/usr/bin/env python3
"""A/B of the fused gate/up call (tcsc_hip_gemm_dev_glu; tsg_i8glu.hip) against
the two-call sequence it replaces, the table of DESIGN.md 4.7.

Needs one MI355X and two built checkouts: this one (the branch) and the commit
before the call (--parent DIR, built with its own `python __graft_entry__.py`).
Everything alternates parent / branch on the same card, each run in a fresh
child process.

  1. The untouched path: plain `python bench.py` of each checkout, --rounds
     times each.  Rule: the branch's median ms_per_step is at most the parent's
     median plus the parent's own max - min spread.
  2. Gate and up of a gated FFN on dense W (from_dense, two thirds nonzero) and
     on s = 4, at (K, N) = (4096, 16384) and (2560, 6912), M = 1, 8, 32, 64,
     512, 4096, bf16 Y, both scales, act relu2; for int8 X and for quant="act"
     with bf16 X; --leg-rounds times each:
       (a) parent: gemm_torch_ex on up into an fp32 U, then on gate with mul = U,
           under set_i8_mfma(2) (the integer kernels: the fastest two-call form);
       (b) branch: gemm_torch_glu; once per cell it checks that its Y is the
           two-call sequence's, byte for byte.
     Per child and cell: warm-up, then --windows windows of --steps steps
     between two device events.

Every measurement is one JSON line of --out (default profiles/glu_ab.jsonl);
the last line is the verdict: per cell the medians, the max - min spreads and
whether (b) wins by more than (a)'s spread.  Exit status 1 when the untouched
path misses its rule.

    scripts/glu_ab.py --parent ../parent-checkout [--rounds 5] [--leg-rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 42
SHAPES_KN = ((4096, 16384), (2560, 6912))
SHAPES_M = (1, 8, 32, 64, 512, 4096)


def handle(T, w, K, N, seed):
    if w != "dense":
        return T.TCSCDevice(*T.gen_tcsc(K, N, int(w[1:]), seed), K, N)
    import numpy as np
    return T.TCSCDevice.from_dense(np.random.default_rng(seed).integers(-1, 2, size=(K, N)).astype(np.int32))


def leg(which, pkg, weights, Ms, steps, windows, warmup):
    """Runs inside a child process: one leg on the checkout whose package is `pkg`."""
    sys.path.insert(0, pkg)
    import torch
    import tspgemm as T
    g = torch.Generator(device="cuda").manual_seed(12345)
    for K, N in SHAPES_KN:
        b, bu = torch.linspace(-1, 1, N, device="cuda"), torch.linspace(1, -0.5, N, device="cuda")
        cs, csu = (torch.rand(N, generator=g, device="cuda") * 0.06 + 0.02 for _ in range(2))
        for w in weights:
            hg, hu = handle(T, w, K, N, SEED), handle(T, w, K, N, SEED + 1)
            for h in (hg, hu):
                h.set_i8_mfma(2)
            for M in Ms:
                X8 = torch.randint(-127, 128, (M, K), generator=g, device="cuda", dtype=torch.int32).to(torch.int8)
                Xb = (torch.randn((M, K), generator=g, device="cuda") * 3).to(torch.bfloat16)
                rs = (torch.rand(M, generator=g, device="cuda") * 1.5 + 0.5) / 127.0
                Y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
                U = torch.empty((M, N), dtype=torch.float32, device="cuda")
                for xname, kw in (("int8", dict(X=X8, row_scale=rs)), ("actquant bf16", dict(X=Xb, quant="act"))):
                    X = kw.pop("X")

                    def two():
                        hu.gemm_torch_ex(X, bu, U, col_scale=csu, **kw)
                        hg.gemm_torch_ex(X, b, Y, act="relu2", mul=U, col_scale=cs, **kw)

                    def one():
                        hg.gemm_torch_glu(hu, X, b, bu, Y, act="relu2", col_scale=cs, col_scale_up=csu, **kw)
                    step = two
                    if which == "b":
                        two()
                        want = Y.clone()
                        Y.zero_()
                        one()
                        torch.cuda.synchronize()
                        assert torch.equal(Y.view(torch.int16), want.view(torch.int16)), (w, K, N, M, xname)
                        step = one
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
                    print("LEG " + json.dumps({"leg": which, "W": w, "M": M, "K": K, "N": N, "x": xname,
                                               "ytype": "bfloat16", "steps": steps, "ms_per_step": ms}), flush=True)
            hg.close(), hu.close()


def child(args, cwd):
    env = dict(os.environ)
    env.pop("TSG_LIB", None)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=1100)
    if r.returncode:
        sys.exit(f"{args} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the commit before the call")
    ap.add_argument("--rounds", type=int, default=5, help="bench.py runs per checkout")
    ap.add_argument("--leg-rounds", type=int, default=3)
    ap.add_argument("--weights", default="dense,s4")
    ap.add_argument("--ms", default=",".join(map(str, SHAPES_M)))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "glu_ab.jsonl"))
    ap.add_argument("--leg", nargs=2, metavar=("LEG", "PKG"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    weights, Ms = a.weights.split(","), [int(m) for m in a.ms.split(",")]
    if a.leg:
        return leg(a.leg[0], a.leg[1], weights, Ms, a.steps, a.windows, a.warmup)
    if not a.parent:
        ap.error("--parent is required")
    trees = {"parent": os.path.abspath(a.parent), "branch": REPO}
    me = os.path.abspath(__file__)
    bench, legs = {}, {}
    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        for rnd in range(a.leg_rounds):
            for which, name in (("a", "parent"), ("b", "branch")):
                out = child([me, "--leg", which, os.path.join(trees[name], "ternary-spgemm_amd"), "--weights", a.weights,
                             "--ms", a.ms, "--steps", str(a.steps), "--windows", str(a.windows), "--warmup",
                             str(a.warmup)], trees[name])
                for rec in (json.loads(ln[4:]) for ln in out.splitlines() if ln.startswith("LEG ")):
                    emit({"what": "leg", "round": rnd, "commit": name, **rec})
                    legs.setdefault((rec["K"], rec["N"], rec["W"], rec["x"], rec["M"], which), []).extend(rec["ms_per_step"])
        for rnd in range(a.rounds):
            for name, tree in trees.items():
                r = json.loads([ln for ln in child(["bench.py"], tree).splitlines() if ln.startswith("{")][-1])
                emit({"what": "bench", "commit": name, "round": rnd, "ms_per_step": r["ms_per_step"], "value": r["value"],
                      "unit": r.get("unit")})
                bench.setdefault(name, []).append(r["ms_per_step"])
        verdict = {"what": "verdict", "cases": []}
        if bench:
            p, b = bench["parent"], bench["branch"]
            pm, bm, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
            verdict["untouched_path"] = {"rule": "branch median <= parent median + (parent max - parent min)",
                                         "parent_median_ms": pm, "branch_median_ms": bm, "parent_spread_ms": spread,
                                         "branch_spread_ms": max(b) - min(b), "ok": bm <= pm + spread}
        for key in sorted(k[:5] for k in legs if k[5] == "a"):
            xa, xb = legs[key + ("a",)], legs[key + ("b",)]
            ma, mb = statistics.median(xa), statistics.median(xb)
            verdict["cases"].append({"K": key[0], "N": key[1], "W": key[2], "x": key[3], "M": key[4], "a_median_ms": ma,
                                     "b_median_ms": mb, "a_spread_ms": max(xa) - min(xa),
                                     "b_spread_ms": max(xb) - min(xb), "a_over_b": ma / mb,
                                     "b_wins_past_spread": mb < ma - (max(xa) - min(xa))})
        emit(verdict)
    return 0 if verdict.get("untouched_path", {"ok": True})["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
