#!/usr/bin/env python3
"""A/B of the fused RMSNorm + activation quantisation, two parts.

1. With --parent DIR (a built checkout of the commit before the normquant
   calls): plain `python bench.py` of each checkout, alternating, --rounds runs
   each -- the path every call shares.  Rule: the branch's median timed step
   lies inside the spread of the parent's own repeats (branch median <= parent
   median + (parent max - parent min)).
2. The one gemm_torch_normquant call against the route it replaces, both on
   this checkout: torch RMSNorm in fp32 (x * rsqrt(mean(x^2) + eps) * g, a
   normalised fp32 copy of X in memory), then gemm_torch_actquant on that copy.
   bf16 X, bf16 Y, a column scale, at (M, K, N) = (512, 4096, 4096) and (4096,
   4096, 16384), s = 4.  The two routes alternate, each round of each route in a
   fresh child process under its own time limit; per child and shape: warm-up,
   then --windows windows of --steps calls between two device events.  torch's
   mean is another sum shape and rsqrt another rounding, so the routes' bits
   can differ in a few elements: the script reports the share and does not
   compare further (the tests pin the bits).  A recorded number, not a gate.

Needs one MI355X.  Every measurement is one JSON line of --out (default
profiles/normquant_ab.jsonl), the last line the medians and the verdict.

    scripts/normquant_ab.py [--parent DIR] [--rounds 5] [--leg-rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((512, 4096, 4096), (4096, 4096, 16384))
S, SEED, EPS = 4, 42, 1e-5


def leg(which, steps, windows, warmup):
    """Runs inside a child process: one route, both shapes."""
    sys.path.insert(0, os.path.join(REPO, "ternary-spgemm_amd"))
    import torch
    import tspgemm as T
    g = torch.Generator(device="cuda").manual_seed(12345)
    for M, K, N in SHAPES:
        h = T.TCSCDevice(*T.gen_tcsc(K, N, S, SEED), K, N)
        h.reserve(M)
        b = torch.linspace(-1, 1, N, device="cuda")
        cs = torch.rand(N, generator=g, device="cuda") * 1.5 + 0.5
        gamma = torch.rand(K, generator=g, device="cuda") + 0.5
        X = torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16)
        Y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        deq = torch.empty(M, device="cuda")

        def torch_route():
            x = X.float()
            xn = x * torch.rsqrt(x.pow(2).mean(dim=1, keepdim=True) + EPS) * gamma
            h.gemm_torch_actquant(xn, b, Y, col_scale=cs, row_scale_out=deq)

        def fused():
            h.gemm_torch_normquant(X, b, gamma, EPS, Y, col_scale=cs, row_scale_out=deq)

        step = fused if which == "fused" else torch_route
        torch_route()
        other = Y.clone()
        fused()
        torch.cuda.synchronize()
        differ = float((Y.view(torch.int16) != other.view(torch.int16)).float().mean())
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
        print("LEG " + json.dumps({"route": which, "M": M, "K": K, "N": N, "s": S, "xtype": "bfloat16",
                                   "ytype": "bfloat16", "kernel": h.call_kernel(M), "steps": steps,
                                   "ms_per_step": ms, "share_of_y_differing_between_routes": differ}), flush=True)
        h.close()


def child(args, cwd, limit):
    env = dict(os.environ)
    env.pop("TSG_LIB", None)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode:
        sys.exit(f"{args} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the commit before the normquant calls (part 1)")
    ap.add_argument("--rounds", type=int, default=5, help="bench.py runs per checkout")
    ap.add_argument("--leg-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "normquant_ab.jsonl"))
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.steps, a.windows, a.warmup)
    me = os.path.abspath(__file__)
    bench, legs = {}, {}
    verdict = {"what": "verdict"}
    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        if a.parent:
            trees = {"parent": os.path.abspath(a.parent), "branch": REPO}
            for rnd in range(a.rounds):
                for name, tree in trees.items():
                    line = [ln for ln in child(["bench.py"], tree, 480).splitlines() if ln.startswith("{")][-1]
                    r = json.loads(line)
                    emit({"what": "bench configs[2]", "commit": name, "round": rnd, "ms_per_step": r["ms_per_step"],
                          "value": r["value"], "unit": r.get("unit")})
                    bench.setdefault(name, []).append(r["ms_per_step"])
            p, b = bench["parent"], bench["branch"]
            pm, bm, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
            verdict["shared_path"] = {"rule": "branch median <= parent median + (parent max - parent min)",
                                      "parent_median_ms": pm, "branch_median_ms": bm, "parent_spread_ms": spread,
                                      "branch_spread_ms": max(b) - min(b), "ok": bm <= pm + spread}
        for rnd in range(a.leg_rounds):
            for which in ("torch", "fused"):
                out = child([me, "--leg", which, "--steps", str(a.steps), "--windows", str(a.windows), "--warmup",
                             str(a.warmup)], REPO, 600)
                for ln in out.splitlines():
                    if ln.startswith("LEG "):
                        rec = json.loads(ln[4:])
                        emit({"what": "leg", "round": rnd, **rec})
                        legs.setdefault((rec["M"], rec["K"], rec["N"], which), []).extend(rec["ms_per_step"])
        cases = []
        for M, K, N in SHAPES:
            if (M, K, N, "torch") not in legs:
                continue
            t, u = legs[(M, K, N, "torch")], legs[(M, K, N, "fused")]
            mt, mu = statistics.median(t), statistics.median(u)
            cases.append({"M": M, "K": K, "N": N, "torch_route_median_ms": mt, "fused_median_ms": mu,
                          "torch_route_spread_ms": max(t) - min(t), "fused_spread_ms": max(u) - min(u),
                          "fused_over_torch": mu / mt})
        verdict["fused_against_torch_route"] = {"expected": "the fused route is not slower (recorded, not a gate)",
                                                "cases": cases}
        emit(verdict)
    return 0 if verdict.get("shared_path", {}).get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
