#!/usr/bin/env python3
"""A/B of the fused activation quantisation: the one gemm_torch_actquant call
against the route a caller had before it -- the torch quantisation ops (abs,
amax, divide, multiply, round, clamp, to(int8)), then gemm_torch_scaled on the
int8 X with the row scale.

Needs one MI355X and this checkout, built.  bf16 X, bf16 Y, a column scale, at
(M, K, N) = (512, 4096, 4096) and (4096, 4096, 16384), s = 4.  The two routes
alternate, each round of each route in a fresh child process; per child and
shape: warm-up, then --windows windows of --steps calls between two device
events.  The torch route's 127 / a is a reciprocal and a multiply (two
roundings), so its bits can differ from the fused call's in a few elements:
the script reports the share and does not compare further (the tests pin the
bits).  A recorded number, not a gate: every measurement is one JSON line of
--out (default profiles/actquant_ab.jsonl), the last line the medians.

    scripts/actquant_ab.py [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((512, 4096, 4096), (4096, 4096, 16384))
S, SEED = 4, 42


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
        X = torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16)
        Y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        deq = torch.empty(M, device="cuda")

        def torch_route():
            x = X.float()
            a = x.abs().amax(dim=1, keepdim=True).clamp_min(1e-5)
            q = (x * (127.0 / a)).round().clamp(-127.0, 127.0).to(torch.int8)
            h.gemm_torch_scaled(q, b, Y, row_scale=(a / 127.0).reshape(M), col_scale=cs)

        def fused():
            h.gemm_torch_actquant(X, b, Y, col_scale=cs, row_scale_out=deq)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "actquant_ab.jsonl"))
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.steps, a.windows, a.warmup)
    me = os.path.abspath(__file__)
    env = dict(os.environ)
    env.pop("TSG_LIB", None)
    legs = {}
    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        for rnd in range(a.rounds):
            for which in ("torch", "fused"):
                r = subprocess.run([sys.executable, me, "--leg", which, "--steps", str(a.steps), "--windows",
                                    str(a.windows), "--warmup", str(a.warmup)], cwd=REPO, env=env, capture_output=True,
                                   text=True, timeout=600)
                if r.returncode:
                    sys.exit(f"leg {which} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                for ln in r.stdout.splitlines():
                    if ln.startswith("LEG "):
                        rec = json.loads(ln[4:])
                        emit({"what": "leg", "round": rnd, **rec})
                        legs.setdefault((rec["M"], rec["K"], rec["N"], which), []).extend(rec["ms_per_step"])
        cases = []
        for M, K, N in SHAPES:
            t, u = legs[(M, K, N, "torch")], legs[(M, K, N, "fused")]
            mt, mu = statistics.median(t), statistics.median(u)
            cases.append({"M": M, "K": K, "N": N, "torch_route_median_ms": mt, "fused_median_ms": mu,
                          "torch_route_spread_ms": max(t) - min(t), "fused_spread_ms": max(u) - min(u),
                          "fused_over_torch": mu / mt})
        emit({"what": "medians", "expected": "the fused route is not slower", "cases": cases})
    return 0


if __name__ == "__main__":
    sys.exit(main())
