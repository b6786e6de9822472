#!/usr/bin/env python3
"""A/B of the fused epilogue (tcsc_hip_gemm_dev_ex), two parts.

1. With --parent DIR (a built checkout of the commit before the descriptor
   call): plain `python bench.py` of each checkout, alternating, --rounds runs
   each -- the default path, which the epilogue must leave as it was.  Rule:
   the branch's median timed step lies inside the spread of the parent's own
   repeats (branch median <= parent median + (parent max - parent min)).
2. One gemm_torch_ex call with relu2, a bf16 gate and a bf16 residual into a
   bf16 Y against the route it replaces, both on this checkout:
   gemm_torch_scaled into an fp32 Y, then torch's relu, square, multiply, add
   and cast as separate elementwise passes.  bf16 X, a column scale, at
   BASELINE.json configs[2]'s shape (M, K, N) = (4096, 4096, 16384), s = 4, and
   at a decode-sized M = 64 of the same W.  The two routes alternate, each
   round of each route in a fresh child process under its own time limit; per
   child and shape: warm-up, then --windows windows between two device events,
   each of as many calls as fill about --window-ms of device time (from a short
   probe of the route, at least --steps: 20 calls of a 70 us step would be a
   window of 1.4 ms, too short to time).  The share of Y whose bits differ between the routes is
   reported (the tests pin the bits).  A recorded number, not a gate.

3. With --parent: the rx fallback kernel (TSG_KERNEL=rx; bench.py never runs
   it), whose store branches the compiler schedules together with the new one:
   its fp32, its 16-bit and its scaled calls, each checkout's own library,
   alternating, at (2048, 2048, 4096), timed like part 2.

Needs one MI355X.  Every measurement is one JSON line of --out (default
profiles/epilogue_ab.jsonl) that names the method, the shape and the commit;
the last line holds the medians and the verdict.

    scripts/epilogue_ab.py [--parent DIR] [--commit NAME] [--rounds 5] [--leg-rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((4096, 4096, 16384), (64, 4096, 16384))
S, SEED = 4, 42


def leg(which, steps, windows, warmup, window_ms):
    """Runs inside a child process: one route, every shape."""
    sys.path.insert(0, os.path.join(REPO, "ternary-spgemm_amd"))
    import torch
    import tspgemm as T
    g = torch.Generator(device="cuda").manual_seed(12345)
    bf16 = torch.bfloat16
    for M, K, N in SHAPES:
        h = T.TCSCDevice(*T.gen_tcsc(K, N, S, SEED), K, N)
        h.reserve(M)
        b = torch.linspace(-1, 1, N, device="cuda")
        cs = (torch.rand(N, generator=g, device="cuda") * 1.5 + 0.5) * 2.0 ** -6
        X = torch.randn((M, K), generator=g, device="cuda").to(bf16)
        G = torch.randn((M, N), generator=g, device="cuda").to(bf16)
        R = torch.randn((M, N), generator=g, device="cuda").to(bf16)
        Y = torch.empty((M, N), dtype=bf16, device="cuda")
        Y32 = torch.empty((M, N), device="cuda")

        def torch_route():
            h.gemm_torch_scaled(X, b, Y32, col_scale=cs)
            r = torch.relu(Y32)
            Y.copy_(r * r * G + R)

        def fused():
            h.gemm_torch_ex(X, b, Y, act="relu2", mul=G, add=R, col_scale=cs)

        step = fused if which == "fused" else torch_route
        torch_route()
        other = Y.clone()
        fused()
        torch.cuda.synchronize()
        differ = float((Y.view(torch.int16) != other.view(torch.int16)).float().mean())
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        e1.synchronize()
        steps = max(steps, int(window_ms / (e0.elapsed_time(e1) / steps)))  # calls per timed window
        ms = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / steps)
        method = "gemm_torch_ex relu2 * G + R -> bf16" if which == "fused" else \
            "gemm_torch_scaled -> fp32, torch relu, square, mul, add, cast"
        print("LEG " + json.dumps({"method": method, "route": which, "M": M, "K": K, "N": N, "s": S,
                                   "xtype": "bfloat16", "ytype": "bfloat16", "kernel": h.call_kernel(M),
                                   "steps": steps, "ms_per_step": ms,
                                   "share_of_y_differing_between_routes": differ}), flush=True)
        h.close()


def rx_leg(pkg, steps, windows, warmup, window_ms):
    """Runs inside a child process with TSG_KERNEL=rx: the existing calls of the package at pkg."""
    sys.path.insert(0, pkg)
    import torch
    import tspgemm as T
    M, K, N = 2048, 2048, 4096
    g = torch.Generator(device="cuda").manual_seed(12345)
    h = T.TCSCDevice(*T.gen_tcsc(K, N, S, SEED), K, N)
    assert h.call_kernel(M) == "tsg_tcsc_rx_kernel", h.call_kernel(M)
    h.reserve(M)
    b = torch.linspace(-1, 1, N, device="cuda")
    cs = (torch.rand(N, generator=g, device="cuda") * 1.5 + 0.5) * 2.0 ** -6
    X = torch.randn((M, K), generator=g, device="cuda")
    Y32 = torch.empty((M, N), device="cuda")
    Y16 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    routes = {"gemm_torch -> fp32": lambda: h.gemm_torch_into(X, b, Y32),
              "gemm_torch_xy -> bf16": lambda: h.gemm_torch_xy(X, b, Y16),
              "gemm_torch_scaled (column scale) -> bf16": lambda: h.gemm_torch_scaled(X, b, Y16, col_scale=cs)}
    for method, step in routes.items():
        n = steps
        for _ in range(warmup):
            step()
        ms = []
        for w in range(windows + 1):  # window 0: the probe that sizes the others
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                step()
            e1.record()
            e1.synchronize()
            if w == 0:
                n = max(steps, int(window_ms / (e0.elapsed_time(e1) / n)))
            else:
                ms.append(e0.elapsed_time(e1) / n)
        print("LEG " + json.dumps({"method": method, "M": M, "K": K, "N": N, "s": S, "kernel": h.call_kernel(M),
                                   "steps": n, "ms_per_step": ms}), flush=True)
    h.close()


def child(args, cwd, limit, extra_env=None):
    env = dict(os.environ)
    env.update(extra_env or {})
    env.pop("TSG_LIB", None)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode:
        sys.exit(f"{args} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the commit before the descriptor call (part 1)")
    ap.add_argument("--keep-bench", help="an earlier --out file whose part 1 lines are kept (parts 2 and 3 are rerun)")
    ap.add_argument("--commit", default="this change", help="how the lines name this checkout")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--rounds", type=int, default=5, help="bench.py runs per checkout")
    ap.add_argument("--leg-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="calls per window at least")
    ap.add_argument("--window-ms", type=float, default=200.0, help="device time a timed window should fill")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "epilogue_ab.jsonl"))
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg and a.leg.startswith("rx:"):
        return rx_leg(a.leg[3:], a.steps, a.windows, a.warmup, a.window_ms)
    if a.leg:
        return leg(a.leg, a.steps, a.windows, a.warmup, a.window_ms)
    me = os.path.abspath(__file__)
    bench, legs = {}, {}
    verdict = {"what": "verdict", "commit": a.commit}
    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        trees = {a.parent_commit: os.path.abspath(a.parent), a.commit: REPO} if a.parent else {}
        if a.keep_bench:
            for rec in map(json.loads, open(a.keep_bench).read().splitlines()):
                if rec.get("what") == "bench":
                    emit(rec)
                elif rec.get("what") == "verdict" and "default_path" in rec:
                    verdict["default_path"] = rec["default_path"]
        if a.parent and not a.keep_bench:
            for rnd in range(a.rounds):
                for name, tree in trees.items():
                    line = [ln for ln in child(["bench.py"], tree, 480).splitlines() if ln.startswith("{")][-1]
                    r = json.loads(line)
                    emit({"what": "bench", "method": "python bench.py (tcsc_hip_gemm_dev, fp32)", "shape": "configs[2]",
                          "M": 4096, "K": 4096, "N": 16384, "commit": name, "round": rnd,
                          "ms_per_step": r["ms_per_step"], "value": r["value"], "unit": r.get("unit")})
                    bench.setdefault(name, []).append(r["ms_per_step"])
            p, b = bench[a.parent_commit], bench[a.commit]
            pm, bm, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
            verdict["default_path"] = {"rule": "branch median <= parent median + (parent max - parent min)",
                                       "parent_median_ms": pm, "branch_median_ms": bm, "parent_spread_ms": spread,
                                       "branch_spread_ms": max(b) - min(b), "ok": bm <= pm + spread}
        for rnd in range(a.leg_rounds):
            for which in ("torch", "fused"):
                out = child([me, "--leg", which, "--steps", str(a.steps), "--windows", str(a.windows), "--warmup",
                             str(a.warmup), "--window-ms", str(a.window_ms)], REPO, 600)
                for ln in out.splitlines():
                    if ln.startswith("LEG "):
                        rec = json.loads(ln[4:])
                        emit({"what": "leg", "commit": a.commit, "round": rnd, **rec})
                        legs.setdefault((rec["M"], rec["K"], rec["N"], which), []).extend(rec["ms_per_step"])
        if a.parent:
            rx = {}
            for rnd in range(a.leg_rounds):
                for name, tree in trees.items():
                    out = child([me, "--leg", "rx:" + os.path.join(tree, "ternary-spgemm_amd"), "--steps", str(a.steps),
                                 "--windows", str(a.windows), "--warmup", str(a.warmup), "--window-ms",
                                 str(a.window_ms)], REPO, 600, {"TSG_KERNEL": "rx"})
                    for ln in out.splitlines():
                        if ln.startswith("LEG "):
                            rec = json.loads(ln[4:])
                            emit({"what": "rx", "commit": name, "round": rnd, **rec})
                            rx.setdefault((rec["method"], name), []).extend(rec["ms_per_step"])
            verdict["rx_kernel"] = [
                {"method": m, "parent_median_ms": statistics.median(rx[(m, a.parent_commit)]),
                 "branch_median_ms": statistics.median(rx[(m, a.commit)]),
                 "parent_spread_ms": max(rx[(m, a.parent_commit)]) - min(rx[(m, a.parent_commit)])}
                for m in sorted({m for m, _ in rx})]
        cases = []
        for M, K, N in SHAPES:
            if (M, K, N, "torch") not in legs:
                continue
            t, u = legs[(M, K, N, "torch")], legs[(M, K, N, "fused")]
            mt, mu = statistics.median(t), statistics.median(u)
            cases.append({"M": M, "K": K, "N": N, "torch_route_median_ms": mt, "fused_median_ms": mu,
                          "torch_route_spread_ms": max(t) - min(t), "fused_spread_ms": max(u) - min(u),
                          "fused_over_torch": mu / mt})
        verdict["fused_against_torch_route"] = {"expected": "recorded, not a gate", "cases": cases}
        emit(verdict)
    return 0 if verdict.get("default_path", {}).get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
