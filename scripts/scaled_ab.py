#!/usr/bin/env python3
"""A/B of the scaled calls: is the unscaled path as fast as before, and what do
the epilogue scales buy over scaling an fp32 Y in a second pass?

Needs one MI355X and two built checkouts: this one (the branch) and the commit
before the scaled calls (--parent DIR, built with its own
`python __graft_entry__.py`).  Everything alternates parent / branch on the
same card, each run in a fresh child process.

  1. The unscaled path: plain `python bench.py` (configs[2]) of each checkout,
     --rounds times each.  Rule: the branch's median ms_per_step is at most
     the parent's median plus the parent's own max - min spread.
  2. What the feature buys, at K = 4096, N = 16384, s = 4 for M = 4096, 64 and
     16, int8 X, bf16 Y, --leg-rounds times each:
       (a) parent: gemm_torch_x(X, zeros, Y32), then
           Y32.mul_(rs[:, None]).mul_(cs).add_(b), then Y16.copy_(Y32) -- all
           inside the timed window (the caller's second pass over Y);
       (b) branch: the one gemm_torch_scaled(X, b, Y16, row_scale=rs,
           col_scale=cs).  Once per shape leg (b) checks that its Y is leg
           (a)'s result bit for bit.
     Per child and shape: warm-up, then --windows windows of --steps calls
     between two device events.  Expectation: b_median <= a_median + a_spread.

Every measurement is one JSON line of --out (default profiles/scaled_ab.jsonl);
the last line is the verdict of both parts.  Exit status 1 when the unscaled
path misses its rule; part 2 is recorded as it comes out.

    scripts/scaled_ab.py --parent ../parent-checkout [--rounds 5] [--leg-rounds 3] [--out FILE]
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


def leg(which, pkg, steps, windows, warmup):
    """Runs inside a child process: one leg on the checkout whose package is `pkg`."""
    sys.path.insert(0, pkg)
    import torch
    import tspgemm as T
    h = T.TCSCDevice(*T.gen_tcsc(K, N, S, SEED), K, N)
    b = torch.linspace(-1, 1, N, device="cuda")
    zeros = torch.zeros(N, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(12345)
    for M in SHAPES_M:
        X = torch.randint(-127, 128, (M, K), generator=g, device="cuda", dtype=torch.int32).to(torch.int8)
        rs = (torch.rand(M, generator=g, device="cuda") * 1.5 + 0.5) / 127.0
        cs = torch.rand(N, generator=g, device="cuda") * 1.5 + 0.5
        Y16 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        Y32 = torch.empty((M, N), device="cuda")

        def step_a():
            h.gemm_torch_x(X, zeros, Y32)
            Y32.mul_(rs[:, None]).mul_(cs).add_(b)
            Y16.copy_(Y32)
        if which == "a":
            step = step_a
        else:
            def step():
                h.gemm_torch_scaled(X, b, Y16, row_scale=rs, col_scale=cs)
            step_a()
            want = Y16.clone()
            Y16.zero_()
            step()
            torch.cuda.synchronize()
            assert torch.equal(Y16.view(torch.int16), want.view(torch.int16)), (M, "scaled epilogue != second pass")
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
        rec = {"leg": which, "M": M, "K": K, "N": N, "s": S, "xtype": "int8", "ytype": "bfloat16",
               "kernel": h.call_kernel(M), "steps": steps, "ms_per_step": ms,
               "y_bytes_stored_by_kernel": (4 if which == "a" else 2) * M * N,
               "second_pass_bytes_per_step": (3 * 8 + 6) * M * N if which == "a" else 0}
        print("LEG " + json.dumps(rec), flush=True)
    h.close()


def child(args, cwd):
    env = dict(os.environ)
    env.pop("TSG_LIB", None)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode:
        sys.exit(f"{args} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the commit before the scaled calls")
    ap.add_argument("--rounds", type=int, default=5, help="bench.py runs per checkout")
    ap.add_argument("--leg-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scaled_ab.jsonl"))
    ap.add_argument("--leg", nargs=2, metavar=("LEG", "PKG"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg[0], a.leg[1], a.steps, a.windows, a.warmup)
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
        for rnd in range(a.rounds):
            for name, tree in trees.items():
                line = [ln for ln in child(["bench.py"], tree).splitlines() if ln.startswith("{")][-1]
                r = json.loads(line)
                emit({"what": "bench configs[2]", "commit": name, "round": rnd, "ms_per_step": r["ms_per_step"],
                      "value": r["value"], "unit": r.get("unit")})
                bench.setdefault(name, []).append(r["ms_per_step"])
        for rnd in range(a.leg_rounds):
            for which, name in (("a", "parent"), ("b", "branch")):
                out = child([me, "--leg", which, os.path.join(trees[name], "ternary-spgemm_amd"), "--steps",
                             str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup)], trees[name])
                for ln in out.splitlines():
                    if ln.startswith("LEG "):
                        rec = json.loads(ln[4:])
                        emit({"what": "leg", "round": rnd, "commit": name, **rec})
                        legs.setdefault((rec["M"], which), []).extend(rec["ms_per_step"])
        p, b = bench["parent"], bench["branch"]
        pm, bm, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
        verdict = {"what": "verdict",
                   "unscaled_path": {"rule": "branch median <= parent median + (parent max - parent min)",
                                 "parent_median_ms": pm, "branch_median_ms": bm, "parent_spread_ms": spread,
                                 "branch_spread_ms": max(b) - min(b), "ok": bm <= pm + spread},
                   "scaled": {"rule": "expected: b_median <= a_median + a_spread (spread = max - min)", "cases": []}}
        for M in SHAPES_M:
            xa, xb = legs[(M, "a")], legs[(M, "b")]
            ma, mb = statistics.median(xa), statistics.median(xb)
            verdict["scaled"]["cases"].append({"M": M, "a_median_ms": ma, "b_median_ms": mb,
                                                 "a_spread_ms": max(xa) - min(xa), "b_spread_ms": max(xb) - min(xb),
                                                 "b_over_a": mb / ma, "as_expected": mb <= ma + (max(xa) - min(xa))})
        emit(verdict)
    return 0 if verdict["unscaled_path"]["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
