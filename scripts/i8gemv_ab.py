#!/usr/bin/env python3
"""A/B of the M <= 32 integer matrix-core kernel (tsg_i8gemv_kernel) against
what the same calls ran before it, the table DESIGN.md 4.7 takes the decode
rule from.

Needs one MI355X and two built checkouts: this one (the branch) and the commit
before the kernel (--parent DIR, built with its own `python __graft_entry__.py`).
Everything alternates parent / branch on the same card, each run in a fresh
child process.

  1. The untouched path: plain `python bench.py` (fp32 X) of each checkout,
     --rounds times each.  Rule: the branch's median ms_per_step is at most the
     parent's median plus the parent's own max - min spread.
  2. The int8 call, gemm_torch_scaled with int8 X, bf16 Y and both scales, at
     (K, N) = (4096, 16384) and (4096, 4096) for M in 1, 8, 16, 32 on W at
     s = 2, 4, 16 and on one dense W drawn two-thirds nonzero (from_dense),
     --leg-rounds times each:
       (a)  parent under mode 0: the walks;
       (a2) parent under mode 2: the 128 x 128 tile kernel (the same child);
       (b)  branch under mode 2: tsg_i8gemv_kernel; once per shape it checks
            that its Y is the walks' (mode 1), byte for byte.
     Per child and shape: warm-up, then --windows windows of --steps calls
     between two device events.
  3. --depth-libs D=PATH,...: leg (b) once more per library built with
     -DTSG_I8GEMV_DEPTH=D (make EXTRA=..., its own BUILD and LIBDIR), on the
     dense W only: the lines that chose the kernel's steps in flight.

Every measurement is one JSON line of --out (default profiles/i8gemv_ab.jsonl);
the last line is the verdict: per (N, W, M) the medians, the spreads, whether
(b) wins by more than (a)'s spread, and (b)'s image bytes per second (K N / 4
bytes over its median).  Exit status 1 when the untouched path misses its rule.

    scripts/i8gemv_ab.py --parent ../parent-checkout [--rounds 5] [--leg-rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SEED = 4096, 42
SHAPES_N = (16384, 4096)
SHAPES_M = (1, 8, 16, 32)


def handle(T, w, N):
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
    g = torch.Generator(device="cuda").manual_seed(12345)
    for N in SHAPES_N:
        b = torch.linspace(-1, 1, N, device="cuda")
        for w in weights:
            h = handle(T, w, N)
            nnz = h.info()["nnz_pos"] + h.info()["nnz_neg"]
            for M in SHAPES_M:
                X = torch.randint(-127, 128, (M, K), generator=g, device="cuda", dtype=torch.int32).to(torch.int8)
                rs = (torch.rand(M, generator=g, device="cuda") * 1.5 + 0.5) / 127.0
                cs = torch.rand(N, generator=g, device="cuda") * 1.5 + 0.5
                Y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")

                def step():
                    h.gemm_torch_scaled(X, b, Y, row_scale=rs, col_scale=cs)
                for name, mode in (("a", 0), ("a2", 2)) if which == "a" else ((which, 2),):
                    h.set_i8_mfma(mode)
                    if which == "a":
                        kernel = "tsg_i8mfma_kernel" if h.call_i8_mfma(M) else h.call_kernel(M)
                    else:
                        h.set_i8_mfma(1)
                        step()
                        want = Y.clone()
                        h.set_i8_mfma(2)
                        assert h.call_i8_kernel(M) == 2
                        kernel = "tsg_i8gemv_kernel"
                        Y.zero_()
                        step()
                        torch.cuda.synchronize()
                        assert torch.equal(Y.view(torch.int16), want.view(torch.int16)), (w, N, M, "split-K != walks")
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
                    rec = {"leg": name, "W": w, "M": M, "K": K, "N": N, "density": nnz / (K * N), "xtype": "int8",
                           "ytype": "bfloat16", "kernel": kernel, "steps": steps, "ms_per_step": ms}
                    print("LEG " + json.dumps(rec), flush=True)
            h.close()


def child(args, cwd, lib=None):
    env = dict(os.environ)
    env.pop("TSG_LIB", None)
    if lib:
        env["TSG_LIB"] = lib
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
    ap.add_argument("--depth-libs", default="", help="D=PATH,... libraries built with -DTSG_I8GEMV_DEPTH=D")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "i8gemv_ab.jsonl"))
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

    def run_leg(which, name, wts, lib=None):
        out = child([me, "--leg", which, os.path.join(trees[name], "ternary-spgemm_amd"), "--weights", wts,
                     "--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup)], trees[name], lib)
        return [json.loads(ln[4:]) for ln in out.splitlines() if ln.startswith("LEG ")]

    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        for rnd in range(a.leg_rounds):
            for which, name in (("a", "parent"), ("b", "branch")):
                for rec in run_leg(which, name, a.weights):
                    emit({"what": "leg", "round": rnd, "commit": name, **rec})
                    legs.setdefault((rec["N"], rec["W"], rec["M"], rec["leg"]), []).extend(rec["ms_per_step"])
                    dens[rec["W"]] = rec["density"]
        for spec in a.depth_libs.split(",") if a.depth_libs else ():
            depth, lib = spec.split("=")
            for rec in run_leg("b", "branch", "dense", os.path.abspath(lib)):
                emit({"what": "depth", "depth": int(depth), "median_ms": statistics.median(rec["ms_per_step"]),
                      "spread_ms": max(rec["ms_per_step"]) - min(rec["ms_per_step"]), **rec})
        for rnd in range(a.rounds):
            for name, tree in trees.items():
                line = [ln for ln in child(["bench.py"], tree).splitlines() if ln.startswith("{")][-1]
                r = json.loads(line)
                emit({"what": "bench fp32 X", "commit": name, "round": rnd, "ms_per_step": r["ms_per_step"],
                      "value": r["value"], "unit": r.get("unit")})
                bench.setdefault(name, []).append(r["ms_per_step"])
        verdict = {"what": "verdict", "cases": []}
        if bench:
            p, b = bench["parent"], bench["branch"]
            pm, bm, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
            verdict["untouched_path"] = {"rule": "branch median <= parent median + (parent max - parent min)",
                                         "parent_median_ms": pm, "branch_median_ms": bm, "parent_spread_ms": spread,
                                         "branch_spread_ms": max(b) - min(b), "ok": bm <= pm + spread}
        for N in SHAPES_N if a.leg_rounds else ():
            for w in weights:
                for M in SHAPES_M:
                    xa, xa2, xb = (legs[(N, w, M, which)] for which in ("a", "a2", "b"))
                    ma, ma2, mb = statistics.median(xa), statistics.median(xa2), statistics.median(xb)
                    verdict["cases"].append({"N": N, "W": w, "density": dens[w], "M": M, "a_median_ms": ma,
                                             "a2_median_ms": ma2, "b_median_ms": mb, "a_spread_ms": max(xa) - min(xa),
                                             "a2_spread_ms": max(xa2) - min(xa2), "b_spread_ms": max(xb) - min(xb),
                                             "a_over_b": ma / mb, "b_image_GBps": K * N / 4 / (mb * 1e-3) / 1e9,
                                             "b_wins_past_spread": mb < ma - (max(xa) - min(xa))})
        emit(verdict)
    return 0 if verdict.get("untouched_path", {"ok": True})["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
