#!/usr/bin/env python3
"""A/B of the output row stride (ldY): does the extra kernel argument and the
64-bit row multiply cost the dense path anything?

Needs one MI355X and two built checkouts: this one (the branch) and the commit
before ldY (--parent DIR, built with its own `python __graft_entry__.py`).
Alternating parent / branch on the same card, --rounds times each:
  * plain `python bench.py --gpus 1` (configs[2]) of each checkout: ms_per_step;
  * the kernel time (tcsc_hip_set_timing / tcsc_hip_kernel_time) of dense
    device-pointer calls at K = 4096, N = 16384, s = 4 for M = 1, 8 and 64.
Acceptance (per series): the branch's median is not worse than the parent's by
more than the parent's own max - min spread.  Informational, branch only: the
configs[2] kernel time when writing into a [4096, 131072] buffer (ldY =
131072) against the dense call.

Every measurement is one JSON line of --out (default profiles/ldy_ab.jsonl),
the verdict the last line.  Exit status 1 when a series misses the rule.

    scripts/ldy_ab.py --parent ../parent-checkout [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, S, SEED = 4096, 16384, 4, 42
PROBE_M = (1, 8, 64)


def probe(pkg, strided):
    """Runs inside a child process: kernel time per call (ms) of checkout `pkg`."""
    sys.path.insert(0, pkg)
    import torch
    import tspgemm as T
    h = T.TCSCDevice(*T.gen_tcsc(K, N, S, SEED), K, N)
    b = torch.linspace(-1, 1, N, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)

    def timed(M, call, calls):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        h.set_timing(True)
        h.kernel_time(reset=True)
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        ms, n = h.kernel_time(reset=True)
        h.set_timing(False)
        assert n > 0, (n, calls)
        return ms / n

    out = {}
    if not strided:
        for M in PROBE_M:
            X = torch.rand((M, K), device="cuda", generator=g)
            Y = torch.empty((M, N), device="cuda")
            out[f"kernel_ms_M{M}"] = timed(M, lambda: h.gemm_torch(X, b, Y), 200)
            out[f"kernel_M{M}"] = h.call_kernel(M)
    else:
        M, LD = 4096, 131072
        X = torch.rand((M, K), device="cuda", generator=g)
        Y = torch.empty((M, N), device="cuda")
        wide = torch.empty((M, LD), device="cuda")
        view = wide[:, 3 * N:4 * N]
        dense, ld = [], []
        for _ in range(3):
            dense.append(timed(M, lambda: h.gemm_torch(X, b, Y), 20))
            ld.append(timed(M, lambda: h.gemm_torch_into(X, b, view), 20))
        assert torch.equal(view.view(torch.int32), Y.view(torch.int32))
        out = {"M": M, "ldY": LD, "kernel": h.call_kernel(M), "dense_kernel_ms": dense, "ldy_kernel_ms": ld}
    h.close()
    print("PROBE " + json.dumps(out))


def child(args, cwd):
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    if r.returncode:
        sys.exit(f"{args} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the commit before ldY")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ldy_ab.jsonl"))
    ap.add_argument("--probe", nargs=2, metavar=("PKG", "MODE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.probe:
        return probe(a.probe[0], a.probe[1] == "strided")
    if not a.parent:
        ap.error("--parent is required")
    trees = {"parent": os.path.abspath(a.parent), "branch": REPO}
    me = os.path.abspath(__file__)
    series = {}
    with open(a.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        for rnd in range(a.rounds):
            for name, tree in trees.items():
                line = [ln for ln in child(["bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", "3"],
                                           tree).splitlines() if ln.startswith("{")][-1]
                bench = json.loads(line)
                emit({"what": "bench configs[2]", "commit": name, "round": rnd, "ms_per_step": bench["ms_per_step"],
                      "value": bench["value"], "unit": bench.get("unit")})
                series.setdefault(("bench_ms_per_step", name), []).append(bench["ms_per_step"])
                pr = [ln for ln in child([me, "--probe", os.path.join(tree, "ternary-spgemm_amd"), "dense"],
                                         tree).splitlines() if ln.startswith("PROBE ")][-1]
                pr = json.loads(pr[6:])
                emit({"what": f"dense kernel time K={K} N={N} s={S}", "commit": name, "round": rnd, **pr})
                for M in PROBE_M:
                    series.setdefault((f"kernel_ms_M{M}", name), []).append(pr[f"kernel_ms_M{M}"])
        st = [ln for ln in child([me, "--probe", os.path.join(REPO, "ternary-spgemm_amd"), "strided"],
                                 REPO).splitlines() if ln.startswith("PROBE ")][-1]
        emit({"what": "configs[2] into a [4096, 131072] buffer vs dense (branch, informational)", **json.loads(st[6:])})
        ok = True
        verdict = {"what": "verdict", "rule": "branch median <= parent median + (parent max - parent min)", "series": {}}
        for key in sorted({k for k, _ in series}):
            p, b = series[(key, "parent")], series[(key, "branch")]
            pm, bm, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
            good = bm <= pm + spread
            ok &= good
            verdict["series"][key] = {"parent_median": pm, "branch_median": bm, "parent_spread": spread,
                                      "branch_spread": max(b) - min(b), "ok": good}
        verdict["ok"] = ok
        emit(verdict)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
