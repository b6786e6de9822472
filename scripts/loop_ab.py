#!/usr/bin/env python3
"""Measurements behind the looping launch of the 64-row dispatcher (DESIGN.md
4.2, 4.6), each part one JSON-lines file under profiles/.  Needs one MI355X.

diag  (profiles/loop_transition_diag.jsonl): what a round of workgroups costs
      outside its K sweep.  The diagnostic library (`make diag`, results
      WRONG) runs BASELINE configs[2] (4096, 4096, 16384, s = 4) and the same
      at s = 16 with TSG_JIT_DIAG unset, nostore (no epilogue), onetile (the
      first round alone) and onetile,nostore; each in a fresh child process:
      warm-up, then --windows windows of --steps calls between two events.
ab    (profiles/loop_ab.jsonl): plain `python bench.py [shape]` of a built
      checkout of the parent commit (--parent DIR), of this checkout as it
      launches by default, and of this checkout with TSG_JIT_LOOP=--grid,
      alternating, --rounds runs each, every run a fresh process (the method of
      scripts/epilogue_ab.py).  Medians, each side's max - min, and the rule:
      the loop passes when parent median - loop median > parent max - min.

    scripts/loop_ab.py diag [--out FILE]
    scripts/loop_ab.py ab --parent DIR [--shape M K N s]... [--rounds 5] [--grid 256] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ternary-spgemm_amd")


def leg(M, K, N, s, steps, windows):
    sys.path.insert(0, PKG)
    import torch
    import tspgemm as T
    h = T.TCSCDevice(*T.gen_tcsc(K, N, s, 42), K, N)
    h.reserve(M)
    g = torch.Generator(device="cuda").manual_seed(12345)
    X = torch.randn((M, K), generator=g, device="cuda")
    b = torch.linspace(-1, 1, N, device="cuda")
    Y = torch.empty((M, N), device="cuda")
    for _ in range(10):
        h.gemm_torch_into(X, b, Y)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            h.gemm_torch_into(X, b, Y)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    print("LEG " + json.dumps({"kernel": h.call_kernel(M), "launch": h.last_launch(), "steps": steps,
                               "ms_per_step": ms}), flush=True)
    h.close()


def child(args, cwd, limit, env_set=None, env_del=()):
    env = dict(os.environ)
    for k in ("TSG_LIB", "TSG_JIT_DIAG", "TSG_JIT_LOOP") + tuple(env_del):
        env.pop(k, None)
    env.update(env_set or {})
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode:
        sys.exit(f"{args} in {cwd} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("diag", "ab", "leg"))
    ap.add_argument("--parent")
    ap.add_argument("--shape", nargs=4, type=int, action="append", metavar=("M", "K", "N", "s"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.what == "leg":
        return leg(*a.shape[0], a.steps, a.windows)
    me = os.path.abspath(__file__)
    out = a.out or os.path.join(REPO, "profiles", "loop_transition_diag.jsonl" if a.what == "diag" else "loop_ab.jsonl")
    with open(out, "a" if a.what == "ab" and a.shape else "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        if a.what == "diag":
            lib = os.path.join(PKG, "lib", "libternary_spgemm_diag.so")
            for s in (4, 16):
                med = {}
                for diag in ("", "nostore", "onetile", "onetile,nostore"):
                    o = child([me, "leg", "--shape", "4096", "4096", "16384", str(s), "--steps", str(a.steps),
                               "--windows", str(a.windows)], REPO, 400,
                              dict({"TSG_LIB": lib}, **({"TSG_JIT_DIAG": diag} if diag else {})))
                    rec = json.loads([ln for ln in o.splitlines() if ln.startswith("LEG ")][-1][4:])
                    med[diag] = statistics.median(rec["ms_per_step"])
                    emit({"what": "diag", "M": 4096, "K": 4096, "N": 16384, "s": s, "TSG_JIT_DIAG": diag or None,
                          "library": "diagnostic (results WRONG with a diag value)", "median_ms": med[diag], **rec})
                full, one = med[""], med["onetile"]
                emit({"what": "split", "s": s, "rounds": 4, "unit": "us",
                      "four_rounds": 1e3 * full, "one_round": 1e3 * one,
                      "per_round_outside_one_round": 1e3 * (full - 4 * one) / 3,
                      "store_and_drain_per_round": 1e3 * (full - med["nostore"]) / 4,
                      "store_and_drain_of_one_round": 1e3 * (one - med["onetile,nostore"]),
                      "note": "per_round_outside_one_round = (four rounds - 4 x one round) / 3 transitions; "
                              "negative: four rounds in one launch cost less than four launches of one"})
            return 0
        shape = a.shape[-1] if a.shape else None
        extra = [] if not shape else ["--M", str(shape[0]), "--K", str(shape[1]), "--N", str(shape[2]), "--s", str(shape[3])]
        sides = (("parent", os.path.abspath(a.parent), {}), ("branch, default launch", REPO, {}),
                 ("branch, TSG_JIT_LOOP=%d" % a.grid, REPO, {"TSG_JIT_LOOP": str(a.grid)}))
        ms = {}
        for rnd in range(a.rounds):
            for name, tree, env in sides:
                o = child(["bench.py"] + extra, tree, 480, env)
                r = json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1])
                emit({"what": "bench", "method": "python bench.py " + " ".join(extra), "side": name, "round": rnd,
                      "ms_per_step": r["ms_per_step"], "value": r.get("value"), "unit": r.get("unit")})
                ms.setdefault(name, []).append(r["ms_per_step"])
        p = ms["parent"]
        pm, spread = statistics.median(p), max(p) - min(p)
        v = {"what": "verdict", "shape": shape or [4096, 4096, 16384, 4], "parent_median_ms": pm,
             "parent_spread_ms": spread}
        for name, x in ms.items():
            if name != "parent":
                m = statistics.median(x)
                v[name] = {"median_ms": m, "spread_ms": max(x) - min(x), "parent_minus_this_ms": pm - m,
                           "faster_by_more_than_parent_spread": pm - m > spread,
                           "no_slower_than_parent_plus_spread": m <= pm + spread}
        emit(v)
    return 0


if __name__ == "__main__":
    sys.exit(main())
