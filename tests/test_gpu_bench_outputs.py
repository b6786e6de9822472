"""A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run on a
small shape: K sets the timed steps, the line carries `ms_per_step` and none
of the --full legs, and DIR/Y.npy is the timed path's Y -- bit for bit the
BaseTCSC oracle (comp.h:25-69) on the inputs the arguments determine."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_step(tsg, oracle_mod, tmp_path):
    import torch
    import tsg_dist as D
    O = oracle_mod
    M, K, N, s, steps = 96, 512, 640, 4, 2
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--clock-warmup", "0", "--M", str(M), "--K", str(K), "--N", str(N),
                        "--s", str(s), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ln = json.loads(r.stdout.strip().splitlines()[-1])
    assert ln["steps"] == steps and ln["n_gpus"] == 1 and ln["dtype"] == "f32" and ln["unit"] == "GFLOP/s"
    assert ln["full"] is False and ln["cpu_baseline"] is None and ln["e2e_host_pointers"] is None
    assert ln["roofline"]["kernel_timing"]["event_pair_kernel_ms"] is None
    arrs = D.ShardedTCSC.draw(K, N, s, 42, 0, 1, "weak")
    nnz = len(arrs[2]) + len(arrs[3])
    assert ln["ms_per_step"] > 0
    # value = adds per step / step time; the line rounds ms_per_step to 1e-4 ms
    rel = 5e-5 / ln["ms_per_step"] + 1e-4
    assert abs(ln["value"] - tsg.flops(M, N, nnz) / (ln["ms_per_step"] * 1e-3) / 1e9) <= rel * ln["value"]
    assert sorted(os.listdir(out)) == ["Y.npy"]
    Y = np.load(out / "Y.npy")
    assert Y.dtype == np.float32 and Y.shape == (M, N)
    g = torch.Generator(device="cuda")
    g.manual_seed(12345)
    X = torch.randint(-512, 513, (M, K), generator=g, device="cuda", dtype=torch.int32).to(torch.float32).cpu().numpy()
    ref = O.base_tcsc(X, O.TCSC(*arrs, K, N), np.full(N, 2.0, np.float32))
    assert np.array_equal(Y.view(np.uint32), ref.view(np.uint32))
