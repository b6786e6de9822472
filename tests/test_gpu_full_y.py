"""Every element of Y at BASELINE's full sizes, on the GPU.

With integer-valued X (the reference's own inputs: initX, sparseUtils.h:6-23,
U[-512, 512]) and integer b, every partial sum of every chain is an integer
of magnitude < 2^24, so it is exact in fp32 whatever the order: the BaseTCSC
chain (comp.h:37-63) and ANY fp32 summation of X @ W + b give the same bits.
That makes a dense fp32 GEMM on the GPU (torch.matmul of X and the dense
+-1 W) an exact reference for the whole [M, N] result at full size -- the
same argument the reference's own correctness check rests on (main.cpp:206-227
compares BaseTCSC against its dense GEMM).  Order for non-integer X is pinned
on every element too (test_full_y_fractional_x): the oracle's BaseTCSC
restatement, OpenMP over rows, at configs[1], configs[2] and configs[3]
s = 2/8/16.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dense_w(csp, csn, rip, rin, K, N, dev):
    import torch
    W = torch.zeros((K, N), dtype=torch.float32, device=dev)
    cols_p = np.repeat(np.arange(N), np.diff(csp))
    cols_n = np.repeat(np.arange(N), np.diff(csn))
    W[torch.from_numpy(rip.astype(np.int64)).to(dev), torch.from_numpy(cols_p).to(dev)] = 1.0
    W[torch.from_numpy(rin.astype(np.int64)).to(dev), torch.from_numpy(cols_n).to(dev)] = -1.0
    return W


@pytest.mark.parametrize("M,K,N,s", [
    (512, 4096, 4096, 4),        # configs[1]
    (4096, 4096, 16384, 4),      # configs[2] (the bench workload)
    (4096, 4096, 16384, 2),      # configs[3]
    (4096, 4096, 16384, 8),
    (4096, 4096, 16384, 16),
    (1000, 2048, 512, 4),        # reference cases (plots/run_benchmark.py:8-33)
    (16000, 8192, 2048, 8),
    (64000, 16384, 4096, 4),     # the reference's largest case (64-row image; the far-X^T image pinned too)
    (64000, 16384, 4096, 8),     # ... sparse, on the 1 x 32 map
    (37, 16384, 16384, 4),       # small M, K in several chunks
])
def test_full_y_integer_x(tsg, M, K, N, s):
    import torch
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    csp, csn, rip, rin = tsg.gen_tcsc(K, N, s, 42)
    h = tsg.TCSCDevice(csp, csn, rip, rin, K, N, device=0)
    g = torch.Generator(device=dev)
    g.manual_seed(12345)
    X = torch.randint(-512, 513, (M, K), generator=g, device=dev, dtype=torch.int32).to(torch.float32)
    b = torch.full((N,), 2.0, device=dev)  # main.cpp:194
    Y = h.gemm_torch(X, b)
    kernel = h.call_kernel(M) + (" (far-X^T image)" if h.call_far(M) else "")
    # round 5: no automatic call takes the far-X^T image (the 64-row image wins, tsg_plan.cpp
    # pick_rows64); the 128-row image pinned takes it at the largest case (far_xt)
    assert not h.call_far(M)
    W = _dense_w(csp, csn, rip, rin, K, N, dev)
    ref = torch.matmul(X, W) + b
    del W
    torch.cuda.synchronize()
    same = torch.equal(Y.view(torch.int32), ref.view(torch.int32))
    bad = int((Y.view(torch.int32) != ref.view(torch.int32)).sum()) if not same else 0
    assert same, f"{bad} of {M * N} elements differ ({kernel})"
    if (M, K, N, s) == (64000, 16384, 4096, 4):
        h.set_tile_rows(128)
        assert h.call_far(M) and h.call_kernel(M) == "tsg_jit_kernel"
        del Y
        Y = h.gemm_torch(X, b)
        torch.cuda.synchronize()
        assert torch.equal(Y.view(torch.int32), ref.view(torch.int32)), "far-X^T image"
    h.close()


def _oracle_threads() -> int:
    """The GPU box's CPU share (OMP_NUM_THREADS = 16 there), at most 16."""
    import os
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        n = 0
    return max(1, min(16, n or len(os.sched_getaffinity(0))))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("M,K,N,s", [
    (512, 4096, 4096, 4),        # configs[1]
    (4096, 4096, 16384, 4),      # configs[2] (the bench workload)
    (4096, 4096, 16384, 2),      # configs[3]
    (4096, 4096, 16384, 8),
    (4096, 4096, 16384, 16),
    (64, 4096, 16384, 4),        # small M at configs[2]'s K, N
])
def test_full_y_fractional_x(tsg, oracle_mod, M, K, N, s):
    """Order-sensitive X (mantissas of 24 bits over a 2^-23..2^0 exponent
    spread: every partial sum rounds) at full BASELINE sizes, EVERY element
    compared bitwise with the BaseTCSC restatement (oracle/tcsc_oracle.c,
    comp.h:37-63) run over all M rows with OpenMP -- the accumulation order
    pinned on the whole result, not on sampled rows."""
    import torch
    O = oracle_mod
    csp, csn, rip, rin = tsg.gen_tcsc(K, N, s, 42)
    t = O.TCSC(csp, csn, rip, rin, K, N)
    X = O.init_x_frac(M, K, 7 + s)
    b = (np.arange(N, dtype=np.float32) % 13 - 6) * np.float32(0.37)
    h = tsg.TCSCDevice(csp, csn, rip, rin, K, N, device=0)
    kernel = h.call_kernel(M)
    Y = h.gemm_torch(torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
    h.close()
    ref = O.base_tcsc(X, t, b, threads=_oracle_threads())
    diff = Y.view(np.uint32) != ref.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} of {M * N} elements differ ({kernel}); first at {np.argwhere(diff)[0]}"
