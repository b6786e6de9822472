"""The looping launch of the 64-row image's 8-wave dispatcher (DESIGN.md 4.2;
tsg_jit_kernel.hip, tsg_plan.cpp loop_wgs): a call with more logical workgroup
ids than the grid launches `grid` workgroups, and workgroup b runs ids b, b +
grid, ... through the unchanged tile map.  TSG_JIT_LOOP caps the grid, so tiny
shapes loop: with caps of 1, 2, 3 and 8 one workgroup runs up to 16 tiles and
the tile count is mostly no multiple of the grid.  Every element of Y, bit for
bit against the BaseTCSC oracle, on fractional (order-sensitive) X:

* K = 188, 376, 564, 752: 1 .. 4 chunks of the row layout, so 2 nch = 2, 4, 6,
  8 steps -- every phase of the 3-buffer ring at the boundary between two
  tiles of one workgroup;
* M = 65, 200, 256: a ragged last M tile, and tiles enough to loop;
* width-16 streams at N = 128, 300 and width-128 streams at N = 1024, 1100;
  at N = 1100 the upper waves of the last column tile have no column below N:
  they skip their epilogue and must still reach every barrier of the loop (run
  by hand, that case gets its own time limit);
* Y in a wider, poisoned buffer: nothing outside the view is written;
* one looped case each through the bf16-Y path, the scaled path and the fused
  epilogue;
* TSG_JIT_LOOP=0 and the default (no loop either) give the same bits;
  tsg_call_grid returns the cap, and tcsc_hip_last_launch reports the same
  grid as what the call handed to the runtime.
"""
import numpy as np
import pytest

from test_gpu_ldy import _assert_only_view_written, _bits, _case, _dev, _fill, _jit_handle

pytestmark = pytest.mark.gpu

CAPS = (1, 2, 3, 8)
KS = (188, 376, 564, 752)
MS = (65, 200, 256)
STREAMS = ((16, 128), (16, 300), (128, 1024), (128, 1100))  # (width, N)


def _tiles(M, N, width):
    return ((M + 63) // 64) * ((N + 8 * width - 1) // (8 * width))


def _nnz(arrays):
    return len(arrays[2]) + len(arrays[3])


@pytest.fixture(autouse=True)
def _no_loop_knob(monkeypatch):
    monkeypatch.delenv("TSG_JIT_LOOP", raising=False)


@pytest.mark.parametrize("width,N", STREAMS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_loop_caps_bit_exact(tsg, oracle_mod, monkeypatch, K, M, width, N):
    import torch
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = _jit_handle(tsg, arrays, K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == width and h.jit_waves(M) == 8
    tiles = _tiles(M, N, width)
    Xd, bd, ad = _dev(X), _dev(b), _dev(alpha)
    buf = torch.empty((M + 2, N + 5), device="cuda")
    view = buf[1:M + 1, 2:N + 2]  # ldY = N + 5 > N
    want, want_p = ref.view(np.uint32), ref_p.view(np.uint32)
    got = {}
    for cap in (None, 0) + CAPS:
        if cap is None:
            monkeypatch.delenv("TSG_JIT_LOOP", raising=False)
        else:
            monkeypatch.setenv("TSG_JIT_LOOP", str(cap))
        tag = (K, M, width, N, "cap", cap, "tiles", tiles)
        # the grid query returns the cap (or every id, when the cap holds them all, or nothing loops)
        grid = (min(cap, tiles) if cap else tiles, tiles)
        assert tsg.call_grid(K, N, _nnz(arrays), M, 64, width) == grid, tag
        for al, w in ((None, want), (ad, want_p)):
            _fill(buf)
            h.gemm_torch_into(Xd, bd, view, alpha=al)
            torch.cuda.synchronize()
            assert h.last_launch() == grid, tag  # ... and it is what the call launched
            y = _bits(view.contiguous())
            bad = y != w
            assert not bad.any(), (tag, int(bad.sum()), "of", w.size, "elements differ, first at",
                                   np.argwhere(bad)[:4].tolist())
            _assert_only_view_written(buf, 1, M + 1, 2, N + 2, tag)
            got[(cap, al is None)] = y
    assert np.array_equal(got[(None, True)], got[(0, True)]) and np.array_equal(got[(None, False)], got[(0, False)])
    h.close()


def test_loop_bf16_and_scaled_paths(tsg, oracle_mod, monkeypatch):
    """The 16-bit store branch and the scaled branch of a looping workgroup
    (test_gpu_scaled's scheme: both scales, one, PReLU, dense and odd views)."""
    from test_gpu_scaled import _scase, check_scaled
    M, K, N, width = 200, 376, 300, 16  # 4 x 3 tiles on 3 and on 8 workgroups
    for ydtype in ("bfloat16", "float32"):
        case = _scase(M, K, N, "float32", ydtype)
        h = _jit_handle(tsg, case[0], K, N, 64, width)
        assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_waves(M) == 8
        for cap in (3, 8):
            monkeypatch.setenv("TSG_JIT_LOOP", str(cap))
            check_scaled(h, case, ydtype, ("loop", cap, ydtype), modes=("both",))
            assert h.last_launch() == (cap, 12)
        h.close()
    # the unscaled 16-bit branch
    import torch
    from test_gpu_ytype import _cast_bits, _ybits
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = _jit_handle(tsg, arrays, K, N, 64, width)
    monkeypatch.setenv("TSG_JIT_LOOP", "3")
    Y = h.gemm_torch_xy(_dev(X), _dev(b), out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert np.array_equal(_ybits(Y), _cast_bits(ref, "bfloat16"))
    h.close()


def test_loop_fused_epilogue_path(tsg, oracle_mod, monkeypatch):
    """The fused-epilogue branch of a looping workgroup (test_gpu_epilogue's scheme)."""
    from test_gpu_epilogue import check_ex, ecase
    M, K, N, width = 200, 376, 300, 16
    key = (M, K, N, "float32", 0, True)
    h = _jit_handle(tsg, ecase(*key).arrays, K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_waves(M) == 8
    monkeypatch.setenv("TSG_JIT_LOOP", "3")
    check_ex(h, key, "bfloat16", [("relu2", "bfloat16", "bfloat16")], "loop-epi")
    check_ex(h, key, "float32", [("relu", "float32", "float32")], "loop-epi")
    assert h.last_launch() == (3, 12)
    h.close()
