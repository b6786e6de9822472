"""The integer matrix-core kernel's packed W image (tsg_i8_build) on the CPU:
unpacked in numpy with the index formula of include/ternary_spgemm_test.h it is
the dense W, zero-padded to the kernel's tile; and the eligibility arithmetic."""
import numpy as np
import pytest


def _unpack(img, Kp, Np):
    k, n = np.meshgrid(np.arange(Kp), np.arange(Np), indexing="ij")
    word = (((n // 64) * (Kp // 64) + k // 64) * 64 + 32 * (k % 32 // 16) + n % 32) * 4 + 2 * (n % 64 // 32) + k % 64 // 32
    code = (img[word] >> (8 * (k % 4) + 2 * (k % 16 // 4)).astype(np.uint32)) & 3
    return np.array([1, 7, -1, 0])[code]  # +1 = 0, -1 = 2, zero = 3; code 1 is never written


@pytest.mark.parametrize("special", [False, True], ids=["random", "full-columns"])
@pytest.mark.parametrize("K,N", [(1, 1), (63, 31), (65, 257), (200, 128)])
def test_image_unpacks_to_dense_w(tsg, oracle_mod, K, N, special):
    W = oracle_mod.gen_ternary(K, N, 2, 100 * K + N)
    if special:  # an all-+1, an all--1 and an empty column (as many as N holds), from the last one down
        for j, v in enumerate((1, -1, 0)[:N]):
            W[:, N - 1 - j] = v
    img, geom = tsg.i8_build(*oracle_mod.tcsc_encode(W).arrays, K, N)
    Kp, Np = -(-K // 64) * 64, -(-N // 128) * 128
    assert geom == (Kp, Np, 128, 128, 64, 64) and img.size == Kp * Np // 16
    want = np.zeros((Kp, Np), np.int64)
    want[:K, :N] = W
    assert np.array_equal(_unpack(img, Kp, Np), want)


def test_eligibility(tsg):
    z, e = np.zeros(2, np.int32), np.zeros(0, np.int32)  # one empty column
    img, geom = tsg.i8_build(z, z, e, e, 131072, 1)
    assert geom[:2] == (131072, 128) and not (img != 0xFFFFFFFF).any()
    for K, B in ((131073, 0), (64, 4)):  # past the exactness bound; a BlockedTCSC
        with pytest.raises(tsg.TSGError) as err:
            tsg.i8_build(z, z, e, e, K, 1, B)
        assert err.value.code == 5, (K, B)
