"""The rx kernel's block stream (build_rx_image, tsg_host.cpp; the production
path for a W too large for one compiled image), checked on the CPU before any
GPU runs it: tsg_rx_build's image is decoded and the kernel's walk
(tsg_tcsc_rx_kernel, tcsc_kernels.hip) replayed in numpy as the comment above
RxImage in tsg_internal.h describes it -- every (256-column tile, wave) stream
has 2 * nch steps (the +1 pass over the 64-row K chunks, then the -1 pass), a
step's blocks run until the header with bit 31, a block's header holds the
byte offset (k0 - chunk base) * 1024 of its first X row in the chunk's LDS
buffer, entry byte e of a column means row k0 + e / 4 - 1 and byte 0 the X slot
that holds +0.0 -- and Y must equal the BaseTCSC oracle (comp.h:25-69) bit for
bit on order-sensitive X.  Along the way: every nonzero appears exactly once,
a column has at most 8 entries per block in ascending k with the empty bytes
after them, every referenced row lies inside the chunk's LDS window (the chunk
and the 23 rows of over-read behind it) and below K, and one readable header
follows each stream's last block (the walk loads one header ahead)."""
import numpy as np
import pytest

import test_gpu_wstruct as G

CHUNK, BLOCK_ROWS, CAP, NW, WAVES = G.CHUNK_RX, G.RX_BLOCK_ROWS, G.RX_CAP, G.RX_NW, G.RX_WAVES
BLOCK_WORDS = 2 + 2 * NW  # kRxBlockWords: [header][0][column c: 2 dwords of entry bytes]
LAST = 1 << 31


def replay(wstart, ent, nch, X, W):
    """The rx walk over every stream; returns Y without the bias."""
    K, N = W.shape
    M = X.shape[0]
    ntiles = -(-N // (NW * WAVES))
    assert nch == max(1, -(-K // CHUNK)) and len(wstart) == ntiles * WAVES
    XT = np.ascontiguousarray(X.T)
    zero = np.zeros(M, np.float32)  # X slot 0 of a block: +0.0
    y = np.zeros((ntiles * NW * WAVES, M), np.float32)
    seen = np.zeros((K, N), np.int32)
    starts = sorted(int(s) for s in wstart)
    for t in range(ntiles):
        for w in range(WAVES):
            pos = int(wstart[t * WAVES + w])
            assert pos % BLOCK_WORDS == 0
            for q in range(2 * nch):
                neg, j = q >= nch, q % nch
                klo = j * CHUNK
                while True:
                    hdr = int(ent[pos])
                    rel = hdr & (LAST - 1)
                    assert rel % 1024 == 0 and rel // 1024 < CHUNK and int(ent[pos + 1]) == 0
                    k0 = klo + rel // 1024
                    col = ent[pos + 2:pos + BLOCK_WORDS].view(np.uint8).reshape(NW, 8)
                    for c in range(NW):
                        n = (t * WAVES + w) * NW + c
                        prev, acc = 0, y[n]
                        for e in col[c]:
                            e = int(e)
                            if e == 0:  # the kernel adds slot 0 for every empty byte
                                prev = 1 << 30
                                acc = acc - zero if neg else acc + zero
                                continue
                            assert e % 4 == 0 and 1 <= e // 4 <= BLOCK_ROWS and e > prev, "entries ascend, empties last"
                            prev = e
                            k = k0 + e // 4 - 1
                            assert klo <= k < klo + CHUNK + BLOCK_ROWS - 1 and k < K and n < N
                            seen[k, n] += -1 if neg else 1
                            assert abs(seen[k, n]) == 1, "a nonzero appears twice"
                            acc = acc - XT[k] if neg else acc + XT[k]
                        y[n] = acc
                    pos += BLOCK_WORDS
                    if hdr & LAST:
                        break
            # the walk has loaded the next header: inside the array, and the stream ended
            # where the next one (or the closing block) starts
            assert pos + BLOCK_WORDS <= len(ent)
            nxt = [s for s in starts if s > int(wstart[t * WAVES + w])]
            assert pos == (nxt[0] if nxt else len(ent) - BLOCK_WORDS)
    assert np.array_equal(seen, W), "every nonzero exactly once, in its pass"
    return np.ascontiguousarray(y[:N].T)


def check(tsg, O, W, X):
    K, N = W.shape
    t = O.tcsc_encode(W)
    wstart, ent, nch = tsg.rx_build(*t.arrays, K, N)
    b = np.linspace(-1, 2, N).astype(np.float32)
    Y = replay(wstart, ent, nch, X, np.asarray(W)) + b
    assert np.array_equal(Y.view(np.uint32), O.base_tcsc(X, t, b).view(np.uint32))
    return wstart, ent, nch


@pytest.mark.parametrize("M,K,N,s", [(3, 70, 33, 2), (5, 300, 40, 4), (2, 1100, 17, 8), (4, 9, 5, 1), (1, 1, 1, 1),
                                     (2, 64, 257, 4), (3, 65, 300, 1), (2, 700, 40, 4)])
def test_rx_replay_equals_base_tcsc(tsg, oracle_mod, M, K, N, s):
    O = oracle_mod
    W = O.gen_ternary(K, N, s, M + K + N)
    for X in (O.init_x_int(M, K, 3), O.init_x_frac(M, K, 4)):
        check(tsg, O, W, X)


@pytest.mark.parametrize("N", [140, 300])
@pytest.mark.parametrize("K", G.KS)
@pytest.mark.parametrize("w", G.FAMILY_NAMES)
def test_rx_replay_on_structured_w(tsg, oracle_mod, w, K, N):
    W = G.families(K, N)[w]
    wstart, ent, nch = check(tsg, oracle_mod, W, oracle_mod.init_x_frac(3, K, 7))
    blocks = len(ent) // BLOCK_WORDS - 1
    streams = len(wstart)
    if w == "one_dense_column":
        # 12 entries of a pass in every 24 rows against the cap of 8: the dense column's stream
        # needs more blocks than rows / 24; every other stream is one empty block per step
        n = G.dense_column(N)
        assert blocks - (streams - 1) * 2 * nch > 2 * -(-K // BLOCK_ROWS)
        assert n // NW < streams
    if w == "last_row_only":
        assert blocks == streams * 2 * nch  # one block per step, the entries in the last step of each pass


def test_rx_all_zero_w_and_errors(tsg, oracle_mod):
    O = oracle_mod
    W = np.zeros((130, 40), np.int32)
    wstart, ent, nch = check(tsg, O, W, O.init_x_frac(2, 130, 1))
    assert nch == 3 and len(ent) == (len(wstart) * 2 * nch + 1) * BLOCK_WORDS
    with pytest.raises(tsg.TSGError):  # a malformed TCSC is refused
        tsg.rx_build(np.array([0, 1]), np.array([0, 0]), np.array([5]), np.zeros(0), 4, 1)
