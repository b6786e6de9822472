import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "oracle"), os.path.join(REPO, "ternary-spgemm_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(REPO, "tests", "golden")


class _GoldenSmall:
    """tests/golden/ref_small*.npz (make_golden.py writes the vectors in parts,
    each under 1 MiB) read as one archive: `.files` and `[key]` as np.load gives."""

    def __init__(self):
        import glob
        import numpy as np
        self._parts = [np.load(p) for p in sorted(glob.glob(os.path.join(GOLDEN, "ref_small*.npz")))]
        self.files = [k for z in self._parts for k in z.files]
        assert len(set(self.files)) == len(self.files)

    def __getitem__(self, key):
        for z in self._parts:
            if key in z.files:
                return z[key]
        raise KeyError(key)


def load_golden_small():
    return _GoldenSmall()


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) GPU; runs through the C-ABI")
    config.addinivalue_line("markers", "slow: long-running CPU case")


def gpu_available() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="session")
def oracle_mod():
    import oracle
    oracle.build(ref=False) if not os.path.exists(os.path.join(REPO, "oracle", "liboracle.so")) else None
    return oracle


@pytest.fixture(scope="session")
def tsg():
    import tspgemm
    if not os.path.exists(tspgemm.LIB_PATH):
        tspgemm.build()
    return tspgemm
