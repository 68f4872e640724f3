"""Bounds tests on the device: the cases of tests/bounds_cases.py at full size, each operand a view into a larger tensor with
sentinel bands on either side (tests/guard_mem.py Banded).  After the call the bands are bit-identical, no promised output still
holds the sentinel, and the results match the oracle.  Inputs stay inside every entry point's contract (the out-of-contract
cases run on the emulator only: tests/test_emu_bounds.py)."""
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
for _p in (str(HERE.parent), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bounds_cases import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case_id", [k for k, c in CASES.items() if c.gpu])
def test_bounds_on_device(case_id, monkeypatch):
    import torch
    from guard_mem import Banded
    from howl_amd import lib as hlib
    c = CASES[case_id]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    al = Banded("cuda")
    c.fn(al, hlib.get(), True, **c.params)
    torch.cuda.synchronize()
    bad = al.problems()
    if bad:
        al.describe()
    assert not bad, "; ".join(bad)
