"""-m gpu: bounds of ``howl_resample_clips`` on the device (tests/guard_mem.py Banded): samples, bank, records and output of the
ragged batch of tests/test_gpu_resample.py at 44.1 kHz -> 16 kHz, each operand a view into a larger tensor with sentinel bands on
either side, once starting right behind the lower band at its natural size and once grown by a spare tail so that the operand the
kernel addresses ENDS right in front of the upper band's first byte whatever the 256-byte rounding of the view.  After the call
the bands are bit-identical, every promised output is written, nothing else in the output is, and the results are the emulator
tests' (within the derived bound: a read of a band would put a NaN into them)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for _p in (str(HERE.parent), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import resample_util as u  # noqa: E402

pytestmark = pytest.mark.gpu


class _AtTheEnd:
    """Banded, with every buffer padded IN FRONT to a multiple of 256 bytes: the operand handed to the library is the tail of the
    view, so its last byte is the last byte before the upper band (Banded alone puts its first byte behind the lower band)."""

    def __init__(self, inner):
        self.inner, self.views = inner, {}

    def buf(self, name, shape, dtype=np.float32, fill=0.0, placement=None, promised=None):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64))
        lead = (-n * dtype.itemsize) % 256 // dtype.itemsize
        data = np.zeros(lead + n, dtype)
        from guard_mem import fill_sentinel
        fill_sentinel(data[:lead])
        if isinstance(fill, str):
            fill_sentinel(data[lead:])
        else:
            data[lead:] = np.asarray(fill).reshape(-1)
        mask = None
        if promised is not None:
            mask = np.zeros(lead + n, bool)
            mask[lead:] = np.asarray(promised, bool).reshape(-1)
        v = self.inner.buf(name, lead + n, dtype, data, promised=mask)
        self.views[id(v)] = (lead, n, dtype, v)
        return v

    def ptr(self, v):
        lead, n, dtype, _ = self.views[id(v)]
        import ctypes
        return ctypes.c_void_p(v.data_ptr() + lead * dtype.itemsize)

    def get(self, v):
        lead, n, dtype, _ = self.views[id(v)]
        whole = self.inner.get(v)
        from guard_mem import sentinel_mask
        assert sentinel_mask(whole[:lead]).all(), "the spare floats in front of the operand changed"
        return whole[lead:]

    def sync(self):
        self.inner.sync()

    def problems(self):
        return self.inner.problems()

    def describe(self):
        self.inner.describe()


@pytest.mark.parametrize("end", ["head", "tail"])
@pytest.mark.parametrize("fmt", list(u.FORMATS))
def test_resample_operands_between_bands(fmt, end):
    from guard_mem import Banded
    from howl_amd import lib
    al = Banded("cuda") if end == "head" else _AtTheEnd(Banded("cuda"))
    u.check_kernel(al, lib.get(), 44100, fmt)
    torch.cuda.synchronize()
    bad = al.problems()
    if bad:
        al.describe()
    assert not bad, "; ".join(bad)
