"""-m gpu: the dense kernels of howl_amd/csrc/howl_gemm.hip.h through include/howl_hip_dense.h on the device: the case table of
tests/dense_util.py (integers bit-equal to the float64 reference, gaussians under the a-priori bound, sentinels, bit-equal repeats,
the reported kernel instance) on guard_mem.Banded, the written-out list of instances, and the weights-stationary kernel at the row
count where the dispatcher stops admitting it.

HOWL_DENSE_REPORT=<file> appends the worst error / bound per instance to that file (profiles/dense_bounds.txt is made this way)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dense_util as u
from gpu_util import DEV
from howl_amd import lib as L

pytestmark = pytest.mark.gpu
ENV = ("HOWL_ROWGEMM_MIN_ROWS", "HOWL_WGRAD_BIG_MIN_ROWS", "HOWL_GEMM_NO_ROWGEMM", "HOWL_WGRAD_NO_DUAL")


@pytest.fixture(scope="module")
def ctx():
    from guard_mem import Banded
    log = open(os.devnull, "w")
    c = u.Ctx(L.get(), lambda: Banded(str(DEV), log=log), "gpu")
    c.ran = set()
    return c


def run(ctx, name, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    u.run_case(ctx, name, monkeypatch.setenv)
    ctx.ran.add(name)


@pytest.mark.parametrize("name", u.names("gpu"))
def test_dense(ctx, name, monkeypatch):
    run(ctx, name, monkeypatch)


def test_every_instance_is_reached(ctx, monkeypatch):
    for name in u.names("gpu"):          # (whatever a -k selection left out)
        if name not in ctx.ran:
            run(ctx, name, monkeypatch)
    assert sorted(ctx.seen) == u.REACHABLE, (sorted(set(u.REACHABLE) - ctx.seen), sorted(ctx.seen - set(u.REACHABLE)))
    assert not ctx.seen & set(u.UNREACHABLE)
    path = os.environ.get("HOWL_DENSE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(u.report_lines("gpu", ctx.ratios)) + "\n")


@pytest.mark.parametrize("inner", [3, 7])
def test_rowgemm_at_the_row_gate(inner, monkeypatch):
    """rowgemm_kernel<3, 4> takes floor(r / inner) through a float reciprocal whose margin is argued for r < 2^20; the dispatcher
    admits M < 2^20.  M = 2^20 - 1 rows of integers (K = 4, N = 512) with a gap after every `inner` rows and NaNs in the gaps: every
    output row must be bit-equal to the float64 product, taken on the device in row chunks; M = 2^20 must go to another kernel."""
    monkeypatch.setenv("HOWL_ROWGEMM_MIN_ROWS", "1")
    lib = L.get()
    M1, N, K, gap = 1 << 20, 512, 4, 4
    gen = torch.Generator().manual_seed(inner)
    m = u.rmap(inner, K, gap)
    rows = torch.arange(M1, dtype=torch.int64)
    offs = ((rows // inner) * m.s_outer + (rows % inner) * m.s_inner).to(DEV)
    xv = torch.randint(-4, 5, (M1, K), generator=gen).float().to(DEV)
    x = torch.full((int(offs[-1]) + K,), float("nan"), device=DEV)
    x[(offs[:, None] + torch.arange(K, device=DEV)[None, :]).reshape(-1)] = xv.reshape(-1)
    w = torch.randint(-4, 5, (N, K), generator=gen).float().to(DEV)
    bias = torch.randint(-4, 5, (N,), generator=gen).float().to(DEV)
    out = torch.empty(M1 * N, device=DEV)

    def call(M):
        out.fill_(float("nan"))
        g = L.HowlDenseGemm(a_major_k=1, a=x.data_ptr(), am=m, a_ks=1, ak=u.lin(0), b=w.data_ptr(), bk=u.lin(1), b_ns=K, M=M, N=N, K=K, splits=1,
                            bias=bias.data_ptr(), relu=0, c=out.data_ptr(), c_ms=N, c_split_stride=M * N, c_floats=M1 * N)
        lib.call("howl_dense_gemm", ctypes.byref(g), None, None, None)
        arr = (L.HowlDenseChoice * 16)()
        assert lib.cdll.howl_dense_choices(arr, 16) == 1
        torch.cuda.synchronize()
        o = out.view(M1, N)
        step = 1 << 16
        for r0 in range(0, M, step):
            r1 = min(M, r0 + step)
            ref = xv[r0:r1].double() @ w.double().T + bias.double()
            bad = (o[r0:r1].double() != ref).any(dim=1)
            assert not bool(bad.any()), f"M={M}: row {r0 + int(bad.nonzero()[0])} differs from the float64 product"
        assert bool(torch.isnan(o[M:]).all()), "rows past M were written"
        return L.DENSE_FAMILIES[arr[0].family], (arr[0].t0, arr[0].t1, arr[0].t2, arr[0].t3), arr[0].gx

    assert call(M1 - 1) == ("rowgemm_kernel", (3, 4, 1, 0), int(lib.cdll.howl_dense_num_cus()))
    assert call(M1)[0] == "gemm_vec_kernel"
