"""The dense kernels of howl_amd/csrc/howl_gemm.hip.h through their door (include/howl_hip_dense.h): the case table, the float64
references and the bounds shared by tests/test_emu_dense.py (hipemu, guard_mem.Arena) and tests/test_gpu_dense.py (guard_mem.Banded).

Every case runs twice over, with two input families:

  integers   operands, bias and upstream gradients are uniform integers in [-4, 4].  Every product and every partial sum is an
             exact float32 (|sum| <= 16 K < 2^24), so the result must be BIT-EQUAL to the float64 reference whatever the order of
             summation: a dropped, doubled or misplaced term of any size shows.
  gaussians  standard normals, each row scaled by a power of two from 2^-6 .. 2^6, against the float64 product under the a-priori
             bound of tests/mb_layerwise.py: with u = 2^-24, K terms and S split slabs folded (1 without a split),
                 |got - ref| <= 2 (K + S + 2) u sum_i |a_i| |b_i|
             per element; a bias adds one term to the count and |bias| to the magnitude; ReLU is 1-Lipschitz and keeps the bound;
             column sums keep a float64 running sum per chunk: 2 (chunks + 2) u sum |x|; the thin second layer is checked
             teacher-forced from the kernel's own y1 (K = 256, one bias term).  None of these figures comes from what the kernels
             give.  The worst error / bound per kernel instance goes to Ctx.ratios (profiles/dense_bounds.txt).

In every case the outputs start as NaN sentinels and every promised element must be written; gap columns of strided outputs and
whatever lies beyond the reported split count keep their sentinels; operand gaps hold NaNs, so a read that is not discarded
poisons the result; a second run is bit-equal.  Each case asserts the kernel instance the dispatcher reports; REACHABLE below is
the written-out list that test_every_instance_is_reached compares the union of all reports with."""
import ctypes
import itertools
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for _p in (str(ROOT), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from guard_mem import fill_sentinel, sentinel_mask  # noqa: E402
from howl_amd import lib as L  # noqa: E402

U = 2.0 ** -24
LIN = L.DENSE_LIN
NARGS = {1: 1, 2: 3, 3: 4, 4: 1, 5: 2, 6: 2, 7: 0, 8: 0, 9: 0, 10: 0, 11: 0, 12: 0}     # template arguments per family


def inst(family, *t):
    return f"{family}<{','.join(str(int(x)) for x in t)}>" if t else family


# ---- the instances the dispatcher can pick, written out -----------------------------------------------------------------------------
REACHABLE = sorted(
    [inst("gemm_kernel", a) for a in (0, 1)] +
    # gemm_vec_kernel<A_UNIT_K, B_UNIT_K, KMAP_LIN>: seven of eight
    [inst("gemm_vec_kernel", *t) for t in ((1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0))] +
    # rowgemm_kernel<KG, NT, W_UNIT_K, NO2>: three shapes x two W layouts, and the head shape with a second layer of 1..8 outputs
    [inst("rowgemm_kernel", kg, nt, w, 0) for kg, nt in ((3, 4), (8, 2), (16, 1)) for w in (0, 1)] +
    [inst("rowgemm_kernel", 8, 2, 1, no2) for no2 in range(1, 9)] +
    [inst("thin_wgrad_kernel", no) for no in range(1, 9)] +
    [inst("wgrad_big_kernel", tn, kl) for tn in (64, 128) for kl in (0, 1)] +
    # the five job kinds of wgrad_big_multi_kernel (192 = the dual job), and its launch
    [inst("wgrad_big_multi_kernel.job", tn, kl) for tn, kl in ((64, 0), (64, 1), (128, 0), (128, 1), (192, 0))] +
    ["wgrad_big_multi_kernel", "wgrad_w8_body", "sum_slabs_kernel", "sum_slabs_multi_kernel", "colsum_kernel", "relu_bwd_kernel"])
# instances that exist in the source and that no argument list can reach, with the reason; the tests assert they are never reported
UNREACHABLE = {
    inst("gemm_vec_kernel", 1, 1, 0): "KMAP_LIN = (a_major_k || is_lin(amap)) && (b_unit_k || is_lin(bmap)) is true whenever both operands are "
                                      "unit-stride along k: no row map is indexed by k inside the kernel",
    inst("wgrad_big_multi_kernel.job", 192, 1): "wgrad_dual_gemm always collects the dual job with klin = 0 (the body is compiled for general maps)",
}


# ---- context ------------------------------------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, lib, make_alloc, backend):
        self.lib, self.make_alloc, self.backend = lib, make_alloc, backend
        self.G = int(lib.cdll.howl_dense_num_cus())
        self.seen = set()
        self.ratios = {}
        self.al = None

    def fresh(self):
        self.al = self.make_alloc()
        return self.al

    def choices(self):
        arr = (L.HowlDenseChoice * 16)()
        n = int(self.lib.cdll.howl_dense_choices(arr, 16))
        assert n <= 16
        out = []
        for e in arr[:n]:
            t = (e.t0, e.t1, e.t2, e.t3)[:NARGS[e.family]]
            rec = dict(inst=inst(L.DENSE_FAMILIES[e.family], *t), grid=(e.gx, e.gy, e.gz), kps=e.kps, t=(e.t0, e.t1, e.t2, e.t3))
            out.append(rec)
            self.seen.add(rec["inst"])
        return out

    def ratio(self, instance, err, bound):
        r = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
        self.ratios[instance] = max(self.ratios.get(instance, 0.0), r)
        return r


def rmap(inner, pitch, gap=0):
    """rows of `pitch` floats, `gap` more floats after every `inner` rows"""
    return L.HowlDenseRowMap(inner, inner * pitch + gap, pitch)


def lin(stride):
    return L.HowlDenseRowMap(LIN, 0, stride)


def off(m, x):
    x = np.asarray(x, np.int64)
    if m.inner >= LIN:
        return x * m.s_inner
    return (x // m.inner) * m.s_outer + (x % m.inner) * m.s_inner


def gen(rng, fam, shape, scaled_axis=0):
    if fam == "int":
        return rng.integers(-4, 5, size=shape).astype(np.float32)
    x = rng.standard_normal(shape).astype(np.float32)
    if len(shape) == 2:
        e = rng.integers(-6, 7, size=shape[scaled_axis])
        s = np.ldexp(np.float32(1.0), e).astype(np.float32)
        x = x * (s[:, None] if scaled_axis == 0 else s[None, :])
    return x.astype(np.float32)


def scatter(al, name, idx, values, extra_front=0):
    """A buffer of exactly max(idx) + 1 floats (+ extra_front in front), NaN sentinels in the gaps, values at idx."""
    n = int(idx.max()) + 1 + extra_front
    host = np.empty(n, np.float32)
    fill_sentinel(host)
    host[idx.reshape(-1) + extra_front] = values.reshape(-1)
    return al.buf(name, n, np.float32, fill=host)


def ptr(al, v, floats=0):
    p = al.ptr(v)
    return p if floats == 0 or p is None else ctypes.c_void_p(p.value + 4 * floats)


def out_buf(al, name, n, mask=None):
    return al.buf(name, n, np.float32, fill="sentinel", promised="all" if mask is None else mask)


def check_close(ctx, instance, fam, got, ref, mag, terms, what):
    """int: bit-equal; gauss: |got - ref| <= 2 terms u mag"""
    got64 = got.astype(np.float64)
    if fam == "int":
        assert np.array_equal(got64, ref), f"{what} [{instance}]: {int((got64 != ref).sum())} of {ref.size} integer results differ " \
                                           f"(first at {np.argwhere(got64 != ref)[0].tolist()})"
        return
    bound = 2.0 * terms * U * mag
    err = np.abs(got64 - ref)
    r = ctx.ratio(instance, err, bound)
    print(f"dense: {what} [{instance}] worst error/bound = {r:.3g}")
    assert not np.isnan(got64).any() and (err <= bound).all(), f"{what} [{instance}]: error/bound = {r:.3g} (terms {terms})"


def twice(ctx, run, outs):
    """runs the call twice; the second run's bits must equal the first's"""
    run()
    ctx.al.sync()
    first = [ctx.al.get(o).copy() for o in outs]
    rec = ctx.choices()
    run()
    ctx.al.sync()
    for o, f in zip(outs, first):
        assert np.array_equal(ctx.al.get(o).view(np.uint32), f.view(np.uint32)), "a second run gave other bits"
    assert [r["inst"] for r in ctx.choices()] == [r["inst"] for r in rec]
    ctx.al.check()
    return first, rec


# ---- gemm ---------------------------------------------------------------------------------------------------------------------------
def gemm_case(ctx, fam, seed, M, N, K, a_major_k=1, am=None, a_ks=1, a_pad=0, ak=None, b="k", bk=None, b_pad=0, splits=1, bias=False,
              relu=False, c_pad=0, cs_pad=0, offset=0, thin_out=0, expect=None, unit_w_stride=None):
    """am / ak / bk: (inner, gap) of a two-level map, None = a plain stride.  b = "k": B(k,n) = b[n * b_ns + k] (a torch Linear
    weight), "n": B(k,n) = b[bk(k) + n].  a_pad / b_pad widen the operand rows; offset moves a's base pointer by that many floats."""
    rng = np.random.default_rng(seed)
    al = ctx.fresh()
    A = gen(rng, fam, (M, K))
    B = gen(rng, fam, (K, N), scaled_axis=1)
    bias_v = gen(rng, fam, (1, N)).reshape(N) if bias else None
    m_i, k_i, n_i = np.arange(M), np.arange(K), np.arange(N)
    if a_major_k:
        pitch = K * a_ks + a_pad
        amap = lin(pitch) if am is None else rmap(am[0], pitch, am[1])
        akmap = lin(0)
        ia = off(amap, m_i)[:, None] + k_i[None, :] * a_ks
    else:
        pitch = M + a_pad
        amap = lin(1)
        akmap = lin(pitch) if ak is None else rmap(ak[0], pitch, ak[1])
        ia = off(amap, m_i)[:, None] + off(akmap, k_i)[None, :]
    if b == "k":
        b_ns = K + b_pad
        bkmap = lin(1)
    else:
        b_ns = 1
        bkmap = lin(N + b_pad) if bk is None else rmap(bk[0], N + b_pad, bk[1])
    ib = off(bkmap, k_i)[:, None] + n_i[None, :] * b_ns
    a_buf = scatter(al, "a", ia, A, extra_front=offset)
    b_buf = scatter(al, "b", ib, B)
    bias_buf = al.buf("bias", N, fill=bias_v) if bias else None
    c_ms = N + c_pad
    z = int(ctx.lib.cdll.howl_dense_gemm_splits(K, splits))
    kps = ((K + splits - 1) // splits + 15) // 16 * 16
    assert z == (K + kps - 1) // kps
    cs = (M - 1) * c_ms + N + cs_pad
    g = L.HowlDenseGemm(a_major_k=a_major_k, a=ptr(al, a_buf, offset), am=amap, a_ks=a_ks, ak=akmap, b=ptr(al, b_buf), bk=bkmap, b_ns=b_ns, M=M,
                        N=N, K=K, splits=splits, bias=ptr(al, bias_buf), relu=int(relu), c_ms=c_ms, c_split_stride=cs, thin_out=thin_out)
    need = int(ctx.lib.cdll.howl_dense_gemm_c_floats(ctypes.byref(g)))
    assert need == (z - 1) * cs + (M - 1) * c_ms + N
    idx_c = (np.arange(z)[:, None, None] * cs + m_i[None, :, None] * c_ms + n_i[None, None, :])
    mask = np.zeros(need, bool)
    mask[idx_c.reshape(-1)] = True
    c_buf = out_buf(al, "c", need, mask)
    g.c, g.c_floats = ptr(al, c_buf), need
    outs = [c_buf]
    if thin_out:
        w2 = gen(rng, fam, (thin_out, N))
        b2 = gen(rng, fam, (1, thin_out)).reshape(thin_out)
        w2_buf, b2_buf = al.buf("w2", (thin_out, N), fill=w2), al.buf("b2", thin_out, fill=b2)
        y2_buf = al.buf("y2", M * thin_out, fill="sentinel")          # promised only when the second layer rides along
        g.w2, g.b2, g.y2 = ptr(al, w2_buf), ptr(al, b2_buf), ptr(al, y2_buf)
        outs.append(y2_buf)
    so, td = ctypes.c_int(-1), ctypes.c_int(-1)
    (first, rec) = twice(ctx, lambda: ctx.lib.call("howl_dense_gemm", ctypes.byref(g), ctypes.byref(so), ctypes.byref(td), None), outs)
    assert len(rec) == 1, rec
    name = rec[0]["inst"]
    if expect is not None:
        assert name == expect, f"dispatcher chose {name}, the case is meant for {expect}"
    rowg = name.startswith("rowgemm")
    assert so.value == (1 if rowg else z) and td.value == (1 if rowg and thin_out else 0), (so.value, td.value, name)
    if not rowg:
        assert rec[0]["grid"] == ((N + 63) // 64, (M + 63) // 64, z) and rec[0]["kps"] == kps, rec
    got = first[0]
    assert sentinel_mask(got)[~mask].all(), "a gap column of c (or a slab beyond the split count) was written"
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    for s in range(z):
        k0, k1 = s * kps, min(K, (s + 1) * kps)
        ref = A64[:, k0:k1] @ B64[k0:k1]
        mag = np.abs(A64[:, k0:k1]) @ np.abs(B64[k0:k1])
        terms = (k1 - k0) + 1 + 2
        if bias:
            ref, mag, terms = ref + bias_v.astype(np.float64), mag + np.abs(bias_v.astype(np.float64)), terms + 1
        if relu:
            ref = np.maximum(ref, 0.0)
        check_close(ctx, name, fam, got[idx_c[s]], ref, mag, terms, f"gemm M{M} N{N} K{K} slab {s}")
    if thin_out:
        assert sentinel_mask(first[1]).all() if not td.value else not sentinel_mask(first[1]).any(), "y2: written although declined, or left unwritten"
    if thin_out and td.value:
        y1 = got[idx_c[0]].astype(np.float64)
        ref2 = y1 @ w2.astype(np.float64).T + b2.astype(np.float64)
        mag2 = np.abs(y1) @ np.abs(w2.astype(np.float64)).T + np.abs(b2.astype(np.float64))
        check_close(ctx, name, fam, first[1].reshape(M, thin_out), ref2, mag2, N + 1 + 2 + 1, f"thin second layer M{M} NO2={thin_out}")
    return rec[0]


# ---- weight gradients ------------------------------------------------------------------------------------------------------------------
def _wjob(ctx, al, rng, fam, tag, n_out, k_in, rows, dm=None, im=None, d_pad=0, i_pad=0, max_splits=64, rows_per_split=512, k2=0, im2=None,
          misalign=0, promise=True):
    D = gen(rng, fam, (rows, n_out))
    X = gen(rng, fam, (rows, k_in))
    r_i = np.arange(rows)
    dmap = lin(n_out + d_pad) if dm is None else rmap(dm[0], n_out + d_pad, dm[1])
    imap = lin(k_in + i_pad) if im is None else rmap(im[0], k_in + i_pad, im[1])
    d_buf = scatter(al, tag + "dout", off(dmap, r_i)[:, None] + np.arange(n_out)[None, :], D, extra_front=misalign)
    x_buf = scatter(al, tag + "in", off(imap, r_i)[:, None] + np.arange(k_in)[None, :], X)
    j = L.HowlDenseWgrad(dout=ptr(al, d_buf, misalign), dm=dmap, n_out=n_out, in_=ptr(al, x_buf), im=imap, k_in=k_in, rows=rows,
                         max_splits=max_splits, rows_per_split=rows_per_split)
    X2 = None
    if k2:
        X2 = gen(rng, fam, (rows, k2))
        i2map = lin(k2) if im2 is None else rmap(im2[0], k2, im2[1])
        x2_buf = scatter(al, tag + "in2", off(i2map, r_i)[:, None] + np.arange(k2)[None, :], X2)
        j.in2, j.im2, j.k2 = ptr(al, x2_buf), i2map, k2
    # scratch and outputs need pointers for the size query's alignment tests only for dout / in: ask first, then allocate exactly
    j.scratch = j.dw = ctypes.c_void_p(16)
    j.scratch2 = j.dw2 = ctypes.c_void_p(16)
    z = int(ctx.lib.cdll.howl_dense_wgrad_splits(ctypes.byref(j)))
    assert z >= 1, "the job does not fit"
    need = int(ctx.lib.cdll.howl_dense_wgrad_scratch_floats(ctypes.byref(j)))
    assert need == z * n_out * k_in
    s_buf = al.buf(tag + "scratch", need, fill="sentinel")
    dw_buf = out_buf(al, tag + "dw", n_out * k_in, None if promise else np.zeros(n_out * k_in, bool))
    j.scratch, j.scratch_floats, j.dw = ptr(al, s_buf), need, ptr(al, dw_buf)
    bufs = dict(scratch=s_buf, dw=dw_buf, D=D, X=X, X2=X2, z=z, rows=rows)
    if k2:
        need2 = int(ctx.lib.cdll.howl_dense_wgrad_scratch2_floats(ctypes.byref(j)))
        assert need2 == z * n_out * k2
        s2_buf = al.buf(tag + "scratch2", need2, fill="sentinel")
        dw2_buf = out_buf(al, tag + "dw2", n_out * k2)
        j.scratch2, j.scratch2_floats, j.dw2 = ptr(al, s2_buf), need2, ptr(al, dw2_buf)
        bufs.update(scratch2=s2_buf, dw2=dw2_buf)
    return j, bufs


def _wcheck(ctx, fam, name, got, D, X, rows, z, what):
    D64, X64 = D.astype(np.float64), X.astype(np.float64)
    check_close(ctx, name, fam, got.reshape(D.shape[1], X.shape[1]), D64.T @ X64, np.abs(D64).T @ np.abs(X64), rows + z + 2, what)


def wgrad_case(ctx, fam, seed, form, jobs, expect, last_split=None):
    """jobs: list of _wjob keyword dicts; expect: the instances of the products, in the order of the jobs"""
    rng = np.random.default_rng(seed)
    al = ctx.fresh()
    built = [_wjob(ctx, al, rng, fam, f"j{q}.", **kw) for q, kw in enumerate(jobs)]
    arr = (L.HowlDenseWgrad * len(built))(*[j for j, _ in built])
    outs = [b["dw"] for _, b in built] + [b["dw2"] for _, b in built if "dw2" in b]
    first, rec = twice(ctx, lambda: ctx.lib.call("howl_dense_wgrad", form, len(built), arr, None), outs)
    products = [r for r in rec if not r["inst"].startswith(("sum_slabs", "wgrad_big_multi_kernel<"))
                and r["inst"] != "wgrad_big_multi_kernel"]
    assert [r["inst"] for r in products] == list(expect), ([r["inst"] for r in rec], expect)
    folds = [r["inst"] for r in rec if r["inst"].startswith("sum_slabs")]
    assert folds == (["sum_slabs_kernel"] * len(built) if form == 0 else ["sum_slabs_multi_kernel"]), rec
    if form == 2:
        collected = [r for r in products if ".job" in r["inst"]]
        assert len(collected) <= 4
        launches = [r for r in rec if r["inst"] == "wgrad_big_multi_kernel"]
        assert len(launches) == (1 if collected else 0)
        if collected:
            assert launches[0]["t"][0] == len(collected) and launches[0]["grid"][0] == sum(int(np.prod(r["grid"])) for r in collected)
    for q, ((j, b), r) in enumerate(zip(built, products)):
        z = b["z"]
        if r["inst"].startswith(("wgrad_big", "gemm")):
            assert r["grid"][2] == z, (r, z)
        if r["inst"].startswith("thin"):
            assert r["grid"][1] == z, (r, z)
        if last_split is not None and q == 0:
            assert z >= 3 and b["rows"] - (z - 1) * r["kps"] == last_split, (r, z)
        _wcheck(ctx, fam, r["inst"], ctx.al.get(b["dw"]), b["D"], b["X"], b["rows"], z, f"wgrad job {q} form {form}")
        if b["X2"] is not None:
            _wcheck(ctx, fam, r["inst"], ctx.al.get(b["dw2"]), b["D"], b["X2"], b["rows"], z, f"wgrad job {q} second product")
        assert not sentinel_mask(ctx.al.get(b["scratch"])).any(), "a slab inside the reported split count was not written"
    return rec


def w8_case(ctx, fam, seed, **kw):
    """One collected 128-column job: slabs from wgrad_w8_body (512 threads) and from wgrad_big_kernel<128, false> must be the same bits."""
    slabs = []
    for eight in (1, 0):
        rng = np.random.default_rng(seed)
        al = ctx.fresh()
        j, b = _wjob(ctx, al, rng, fam, "w8.", promise=False, **kw)
        so = ctypes.c_int(-1)
        first, rec = twice(ctx, lambda: ctx.lib.call("howl_dense_wgrad_slabs", ctypes.byref(j), eight, ctypes.byref(so), None), [b["scratch"]])
        want = "wgrad_w8_body" if eight else inst("wgrad_big_kernel", 128, 0)
        assert [r["inst"] for r in rec] == [inst("wgrad_big_multi_kernel.job", 128, rec[0]["t"][1]), want], rec
        assert so.value == b["z"] and sentinel_mask(ctx.al.get(b["dw"])).all()          # slabs only: no fold ran
        got = first[0].reshape(b["z"], kw["n_out"], kw["k_in"])
        kps = rec[0]["kps"]
        D64, X64 = b["D"].astype(np.float64), b["X"].astype(np.float64)
        for s in range(b["z"]):
            r0, r1 = s * kps, min(b["rows"], (s + 1) * kps)
            check_close(ctx, want, fam, got[s], D64[r0:r1].T @ X64[r0:r1], np.abs(D64[r0:r1]).T @ np.abs(X64[r0:r1]), (r1 - r0) + 1 + 2,
                        f"wgrad slabs eight={eight} slab {s}")
        slabs.append(first[0])
    assert np.array_equal(slabs[0].view(np.uint32), slabs[1].view(np.uint32)), "the eight-wave body's slabs differ from the sixteen-wave body's"


# ---- slab sums --------------------------------------------------------------------------------------------------------------------------
def sum_slabs_case(ctx, fam, seed, nparts, n):
    rng = np.random.default_rng(seed)
    al = ctx.fresh()
    P = gen(rng, fam, (nparts, n))
    p_buf = al.buf("part", (nparts, n), fill=P)
    o_buf = out_buf(al, "out", n)
    first, rec = twice(ctx, lambda: ctx.lib.call("howl_dense_sum_slabs", ptr(al, p_buf), nparts, n, ptr(al, o_buf), None), [o_buf])
    assert [r["inst"] for r in rec] == ["sum_slabs_kernel"] and rec[0]["kps"] == nparts
    P64 = P.astype(np.float64)
    check_close(ctx, "sum_slabs_kernel", fam, first[0], P64.sum(0), np.abs(P64).sum(0), nparts + 2, f"sum_slabs nparts {nparts} n {n}")


ADAMW = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, step=3, grad_scale=0.5)


def slab_multi_case(ctx, fam, seed, jobs, adamw=False, mean=None):
    """jobs: (nparts, n, stride_pad, out2) each.  adamw: every out / out2 lies in one flat gradient buffer; p, m, v must be bit-equal to
    howl_adamw_step applied to the gradient the fold wrote.  mean: target lengths of the rider (zero-length targets count as 1)."""
    rng = np.random.default_rng(seed)
    al = ctx.fresh()
    sizes = [n for _, n, _, o2 in jobs for _ in range(2 if o2 else 1)]
    total = sum(sizes) + 5                                  # five floats of the gradient buffer belong to no job
    g_buf = out_buf(al, "grad", total, np.arange(total) < total - 5)
    arr = (L.HowlDenseSlabJob * len(jobs))()
    parts, places = [], []
    cur = 0
    for q, (nparts, n, pad, o2) in enumerate(jobs):
        P = gen(rng, fam, (nparts, n))
        stride = n + pad
        parts.append(P)
        p_buf = scatter(al, f"part{q}", np.arange(nparts)[:, None] * stride + np.arange(n)[None, :], P)
        arr[q] = L.HowlDenseSlabJob(part=ptr(al, p_buf), nparts=nparts, stride=stride, n=n, out=ptr(al, g_buf, cur),
                                    out2=ptr(al, g_buf, cur + n) if o2 else None)
        places.append((cur, cur + n if o2 else None))
        cur += 2 * n if o2 else n
    outs = [g_buf]
    opt = None
    if adamw:
        state0 = [gen(rng, "gauss", (1, total)).reshape(total) for _ in range(3)]
        state0[2] = np.abs(state0[2])
        p_b, m_b, v_b = (al.buf(nm, total, fill=s) for nm, s in zip("pmv", state0))
        opt = L.HowlAdamW(p=ptr(al, p_b), g=ptr(al, g_buf), m=ptr(al, m_b), v=ptr(al, v_b), n=total, **ADAMW)
    mean_arg = None
    if mean is not None:
        Bm = len(mean)
        nll = np.abs(gen(rng, "gauss", (1, Bm)).reshape(Bm)) * 8
        tl = np.asarray(mean, np.int64)
        nll_b, tl_b = al.buf("nll", Bm, fill=nll), al.buf("tl", Bm, np.int64, fill=tl)
        loss_b = out_buf(al, "loss", 1)
        mean_arg = L.HowlCtcMean(nll=ptr(al, nll_b), target_lengths=ptr(al, tl_b), B=Bm, loss=ptr(al, loss_b))
        outs.append(loss_b)
    call = lambda: ctx.lib.call("howl_dense_slab_sums", len(jobs), arr, ctypes.byref(opt) if opt else None,
                                ctypes.byref(mean_arg) if mean_arg else None, None)
    if adamw:       # the step changes p, m, v: one run only, then the separate launch on copies of the state
        call()
        al.sync()
        rec = ctx.choices()
        first = [al.get(o).copy() for o in outs]
        al.check()
    else:
        first, rec = twice(ctx, call, outs)
    assert [r["inst"] for r in rec] == ["sum_slabs_multi_kernel"] and rec[0]["t"][:3] == (len(jobs), int(adamw), int(mean is not None)), rec
    assert rec[0]["grid"][0] == max((max(n for _, n, _, _ in jobs) + 63) // 64, 1) if jobs else True
    g = first[0]
    assert sentinel_mask(g[total - 5:]).all()
    for P, (o1, o2), (nparts, n, _, _) in zip(parts, places, jobs):
        P64 = P.astype(np.float64)
        check_close(ctx, "sum_slabs_multi_kernel", fam, g[o1:o1 + n], P64.sum(0), np.abs(P64).sum(0), nparts + 2, f"fold nparts {nparts} n {n}")
        if o2 is not None:
            assert np.array_equal(g[o2:o2 + n].view(np.uint32), g[o1:o1 + n].view(np.uint32)), "out2 differs from out"
    if adamw:
        n_used = total - 5
        g2 = al.buf("g.ref", n_used, fill=g[:n_used])
        p2, m2, v2 = (al.buf(nm + ".ref", n_used, fill=s[:n_used]) for nm, s in zip("pmv", state0))
        ctx.lib.call("howl_adamw_step", ptr(al, p2), ptr(al, g2), ptr(al, m2), ptr(al, v2), n_used, ADAMW["lr"], ADAMW["beta1"], ADAMW["beta2"],
                     ADAMW["eps"], ADAMW["weight_decay"], ADAMW["step"], ADAMW["grad_scale"], None)
        al.sync()
        for nm, rode, alone, s0 in zip("pmv", (p_b, m_b, v_b), (p2, m2, v2), state0):
            r = al.get(rode)
            assert np.array_equal(r[:n_used].view(np.uint32), al.get(alone).view(np.uint32)), f"AdamW rider: {nm} differs from howl_adamw_step"
            assert np.array_equal(r[n_used:].view(np.uint32), s0[n_used:].view(np.uint32)), f"AdamW rider: {nm} changed outside the jobs"
            assert not np.array_equal(r[:n_used], s0[:n_used])
    if mean is not None:
        terms = nll.astype(np.float64) / np.maximum(tl, 1)
        ref = terms.mean()
        got = float(first[-1][0])
        # each quotient and the final rounding are float32 (relative u each), the running sum is float64: 4 u mean|nll_b / L_b| leaves
        # a factor of two
        assert abs(got - ref) <= 4.0 * U * np.abs(terms).mean(), (got, ref)
    return rec


def slab_overflow_case(ctx):
    al = ctx.fresh()
    part = al.buf("part", 9 * 4, fill=1.0)
    out = out_buf(al, "out", 9 * 4, np.zeros(36, bool))
    arr = (L.HowlDenseSlabJob * 9)(*[L.HowlDenseSlabJob(part=ptr(al, part, 4 * q), nparts=1, stride=4, n=4, out=ptr(al, out, 4 * q)) for q in range(9)])
    rc = ctx.lib.cdll.howl_dense_slab_sums(9, arr, None, None, None)
    al.sync()
    assert rc != 0 and b"more than 8 folds queued" in ctx.lib.cdll.howl_last_error()
    assert sentinel_mask(al.get(out)).all(), "an overflowing collector launched something"
    ctx.lib.call("howl_dense_slab_sums", 8, arr, None, None, None)          # eight fit, and the collector is clean again
    al.sync()
    assert np.array_equal(al.get(out)[:32], np.ones(32, np.float32)) and sentinel_mask(al.get(out)[32:]).all()
    ctx.choices()
    al.check()


# ---- column sums, ReLU backward ------------------------------------------------------------------------------------------------------------
def colsum_case(ctx, fam, seed, rows, n, rm=None, pad=0, max_chunks=64, rows_per_chunk=256, deferred=0, out1=False):
    rng = np.random.default_rng(seed)
    al = ctx.fresh()
    X = gen(rng, fam, (rows, n))
    m = lin(n + pad) if rm is None else rmap(rm[0], n + pad, rm[1])
    x_buf = scatter(al, "x", off(m, np.arange(rows))[:, None] + np.arange(n)[None, :], X)
    chunks = int(ctx.lib.cdll.howl_dense_colsum_chunks(rows, max_chunks, rows_per_chunk))
    assert chunks == min(max(rows // rows_per_chunk, 1), max_chunks)
    s_buf = out_buf(al, "scratch", chunks * n)
    o0 = out_buf(al, "out0", n)
    o1 = out_buf(al, "out1", n) if out1 else None
    outs = [o0, s_buf] + ([o1] if out1 else [])
    first, rec = twice(ctx, lambda: ctx.lib.call("howl_dense_colsum", ptr(al, x_buf), ctypes.byref(m), rows, n, ptr(al, s_buf), chunks * n,
                                                 ptr(al, o0), ptr(al, o1), max_chunks, rows_per_chunk, deferred, None), outs)
    folds = ["sum_slabs_multi_kernel"] if deferred else ["sum_slabs_kernel"] * (2 if out1 else 1)
    assert [r["inst"] for r in rec] == ["colsum_kernel"] + folds, rec
    rpc = (rows + chunks - 1) // chunks
    assert rec[0]["grid"] == ((n + 63) // 64, chunks, 1) and rec[0]["kps"] == rpc
    X64 = X.astype(np.float64)
    check_close(ctx, "colsum_kernel", fam, first[0], X64.sum(0), np.abs(X64).sum(0), chunks + 2, f"colsum rows {rows} n {n}")
    if out1:
        assert np.array_equal(first[2].view(np.uint32), first[0].view(np.uint32))


def relu_bwd_case(ctx, fam, seed, n, in_place):
    rng = np.random.default_rng(seed)
    al = ctx.fresh()
    dy, y = gen(rng, fam, (1, n)).reshape(n), gen(rng, fam, (1, n)).reshape(n)
    y[::7] = 0.0
    y[3::11] = -0.0
    y_buf = al.buf("y", n, fill=y)
    if in_place:
        dz_buf = al.buf("dy", n, fill=dy, promised=None)
        ctx.lib.call("howl_dense_relu_bwd", ptr(al, dz_buf), ptr(al, y_buf), n, ptr(al, dz_buf), None)
    else:
        dy_buf = al.buf("dy", n, fill=dy)
        dz_buf = out_buf(al, "dz", n)
        ctx.lib.call("howl_dense_relu_bwd", ptr(al, dy_buf), ptr(al, y_buf), n, ptr(al, dz_buf), None)
    al.sync()
    assert [r["inst"] for r in ctx.choices()] == ["relu_bwd_kernel"]
    got = al.get(dz_buf)
    assert np.array_equal(got.view(np.uint32), np.where(y > 0, dy, np.float32(0.0)).astype(np.float32).view(np.uint32))   # exact, both families
    al.check()


# ---- refusals (valid memory only; nothing may launch) -----------------------------------------------------------------------------------------
def refusals_case(ctx, setenv):
    lib, al = ctx.lib, ctx.fresh()
    rng = np.random.default_rng(5)

    def refused(name, match, *args):
        rc = getattr(lib.cdll, name)(*args)
        msg = lib.cdll.howl_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and match in msg, (name, rc, msg)

    a, b = al.buf("a", (8, 16), fill=1.0), al.buf("b", (4, 16), fill=1.0)
    c = out_buf(al, "c", 8 * 4, np.zeros(32, bool))
    g = L.HowlDenseGemm(a_major_k=1, a=ptr(al, a), am=lin(16), a_ks=1, ak=lin(0), b=ptr(al, b), bk=lin(1), b_ns=16, M=8, N=4, K=16, splits=1,
                        c=ptr(al, c), c_ms=4, c_split_stride=32, c_floats=31)
    refused("howl_dense_gemm", "32 floats (got 31)", ctypes.byref(g), None, None, None)
    g.c_floats, g.a = 32, None
    refused("howl_dense_gemm", "null pointer", ctypes.byref(g), None, None, None)
    g.a, g.thin_out = ptr(al, a), 3
    refused("howl_dense_gemm", "null pointer (second layer)", ctypes.byref(g), None, None, None)
    g.thin_out, g.c_ms = 0, 3
    refused("howl_dense_gemm", "rows of c overlap", ctypes.byref(g), None, None, None)
    j, bufs = _wjob(ctx, al, rng, "int", "r.", n_out=5, k_in=6, rows=9, rows_per_split=4, promise=False)
    assert bufs["z"] == 2
    j.scratch_floats -= 1
    refused("howl_dense_wgrad", "60 floats (got 59)", 0, 1, ctypes.byref(j), None)
    j.scratch_floats += 1
    j.dw = None
    refused("howl_dense_wgrad", "null pointer", 0, 1, ctypes.byref(j), None)
    refused("howl_dense_wgrad", "form=3", 3, 1, ctypes.byref(j), None)
    # the dual job and the slabs-only job need max_splits >= 16 (the 128-row kernel's condition); 15 is refused before any launch
    setenv("HOWL_WGRAD_BIG_MIN_ROWS", "1")
    d, dbufs = _wjob(ctx, al, rng, "int", "d.", n_out=128, k_in=128, rows=5, max_splits=15, promise=False)
    dual = L.HowlDenseWgrad.from_buffer_copy(d)
    x2 = al.buf("d.in2", (5, 4), fill=1.0)
    dual.in2, dual.im2, dual.k2 = ptr(al, x2), lin(4), 4
    dual.scratch2 = dual.dw2 = d.scratch
    dual.scratch2_floats = d.scratch_floats
    assert lib.cdll.howl_dense_wgrad_splits(ctypes.byref(dual)) == 0
    refused("howl_dense_wgrad", "the dual job does not fit", 2, 1, ctypes.byref(dual), None)
    refused("howl_dense_wgrad", "needs form 2", 1, 1, ctypes.byref(dual), None)
    refused("howl_dense_wgrad_slabs", "max_splits >= 16", ctypes.byref(d), 1, None, None)
    assert sentinel_mask(al.get(dbufs["scratch"])).all() and sentinel_mask(al.get(dbufs["dw"])).all()
    x = al.buf("x", (300, 3), fill=1.0)
    s = out_buf(al, "s", 3, np.zeros(3, bool))
    o = out_buf(al, "o", 3, np.zeros(3, bool))
    m = lin(3)
    refused("howl_dense_colsum", "3 floats (got 2)", ptr(al, x), ctypes.byref(m), 300, 3, ptr(al, s), 2, ptr(al, o), None, 64, 256, 0, None)
    refused("howl_dense_colsum", "null pointer", ptr(al, x), ctypes.byref(m), 300, 3, ptr(al, s), 3, None, None, 64, 256, 0, None)
    refused("howl_dense_sum_slabs", "null pointer", None, 1, 3, ptr(al, o), None)
    refused("howl_dense_relu_bwd", "null pointer", ptr(al, x), None, 3, ptr(al, o), None)
    refused("howl_dense_slab_sums", "nothing to do", 0, None, None, None, None)
    al.sync()
    for v in (c, s, o, bufs["scratch"], bufs["dw"]):
        assert sentinel_mask(al.get(v)).all(), "a refused call wrote"
    al.check()


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, group, fn, kw, emu, gpu, env, families):
        self.name, self.group, self.fn, self.kw, self.emu, self.gpu, self.env, self.families = name, group, fn, kw, emu, gpu, env, families


CASES = {}
ROWG = {"HOWL_ROWGEMM_MIN_ROWS": "1"}
WBIG = {"HOWL_WGRAD_BIG_MIN_ROWS": "1"}
FAMS = ("int", "gauss")


def register(name, group, fn, emu=True, gpu=True, env=None, families=FAMS, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, group, fn, kw, emu, gpu, env or {}, families)


def G_rows(k):
    """a row count that depends on the launcher's workgroup count G: resolved when the case runs"""
    return lambda ctx: k[0] * ctx.G + k[1]


def _resolve(ctx, kw):
    def r(v):
        if callable(v):
            return v(ctx)
        if isinstance(v, dict):
            return {a: r(b) for a, b in v.items()}
        if isinstance(v, list):
            return [r(b) for b in v]
        return v
    return {a: r(b) for a, b in kw.items()}


def run_case(ctx, name, setenv):
    """setenv(name, value): monkeypatch.setenv in the tests"""
    c = CASES[name]
    for k, v in c.env.items():
        setenv(k, v)
    kw = _resolve(ctx, c.kw)
    for i, fam in enumerate(c.families):
        seed = (abs(hash_name(name)) + i) % (1 << 31)
        if c.fn is refusals_case:
            c.fn(ctx, setenv)
            break
        if c.fn is slab_overflow_case:
            c.fn(ctx)
            break
        c.fn(ctx, fam, seed, **kw)


def hash_name(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


_cyc = lambda xs: itertools.cycle(xs)

# 64 x 64 tiles, scalar loads (gemm_kernel): forced by an odd K, a pitch that is no multiple of 4, or a base pointer moved by one float
_Ms, _Ns = _cyc([1, 4, 63, 64, 65, 68]), _cyc([65, 68, 1, 4, 63, 64])
_inn = _cyc([1, 3, 7, 16, 17])
for _i, _K in enumerate([4, 16, 17, 20, 32, 36, 48, 100, 100, 17, 36, 48]):
    _M, _N, _sp = next(_Ms), next(_Ns), 1 + _i % 3
    _force = dict(offset=1) if _K % 4 == 0 and _i % 2 == 0 else dict(a_pad=1, b_pad=1) if _K % 4 == 0 else {}
    register(f"gemm_scalar_ak_M{_M}_N{_N}_K{_K}_s{_sp}", "gemm", gemm_case, M=_M, N=_N, K=_K, splits=_sp, am=(next(_inn), 5), b="k" if _i % 2 else "n",
             bk=(next(_inn), 3), bias=_i % 2 == 0, relu=_i % 3 == 0, c_pad=(0, 3)[_i % 2], cs_pad=(0, 7)[_i // 2 % 2], a_ks=1 + (_i == 5),
             expect=inst("gemm_kernel", 1), **_force)
for _i, _K in enumerate([4, 17, 32, 48, 100, 20]):
    _M, _N, _sp = next(_Ms), next(_Ns), 1 + _i % 3
    register(f"gemm_scalar_am_M{_M}_N{_N}_K{_K}_s{_sp}", "gemm", gemm_case, a_major_k=0, M=_M, N=_N, K=_K, splits=_sp, ak=(next(_inn), 2), a_pad=1,
             b="n", bk=(next(_inn), 1), b_pad=_i % 2, bias=_i % 2 == 1, relu=_i % 2 == 0, c_pad=_i % 3, cs_pad=_i % 2 * 5,
             expect=inst("gemm_kernel", 0))
# 64 x 64 tiles, 16-byte loads (gemm_vec_kernel): every reachable instance at one, two and three K tiles, both loop exits, with splits
_V4 = [4, 64, 68]
for _t, (_ak, _bk, _kl) in enumerate([(1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0)]):
    for _i, (_K, _sp) in enumerate([(4, 1), (16, 1), (20, 2), (32, 1), (36, 1), (48, 2), (100, 3), (100, 1)]):
        _M = _V4[(_i + _t) % 3] if not _ak else [1, 63, 65, 4, 64, 68][(_i + _t) % 6]
        _N = _V4[(_i + 2 * _t + 1) % 3] if not _bk else [65, 1, 63, 68, 4, 64][(_i + _t) % 6]
        _kw = dict(a_major_k=_ak, M=_M, N=_N, K=_K, splits=_sp, b="k" if _bk else "n", bias=_i % 2 == 0, relu=_i % 3 == 1, c_pad=(0, 4, 1)[_i % 3],
                   cs_pad=(0, 9)[_i % 2], a_pad=4 * (_i % 2), b_pad=4 * ((_i + 1) % 2))
        if _ak:
            _kw["am"] = (next(_inn), 8)
            if not _bk and not _kl:
                _kw["bk"] = (next(_inn), 4)
        else:
            if _bk:
                _kw["ak"] = None if _kl else (next(_inn), 8)
            elif _kl:
                pass
            else:                       # one of the two k-indexed maps two-level is enough; alternate
                _kw["ak"] = (next(_inn), 4) if _i % 2 else None
                _kw["bk"] = (next(_inn), 8) if not _i % 2 else None
        register(f"gemm_vec{_ak}{_bk}{_kl}_M{_M}_N{_N}_K{_K}_s{_sp}", "gemm", gemm_case, expect=inst("gemm_vec_kernel", _ak, _bk, _kl),
                 **_kw)

# the weights-stationary kernel (HOWL_ROWGEMM_MIN_ROWS = 1)
_ROWS = [1, 15, 16, 17, G_rows((16, 1)), G_rows((32, 5)), G_rows((48, 16))]
_rinn = _cyc([1, 3, 7, 82])
for (_kg, _nt, _N, _Ks) in ((3, 4, 512, [4, 40, 48]), (8, 2, 256, [68, 100, 128]), (16, 1, 128, [132, 200, 256])):
    for _w in (1, 0):
        for _ri, _rows in enumerate(_ROWS):
            _K = _Ks[_ri % 3]
            _tag = _rows if isinstance(_rows, int) else ("16G+1", "32G+5", "48G+16")[_ri - 4]
            _in = next(_rinn)
            register(f"rowgemm{_kg}_{_nt}_w{_w}_rows{_tag}_K{_K}", "rowgemm", gemm_case, env=ROWG, M=_rows, N=_N, K=_K, am=(_in, 4) if _in > 1 or _ri % 2 else None,
                     b="k" if _w else "n", b_pad=4 * (_ri % 2), bias=_ri % 2 == 0, relu=_ri % 3 == 0, c_pad=_N * (_ri % 2),
                     expect=inst("rowgemm_kernel", _kg, _nt, _w, 0))
for _no in range(1, 9):
    for _ri, _rows in enumerate([1, 17, G_rows((32, 5))]):
        _tag = _rows if isinstance(_rows, int) else "32G+5"
        register(f"rowgemm_thin{_no}_rows{_tag}", "rowgemm", gemm_case, env=ROWG, M=_rows, N=256, K=[128, 68, 100][(_no + _ri) % 3], am=(7, 4) if _ri else None,
                 b="k", bias=True, relu=_ri != 1, thin_out=_no,
                 expect=inst("rowgemm_kernel", 8, 2, 1, _no))
# the same arguments one row map stride off the kernel's alignment rule: the tiles take over, the second layer is left to the caller
register("rowgemm_thin_declined", "rowgemm", gemm_case, env=ROWG, M=17, N=256, K=128, a_pad=1, b="k", bias=True, relu=True, thin_out=5,
         expect=inst("gemm_kernel", 1))

# the 128-row weight-gradient kernel (HOWL_WGRAD_BIG_MIN_ROWS = 1)
_winn = _cyc([1, 3, 7, 16, 17, 40])
_wrows = _cyc([1, 15, 16, 17, 63, 64, 65])
for _i, (_no, _ki) in enumerate([(128, 16), (132, 20), (260, 64), (128, 68), (132, 128), (260, 132), (128, 132)]):
    for _lin in (0, 1):
        _rows = next(_wrows)
        _maps = {} if _lin else dict(dm=(next(_winn), 4), im=(next(_winn), 8))
        _tn = 128 if _ki > 64 else 64
        register(f"wgrad_big_n{_no}_k{_ki}_rows{_rows}_lin{_lin}", "wgrad_big", wgrad_case, env=WBIG, form=0, jobs=[dict(n_out=_no, k_in=_ki, rows=_rows, d_pad=4 * _lin, i_pad=4 * (1 - _lin), **_maps)],
                 expect=[inst("wgrad_big_kernel", _tn, _lin)])
for _lin, _ki in ((0, 128), (1, 64), (0, 20)):
    register(f"wgrad_big_three_splits_k{_ki}_lin{_lin}", "wgrad_big", wgrad_case, env=WBIG, form=1, last_split=5,
             jobs=[dict(n_out=128, k_in=_ki, rows=133, **({} if _lin else dict(dm=(7, 4), im=(3, 12))))],
             expect=[inst("wgrad_big_kernel", 128 if _ki > 64 else 64, _lin)])
_J = lambda no, ki, rows, lin_, **kw: dict(n_out=no, k_in=ki, rows=rows, **({} if lin_ else dict(dm=(next(_winn), 4), im=(next(_winn), 4))), **kw)
register("wgrad_jobs_one", "wgrad_big", wgrad_case, env=WBIG, form=2, jobs=[_J(132, 68, 65, 0)], expect=[inst("wgrad_big_multi_kernel.job", 128, 0)])
register("wgrad_jobs_two_mixed", "wgrad_big", wgrad_case, env=WBIG, form=2, jobs=[_J(128, 20, 17, 1), _J(132, 132, 63, 0)],
         expect=[inst("wgrad_big_multi_kernel.job", 64, 1), inst("wgrad_big_multi_kernel.job", 128, 0)])
register("wgrad_jobs_three_mixed", "wgrad_big", wgrad_case, env=WBIG, form=2, jobs=[_J(260, 132, 16, 0), _J(128, 64, 64, 1), _J(132, 20, 65, 0)],
         expect=[inst("wgrad_big_multi_kernel.job", 128, 0), inst("wgrad_big_multi_kernel.job", 64, 1), inst("wgrad_big_multi_kernel.job", 64, 0)])
# an operand one float off the 16-byte line: the scalar tiles take the job although the threshold admits the 128-row kernel
register("wgrad_misaligned_goes_to_scalar_tiles", "wgrad_big", wgrad_case, env=WBIG, form=1, jobs=[dict(n_out=132, k_in=20, rows=65, misalign=1, dm=(3, 4))],
         expect=[inst("gemm_kernel", 0)])
register("wgrad_jobs_four_mixed", "wgrad_big", wgrad_case, env=WBIG, form=2,
         jobs=[_J(128, 16, 15, 0), _J(128, 128, 133, 1), _J(260, 64, 1, 1), _J(128, 68, 16, 0)],
         expect=[inst("wgrad_big_multi_kernel.job", 64, 0), inst("wgrad_big_multi_kernel.job", 128, 1), inst("wgrad_big_multi_kernel.job", 64, 1),
                 inst("wgrad_big_multi_kernel.job", 128, 0)])
# a fifth job launches on its own (its fold still rides in the one flush); a thin job and a tile job pass through the same call
register("wgrad_jobs_fifth_falls_back", "wgrad_big", wgrad_case, env=WBIG, form=2,
         jobs=[_J(128, 16, 17, 1), _J(128, 20, 64, 0), _J(128, 16, 5, 1), _J(128, 20, 33, 0), _J(132, 68, 65, 0), dict(n_out=5, k_in=33, rows=40),
               dict(n_out=12, k_in=16, rows=40)],
         expect=[inst("wgrad_big_multi_kernel.job", 64, 1), inst("wgrad_big_multi_kernel.job", 64, 0), inst("wgrad_big_multi_kernel.job", 64, 1),
                 inst("wgrad_big_multi_kernel.job", 64, 0), inst("wgrad_big_kernel", 128, 0), inst("thin_wgrad_kernel", 5), inst("gemm_vec_kernel", 0, 0, 1)])
for _k2, _rows in ((4, 65), (40, 133), (64, 17)):
    register(f"wgrad_dual_k2_{_k2}", "wgrad_big", wgrad_case, env=WBIG, form=2,
             jobs=[dict(n_out=132 if _k2 == 40 else 128, k_in=128, rows=_rows, dm=(next(_winn), 4), im=(next(_winn), 4), k2=_k2, im2=(next(_winn), 8), max_splits=16),
                   _J(128, 16, 15, 1)],
             expect=[inst("wgrad_big_multi_kernel.job", 192, 0), inst("wgrad_big_multi_kernel.job", 64, 1)])
for _i, (_no, _ki, _rows) in enumerate([(128, 128, 133), (132, 132, 65), (260, 68, 17), (128, 100, 1)]):
    register(f"wgrad_w8_n{_no}_k{_ki}_rows{_rows}", "wgrad_big", w8_case, env=WBIG, n_out=_no, k_in=_ki, rows=_rows,
             **({} if _i == 3 else dict(dm=(next(_winn), 4), im=(next(_winn), 8))))
# below the threshold (the default 2048 rows) the same job goes to the 64 x 64 tiles
register("wgrad_small_goes_to_tiles", "wgrad_big", wgrad_case, form=0, jobs=[dict(n_out=128, k_in=20, rows=65, rows_per_split=16, dm=(7, 4))],
         expect=[inst("gemm_vec_kernel", 0, 0, 0)])

# thin outputs
_tk = _cyc([1, 3, 5, 31, 32, 33, 40, 64, 65, 130])
_tr = _cyc([(1, 512), (3, 512), (4, 512), (5, 512), (255, 512), (513, 256)])
for _no in range(1, 9):
    for _rep in range(3):
        _k = next(_tk)
        while _no in (4, 8) and _k % 4 == 0:
            _k = next(_tk)
        _rows, _rps = next(_tr)
        register(f"thin_wgrad_n{_no}_k{_k}_rows{_rows}", "thin", wgrad_case, form=_rep % 2,
                 jobs=[dict(n_out=_no, k_in=_k, rows=_rows, rows_per_split=_rps, dm=(3, 2) if _rep else None, im=(7, 1) if _rep != 1 else None,
                            i_pad=_rep)], expect=[inst("thin_wgrad_kernel", _no)])
for _no, _k in ((4, 32), (8, 40)):     # the aligned pair goes to the vector tiles
    register(f"thin_aligned_n{_no}_k{_k}_goes_elsewhere", "thin", wgrad_case, form=0, jobs=[dict(n_out=_no, k_in=_k, rows=5)],
             expect=[inst("gemm_vec_kernel", 0, 0, 1)])

# slab folds
_NPARTS = [1, 2, 3, 4, 5, 12, 13, 16, 17, 28, 29, 32, 33, 45, 64, 65]
_sn = _cyc([1, 63, 64, 65, 130])
for _np in _NPARTS:
    register(f"sum_slabs_p{_np}", "slabs", sum_slabs_case, nparts=_np, n=next(_sn))
for _b in range(0, 16, 4):           # four jobs per launch, different n, padded strides, an out2
    register(f"slab_multi_p{'_'.join(str(p) for p in _NPARTS[_b:_b + 4])}", "slabs", slab_multi_case,
             jobs=[(p, next(_sn), (0, 3)[q % 2], q == 1) for q, p in enumerate(_NPARTS[_b:_b + 4])])
register("slab_multi_eight_jobs", "slabs", slab_multi_case, jobs=[(p, next(_sn), q % 3, q == 7) for q, p in enumerate([1, 4, 5, 16, 17, 32, 33, 65])])
register("slab_multi_adamw", "slabs", slab_multi_case, adamw=True, jobs=[(3, 65, 2, False), (13, 1, 0, True), (29, 130, 0, False)])
register("slab_multi_mean", "slabs", slab_multi_case, jobs=[(2, 63, 0, False)], mean=[3, 0, 7, 1, 31])
register("slab_multi_mean_only", "slabs", slab_multi_case, jobs=[], mean=[0] + list(range(1, 300)), families=("gauss",))
register("slab_multi_adamw_mean", "slabs", slab_multi_case, adamw=True, jobs=[(5, 64, 0, True)], mean=[0, 2])
register("slab_ninth_job_overflows", "slabs", slab_overflow_case, families=("int",))

# column sums
_cn = _cyc([1, 63, 64, 65])
for _i, _rows in enumerate([1, 3, 4, 5, 16, 17, 255, 256, 257, 64 * 256 + 3]):
    register(f"colsum_rows{_rows}", "colsum", colsum_case, rows=_rows, n=next(_cn), rm=(3, 2) if _i % 2 else None, pad=_i % 3, deferred=_i % 2, out1=_i % 3 != 1,
             rows_per_chunk=256 if _rows > 17 else (256, 4)[_i % 2])
register("colsum_small_max_chunks", "colsum", colsum_case, rows=1000, n=65, rm=(7, 5), max_chunks=3, rows_per_chunk=16, out1=True)
for _n, _ip in ((1, 0), (255, 1), (257, 0), (70000, 1)):
    register(f"relu_bwd_n{_n}_inplace{_ip}", "colsum", relu_bwd_case, n=_n, in_place=bool(_ip))
register("refusals", "colsum", refusals_case, families=("int",))

GROUPS = sorted({c.group for c in CASES.values()})


def names(backend, group=None):
    return [n for n, c in CASES.items() if getattr(c, backend) and (group is None or c.group == group)]


def report_lines(backend, ratios):
    return [f"{backend:<4} {k:<36} {v:.4f}" for k, v in sorted(ratios.items())]


# ---- child process of tests/test_emu_dense.py: one group of cases on guarded host memory ------------------------------------------------------
def main(group, placement):
    import contextlib
    import emu_util
    from guard_mem import Arena
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    ctx = Ctx(lib, lambda: Arena(placement), "emu")
    real_call = lib.call

    def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
        print(f"guard_mem: --- {name} ({placement})", file=sys.stderr)
        ctx.al.describe()
        return real_call(name, *args)
    lib.call = call
    results = {}
    for name in names("emu", group):
        saved = dict(os.environ)
        print(f"dense: --- {name} ({placement})", file=sys.stderr, flush=True)
        t0 = time.time()
        try:
            with contextlib.redirect_stdout(sys.stderr):
                run_case(ctx, name, os.environ.__setitem__)
            results[name] = dict(ok=True)
        except AssertionError as e:
            results[name] = dict(ok=False, msg=str(e)[:2000])
        results[name]["seconds"] = round(time.time() - t0, 2)
        os.environ.clear()
        os.environ.update(saved)
    print(json.dumps(dict(results=results, seen=sorted(ctx.seen), ratios=ctx.ratios)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
