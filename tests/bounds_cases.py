"""The bounds cases shared by tests/test_emu_bounds.py (guarded host pages on the hipemu emulator) and tests/test_gpu_bounds.py
(sentinel bands on the device).  A case builds every argument of its entry point(s) through an allocator (`al.buf`), one buffer
per operand (each parameter and each gradient on its own, workspaces at exactly the size the library's query returns), calls the
C ABI, compares with the oracle (or a float64 reference for the cheap ops) and leaves `al.check()` to the runner.

CASES: case id -> Case(entry points, env switches, function(al, lib, big)); `big` selects the device-sized shapes."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from ctc_util import make_case, reference as ctc_reference
from howl_amd.lib import (FB_PACKED_FLOATS, HowlAdamW, HowlHeadGrads, HowlHeadParams, HowlLogmelArgs, HowlLstmGrads, HowlLstmParams,
                          HowlLstmSaved, HowlMelPoints, HowlRes8Grads, HowlRes8Params, HowlRes8Saved, fb_packed_floats)
from oracle import frontend as fe
from oracle import models as om


@dataclass
class Case:
    entry_points: tuple
    fn: object
    env: dict = field(default_factory=dict)
    params: dict = field(default_factory=dict)
    emu: bool = True          # runs on the emulator (out-of-contract cases: the emulator only)
    gpu: bool = True


CASES = {}


def register(name, entry_points, fn, env=None, emu=True, gpu=True, **params):
    CASES[name] = Case(tuple(entry_points), fn, dict(env or {}), params, emu, gpu)


def close(a, b, atol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    assert np.all(np.isfinite(a) == np.isfinite(b)), f"{what}: finiteness differs"
    fin = np.isfinite(b)
    if fin.any() and err[fin].max() > atol:
        worst = np.unravel_index(np.argmax(np.where(fin, err, -1.0)), err.shape)
        raise AssertionError(f"{what}: max |err| {err[fin].max():.3g} > {atol:.3g} at {list(map(int, worst))} "
                             f"({int((err[fin] > atol).sum())} elements over)")


# ---- frontend -------------------------------------------------------------------------------------------------------------

def _fb(M, rng):
    """The standard filterbank (M >= 40) or a dense random one (M < 40: the triangles of so few bins are degenerate)."""
    return fe.mel_fb(M).numpy() if M >= 40 else rng.uniform(0.1, 1.0, (257, M)).astype(np.float32)


def _pack(al, lib, fb, name="fbp"):
    M = fb.shape[1]
    n = int(lib.cdll.howl_fb_packed_floats(M))
    assert n == fb_packed_floats(M)
    src = al.buf(name + ".fb", fb.shape, np.float32, np.ascontiguousarray(fb, np.float32))
    fbp = al.buf(name, n, np.float32, "sentinel", promised="all")
    lib.call("howl_fb_pack", al.ptr(src), M, al.ptr(fbp), None)
    return fbp


def logmel_case(al, lib, big, B, L, ld, M, layout=0, zmuv=False):
    rng = np.random.default_rng(B * 1000 + L + M)
    if big:
        B, L, ld = 512, 16000, 16000
    ld = ld or L
    T = 1 + L // 200
    n = (B - 1) * ld + L                              # the last row ends the buffer: the pcm tail flush
    flat = (0.1 * rng.standard_normal(n)).astype(np.float32)
    pcm = al.buf("pcm", n, np.float32, flat)
    fb = _fb(M, rng)
    fbp = _pack(al, lib, fb)
    zm = al.buf("zmuv", 2, np.float32, np.array([-2.0, 1.5], np.float32)) if zmuv else None
    shape = (B, M, T) if layout == 0 else (B, T, M)
    out = al.buf("out", shape, np.float32, "sentinel", promised="all")
    lib.call("howl_logmel_fwd", al.ptr(pcm), B, L, ld, al.ptr(fbp), M, 1e-7, al.ptr(zm), al.ptr(out), layout, None)
    al.sync()
    got = al.get(out)
    rows = np.stack([flat[b * ld:b * ld + L] for b in range(B)]) if not big else None
    if big:       # the device-sized case: every row against the oracle would take minutes on the CPU; a sample of rows
        pick = [0, 1, B // 2, B - 1]
        rows = np.stack([flat[b * ld:b * ld + L] for b in pick])
        got = got[pick]
    power = fe.power_spectrogram(torch.from_numpy(rows).double())
    ref = torch.log(torch.matmul(power.transpose(-1, -2), torch.from_numpy(fb).double()) + 1e-7)       # (B, T, M)
    if zmuv:
        ref = (ref + 2.0) / 1.5
    ref = ref.numpy() if layout == 1 else ref.transpose(-1, -2).numpy()
    # test_emu_frontend's bounds: 1e-4 for the standard filterbank, 3e-4 for a dense random one
    close(got, ref, 1e-4 if M >= 40 else 3e-4, "log-mels")
    assert np.isfinite(al.get(out)).all()     # (every row: an over-read of a NaN band would show here)
    # the packed image holds the matrix (both banks for M > 48)
    fbp_h = al.get(fbp)
    lo = M if M <= 48 else 4 * ((M + 7) // 8)
    assert np.array_equal(fbp_h[:260 * 48].reshape(260, 48)[:257, :lo], fb[:, :lo])
    if M > 48:
        assert np.array_equal(fbp_h[FB_PACKED_FLOATS:FB_PACKED_FLOATS + 260 * 48].reshape(260, 48)[:257, :M - lo], fb[:, lo:])


for _B, _L, _ld, _M, _lay, _z in [(1, 257, 0, 40, 0, False), (3, 399, 0, 1, 1, False), (3, 400, 0, 48, 0, True),
                                  (1, 401, 0, 49, 1, False), (3, 401, 7, 40, 0, False), (2, 455, 200, 80, 1, True),
                                  (3, 1000, 0, 80, 0, False)]:
    register(f"logmel_B{_B}_L{_L}_ld{_ld or _L}_M{_M}_layout{_lay}", ["howl_logmel_fwd", "howl_fb_pack"], logmel_case,
             B=_B, L=_L, ld=_ld, M=_M, layout=_lay, zmuv=_z, gpu=(_M == 80 and _lay == 0))
register("logmel_M80_two_launches", ["howl_logmel_fwd", "howl_fb_pack"], logmel_case, env={"HOWL_LOGMEL_TWO_LAUNCHES": "1"},
         B=3, L=401, ld=0, M=80, layout=1, zmuv=True)


def fb_points_case(al, lib, big, M):
    import math
    m_pts = torch.linspace(0.0, 2595.0 * math.log10(1.0 + 8000.0 / 700.0), M + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    pts = HowlMelPoints()
    for i, v in enumerate(f_pts.tolist()):
        pts.f[i] = v
    n = fb_packed_floats(M)
    lo = M if M <= 48 else 4 * ((M + 7) // 8)

    out = al.buf("fbp", n, np.float32, "sentinel", promised="all")
    lib.call("howl_fb_from_points", pts, M, 8000.0, al.ptr(out), None)
    al.sync()
    got = al.get(out)
    ref = fe.mel_fb(M).numpy()
    close(got[:260 * 48].reshape(260, 48)[:257, :lo], ref[:, :lo], 2e-7, "bank 0")
    if M > 48:
        close(got[FB_PACKED_FLOATS:FB_PACKED_FLOATS + 260 * 48].reshape(260, 48)[:257, :M - lo], ref[:, lo:], 2e-7, "bank 1")


for _M in (1, 40, 49, 80):
    register(f"fb_from_points_M{_M}", ["howl_fb_from_points"], fb_points_case, M=_M, gpu=_M == 80)


def deltas_case(al, lib, big, B, M, T, zmuv):
    rng = np.random.default_rng(B + M + T)
    if big:
        B, T = 512, 81
    x = al.buf("logmel", (B, M, T), np.float32, rng.standard_normal((B, M, T)).astype(np.float32))
    zm = al.buf("zmuv", 2, np.float32, np.array([0.5, 2.0], np.float32)) if zmuv else None
    out = al.buf("out3", (B, 3, M, T), np.float32, "sentinel", promised="all")
    lib.call("howl_deltas_fwd", al.ptr(x), B, M, T, al.ptr(zm), al.ptr(out), None)
    al.sync()
    ref = fe.standard_audio_transform(torch.from_numpy(al.get(x).copy()).double(), None, deltas_only=True).numpy()
    if zmuv:
        ref = (ref - 0.5) / 2.0
    close(al.get(out), ref, 1e-6, "deltas")


for _B, _M, _T, _z in [(1, 1, 1, False), (3, 3, 2, True), (1, 40, 3, False), (3, 7, 9, True)]:
    register(f"deltas_B{_B}_M{_M}_T{_T}", ["howl_deltas_fwd"], deltas_case, B=_B, M=_M, T=_T, zmuv=_z, gpu=_T == 9)


def zmuv_case(al, lib, big, n):
    rng = np.random.default_rng(n)
    if big:
        n = 512 * 40 * 81 + 3
    total, mean, mean2 = (al.buf(k, 1, np.float32, 0.0) for k in ("total", "mean", "mean2"))
    s2 = al.buf("scratch2", 2, np.float64, 0.0)
    s3 = al.buf("scratch3", 3, np.float64, 0.0)
    xs = (rng.standard_normal(n) * 3 - 7).astype(np.float32)
    xs2 = (rng.standard_normal(n) * 2 + 1).astype(np.float32)
    ms = (rng.uniform(size=n) < 0.6).astype(np.float32)
    ms[0] = 1.0                                       # n = 1: two different values, a variance that is not zero
    x = al.buf("x", n, np.float32, xs)
    x2 = al.buf("x2", n, np.float32, xs2)
    msk = al.buf("mask", n, np.float32, ms)
    lib.call("howl_zmuv_update", al.ptr(x), n, al.ptr(total), al.ptr(mean), al.ptr(mean2), al.ptr(s2), None)
    lib.call("howl_zmuv_update_masked", al.ptr(x2), al.ptr(msk), n, 1.0, al.ptr(total), al.ptr(mean), al.ptr(mean2), al.ptr(s3), None)
    pair = al.buf("pair", 2, np.float32, "sentinel", promised="all")
    lib.call("howl_zmuv_pair", al.ptr(mean), al.ptr(mean2), al.ptr(pair), None)
    out = al.buf("out", n, np.float32, "sentinel", promised="all")
    lib.call("howl_zmuv_apply", al.ptr(x), n, al.ptr(pair), al.ptr(out), None)
    al.sync()
    x64, y64, m64 = xs.astype(np.float64), xs2.astype(np.float64), ms.astype(np.float64)
    cnt = n + m64.sum()
    mu = (x64.sum() + (y64 * m64).sum()) / cnt
    mu2 = ((x64 ** 2).sum() + ((y64 * m64) ** 2).sum()) / cnt
    assert al.get(total)[0] == cnt
    close(al.get(mean), [mu], 1e-6 * abs(mu), "mean")
    close(al.get(mean2), [mu2], 1e-6 * abs(mu2), "mean2")
    p = al.get(pair).astype(np.float64)
    close(p, [al.get(mean)[0], np.sqrt(float(al.get(mean2)[0]) - float(al.get(mean)[0]) ** 2)], 1e-5 * abs(p[1]) + 1e-6, "pair")
    close(al.get(out), (x64 - p[0]) / p[1], 1e-5, "apply")


for _n in (1, 3, 4097):
    register(f"zmuv_n{_n}", ["howl_zmuv_update", "howl_zmuv_update_masked", "howl_zmuv_pair", "howl_zmuv_apply"], zmuv_case, n=_n,
             gpu=_n == 4097)


def specaug_case(al, lib, big, B, C, M, T):
    rng = np.random.default_rng(B + T)
    if big:
        B = 512
    x0 = rng.standard_normal((B, C, M, T)).astype(np.float32)
    x = al.buf("x", (B, C, M, T), np.float32, x0)
    f0 = np.array([(M - 3) % M if b % 3 == 0 else 0 for b in range(B)], np.int32)
    f = np.array([M - f0[b] if b % 2 == 0 else (0 if b % 3 == 1 else 1) for b in range(B)], np.int32)   # ends exactly at M
    t0 = np.array([T - 1 if b % 2 == 1 else 0 for b in range(B)], np.int32)
    t = np.array([T - t0[b] if b % 3 != 2 else 0 for b in range(B)], np.int32)                         # ends exactly at T
    bufs = [al.buf(k, B, np.int32, v) for k, v in (("f0", f0), ("f", f), ("t0", t0), ("t", t))]
    lib.call("howl_specaug_mask", al.ptr(x), B, C, M, T, C * M * T, M * T, T, 1, *[al.ptr(b) for b in bufs], None)
    al.sync()
    ref = x0.copy()
    for b in range(B):
        if f[b] > 0:
            ref[b, :, f0[b]:f0[b] + f[b], :] = 0.0
        if t[b] > 0:
            ref[b, :, :, t0[b]:t0[b] + t[b]] = 0.0
    assert np.array_equal(al.get(x), ref)


register("specaug_B3_T1", ["howl_specaug_mask"], specaug_case, B=3, C=3, M=40, T=1, gpu=False)
register("specaug_B5_T81", ["howl_specaug_mask"], specaug_case, B=5, C=3, M=40, T=81)


def collate_case(al, lib, big, kind):
    rng = np.random.default_rng(7)
    nrow, ld = (4, 1003) if not big else (600, 16003)
    Lout = ld - 50
    B = 5 if not big else 512
    bank_h = (0.1 * rng.standard_normal((nrow, ld))).astype(np.float32)
    bank = al.buf("bank", (nrow, ld), np.float32, bank_h)
    idx = np.array([(nrow - 1) if b % 2 == 0 else b % nrow for b in range(B)], np.int32)       # the last bank row: its tail flush
    src_len = np.array([ld if b % 3 == 0 else ld // 2 + b for b in range(B)], np.int32)
    shift = np.array([ld + 5 if b % 4 == 1 else (b * 37) % 400 for b in range(B)], np.int32)     # a shift past the clip's end
    head = np.array([b % 2 for b in range(B)], np.int32)
    i32 = lambda k, v: al.buf(k, B, np.int32, v)
    f32 = lambda k, v: al.buf(k, B, np.float32, v)
    ib = [i32("idx", idx), i32("src_len", src_len), i32("shift", shift), i32("from_head", head)]
    zero = np.zeros(B, np.float32)
    sg, sp = f32("sigma", zero), f32("sp_prob", zero)
    out = al.buf("out", (B, Lout), np.float32, "sentinel", promised="all")
    # the host form of the chain: crop [shift, src_len) (from_head) or [0, src_len - shift), pad right
    clips = []
    if kind == "plain":
        lib.call("howl_collate_augment", al.ptr(bank), ld, *[al.ptr(b) for b in ib], al.ptr(sg), al.ptr(sp), 3, B, Lout, al.ptr(out), None)
        mixed = [bank_h[idx[b], :src_len[b]].astype(np.float64) for b in range(B)]
    else:
        nbg, bld = 3, 2 * ld
        bg_h = (0.2 * rng.standard_normal((nbg, bld))).astype(np.float32)
        bg = al.buf("bg", (nbg, bld), np.float32, bg_h)
        bg_idx = np.array([nbg - 1 if b % 2 == 0 else b % nbg for b in range(B)], np.int32)
        bg_off = np.array([bld - src_len[b] for b in range(B)], np.int32)          # the background window ends at its row's end
        alpha = np.array([0.15, 0.0, 1.0, 0.5, 0.25] * (B // 5 + 1), np.float32)[:B]
        extra = [i32("bg_idx", bg_idx), i32("bg_off", bg_off), f32("alpha", alpha)]
        mixed = [bank_h[idx[b], :src_len[b]].astype(np.float32) * np.float32(1 - alpha[b]) +
                 bg_h[bg_idx[b], bg_off[b]:bg_off[b] + src_len[b]] * np.float32(alpha[b]) for b in range(B)]
        mixed = [m.astype(np.float64) for m in mixed]
        if kind == "mix":
            lib.call("howl_collate_augment_mix", al.ptr(bank), ld, *[al.ptr(b) for b in ib], al.ptr(sg), al.ptr(sp), 3, al.ptr(bg),
                     bld, *[al.ptr(b) for b in extra], B, Lout, al.ptr(out), None)
        else:
            dst = np.array([(b * 11) % 40 for b in range(B)], np.int32)
            extra.append(i32("dst_off", dst))
            lib.call("howl_collate_augment_window", al.ptr(bank), ld, *[al.ptr(b) for b in ib], al.ptr(sg), al.ptr(sp), 3,
                     al.ptr(bg), bld, *[al.ptr(b) for b in extra], B, Lout, al.ptr(out), None)
    al.sync()
    got = al.get(out)
    for b in range(B):
        m = mixed[b]
        s = min(int(shift[b]), len(m))
        seg = m[s:] if head[b] else m[:len(m) - s]
        exp = np.zeros(Lout)
        off = 0 if kind != "window" else int((b * 11) % 40)
        k = max(0, min(len(seg), Lout - off))
        exp[off:off + k] = seg[:k]
        close(got[b], exp, 1e-7, f"row {b}")


for _k, _eps in (("plain", ["howl_collate_augment"]), ("mix", ["howl_collate_augment_mix"]), ("window", ["howl_collate_augment_window"])):
    register(f"collate_{_k}", _eps, collate_case, kind=_k)


def gather_case(al, lib, big, width):
    rng = np.random.default_rng(width)
    nrow, ld = (3, 1000)
    B = 5 if not big else 8192
    bank_h = rng.standard_normal((nrow, ld)).astype(np.float32)
    bank = al.buf("bank", (nrow, ld), np.float32, bank_h)
    idx = np.array([nrow - 1, 0, 1, 1, nrow - 1] * (B // 5 + 1), np.int32)[:B]
    length = np.array([min(width, ld), 0, min(3, width), min(width, 7), min(width, 5)] * (B // 5 + 1), np.int32)[:B]
    start = np.array([ld - length[b] if b % 5 == 4 else (0, 10, 997, 500, 0)[b % 5] for b in range(B)], np.int32)  # ends at the row's end
    dst = np.array([width - length[b] if b % 5 in (0, 2) else 0 for b in range(B)], np.int32)
    bufs = [al.buf(k, B, np.int32, v) for k, v in (("idx", idx), ("start", start), ("len", length), ("dst_off", dst))]
    out = al.buf("out", (B, width), np.float32, "sentinel", promised="all")
    lib.call("howl_gather_windows", al.ptr(bank), ld, *[al.ptr(b) for b in bufs], B, width, al.ptr(out), None)
    al.sync()
    got = al.get(out)
    for b in range(B):
        exp = np.zeros(width, np.float32)
        exp[dst[b]:dst[b] + length[b]] = bank_h[idx[b], start[b]:start[b] + length[b]]
        assert np.array_equal(got[b], exp), b


for _w in (1, 5, 1003):
    register(f"gather_windows_w{_w}", ["howl_gather_windows"], gather_case, width=_w, gpu=_w == 1003)


# ---- cross-entropy, AdamW, dropout ---------------------------------------------------------------------------------------------

def xent_case(al, lib, big, B, C):
    rng = np.random.default_rng(B * 100 + C)
    if big:
        B = 4097
    z = (80.0 * np.sign(rng.standard_normal((B, C)))).astype(np.float32) * rng.uniform(0.5, 1.0, (B, C)).astype(np.float32)
    lab = (np.arange(B) * 7 % C).astype(np.int64)
    logits = al.buf("logits", (B, C), np.float32, z)
    labels = al.buf("labels", B, np.int64, lab)
    loss = al.buf("loss", 1, np.float32, "sentinel", promised="all")
    dl = al.buf("dlogits", (B, C), np.float32, "sentinel", promised="all")
    lib.call("howl_xent_fwd_bwd", al.ptr(logits), al.ptr(labels), B, C, al.ptr(loss), al.ptr(dl), None)
    al.sync()
    t = torch.from_numpy(z).double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(t, torch.from_numpy(lab))
    ref.backward()
    t32 = torch.from_numpy(z).requires_grad_(True)
    torch.nn.functional.cross_entropy(t32, torch.from_numpy(lab)).backward()
    noise = float((t32.grad.double() - t.grad).abs().max())       # torch-fp32's own distance from fp64
    # the kernel takes softmax as exp(z - lse) with lse rounded to fp32: one ulp of |lse| (<= 80 here) in the exponent
    lse_ulp = float(torch.logsumexp(t.detach(), 1).abs().max()) * 2.0 ** -23
    close(al.get(loss), [ref.item()], 1e-5 * max(1.0, abs(ref.item())), "loss")
    close(al.get(dl), t.grad.numpy(), 2 * noise + lse_ulp + 1e-6, "dlogits")


for _B, _C in ((1, 1), (1, 2), (1, 64), (3, 2), (5, 64)):
    register(f"xent_B{_B}_C{_C}", ["howl_xent_fwd_bwd"], xent_case, B=_B, C=_C, gpu=(_B, _C) == (5, 64))


def adamw_case(al, lib, big, n):
    rng = np.random.default_rng(n)
    if big:
        n = (1 << 20) + 3
    p0 = rng.standard_normal(n).astype(np.float32)
    p = al.buf("p", n, np.float32, p0)
    m = al.buf("m", n, np.float32, 0.0)
    v = al.buf("v", n, np.float32, 0.0)
    tp = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.AdamW([tp], 0.01, weight_decay=1e-2)
    for step in range(1, 3):
        g0 = rng.standard_normal(n).astype(np.float32)
        g = al.buf(f"g{step}", n, np.float32, g0)
        lib.call("howl_adamw_step", al.ptr(p), al.ptr(g), al.ptr(m), al.ptr(v), n, 0.01, 0.9, 0.999, 1e-8, 1e-2, step, 1.0, None)
        tp.grad = torch.from_numpy(g0.astype(np.float64))
        opt.step()
    al.sync()
    close(al.get(p), tp.detach().numpy(), 2e-6, "p")
    st = opt.state[tp]
    close(al.get(m), st["exp_avg"].numpy(), 1e-6, "m")
    close(al.get(v), st["exp_avg_sq"].numpy(), 1e-6, "v")


for _n in (1, 3, 4097):
    register(f"adamw_n{_n}", ["howl_adamw_step"], adamw_case, n=_n, gpu=_n == 4097)


def dropout_case(al, lib, big, n):
    if big:
        n = 512 * 1280 + 1
    mask = al.buf("mask", n, np.float32, "sentinel", promised="all")
    lib.call("howl_dropout_mask", al.ptr(mask), n, 0.5, 1234, None)
    al.sync()
    got = al.get(mask)
    assert np.all((got == 0.0) | (got == 1.0))
    if n > 1000:
        assert 0.45 < got.mean() < 0.55


for _n in (1, 3, 4097):
    register(f"dropout_n{_n}", ["howl_dropout_mask"], dropout_case, n=_n, gpu=_n == 4097)


# ---- CTC -------------------------------------------------------------------------------------------------------------------

def _ctc_call(al, lib, z, tg, L, il, tl, blank, want_grad=True, tag=""):
    """howl_ctc_loss on guarded copies; targets of width L == max_target_length (the last row ends the buffer)."""
    B, T, C = z.shape
    zb = al.buf("logits" + tag, (B, T, C), np.float32, z)
    tb = al.buf("targets" + tag, (B, L), np.int64, np.ascontiguousarray(tg[:, :L]))
    ilb = al.buf("in_len" + tag, B, np.int64, il)
    tlb = al.buf("tgt_len" + tag, B, np.int64, tl)
    nll = al.buf("nll" + tag, B, np.float32, "sentinel", promised="all")
    loss = al.buf("loss" + tag, 1, np.float32, "sentinel", promised="all")
    dz = al.buf("dlogits" + tag, (B, T, C), np.float32, "sentinel", promised="all") if want_grad else None
    nws = int(lib.cdll.howl_ctc_workspace_floats(T, B)) if want_grad else 0
    ws = al.buf("workspace" + tag, nws, np.float32, "sentinel") if nws else None
    lib.call("howl_ctc_loss", al.ptr(zb), C, T * C, T, B, C, al.ptr(tb), L, L, al.ptr(ilb), al.ptr(tlb), blank, al.ptr(nll),
             al.ptr(loss), al.ptr(dz), C, T * C, al.ptr(ws), nws, None)
    al.sync()
    return al.get(nll).copy(), float(al.get(loss)[0]), None if dz is None else al.get(dz).copy()


def ctc_case(al, lib, big, T, B, C, L, blank, tight=False):
    if big:
        T, B, C, L = 8192, 2, 64, 31
    blank = 0 if blank == 0 else C - 1
    logits, targets, in_len, tgt_len, blank = make_case(T, B, C, L, T + C + L, blank=blank, tight=tight)
    Lw = max(L, int(tgt_len.max()))
    nll, loss, dz = _ctc_call(al, lib, logits.numpy(), targets.numpy(), Lw, in_len.numpy(), tgt_len.numpy(), blank)
    per, ref_loss, grad = ctc_reference(logits.double(), targets, in_len, tgt_len, blank)
    assert np.isfinite(per.numpy()).all()
    close(nll, per.numpy(), 2e-5 * max(1.0, float(per.abs().max())), "nll")
    close([loss], [float(ref_loss)], 2e-5 * max(1.0, abs(float(ref_loss))), "loss")
    # torch-fp32's own distance from fp64 bounds the fp32 log-space recursion (test_emu_ctc's whole-clip bounds): alpha + beta
    # reach -700 over long utterances and a target of length 0 (one fp32 ulp there is 6e-5)
    _, _, g32 = ctc_reference(logits, targets, in_len, tgt_len, blank)
    noise = float((g32.double() - grad).abs().max())
    close(dz, grad.numpy(), 1.5 * noise + 1e-5, "dlogits vs fp64")
    close(dz, g32.numpy(), 2.5 * noise + 1e-5, "dlogits vs torch fp32")
    for b in range(B):
        assert not dz[b, int(in_len[b]):].any()


def _ctc_L(T, C):
    """The longest target make_case can always align: all labels alike at C = 2 needs 2L - 1 frames."""
    return min(31, (T + 1) // 2 if C == 2 else T)


for _T in (1, 127, 128, 129, 256, 257):
    for _C in (2, 64):
        for _L in sorted({0, _ctc_L(_T, _C)}):
            register(f"ctc_T{_T}_C{_C}_L{_L}_blank{'0' if _T % 2 else 'last'}", ["howl_ctc_loss"], ctc_case, T=_T, B=3, C=_C, L=_L,
                     blank=0 if _T % 2 else -1, tight=_L > 1, gpu=(_T, _C, _L) == (257, 64, 31))


BAD_KINDS = ("label_high", "label_negative", "length_over_max", "length_negative", "input_negative")


def _spoil(kind, tg, il, tl, b, C, L):
    tg, il, tl = tg.copy(), il.copy(), tl.copy()
    if kind == "label_high":
        tg[b, max(0, tl[b] - 1)] = C
        tl[b] = max(tl[b], 1)
    elif kind == "label_negative":
        tg[b, 0] = -1
        tl[b] = max(tl[b], 1)
    elif kind == "length_over_max":
        tl[b] = L + 1
    elif kind == "length_negative":
        tl[b] = -1
    else:
        il[b] = -1
    return tg, il, tl


def ctc_contract_case(al, lib, big, where, kind, T=12):
    """One utterance outside the contract (include/howl_hip.h): nll = +inf, zero gradient rows, the others bit-identical.
    T = 129: the windowed path (alpha rows in the workspace)."""
    B, C, L = 4, 5, 3
    logits, targets, in_len, tgt_len, blank = make_case(T, B, C, L, 17)
    z, tg, il, tl = logits.numpy(), targets.numpy()[:, :L].copy(), in_len.numpy(), tgt_len.numpy()
    tl[:] = np.minimum(np.maximum(tl, 1), L)
    b = {"first": 0, "middle": B // 2, "last": B - 1}[where]
    nll0, _, dz0 = _ctc_call(al, lib, z, tg, L, il, tl, blank, tag=".valid")
    tg1, il1, tl1 = _spoil(kind, tg, il, tl, b, C, L)
    nll1, loss1, dz1 = _ctc_call(al, lib, z, tg1, L, il1, tl1, blank, tag=".spoilt")
    assert nll1[b] == np.inf and loss1 == np.inf
    assert not dz1[b].any()
    others = [i for i in range(B) if i != b]
    assert np.array_equal(nll1[others], nll0[others])
    assert np.array_equal(dz1[others], dz0[others])


for _where in ("first", "middle", "last"):
    for _kind in BAD_KINDS:
        register(f"ctc_contract_{_kind}_{_where}", ["howl_ctc_loss"], ctc_contract_case, where=_where, kind=_kind, gpu=False)
    register(f"ctc_contract_{_where}_T129", ["howl_ctc_loss"], ctc_contract_case, where=_where, kind="label_high", T=129, gpu=False)


# ---- the sequence head: howl_head_fwd / _bwd, howl_seq_head_ctc ----------------------------------------------------------------

def _head_params(al, C, rng, n_in=128, n_hid=256, tag=""):
    sd = {"w1": (rng.standard_normal((n_hid, n_in)) / np.sqrt(n_in)).astype(np.float32),
          "b1": (0.1 * rng.standard_normal(n_hid)).astype(np.float32),
          "w2": (rng.standard_normal((C, n_hid)) / np.sqrt(n_hid)).astype(np.float32),
          "b2": (0.1 * rng.standard_normal(C)).astype(np.float32)}
    bufs = {k: al.buf(f"head.{k}{tag}", v.shape, np.float32, v) for k, v in sd.items()}
    return sd, bufs, HowlHeadParams(al.ptr(bufs["w1"]), al.ptr(bufs["b1"]), al.ptr(bufs["w2"]), al.ptr(bufs["b2"]))


def head_case(al, lib, big, rows, n_out):
    """howl_head_fwd + howl_head_bwd on rows inside a longer (B, T + 1, 128) buffer, every gradient on its own."""
    rng = np.random.default_rng(rows + n_out)
    if big:
        rows = 2049 * 8
    T = 7 if rows % 7 == 0 else 1
    B = rows // T
    n_in, n_hid = 128, 256
    xs = rng.standard_normal((B, T + 1, n_in)).astype(np.float32)
    x = al.buf("x", (B, T + 1, n_in), np.float32, xs)
    sd, hb, hp = _head_params(al, n_out, rng)
    y1 = al.buf("y1", (rows, n_hid), np.float32, "sentinel", promised="all")
    y2 = al.buf("y2", (rows, n_out), np.float32, "sentinel", promised="all")
    geom = (T, (T + 1) * n_in, n_in, rows, n_in, n_hid, n_out)
    lib.call("howl_head_fwd", ctypes.byref(hp), al.ptr(x), *geom, al.ptr(y1), al.ptr(y2), None)
    dys = rng.standard_normal((rows, n_out)).astype(np.float32)
    dy2 = al.buf("dy2", (rows, n_out), np.float32, dys)
    dz1 = al.buf("dz1", (rows, n_hid), np.float32, "sentinel", promised="all")
    dx = al.buf("dx", (rows, n_in), np.float32, "sentinel", promised="all")
    gb = {k: al.buf(f"grad.{k}", sd[k].shape, np.float32, "sentinel", promised="all") for k in sd}
    gr = HowlHeadGrads(*[al.ptr(gb[k]) for k in ("w1", "b1", "w2", "b2")])
    nws = int(lib.cdll.howl_head_workspace_bytes(n_in, n_hid, n_out))
    ws = al.buf("head_ws", nws, np.uint8, "sentinel")
    lib.call("howl_head_bwd", ctypes.byref(hp), al.ptr(x), *geom, al.ptr(y1), al.ptr(dy2), al.ptr(dz1), al.ptr(dx), ctypes.byref(gr),
             None, al.ptr(ws), nws, None)
    al.sync()
    # float64 reference; the backward takes the ReLU mask of the kernel's own y1 (checked against the reference first): a
    # pre-activation within rounding of 0 may fall on either side, and a flipped mask bit moves a whole dz1 element
    xr = xs[:, :T].reshape(rows, n_in).astype(np.float64)
    w1, b1, w2, b2 = (sd[k].astype(np.float64) for k in ("w1", "b1", "w2", "b2"))
    y1_ref = np.maximum(xr @ w1.T + b1, 0.0)
    close(al.get(y1), y1_ref, 1e-4, "y1")
    close(al.get(y2), y1_ref @ w2.T + b2, 1e-4, "y2")
    dy = dys.astype(np.float64)
    dz1_ref = (dy @ w2) * (al.get(y1) > 0)
    close(al.get(dz1), dz1_ref, 1e-4, "dz1")
    close(al.get(dx), dz1_ref @ w1, 1e-4, "dx")
    refs = {"w1": dz1_ref.T @ xr, "b1": dz1_ref.sum(0), "w2": dy.T @ y1_ref, "b2": dy.sum(0)}
    for k, ref in refs.items():
        close(al.get(gb[k]), ref, 1e-4 * max(1.0, np.abs(ref).max()), "grad " + k)


register("head_rows1_out1", ["howl_head_fwd", "howl_head_bwd"], head_case, rows=1, n_out=1, gpu=False)
register("head_rows531_out8", ["howl_head_fwd", "howl_head_bwd"], head_case, rows=531, n_out=8)
register("head_rows531_out8_rowgemm", ["howl_head_fwd", "howl_head_bwd"], head_case, env={"HOWL_ROWGEMM_MIN_ROWS": "1"},
         rows=531, n_out=8, gpu=False)
register("head_rows35_out5_no_rowgemm", ["howl_head_fwd", "howl_head_bwd"], head_case, env={"HOWL_GEMM_NO_ROWGEMM": "1"},
         rows=35, n_out=5, gpu=False)


def _seq_head_call(al, lib, B, T, C, xs, sd_tag, rng_seed, tg, L, il, tl, blank, tag):
    rng = np.random.default_rng(rng_seed)
    n_in, n_hid = 128, 256
    x = al.buf("x" + tag, (B, T, n_in), np.float32, xs)
    sd, hb, hp = _head_params(al, C, rng, tag=tag)
    tb = al.buf("targets" + tag, (B, L), np.int64, np.ascontiguousarray(tg[:, :L]))
    ilb = al.buf("in_len" + tag, B, np.int64, il)
    tlb = al.buf("tgt_len" + tag, B, np.int64, tl)
    y2 = al.buf("y2" + tag, (B, T, C), np.float32, "sentinel", promised="all")
    nll = al.buf("nll" + tag, B, np.float32, "sentinel", promised="all")
    dz1 = al.buf("dz1" + tag, (B, T, n_hid), np.float32, "sentinel", promised="all")
    dhs = al.buf("dhs" + tag, (B, T, n_in), np.float32, "sentinel", promised="all")
    nws = int(lib.cdll.howl_head_workspace_bytes(n_in, n_hid, C))
    ws = al.buf("head_ws" + tag, nws, np.uint8, "sentinel")
    assert lib.cdll.howl_seq_head_ctc_supported(B, T, n_in, n_hid, C, L) == 1
    lib.call("howl_seq_head_ctc", ctypes.byref(hp), al.ptr(x), T * n_in, n_in, B, T, n_in, n_hid, C, al.ptr(tb), L, L, al.ptr(ilb),
             al.ptr(tlb), blank, al.ptr(y2), al.ptr(nll), al.ptr(dz1), al.ptr(dhs), al.ptr(ws), nws, None)
    al.sync()
    return sd, {k: al.get(v).copy() for k, v in (("y2", y2), ("nll", nll), ("dz1", dz1), ("dhs", dhs))}


def seq_head_case(al, lib, big, B, T, C):
    """howl_seq_head_ctc against a float64 head + torch's CTC: targets of width == max_target_length == 8."""
    if big:
        B, T = 2500, 1
    L = 8 if T >= 8 else 1
    rng = np.random.default_rng(B * 10 + T)
    xs = rng.standard_normal((B, T, 128)).astype(np.float32)
    blank = C - 1
    il = np.full(B, T, np.int64)
    tl = np.array([min(L, (T + 1) // 2) if b % 2 == 0 else 0 for b in range(B)], np.int64)
    tg = np.zeros((B, L), np.int64)
    for b in range(B):
        tg[b] = rng.integers(0, C - 1, L)
    sd, got = _seq_head_call(al, lib, B, T, C, xs, "", 99, tg, L, il, tl, blank, "")
    x = xs.astype(np.float64)
    w1, b1, w2, b2 = (sd[k].astype(np.float64) for k in ("w1", "b1", "w2", "b2"))
    pre = x @ w1.T + b1                                     # (B, T, 256)
    z = np.maximum(pre, 0.0) @ w2.T + b2
    per, loss, dlog = ctc_reference(torch.from_numpy(z), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl), blank)
    close(got["y2"], z, 1e-4, "y2")
    ok = np.isfinite(per.numpy())
    close(got["nll"][ok], per.numpy()[ok], 1e-4 * max(1.0, float(per[torch.from_numpy(ok)].abs().max())), "nll")
    # the head's backward rows; a row with a pre-activation within rounding of zero (its ReLU may fall either way) is left out
    dz1_ref = (dlog.numpy() @ w2) * (pre > 0)
    dhs_ref = dz1_ref @ w1
    solid = np.abs(pre).min(-1) > 1e-5                      # (B, T)
    scale = max(np.abs(dz1_ref).max(), 1e-30)
    close(got["dz1"][solid], dz1_ref[solid], 1e-4 * scale, "dz1")
    close(got["dhs"][solid], dhs_ref[solid], 1e-4 * max(np.abs(dhs_ref).max(), 1e-30), "dhs")
    assert np.isfinite(got["dz1"]).all() and np.isfinite(got["dhs"]).all()


register("seq_head_ctc_B1_T1", ["howl_seq_head_ctc"], seq_head_case, env={"HOWL_ROWGEMM_MIN_ROWS": "1"}, B=1, T=1, C=2, gpu=False)
register("seq_head_ctc_B3_T3", ["howl_seq_head_ctc"], seq_head_case, env={"HOWL_ROWGEMM_MIN_ROWS": "1"}, B=3, T=3, C=5, gpu=False)
register("seq_head_ctc_B5_T17_L8", ["howl_seq_head_ctc"], seq_head_case, env={"HOWL_ROWGEMM_MIN_ROWS": "1"}, B=5, T=17, C=8)


def seq_head_contract_case(al, lib, big, where, kind):
    B, T, C, L = 5, 6, 5, 3
    rng = np.random.default_rng(5)
    xs = rng.standard_normal((B, T, 128)).astype(np.float32)
    tg = rng.integers(0, C - 1, (B, L)).astype(np.int64)
    il = np.array([6, 6, 5, 4, 6], np.int64)
    tl = np.array([3, 2, 1, 3, 2], np.int64)
    b = {"first": 0, "middle": B // 2, "last": B - 1}[where]
    _, a = _seq_head_call(al, lib, B, T, C, xs, "", 7, tg, L, il, tl, C - 1, ".valid")
    tg1, il1, tl1 = _spoil(kind, tg, il, tl, b, C, L)
    _, s = _seq_head_call(al, lib, B, T, C, xs, "", 7, tg1, L, il1, tl1, C - 1, ".spoilt")
    assert s["nll"][b] == np.inf
    assert not s["dz1"][b].any() and not s["dhs"][b].any()
    others = [i for i in range(B) if i != b]
    for k in ("y2", "nll", "dz1", "dhs"):
        assert np.array_equal(s[k][others], a[k][others]), k
    assert np.array_equal(s["y2"], a["y2"])


for _where in ("first", "middle", "last"):
    for _kind in BAD_KINDS:
        register(f"seq_head_ctc_contract_{_kind}_{_where}", ["howl_seq_head_ctc"], seq_head_contract_case,
                 env={"HOWL_ROWGEMM_MIN_ROWS": "1"}, where=_where, kind=_kind, gpu=False)


# ---- LSTM ------------------------------------------------------------------------------------------------------------------

def lstm_case(al, lib, big, B, T, M, lengths, x_extra):
    """howl_lstm_fwd + howl_lstm_bwd with x inside a longer (B, T + x_extra, M) buffer; every parameter / gradient on its own."""
    if big:
        B, T, lengths = 2049, 8, None
    rng = np.random.default_rng(B * 10 + T)
    sd = om.lstm_init(5)
    keys = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    pb = {k: al.buf("lstm." + k, sd["lstm." + k].shape, np.float32, sd["lstm." + k].numpy()) for k in keys}
    prm = HowlLstmParams(*[al.ptr(pb[k]) for k in keys])
    xf = T + x_extra
    xs = rng.standard_normal((B, xf, M)).astype(np.float32)
    x = al.buf("x", (B, xf, M), np.float32, xs)
    ln = None if lengths is None else np.array(lengths, np.int64)
    lnb = None if ln is None else al.buf("lengths", B, np.int64, ln)
    t_out = T if ln is None else int(ln.max())
    gx = al.buf("gx", (B, T, 512), np.float32, "sentinel")
    gates = al.buf("gates", (B, T, 512), np.float32, "sentinel")
    cc = al.buf("c", (B, T, 128), np.float32, "sentinel")
    hseq = al.buf("hseq", (B, T + 1, 128), np.float32, "sentinel",
                  promised=lambda a: np.arange(T + 1)[None, :, None] <= t_out)
    dg = al.buf("dgates", (B, T, 512), np.float32, "sentinel")
    sv = HowlLstmSaved(al.ptr(gx), al.ptr(gates), al.ptr(cc), al.ptr(hseq), al.ptr(dg), t_out, xf if x_extra else 0)
    hT = al.buf("hT", (B, 128), np.float32, "sentinel", promised="all")
    cT = al.buf("cT", (B, 128), np.float32, "sentinel", promised="all")
    nws = int(lib.cdll.howl_lstm_workspace_bytes(B, T))
    ws = al.buf("workspace", nws, np.uint8, "sentinel")
    lib.call("howl_lstm_fwd", ctypes.byref(prm), al.ptr(x), B, T, M, al.ptr(lnb), None, None, ctypes.byref(sv), al.ptr(hT), al.ptr(cT),
             al.ptr(ws), nws, None)
    dys = np.zeros((B, T, 128), np.float32)
    dys[:, :t_out] = rng.standard_normal((B, t_out, 128)).astype(np.float32)
    dy = al.buf("dy", (B, T, 128), np.float32, dys)
    dh = rng.standard_normal((B, 128)).astype(np.float32)
    dc = rng.standard_normal((B, 128)).astype(np.float32)
    dhT, dcT = al.buf("dhT", (B, 128), np.float32, dh), al.buf("dcT", (B, 128), np.float32, dc)
    gb = {k: al.buf("grad." + k, sd["lstm." + k].shape, np.float32, "sentinel", promised="all") for k in keys}
    gr = HowlLstmGrads(*[al.ptr(gb[k]) for k in keys])
    lib.call("howl_lstm_bwd", ctypes.byref(prm), al.ptr(x), B, T, M, al.ptr(lnb), None, ctypes.byref(sv), al.ptr(dy), al.ptr(dhT),
             al.ptr(dcT), ctypes.byref(gr), al.ptr(ws), nws, None)
    al.sync()
    p = {k: v.clone().double().requires_grad_(True) for k, v in sd.items() if k.startswith("lstm.")}
    xr = torch.from_numpy(xs[:, :T]).double().permute(1, 0, 2).contiguous()
    lens = torch.from_numpy(ln) if ln is not None else torch.full((B,), T, dtype=torch.int64)
    seq, (h_ref, c_ref) = om._lstm_cell_seq(p, xr, lens, None)
    # test_emu_lstm's bounds on the emulator's shapes, test_gpu_lstm's at the device's
    otol, gtol = (2e-6, 2e-5) if not big else (2e-5, 5e-5)
    close(al.get(hseq)[:, 1:t_out + 1], seq.detach().permute(1, 0, 2).numpy(), otol, "hseq")
    close(al.get(hT), h_ref[0].detach().numpy(), otol, "hT")
    close(al.get(cT), c_ref[0].detach().numpy(), otol, "cT")
    loss = (seq * torch.from_numpy(dys[:, :t_out]).double().permute(1, 0, 2)).sum() + (h_ref[0] * torch.from_numpy(dh).double()).sum() \
        + (c_ref[0] * torch.from_numpy(dc).double()).sum()
    loss.backward()
    for k in keys:
        ref = p["lstm." + k].grad.numpy()
        close(al.get(gb[k]), ref, gtol * max(1.0, np.abs(ref).max()), "grad " + k)


for _rows in ("4", "16"):
    register(f"lstm_B5_T7_ragged_rows{_rows}", ["howl_lstm_fwd", "howl_lstm_bwd"], lstm_case, env={"HOWL_LSTM_ROWS": _rows},
             B=5, T=7, M=40, lengths=[7, 7, 6, 0, 2], x_extra=3, gpu=_rows == "16")
register("lstm_B3_T1", ["howl_lstm_fwd", "howl_lstm_bwd"], lstm_case, B=3, T=1, M=40, lengths=None, x_extra=0, gpu=False)
register("lstm_B17_T3_no_fused_x", ["howl_lstm_fwd", "howl_lstm_bwd"], lstm_case, env={"HOWL_LSTM_NO_FUSED_X": "1"},
         B=17, T=3, M=40, lengths=[3] * 16 + [1], x_extra=2, gpu=False)
register("lstm_B5_T4_rowgemm", ["howl_lstm_fwd", "howl_lstm_bwd"], lstm_case, env={"HOWL_ROWGEMM_MIN_ROWS": "1"},
         B=5, T=4, M=40, lengths=[4, 3, 3, 2, 1], x_extra=1, gpu=False)


# ---- res8 ------------------------------------------------------------------------------------------------------------------

class Res8Bufs:
    """res8's operands through an allocator: each parameter, BatchNorm buffer, saved activation and gradient on its own."""

    def __init__(self, al, lib, B, T, C, M, sd, train=True):
        self.al, self.B, self.T, self.C, self.M = al, B, T, C, M
        self.sd = sd
        self.p = {k: al.buf(k, v.shape, np.float32 if v.dtype == torch.float32 else np.int64, v.numpy()) for k, v in sd.items()}
        self.prm = HowlRes8Params()
        self.prm.conv0_w = al.ptr(self.p["conv0.weight"])
        for i in range(6):
            self.prm.conv_w[i] = al.ptr(self.p[f"conv{i+1}.weight"]).value
            self.prm.bn_running_mean[i] = al.ptr(self.p[f"bn{i+1}.running_mean"]).value
            self.prm.bn_running_var[i] = al.ptr(self.p[f"bn{i+1}.running_var"]).value
            self.prm.bn_num_batches[i] = al.ptr(self.p[f"bn{i+1}.num_batches_tracked"]).value
        self.prm.out_w = al.ptr(self.p["output.weight"])
        self.prm.out_b = al.ptr(self.p["output.bias"])
        ns = int(lib.cdll.howl_res8_saved_floats(B, T, M))
        self.s = [al.buf(f"saved.s{i}", ns, np.float32, "sentinel") for i in range(7)]
        self.saved = HowlRes8Saved()
        for i in range(7):
            self.saved.s[i] = al.ptr(self.s[i]).value
        self.bn_stats = al.buf("saved.bn_stats", (6, 2, 48), np.float32, "sentinel")
        self.pooled = al.buf("saved.pooled", (B, 48), np.float32, "sentinel")
        self.mask0 = al.buf("saved.mask0", ns, np.uint16, "sentinel")
        self.saved.bn_stats, self.saved.pooled, self.saved.mask0 = (al.ptr(self.bn_stats), al.ptr(self.pooled), al.ptr(self.mask0))
        self.g = {k: al.buf("grad." + k, sd[k].shape, np.float32, "sentinel", promised="all" if train else None)
                  for k in om.res8_param_names()}
        self.gr = HowlRes8Grads()
        self.gr.conv0_w = al.ptr(self.g["conv0.weight"])
        for i in range(6):
            self.gr.conv_w[i] = al.ptr(self.g[f"conv{i+1}.weight"]).value
        self.gr.out_w = al.ptr(self.g["output.weight"])
        self.gr.out_b = al.ptr(self.g["output.bias"])
        self.nws = int(lib.cdll.howl_res8_workspace_bytes_mels(B, T, M))
        self.ws = al.buf("workspace", self.nws, np.uint8, "sentinel")


def _res8_ref(sd, x, labels):
    names = om.res8_param_names()
    params = {n: sd[n].clone().requires_grad_(True) for n in names}
    sd_ref = dict(sd)
    sd_ref.update(params)
    logits = om.res8_forward(sd_ref, x, True)
    loss = torch.nn.functional.cross_entropy(logits, labels)
    grads = torch.autograd.grad(loss, [params[n] for n in names])
    return sd_ref, logits.detach().numpy(), loss.item(), dict(zip(names, grads))


def res8_train_case(al, lib, big, B, T, C, M, api):
    """A training step: howl_res8_fwd + howl_xent_fwd_bwd + howl_res8_bwd (api "plain"), howl_res8_fwd_xent + howl_res8_bwd_xent
    ("xent") or howl_res8_fwd + howl_res8_bwd_part 1, 2 ("part").  The input is the (B, T, M) log-mel channel view."""
    if big:
        B, T, C = big
    rng = np.random.default_rng(B * 1000 + T + M)
    x4 = torch.from_numpy(rng.standard_normal((B, 3, M, T)).astype(np.float32))
    feat_h = np.ascontiguousarray(x4[:, 0].permute(0, 2, 1).numpy())
    feat = al.buf("feat", (B, T, M), np.float32, feat_h)
    sd = om.res8_init(C)
    r = Res8Bufs(al, lib, B, T, C, M, {k: v.clone() for k, v in sd.items()})
    lab_h = (np.arange(B) % C).astype(np.int64)
    labels = al.buf("labels", B, np.int64, lab_h)
    logits = al.buf("logits", (B, C), np.float32, "sentinel", promised="all")
    dl = al.buf("dlogits", (B, C), np.float32, "sentinel", promised="all")
    loss = al.buf("loss", 1, np.float32, "sentinel", promised="all")
    geo = (T * M, M, 1, B, T, M, C)
    if api == "xent":
        nll = al.buf("nll", B, np.float32, "sentinel", promised="all")
        lib.call("howl_res8_fwd_xent", ctypes.byref(r.prm), al.ptr(feat), *geo, ctypes.byref(r.saved), al.ptr(labels), al.ptr(logits),
                 al.ptr(nll), al.ptr(dl), al.ptr(r.ws), r.nws, None)
        lib.call("howl_res8_bwd_xent", ctypes.byref(r.prm), al.ptr(feat), *geo, ctypes.byref(r.saved), al.ptr(dl), al.ptr(nll),
                 al.ptr(loss), ctypes.byref(r.gr), al.ptr(r.ws), r.nws, 0, None, None)
    else:
        lib.call("howl_res8_fwd", ctypes.byref(r.prm), al.ptr(feat), *geo, 1, ctypes.byref(r.saved), al.ptr(logits), al.ptr(r.ws), r.nws,
                 None)
        lib.call("howl_xent_fwd_bwd", al.ptr(logits), al.ptr(labels), B, C, al.ptr(loss), al.ptr(dl), None)
        if api == "plain":
            lib.call("howl_res8_bwd", ctypes.byref(r.prm), al.ptr(feat), *geo, ctypes.byref(r.saved), al.ptr(dl), ctypes.byref(r.gr),
                     al.ptr(r.ws), r.nws, None)
        else:
            for part in (1, 2):
                lib.call("howl_res8_bwd_part", ctypes.byref(r.prm), al.ptr(feat), *geo, ctypes.byref(r.saved), al.ptr(dl), ctypes.byref(r.gr),
                         al.ptr(r.ws), r.nws, part, None)
    al.sync()
    sd_ref, ref_logits, ref_loss, gref = _res8_ref(sd, x4, torch.from_numpy(lab_h))
    # test_emu_res8's bounds on the emulator's small batches, test_gpu_res8's at the device's batches
    tol = dict(logits=2e-5, loss=1e-5, mean=1e-6, var=1e-6, grad=2e-5) if not big else \
        dict(logits=2e-5, loss=1e-4, mean=1e-5, var=1e-4, grad=5e-5)
    close(al.get(logits), ref_logits, tol["logits"], "logits")
    close(al.get(loss), [ref_loss], tol["loss"], "loss")
    for i in (1, 3, 6):
        close(al.get(r.p[f"bn{i}.running_mean"]), sd_ref[f"bn{i}.running_mean"].numpy(), tol["mean"], f"bn{i} mean")
        close(al.get(r.p[f"bn{i}.running_var"]), sd_ref[f"bn{i}.running_var"].numpy(), tol["var"], f"bn{i} var")
    if not big:
        for n, g in gref.items():
            close(al.get(r.g[n]), g.numpy(), tol["grad"] * max(1.0, float(g.abs().max())), "grad " + n)
        return
    # the device's batches: test_gpu_res8's comparison -- the oracle with the kernels' own ReLU decisions (a pre-activation within
    # rounding of zero may come out on either side; asserted to be the only difference) at 2e-5, and from 512 utterances on the
    # oracle's own decisions at 5e-5
    from types import SimpleNamespace
    from gpu_util import res8_oracle_with_kernel_relus
    saved = SimpleNamespace(mask0=torch.from_numpy(al.get(r.mask0).astype(np.int32)),
                            s=[torch.from_numpy(np.ascontiguousarray(al.get(si))) for si in r.s])
    kernel_model = SimpleNamespace(_buffers_cache={(B, T, M): saved})
    _, shared, flips, _ = res8_oracle_with_kernel_relus(kernel_model, x4, torch.from_numpy(lab_h), B, T, M, C)
    for n, g in shared.items():
        close(al.get(r.g[n]), g.numpy(), 2e-5 * max(1.0, float(g.abs().max())), f"grad {n} (shared ReLU decisions, {flips} flipped)")
    if B >= 512:
        for n, g in gref.items():
            close(al.get(r.g[n]), g.numpy(), tol["grad"] * max(1.0, float(g.abs().max())), "grad " + n)


for _B, _T, _C, _M, _api, _env, _big in [
        (3, 84, 12, 40, "plain", None, (512, 81, 12)), (1, 250, 4, 40, "plain", None, (3, 250, 4)),
        (1, 86, 4, 80, "xent", None, (33, 84, 12)), (3, 83, 12, 40, "part", None, (64, 81, 30)),
        (3, 82, 5, 40, "plain", {"HOWL_RES8_SLICES": "0", "HOWL_RES8_BWD_PAIR": "0", "HOWL_RES8_BWD_FUSED": "0"}, None),
        (1, 3, 4, 40, "xent", None, None)]:
    _name = f"res8_{_api}_B{_B}_T{_T}_M{_M}" + ("_switches_off" if _env else "")
    _eps = {"plain": ["howl_res8_fwd", "howl_res8_bwd", "howl_xent_fwd_bwd"], "xent": ["howl_res8_fwd_xent", "howl_res8_bwd_xent"],
            "part": ["howl_res8_fwd", "howl_res8_bwd_part", "howl_xent_fwd_bwd"]}[_api]
    register(_name, _eps, (lambda big_shape: (lambda al, lib, big, **kw: res8_train_case(al, lib, big_shape if big else None, **kw)))(_big),
             env=_env, B=_B, T=_T, C=_C, M=_M, api=_api, gpu=_big is not None)


def res8_eval_case(al, lib, big, B, T, C, M, long):
    if big:
        B, T = 3, 250
    rng = np.random.default_rng(B + T + M)
    x4 = torch.from_numpy(rng.standard_normal((B, 3, M, T)).astype(np.float32))
    sd = om.res8_init(C)
    for i in range(1, 7):
        sd[f"bn{i}.running_mean"] = 0.1 * torch.arange(45, dtype=torch.float32).sin()
        sd[f"bn{i}.running_var"] = 0.5 + 0.3 * torch.arange(45, dtype=torch.float32).cos() ** 2
    feat = al.buf("feat", (B, T, M), np.float32, np.ascontiguousarray(x4[:, 0].permute(0, 2, 1).numpy()))
    logits = al.buf("logits", (B, C), np.float32, "sentinel", promised="all")
    if long:
        p = {k: al.buf(k, v.shape, np.float32 if v.dtype == torch.float32 else np.int64, v.numpy()) for k, v in sd.items()}
        prm = HowlRes8Params()
        prm.conv0_w = al.ptr(p["conv0.weight"])
        for i in range(6):
            prm.conv_w[i] = al.ptr(p[f"conv{i+1}.weight"]).value
            prm.bn_running_mean[i] = al.ptr(p[f"bn{i+1}.running_mean"]).value
            prm.bn_running_var[i] = al.ptr(p[f"bn{i+1}.running_var"]).value
            prm.bn_num_batches[i] = al.ptr(p[f"bn{i+1}.num_batches_tracked"]).value
        prm.out_w, prm.out_b = al.ptr(p["output.weight"]), al.ptr(p["output.bias"])
        nws = int(lib.cdll.howl_res8_long_workspace_bytes_mels(B, T, M))
        ws = al.buf("workspace", nws, np.uint8, "sentinel")
        lib.call("howl_res8_fwd_long", ctypes.byref(prm), al.ptr(feat), T * M, M, 1, B, T, M, C, al.ptr(logits), al.ptr(ws), nws, None)
    else:
        r = Res8Bufs(al, lib, B, T, C, M, {k: v.clone() for k, v in sd.items()}, train=False)
        nws = int(lib.cdll.howl_res8_eval_workspace_bytes_mels(B, T, M))
        ws = al.buf("eval_workspace", nws, np.uint8, "sentinel")
        lib.call("howl_res8_fwd", ctypes.byref(r.prm), al.ptr(feat), T * M, M, 1, B, T, M, C, 0, ctypes.byref(r.saved), al.ptr(logits),
                 al.ptr(ws), nws, None)
    al.sync()
    ref = om.res8_forward(sd, x4, False).numpy()
    close(al.get(logits), ref, 2e-5, "logits")


register("res8_eval_B3_T3_M40", ["howl_res8_fwd"], res8_eval_case, B=3, T=3, C=4, M=40, long=False, gpu=False)
register("res8_eval_B1_T250_M80", ["howl_res8_fwd"], res8_eval_case, B=1, T=250, C=4, M=80, long=False)
register("res8_fwd_long_B1_T120_M40", ["howl_res8_fwd_long"], res8_eval_case, B=1, T=120, C=4, M=40, long=True)
register("res8_fwd_long_B3_T164_M80", ["howl_res8_fwd_long"], res8_eval_case, B=3, T=164, C=4, M=80, long=True, gpu=False)


# ---- the optimiser step folded into a backward call (FusedTrainer's flat parameter / gradient buffers) ----------------------

def _adamw_ref(p, g, m, v, step, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2):
    """torch.optim.AdamW's step in float64 on the kernel's own gradient, with the hyper-parameters the C ABI passes (float32:
    1 - beta2 is then 1.3e-5 away from 0.001, which shows in v once gradients reach O(100))."""
    lr, b1, b2, eps, wd = (float(np.float32(h)) for h in (lr, b1, b2, eps, wd))
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr * (m / (1.0 - b1 ** step)) / (np.sqrt(v / (1.0 - b2 ** step)) + eps)
    return p, m, v


def _flat_views(al, flat, sizes):
    """Pointers into a flat buffer, one per tensor (the layout FusedTrainer keeps its parameters and gradients in)."""
    base, out, off = al.ptr(flat).value, [], 0
    for n in sizes:
        out.append(ctypes.c_void_p(base + 4 * off))
        off += n
    return out


def res8_adamw_case(al, lib, big, B, T, C, M):
    """howl_res8_fwd_xent + howl_res8_bwd_xent with a HowlAdamW on flat parameter / gradient / moment buffers: the step rides in
    the gradient fold (or, HOWL_NO_FOLD_ADAMW, runs as its own launch).  Gradients against the oracle, parameters and moments
    against AdamW in float64 on the kernel's gradients."""
    if big:
        B, T, C = 64, 81, 12
    rng = np.random.default_rng(B * 100 + T)
    names = om.res8_param_names()
    sd = om.res8_init(C)
    sizes = [sd[n].numel() for n in names]
    n = int(sum(sizes))
    p0 = np.concatenate([sd[k].numpy().reshape(-1) for k in names]).astype(np.float32)
    m0 = (0.01 * rng.standard_normal(n)).astype(np.float32)
    v0 = (1e-4 * (0.5 + np.abs(rng.standard_normal(n)))).astype(np.float32)
    pf = al.buf("flat.p", n, np.float32, p0)
    gf = al.buf("flat.g", n, np.float32, "sentinel", promised="all")
    mf = al.buf("flat.m", n, np.float32, m0)
    vf = al.buf("flat.v", n, np.float32, v0)
    pv, gv = _flat_views(al, pf, sizes), _flat_views(al, gf, sizes)
    bn = {k: al.buf(k, v.shape, np.float32 if v.dtype == torch.float32 else np.int64, v.numpy()) for k, v in sd.items()
          if k.startswith("bn")}
    prm = HowlRes8Params()
    prm.conv0_w = pv[0]
    for i in range(6):
        prm.conv_w[i] = pv[1 + i].value
        prm.bn_running_mean[i] = al.ptr(bn[f"bn{i+1}.running_mean"]).value
        prm.bn_running_var[i] = al.ptr(bn[f"bn{i+1}.running_var"]).value
        prm.bn_num_batches[i] = al.ptr(bn[f"bn{i+1}.num_batches_tracked"]).value
    prm.out_w, prm.out_b = pv[7], pv[8]
    gr = HowlRes8Grads()
    gr.conv0_w = gv[0]
    for i in range(6):
        gr.conv_w[i] = gv[1 + i].value
    gr.out_w, gr.out_b = gv[7], gv[8]
    r = Res8Bufs(al, lib, B, T, C, M, {k: v.clone() for k, v in sd.items()}, train=False)   # (its saved buffers and workspace)
    x4 = torch.from_numpy(rng.standard_normal((B, 3, M, T)).astype(np.float32))
    feat = al.buf("feat", (B, T, M), np.float32, np.ascontiguousarray(x4[:, 0].permute(0, 2, 1).numpy()))
    lab_h = (np.arange(B) % C).astype(np.int64)
    labels = al.buf("labels", B, np.int64, lab_h)
    logits = al.buf("logits", (B, C), np.float32, "sentinel", promised="all")
    nll = al.buf("nll", B, np.float32, "sentinel", promised="all")
    dl = al.buf("dlogits", (B, C), np.float32, "sentinel", promised="all")
    loss = al.buf("loss", 1, np.float32, "sentinel", promised="all")
    geo = (T * M, M, 1, B, T, M, C)
    opt = HowlAdamW(al.ptr(pf), al.ptr(gf), al.ptr(mf), al.ptr(vf), n, 0.01, 0.9, 0.999, 1e-8, 1e-2, 3, 1.0)
    lib.call("howl_res8_fwd_xent", ctypes.byref(prm), al.ptr(feat), *geo, ctypes.byref(r.saved), al.ptr(labels), al.ptr(logits),
             al.ptr(nll), al.ptr(dl), al.ptr(r.ws), r.nws, None)
    lib.call("howl_res8_bwd_xent", ctypes.byref(prm), al.ptr(feat), *geo, ctypes.byref(r.saved), al.ptr(dl), al.ptr(nll), al.ptr(loss),
             ctypes.byref(gr), al.ptr(r.ws), r.nws, 0, ctypes.byref(opt), None)
    al.sync()
    _, ref_logits, ref_loss, gref = _res8_ref(sd, x4, torch.from_numpy(lab_h))
    close(al.get(logits), ref_logits, 2e-5, "logits")
    g = al.get(gf).copy()
    off = 0
    tol = 2e-5
    if big:      # 64 utterances: test_gpu_res8's comparison, the oracle with the kernels' own ReLU decisions
        from types import SimpleNamespace
        from gpu_util import res8_oracle_with_kernel_relus
        saved = SimpleNamespace(mask0=torch.from_numpy(al.get(r.mask0).astype(np.int32)),
                                s=[torch.from_numpy(np.ascontiguousarray(al.get(si))) for si in r.s])
        _, gref, _, _ = res8_oracle_with_kernel_relus(SimpleNamespace(_buffers_cache={(B, T, M): saved}), x4,
                                                      torch.from_numpy(lab_h), B, T, M, C)
    for name, k in zip(names, sizes):
        ref = gref[name].numpy().reshape(-1)
        close(g[off:off + k], ref, tol * max(1.0, float(np.abs(ref).max())), "grad " + name)
        off += k
    p1, m1, v1 = _adamw_ref(p0, g, m0, v0, 3)
    close(al.get(pf), p1, 2e-6, "p after the step")
    close(al.get(mf), m1, 1e-6 * max(1.0, np.abs(m1).max()), "m after the step")
    close(al.get(vf), v1, 1e-6 * max(1.0, np.abs(v1).max()), "v after the step")


for _fold in ("fold", "own_launch"):
    register(f"res8_bwd_xent_adamw_{_fold}", ["howl_res8_fwd_xent", "howl_res8_bwd_xent"], res8_adamw_case,
             env={} if _fold == "fold" else {"HOWL_NO_FOLD_ADAMW": "1"}, B=3, T=82, C=5, M=40)


# ---- the sequence model's other launches: howl_lstm_fwd_next, howl_seq_lstm_bwd ----------------------------------------------

def _lstm_operands(al, B, T, M, sd, tag=""):
    keys = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    pb = {k: al.buf("lstm." + k + tag, sd["lstm." + k].shape, np.float32, sd["lstm." + k].numpy()) for k in keys}
    return keys, pb, HowlLstmParams(*[al.ptr(pb[k]) for k in keys])


def lstm_fwd_next_case(al, lib, big, B, T, Bn, L, layout):
    """howl_lstm_fwd_next: the forward recurrence with the NEXT batch's log-mel frontend riding in its launch (or, with
    HOWL_LSTM_RIDE_LOGMEL=0, as its own launch behind it).  Recurrence against the oracle, features against float64."""
    if big:
        B, T, Bn, L = 512, 38, 512, 8000
    M = 40
    rng = np.random.default_rng(B + T + L)
    sd = om.lstm_init(5)
    keys, pb, prm = _lstm_operands(al, B, T, M, sd)
    xs = rng.standard_normal((B, T, M)).astype(np.float32)
    x = al.buf("x", (B, T, M), np.float32, xs)
    ln = np.sort(rng.integers(1, T + 1, B))[::-1].astype(np.int64)
    ln[0] = T
    lnb = al.buf("lengths", B, np.int64, ln)
    gates = al.buf("gates", (B, T, 512), np.float32, "sentinel")
    cc = al.buf("c", (B, T, 128), np.float32, "sentinel")
    hseq = al.buf("hseq", (B, T + 1, 128), np.float32, "sentinel", promised=lambda a: np.arange(T + 1)[None, :, None] >= 1)
    sv = HowlLstmSaved(None, al.ptr(gates), al.ptr(cc), al.ptr(hseq), None, T, 0)
    hT = al.buf("hT", (B, 128), np.float32, "sentinel", promised="all")
    cT = al.buf("cT", (B, 128), np.float32, "sentinel", promised="all")
    nws = int(lib.cdll.howl_lstm_workspace_bytes(B, T))
    ws = al.buf("workspace", nws, np.uint8, "sentinel")
    flat = (0.3 * rng.standard_normal(Bn * L)).astype(np.float32)
    pcm = al.buf("next.pcm", Bn * L, np.float32, flat)
    fb = fe.mel_fb(40).numpy()
    fbp = _pack(al, lib, fb, "next.fbp")
    zm = al.buf("next.zmuv", 2, np.float32, np.array([-3.0, 2.5], np.float32))
    Tn = 1 + L // 200
    feats = al.buf("next.out", (Bn, Tn, 40) if layout else (Bn, 40, Tn), np.float32, "sentinel", promised="all")
    nxt = HowlLogmelArgs(al.ptr(pcm), Bn, L, L, al.ptr(fbp), 40, 1e-7, al.ptr(zm), al.ptr(feats), layout)
    lib.call("howl_lstm_fwd_next", ctypes.byref(prm), al.ptr(x), B, T, M, al.ptr(lnb), None, None, ctypes.byref(sv), al.ptr(hT),
             al.ptr(cT), al.ptr(ws), nws, ctypes.byref(nxt), None)
    al.sync()
    p = {k: v.clone().double() for k, v in sd.items() if k.startswith("lstm.")}
    seq, (h_ref, c_ref) = om._lstm_cell_seq(p, torch.from_numpy(xs).double().permute(1, 0, 2).contiguous(), torch.from_numpy(ln), None)
    otol = 2e-6 if not big else 2e-5
    hs = al.get(hseq)[:, 1:]
    live = np.arange(T)[None, :] < ln[:, None]
    close(hs[live], seq.permute(1, 0, 2).numpy()[live], otol, "hseq")
    close(al.get(hT), h_ref[0].numpy(), otol, "hT")
    close(al.get(cT), c_ref[0].numpy(), otol, "cT")
    pick = list(range(Bn)) if not big else [0, 1, Bn // 2, Bn - 1]
    rows = torch.from_numpy(flat.reshape(Bn, L)[pick]).double()
    ref = (torch.log(torch.matmul(fe.power_spectrogram(rows).transpose(-1, -2), torch.from_numpy(fb).double()) + 1e-7) + 3.0) / 2.5
    ref = ref.numpy() if layout else ref.transpose(-1, -2).numpy()
    close(al.get(feats)[pick], ref, 1e-4, "next batch's log-mels")
    assert np.isfinite(al.get(feats)).all()


for _ride in ("1", "0"):
    for _layout in (0, 1):
        register(f"lstm_fwd_next_ride{_ride}_layout{_layout}", ["howl_lstm_fwd_next", "howl_fb_pack"], lstm_fwd_next_case,
                 env={"HOWL_LSTM_RIDE_LOGMEL": _ride}, B=5, T=4, Bn=3, L=401, layout=_layout, gpu=_layout == 1)


def seq_lstm_bwd_case(al, lib, big, B, T, adamw):
    """howl_seq_lstm_bwd after howl_lstm_fwd + howl_head_fwd: the head's backward and the LSTM's BPTT in one call.  adamw: the
    eight gradients are views of one flat buffer and the optimiser step rides in the call (HOWL_NO_FOLD_ADAMW: behind it).
    Gradients against a float64 head + LSTM backward, the step against AdamW in float64 on the kernel's gradients."""
    if big:
        B, T = 513, 38
    M, C = 40, 5
    rng = np.random.default_rng(B * 10 + T)
    sd = om.lstm_init(C)
    names = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "dnn.0.weight", "dnn.0.bias",
             "dnn.2.weight", "dnn.2.bias"]
    sizes = [sd[k].numel() for k in names]
    n = int(sum(sizes))
    keys, pb, prm = _lstm_operands(al, B, T, M, sd)
    hd = {k: al.buf(k, sd[k].shape, np.float32, sd[k].numpy()) for k in names[4:]}
    hp = HowlHeadParams(*[al.ptr(hd[k]) for k in names[4:]])
    xs = rng.standard_normal((B, T, M)).astype(np.float32)
    x = al.buf("x", (B, T, M), np.float32, xs)
    ln = np.full(B, T, np.int64)
    lnb = al.buf("lengths", B, np.int64, ln)
    gx = al.buf("gx", (B, T, 512), np.float32, "sentinel")
    gates = al.buf("gates", (B, T, 512), np.float32, "sentinel")
    cc = al.buf("c", (B, T, 128), np.float32, "sentinel")
    hseq = al.buf("hseq", (B, T + 1, 128), np.float32, "sentinel")
    dg = al.buf("dgates", (B, T, 512), np.float32, "sentinel")
    sv = HowlLstmSaved(al.ptr(gx), al.ptr(gates), al.ptr(cc), al.ptr(hseq), al.ptr(dg), T, 0)
    hT = al.buf("hT", (B, 128), np.float32, "sentinel")
    cT = al.buf("cT", (B, 128), np.float32, "sentinel")
    nws = int(lib.cdll.howl_lstm_workspace_bytes(B, T))
    ws = al.buf("workspace", nws, np.uint8, "sentinel")
    lib.call("howl_lstm_fwd", ctypes.byref(prm), al.ptr(x), B, T, M, al.ptr(lnb), None, None, ctypes.byref(sv), al.ptr(hT), al.ptr(cT),
             al.ptr(ws), nws, None)
    h1 = ctypes.c_void_p(al.ptr(hseq).value + 128 * 4)          # rows (b, t) = hseq[b][t + 1]
    y1 = al.buf("y1", (B * T, 256), np.float32, "sentinel", promised="all")
    y2 = al.buf("y2", (B * T, C), np.float32, "sentinel", promised="all")
    lib.call("howl_head_fwd", ctypes.byref(hp), h1, T, (T + 1) * 128, 128, B * T, 128, 256, C, al.ptr(y1), al.ptr(y2), None)
    dys = rng.standard_normal((B * T, C)).astype(np.float32)
    dy2 = al.buf("dy2", (B * T, C), np.float32, dys)
    dz1 = al.buf("dz1", (B * T, 256), np.float32, "sentinel", promised="all")
    dhs = al.buf("dhs", (B, T, 128), np.float32, "sentinel", promised="all")
    hws_n = int(lib.cdll.howl_head_workspace_bytes(128, 256, C))
    head_ws = al.buf("head_ws", hws_n, np.uint8, "sentinel")
    if adamw:
        p0 = np.concatenate([sd[k].numpy().reshape(-1) for k in names]).astype(np.float32)
        m0 = (0.01 * rng.standard_normal(n)).astype(np.float32)
        v0 = (1e-4 * (0.5 + np.abs(rng.standard_normal(n)))).astype(np.float32)
        pf = al.buf("flat.p", n, np.float32, p0)
        gf = al.buf("flat.g", n, np.float32, "sentinel", promised="all")
        mf, vf = al.buf("flat.m", n, np.float32, m0), al.buf("flat.v", n, np.float32, v0)
        gv = _flat_views(al, gf, sizes)
        opt = HowlAdamW(al.ptr(pf), al.ptr(gf), al.ptr(mf), al.ptr(vf), n, 0.01, 0.9, 0.999, 1e-8, 1e-2, 3, 1.0)
    else:
        gb = [al.buf("grad." + k, sd[k].shape, np.float32, "sentinel", promised="all") for k in names]
        gv = [al.ptr(b_) for b_ in gb]
        opt = None
    lgs, hgs = HowlLstmGrads(*gv[:4]), HowlHeadGrads(*gv[4:])
    lib.call("howl_seq_lstm_bwd", ctypes.byref(hp), 256, C, al.ptr(y1), al.ptr(dy2), al.ptr(dz1), al.ptr(dhs), ctypes.byref(hgs), None,
             al.ptr(head_ws), hws_n, ctypes.byref(prm), al.ptr(x), B, T, M, al.ptr(lnb), None, ctypes.byref(sv), ctypes.byref(lgs),
             al.ptr(ws), nws, ctypes.byref(opt) if opt is not None else None, None)
    al.sync()
    # float64 reference: head on the LSTM's outputs, loss = sum(y2 * dy2); the head's ReLU takes the kernel's own y1 decisions
    p = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
    seq, _ = om._lstm_cell_seq(p, torch.from_numpy(xs).double().permute(1, 0, 2).contiguous(), torch.from_numpy(ln), None)
    hrows = seq.permute(1, 0, 2).reshape(B * T, 128)
    mask = torch.from_numpy(al.get(y1) > 0)
    yh = (hrows @ p["dnn.0.weight"].T + p["dnn.0.bias"]) * mask
    out = yh @ p["dnn.2.weight"].T + p["dnn.2.bias"]
    (out * torch.from_numpy(dys).double()).sum().backward()
    tol = 2e-5 if not big else 5e-5
    g = np.concatenate([al.get(gf).reshape(-1)]) if adamw else np.concatenate([al.get(b_).reshape(-1) for b_ in gb])
    off = 0
    for name, k in zip(names, sizes):
        ref = p[name].grad.numpy().reshape(-1)
        close(g[off:off + k], ref, tol * max(1.0, float(np.abs(ref).max())), "grad " + name)
        off += k
    if adamw:
        p1, m1, v1 = _adamw_ref(p0, g, m0, v0, 3)
        close(al.get(pf), p1, 2e-6, "p after the step")
        close(al.get(mf), m1, 1e-6 * max(1.0, np.abs(m1).max()), "m after the step")
        close(al.get(vf), v1, 1e-6 * max(1.0, np.abs(v1).max()), "v after the step")


for _opt, _env in (("", {}), ("_adamw_fold", {"HOWL_WGRAD_BIG_MIN_ROWS": "1", "HOWL_ROWGEMM_MIN_ROWS": "1"}),
                   ("_adamw_own_launch", {"HOWL_NO_FOLD_ADAMW": "1"})):
    for _ride in ("1", "0"):
        register(f"seq_lstm_bwd{_opt}_ride{_ride}", ["howl_seq_lstm_bwd", "howl_lstm_fwd", "howl_head_fwd"], seq_lstm_bwd_case,
                 env=dict(_env, HOWL_LSTM_RIDE=_ride), B=9, T=5, adamw=bool(_opt), gpu=_ride == "1")


# ---- MobileNetClassifier ---------------------------------------------------------------------------------------------------

def mobilenet_case(al, lib, big, B, T, dropout):
    """howl_mobilenet_fwd (training, then eval) + howl_mobilenet_bwd: parameters, BatchNorm buffers, gradients and the dropout mask
    each one flat buffer (the entry points' own layout), the workspace at exactly howl_mobilenet_workspace_bytes.  test_emu_mobilenet's
    comparisons."""
    from mb_util import check_grads, oracle_step
    from oracle import mobilenet as omb
    if big:
        B, T = 96, 101
    C, M = 5, 40
    torch.manual_seed(B * 100 + T)
    x = torch.randn(B, 3, M, T) * 1.5
    labels = torch.arange(B) % C
    keep = (torch.rand(B, omb.LAST_CHANNEL) >= 0.2).float() if dropout else None
    sd = omb.mobilenet_init(C)
    names = omb.mobilenet_param_names()
    flat_h = np.concatenate([sd[k].numpy().reshape(-1) for k in names]).astype(np.float32)
    assert flat_h.size == lib.cdll.howl_mobilenet_param_floats(C)
    bufs_h = np.concatenate([np.concatenate([sd[l["bn"] + ".running_mean"].numpy(), sd[l["bn"] + ".running_var"].numpy()])
                             for l in omb.layer_table()]).astype(np.float32)
    assert bufs_h.size == lib.cdll.howl_mobilenet_buffer_floats()
    flat = al.buf("params", flat_h.size, np.float32, flat_h)
    bufs = al.buf("bn_buffers", bufs_h.size, np.float32, bufs_h)
    xb = al.buf("x", (B, 3, M, T), np.float32, np.ascontiguousarray(x.numpy()))
    mask = al.buf("drop_mask", (B, omb.LAST_CHANNEL), np.float32, keep.numpy()) if dropout else None
    scale = 1.0 / (1.0 - omb.DROPOUT_P) if dropout else 1.0
    nws = int(lib.cdll.howl_mobilenet_workspace_bytes(B, M, T, C))
    ws = al.buf("workspace", nws, np.uint8, "sentinel")
    logits = al.buf("logits", (B, C), np.float32, "sentinel", promised="all")
    sb, sm, st = 3 * M * T, T, 1
    lib.call("howl_mobilenet_fwd", al.ptr(flat), al.ptr(bufs), C, al.ptr(xb), sb, sm, st, B, M, T, 1, al.ptr(mask), scale, al.ptr(logits),
             al.ptr(ws), nws, None)
    al.sync()
    ref, grads, osd = oracle_step(sd, x, labels, keep)
    close(al.get(logits), ref.numpy(), 5e-4, "logits")
    osd_bufs = np.concatenate([np.concatenate([osd[l["bn"] + ".running_mean"].numpy(), osd[l["bn"] + ".running_var"].numpy()])
                               for l in omb.layer_table()])
    np.testing.assert_allclose(al.get(bufs), osd_bufs, rtol=1e-4, atol=1e-5)
    pr = torch.softmax(ref, 1)
    pr[torch.arange(B), labels] -= 1
    dl = al.buf("dlogits", (B, C), np.float32, (pr / B).numpy().astype(np.float32))
    g = al.buf("grads", flat_h.size, np.float32, "sentinel", promised="all")
    lib.call("howl_mobilenet_bwd", al.ptr(flat), C, al.ptr(xb), sb, sm, st, B, M, T, al.ptr(mask), scale, al.ptr(dl), al.ptr(g),
             al.ptr(ws), nws, None)
    al.sync()
    gh = al.get(g).copy()
    assert np.isfinite(gh).all()
    views, off = [], 0
    for gr_ in grads:
        views.append(gh[off:off + gr_.numel()].reshape(gr_.shape))
        off += gr_.numel()
    assert off == gh.size
    check_grads(views, sd, x, labels, keep, grads)
    elog = al.buf("eval_logits", (B, C), np.float32, "sentinel", promised="all")
    lib.call("howl_mobilenet_fwd", al.ptr(flat), al.ptr(bufs), C, al.ptr(xb), sb, sm, st, B, M, T, 0, None, 1.0, al.ptr(elog), al.ptr(ws),
             nws, None)
    al.sync()
    esd = {k: v.clone() for k, v in sd.items()}
    bh, off = al.get(bufs).copy(), 0
    for l in omb.layer_table():
        for nm in (".running_mean", ".running_var"):
            k = esd[l["bn"] + nm].numel()
            esd[l["bn"] + nm] = torch.from_numpy(bh[off:off + k].copy())
            off += k
    close(al.get(elog), omb.mobilenet_forward(esd, x, False).numpy(), 5e-5, "eval logits")


register("mobilenet_B5_T31_dropout", ["howl_mobilenet_fwd", "howl_mobilenet_bwd"], mobilenet_case, B=5, T=31, dropout=True)
register("mobilenet_B3_T29", ["howl_mobilenet_fwd", "howl_mobilenet_bwd"], mobilenet_case, B=3, T=29, dropout=False, gpu=False)
