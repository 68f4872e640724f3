"""Yardstick and runners of the gru tests (tests/test_emu_gru.py on the hipemu emulator, tests/test_gpu_gru.py on the device).

``RefGru`` restates the model of include/howl_hip_gru.h on torch CPU modules -- conv encoder with BatchNorm, packed GRU(40 -> 96),
Linear - ReLU - mask - Linear -- with the reference's module names, so a ``state_dict`` loads into it unchanged.  ``reference()``
runs it in float64 (the yardstick) or float32 (the noise of the same model in the kernels' precision) with an explicit keep mask
and returns logits, loss, every parameter gradient and the updated running statistics.  ``run_library()`` drives the C ABI of any
build on the buffers of an allocator with tests/guard_mem.py's interface (``Plain`` or ``Arena`` host memory for the emulator,
``Banded`` on the device).
"""
import ctypes
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence

GOLDEN = Path(__file__).resolve().parent / "golden" / "g16_gru.npz"
PARAMS = ["conv_encoder.0.weight", "conv_encoder.0.bias", "conv_encoder.1.weight", "conv_encoder.1.bias", "conv_encoder.4.weight",
          "conv_encoder.4.bias", "conv_encoder.6.weight", "conv_encoder.6.bias", "lstm_encoder.weight_ih_l0", "lstm_encoder.weight_hh_l0",
          "lstm_encoder.bias_ih_l0", "lstm_encoder.bias_hh_l0", "dnn.0.weight", "dnn.0.bias", "dnn.3.weight", "dnn.3.bias"]
BUFFERS = ["conv_encoder.1.running_mean", "conv_encoder.1.running_var", "conv_encoder.1.num_batches_tracked",
           "conv_encoder.6.running_mean", "conv_encoder.6.running_var", "conv_encoder.6.num_batches_tracked"]
KEEP = 0.8
# name -> (B, T, labels, lengths or None, seed): odd and even T + 4, B no multiple of four, a one-frame utterance, ragged stops
# inside a workgroup's four, the smallest problem, and the 1 s window (52 steps, three workgroups with a one-sequence tail)
CASES = {"A": (5, 21, 4, [21, 17, 9, 3, 1], 11), "B": (4, 22, 4, None, 12), "one": (1, 1, 4, None, 13), "window": (9, 101, 12, [101] * 9, 14)}


class RefGru(nn.Module):
    def __init__(self, num_labels):
        super().__init__()
        self.conv_encoder = nn.Sequential(nn.Conv2d(1, 8, 3, padding=(1, 3)), nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d((1, 2)),
                                          nn.Conv2d(8, 1, 3, padding=1), nn.ReLU(), nn.BatchNorm2d(1))
        self.lstm_encoder = nn.GRU(40, 96)
        self.dnn = nn.Sequential(nn.Linear(96, 192), nn.ReLU(), nn.Dropout(0.2), nn.Linear(192, num_labels))

    def forward(self, x, lengths, keep_mask=None):
        """x (B, C, 40, T); lengths: frame counts or None; keep_mask (B, 192) of 0/1 or None (no dropout)."""
        B, T = x.size(0), x.size(-1)
        frames = torch.full((B,), T, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths, dtype=torch.int64)
        steps = (frames + 4) // 2
        seq = self.conv_encoder(x[:, :1]).squeeze(1).permute(2, 0, 1).contiguous()       # (T1, B, 40)
        _, h = self.lstm_encoder(pack_padded_sequence(seq, steps))
        y1 = self.dnn[1](self.dnn[0](h[0]))
        if keep_mask is not None:
            y1 = y1 * keep_mask.to(y1.dtype) * (1.0 / KEEP)
        return self.dnn[3](y1)


def make_state(num_labels, seed):
    """A seeded float32 state with every BatchNorm tensor away from its initial value."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in RefGru(num_labels).state_dict().items()}
    for i, n in ((1, 8), (6, 1)):
        sd[f"conv_encoder.{i}.weight"] = 0.5 + torch.rand(n, generator=g)
        sd[f"conv_encoder.{i}.bias"] = 0.6 * torch.rand(n, generator=g) - 0.3
        sd[f"conv_encoder.{i}.running_mean"] = 0.4 * torch.rand(n, generator=g) - 0.2
        sd[f"conv_encoder.{i}.running_var"] = 0.5 + torch.rand(n, generator=g)
        sd[f"conv_encoder.{i}.num_batches_tracked"] = torch.tensor(3)
    return sd


def make_case(name):
    """-> (state, x (B,3,40,T) float32, lengths list or None, labels, keep mask (B,192))."""
    B, T, C, lengths, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, 40, T, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    mask = (torch.rand(B, 192, generator=g) < KEEP).float()
    return make_state(C, seed), x, lengths, labels, mask


def reference(state, x, lengths, labels=None, mask=None, train=False, dtype=torch.float64):
    """-> dict(logits, loss, grads {name: tensor}, buffers {name: tensor}) of the restated model in ``dtype`` on the CPU."""
    C = state["dnn.3.bias"].numel()
    m = RefGru(C).to(dtype)
    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()})
    m.train(train)
    logits = m(x.to(dtype), lengths, mask if train else None)
    out = {"logits": logits.detach(), "loss": None, "grads": None}
    if labels is not None:
        loss = F.cross_entropy(logits, labels)
        out["loss"] = loss.detach()
        if train:
            loss.backward()
            named = dict(m.named_parameters())
            out["grads"] = {k: named[k].grad.detach() for k in PARAMS}
    out["buffers"] = {k: v.detach().clone() for k, v in m.state_dict().items() if k in BUFFERS}
    return out


_REF = {}


def case_reference(name):
    """fp64 and fp32 results of a case in training mode, the fp64 eval logits, and the cross-entropy's d loss / d logits at the
    fp64 logits (what the library's backward is fed) -- computed once per process and shared."""
    if name not in _REF:
        state, x, lengths, labels, mask = make_case(name)
        r64 = reference(state, x, lengths, labels, mask, train=True)
        r32 = reference(state, x, lengths, labels, mask, train=True, dtype=torch.float32)
        e64 = reference(state, x, lengths, labels)
        e32 = reference(state, x, lengths, labels, dtype=torch.float32)
        z = r64["logits"].clone().requires_grad_(True)
        F.cross_entropy(z, labels).backward()
        _REF[name] = dict(state=state, x=x, lengths=lengths, labels=labels, mask=mask, train64=r64, train32=r32, eval64=e64, eval32=e32,
                          dlogits=z.grad.float())
    return _REF[name]


def maxerr(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def check_logits(name, got, ref, what):
    err = maxerr(got, ref["logits"])
    print(f"gru {name} {what}: |dlogits| = {err:.3e}")
    assert err < 5e-5, (name, what, err)              # tests/test_gpu_lstm.py's bound on golden logits


def check_loss(name, got_logits, labels, ref):
    loss = float(F.cross_entropy(torch.as_tensor(got_logits).float(), labels))
    err = abs(loss - float(ref["loss"]))
    print(f"gru {name}: loss {loss:.6f}, |dloss| = {err:.3e}")
    assert err < 1e-4 * max(1.0, abs(float(ref["loss"]))), (name, err)


def check_grads(name, grads, r64, r32):
    """tests/test_gpu_lstm.py's noise idiom: maxerr(g, g64) < 4 noise + 2e-5 max(1, |g64|max), noise = the fp32 CPU model's error."""
    bad = []
    for k, g in zip(PARAMS, grads):
        g64 = r64["grads"][k]
        noise = maxerr(r32["grads"][k], g64)
        bound = 4 * noise + 2e-5 * max(1.0, float(g64.abs().max()))
        err = maxerr(torch.as_tensor(g).reshape(g64.shape), g64)
        print(f"gru {name} grad {k}: err {err:.3e}  noise {noise:.3e}  bound {bound:.3e}  |g|max {float(g64.abs().max()):.3e}")
        if not err < bound:
            bad.append((k, err, bound))
    assert not bad, (name, bad)


def check_buffers(name, got, ref):
    for k in BUFFERS:
        a, b = torch.as_tensor(got[k]), ref["buffers"][k]
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b), (name, k, int(a), int(b))
        else:
            err = maxerr(a.reshape(b.shape), b)
            print(f"gru {name} {k}: err {err:.3e}")
            assert err < 2e-6 * max(1.0, float(b.abs().max())), (name, k, err)      # a few fp32 roundings of O(1) numbers


# ---- the C ABI on any build ---------------------------------------------------------------------------------------------------------

class Plain:
    """Ordinary host memory with the allocator interface of tests/guard_mem.py (``Arena`` on the host, ``Banded`` on the device)."""

    def buf(self, name, shape, dtype=np.float32, fill=0.0, placement=None, promised=None):
        a = np.zeros(shape, dtype=dtype)
        if isinstance(fill, str):
            a.reshape(-1).view(np.uint8)[:] = 0xFF          # NaN in every float
        else:
            a[...] = fill.reshape(a.shape) if isinstance(fill, np.ndarray) else fill
        return a

    ptr = staticmethod(lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data))
    get = staticmethod(lambda a: a)


def run_library(lib, al, state, x, lengths, training, mask=None, dlogits=None, x_time_major=False, stream=None):
    """howl_gru_fwd (and howl_gru_bwd when ``dlogits`` is given) on the buffers of allocator ``al`` -> dict(logits, grads list in
    PARAMS order, buffers).  The features are handed over as channel 0 of the (B, 3, 40, T) tensor in place (strides), or
    time-major (B, T, 40) as the fused frontend leaves them.  The workspace is exactly howl_gru_workspace_bytes long and starts out
    as NaN, like every output: whatever a kernel reads, an earlier launch of the call has written."""
    from howl_amd import lib as L
    B, _, M, T = x.shape
    C = state["dnn.3.bias"].numel()

    def put(t, tag):
        a = np.ascontiguousarray(torch.as_tensor(t).numpy())
        return al.buf(tag, a.shape if a.ndim else (1,), a.dtype, fill=a)

    def get(v):
        return torch.from_numpy(np.array(al.get(v)))
    if x_time_major:
        xd = put(x[:, 0].permute(0, 2, 1).contiguous(), "x")
        sb, sm, st = T * M, 1, M
    else:
        xd = put(x, "x")
        sb, sm, st = 3 * M * T, T, 1
    ps = [put(state[k], k) for k in PARAMS]
    bs = [put(state[k], k) for k in BUFFERS]
    ld = None if lengths is None else put(torch.as_tensor(lengths, dtype=torch.int64), "lengths")
    md = None if mask is None else put(mask, "mask")
    n = lib.cdll.howl_gru_workspace_bytes(B, T)
    ws = al.buf("workspace", n // 4, np.float32, fill="sentinel")
    logits = al.buf("logits", (B, C), np.float32, fill="sentinel", promised="all")
    prm = L.HowlGruParams(*[al.ptr(p) for p in ps])
    buf = L.HowlGruBuffers(*[al.ptr(b) for b in bs])
    scale = 1.0 / KEEP if mask is not None else 1.0
    lib.call("howl_gru_fwd", ctypes.byref(prm), ctypes.byref(buf), al.ptr(xd), sb, sm, st, B, M, T, C, al.ptr(ld), int(training), al.ptr(md),
             scale, al.ptr(logits), al.ptr(ws), n, stream)
    out = {"logits": get(logits), "grads": None}
    if dlogits is not None:
        dl = put(dlogits, "dlogits")
        gs = [al.buf("grad " + k, tuple(state[k].shape), np.float32, fill="sentinel", promised="all") for k in PARAMS]
        gr = L.HowlGruGrads(*[al.ptr(g) for g in gs])
        lib.call("howl_gru_bwd", ctypes.byref(prm), al.ptr(xd), sb, sm, st, B, M, T, C, al.ptr(ld), scale, al.ptr(dl), ctypes.byref(gr),
                 al.ptr(ws), n, stream)
        out["grads"] = [get(g) for g in gs]
    out["buffers"] = {k: get(b).reshape(state[k].shape) for k, b in zip(BUFFERS, bs)}
    out["params"] = {k: get(p) for k, p in zip(PARAMS, ps)}
    return out


def check_refusals(lib, al, stream=None):
    """Every refusal of include/howl_hip_gru.h on a (B=2, T=6, 4 labels) problem: the code, a message that names the entry point and
    the reason, nothing launched (logits, gradients, workspace and BatchNorm buffers keep their bytes) -- and the next valid call
    succeeds, so no refusal leaves an error pending."""
    from howl_amd import lib as L
    B, T, C, M = 2, 6, 4, 40
    state = make_state(C, 5)
    g = torch.Generator().manual_seed(5)

    def put(t, tag):
        a = np.ascontiguousarray(torch.as_tensor(t).numpy())
        return al.buf(tag, a.shape if a.ndim else (1,), a.dtype, fill=a)
    x = put(torch.randn(B, 1, M, T, generator=g), "x")
    ps = [put(state[k], k) for k in PARAMS]
    bs = [put(state[k], k) for k in BUFFERS]
    dl = put(torch.randn(B, C, generator=g), "dlogits")
    n = lib.cdll.howl_gru_workspace_bytes(B, T)
    ws = al.buf("workspace", n // 4, np.float32, fill="sentinel")
    logits = al.buf("logits", (B, C), np.float32, fill="sentinel")
    gs = [al.buf("grad " + k, tuple(state[k].shape), np.float32, fill="sentinel") for k in PARAMS]
    watched = [ws, logits] + gs + bs

    def snapshot():
        return [np.array(al.get(v)).tobytes() for v in watched]

    def call(which, null=None, M=M, T=T, C=C, B=B, short=False, training=1):
        pp = [None if null == k else al.ptr(p) for k, p in zip(PARAMS, ps)]
        prm = None if null == "params" else ctypes.byref(L.HowlGruParams(*pp))
        buf = None if null == "buffers" else ctypes.byref(L.HowlGruBuffers(*[al.ptr(b) for b in bs]))
        gr = None if null == "grads" else ctypes.byref(L.HowlGruGrads(*[None if null == "grad " + k else al.ptr(v) for k, v in zip(PARAMS, gs)]))
        xp = None if null == "x" else al.ptr(x)
        wp = None if null == "ws" else al.ptr(ws)
        nb = n - 4 if short else n
        if which == "howl_gru_fwd":
            return lib.cdll.howl_gru_fwd(prm, buf, xp, M * T, T, 1, B, M, T, C, None, training, None, 1.0,
                                         None if null == "logits" else al.ptr(logits), wp, nb, stream)
        return lib.cdll.howl_gru_bwd(prm, xp, M * T, T, 1, B, M, T, C, None, 1.0, None if null == "dlogits" else al.ptr(dl), gr, wp, nb, stream)
    common = [(dict(null="x"), -1, "null pointer"), (dict(null="params"), -1, "null pointer"), (dict(null="ws"), -1, "null pointer"),
              (dict(null="lstm_encoder.weight_hh_l0"), -1, "null pointer"), (dict(M=80), -1, "M=80"), (dict(T=0), -1, "T=0"),
              (dict(T=8193), -1, "T=8193"), (dict(C=0), -1, "num_labels=0"), (dict(B=0), -1, "B=0"), (dict(short=True), -3, "workspace too small")]
    only = {"howl_gru_fwd": [(dict(null="logits"), -1, "null pointer"), (dict(null="buffers"), -1, "null pointer")],
            "howl_gru_bwd": [(dict(null="dlogits"), -1, "null pointer"), (dict(null="grads"), -1, "null pointer"),
                             (dict(null="grad dnn.3.bias"), -1, "null pointer")]}
    for which in ("howl_gru_fwd", "howl_gru_bwd"):
        for kw, code, text in common + only[which]:
            before = snapshot()
            rc = call(which, **kw)
            msg = lib.cdll.howl_last_error().decode()
            assert rc == code, (which, kw, rc, msg)
            assert msg.startswith(which + ":") and text in msg, (which, kw, msg)
            if hasattr(al, "sync"):
                al.sync()
            assert snapshot() == before, (which, kw, "a refused call wrote something")
        if which == "howl_gru_fwd":      # the next valid call succeeds
            assert call("howl_gru_fwd") == 0, lib.cdll.howl_last_error().decode()
        else:
            assert call("howl_gru_bwd") == 0, lib.cdll.howl_last_error().decode()
    if hasattr(al, "sync"):
        al.sync()
    assert np.isfinite(np.array(al.get(logits))).all() and all(np.isfinite(np.array(al.get(v))).all() for v in gs)
    assert lib.cdll.howl_gru_supported(B, M, T, C) == 1
    for bad in ((0, M, T, C), (B, 80, T, C), (B, M, 0, C), (B, M, 8193, C), (B, M, T, 0), (B, M, T, 65)):
        assert lib.cdll.howl_gru_supported(*bad) == 0, bad
    assert lib.cdll.howl_gru_workspace_bytes(B, 0) == 0 and lib.cdll.howl_gru_workspace_bytes(B, 8192) > lib.cdll.howl_gru_workspace_bytes(B, T) > 0
