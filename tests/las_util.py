"""Yardstick and runners of the las tests (tests/test_emu_las.py on the hipemu emulator, tests/test_gpu_las.py on the device).

``RefLas`` restates the model of include/howl_hip_las.h on torch CPU modules -- conv encoder with two BatchNorms, packed
bidirectional LSTM(352 -> 96), the four-head fixed attention WITH the reference's additive -100 on the batch's padded steps (the
kernels leave those steps out), Linear - ReLU - mask - Linear -- with the reference's module names and its double registration of
conv1 / conv2, so a ``state_dict`` loads into it unchanged.  ``reference()`` runs it in float64 (the yardstick) or float32 (the
noise of the same model in the kernels' precision) with an explicit keep mask and returns logits, loss, every parameter gradient
and the updated running statistics.  ``run_library()`` drives the C ABI of any build on the buffers of an allocator with
tests/guard_mem.py's interface (``Plain`` or ``Arena`` host memory for the emulator, ``Banded`` on the device).
"""
import ctypes
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from gru_util import Plain, maxerr  # noqa: F401

GOLDEN_DIR = Path(__file__).resolve().parent / "golden"
GOLDEN_PARTS = ("g17_las.npz", "g17_las_lstm_fwd.npz", "g17_las_lstm_rev.npz")
_L = "encoder.lstm_encoder."
# the 25 distinct parameters in state_dict order (HowlLasParams); ALIASES: the second names of conv1 / conv2
PARAMS = ["encoder.conv1.weight", "encoder.conv1.bias", "encoder.conv2.weight", "encoder.conv2.bias", "encoder.conv_encoder.1.weight",
          "encoder.conv_encoder.1.bias", "encoder.conv_encoder.5.weight", "encoder.conv_encoder.5.bias",
          _L + "weight_ih_l0", _L + "weight_hh_l0", _L + "bias_ih_l0", _L + "bias_hh_l0",
          _L + "weight_ih_l0_reverse", _L + "weight_hh_l0_reverse", _L + "bias_ih_l0_reverse", _L + "bias_hh_l0_reverse",
          "attn.context_vec", "attn.v_proj.weight", "attn.v_proj.bias", "attn.k_proj.weight", "attn.k_proj.bias",
          "fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias"]
ALIASES = {"encoder.conv_encoder.0.weight": "encoder.conv1.weight", "encoder.conv_encoder.0.bias": "encoder.conv1.bias",
           "encoder.conv_encoder.4.weight": "encoder.conv2.weight", "encoder.conv_encoder.4.bias": "encoder.conv2.bias"}
BUFFERS = ["encoder.conv_encoder.1.running_mean", "encoder.conv_encoder.1.running_var", "encoder.conv_encoder.1.num_batches_tracked",
           "encoder.conv_encoder.5.running_mean", "encoder.conv_encoder.5.running_var", "encoder.conv_encoder.5.num_batches_tracked"]
ZERO_GRADS = ("encoder.conv1.bias", "encoder.conv2.bias", "attn.v_proj.bias")
KEEP = 0.9
HID = 256
# name -> (B, T, labels, lengths or None, seed).  A: n_b = 6,5,3,2,1, a one-step reverse direction, B no multiple of four, both
# pools drop a column; B: neither pool drops; C: only the second pool drops (and for the length 19 only the first); one: the
# smallest problem; window: the frontend's 1 s window, three workgroups per direction, several encoder tiles.  tile16 / tile17:
# conv2's output is 16 and 17 columns wide (C: 15), one column either side of the encoder tile's width.
CASES = {"A": (5, 21, 4, [21, 17, 9, 3, 1], 21), "B": (4, 22, 4, None, 22), "C": (3, 24, 4, [24, 19, 2], 23), "one": (1, 1, 4, None, 24),
         "tile16": (2, 26, 4, [26, 11], 25), "tile17": (2, 28, 4, [28, 13], 26), "window": (9, 81, 12, [81] * 9, 27)}


def steps_of(frames):
    return (((frames + 2) // 2) + 2) // 2


class RefEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = conv1 = nn.Conv2d(3, 8, 3, padding=2)
        self.conv2 = conv2 = nn.Conv2d(8, 8, 3, padding=2)
        self.conv_encoder = nn.Sequential(conv1, nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d((1, 2)), conv2, nn.BatchNorm2d(8), nn.ReLU(),
                                          nn.MaxPool2d((1, 2)))
        self.lstm_encoder = nn.LSTM(352, 96, 1, bias=True, bidirectional=True)


class RefAttn(nn.Module):
    def __init__(self):
        super().__init__()
        self.context_vec = nn.Parameter(torch.empty(192).uniform_(-0.25, 0.25))
        self.v_proj = nn.Linear(192, 192)
        self.k_proj = nn.Linear(192, 192)


class RefLas(nn.Module):
    def __init__(self, num_labels):
        super().__init__()
        self.encoder = RefEncoder()
        self.attn = RefAttn()
        self.fc = nn.Sequential(nn.Linear(192, HID), nn.ReLU(), nn.Dropout(1.0 - KEEP), nn.Linear(HID, num_labels))

    def forward(self, x, lengths, keep_mask=None):
        """x (B, 3, 40, T); lengths: frame counts or None; keep_mask (B, 256) of 0/1 or None (no dropout)."""
        B, T = x.size(0), x.size(-1)
        frames = torch.full((B,), T, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths, dtype=torch.int64)
        steps = steps_of(frames)
        e = self.encoder.conv_encoder(x)                                   # (B, 8, 44, T2)
        seq = e.permute(3, 0, 1, 2).contiguous().view(e.size(3), B, 352)
        rnn_seq, _ = self.encoder.lstm_encoder(pack_padded_sequence(seq, steps))
        rnn_seq, n = pad_packed_sequence(rnn_seq)                          # (max n_b, B, 192), zero past n_b
        mask = (torch.arange(rnn_seq.size(0)).unsqueeze(1) < n.unsqueeze(0)).to(rnn_seq.dtype)
        values = self.attn.v_proj(rnn_seq).view(rnn_seq.size(0), B, 4, 48)
        keys = self.attn.k_proj(rnn_seq).view(rnn_seq.size(0), B, 4, 48)
        logits = torch.einsum("ijkl,lk->ijk", values, self.attn.context_vec.view(48, 4))
        logits = logits + ((1 - mask) * -100).unsqueeze(-1)
        ctx = torch.einsum("ijk,ijkl->jkl", F.softmax(logits, 0), keys).reshape(B, 192)
        y1 = self.fc[1](self.fc[0](ctx))
        if keep_mask is not None:
            y1 = y1 * keep_mask.to(y1.dtype) * (1.0 / KEEP)
        return self.fc[3](y1)


def make_state(num_labels, seed):
    """A seeded float32 state (35 keys) with every BatchNorm tensor away from its initial value."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in RefLas(num_labels).state_dict().items()}
    for i in (1, 5):
        p = f"encoder.conv_encoder.{i}."
        sd[p + "weight"] = 0.5 + torch.rand(8, generator=g)
        sd[p + "bias"] = 0.6 * torch.rand(8, generator=g) - 0.3
        sd[p + "running_mean"] = 0.4 * torch.rand(8, generator=g) - 0.2
        sd[p + "running_var"] = 0.5 + torch.rand(8, generator=g)
        sd[p + "num_batches_tracked"] = torch.tensor(3)
    for a, k in ALIASES.items():
        sd[a] = sd[k]
    return sd


def make_case(name):
    """-> (state, x (B,3,40,T) float32, lengths list or None, labels, keep mask (B,256))."""
    B, T, C, lengths, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, 40, T, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    mask = (torch.rand(B, HID, generator=g) < KEEP).float()
    return make_state(C, seed), x, lengths, labels, mask


def reference(state, x, lengths, labels=None, mask=None, train=False, dtype=torch.float64):
    """-> dict(logits, loss, grads {name: tensor}, buffers {name: tensor}) of the restated model in ``dtype`` on the CPU."""
    C = state["fc.3.bias"].numel()
    m = RefLas(C).to(dtype)
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


def check_logits(name, got, ref, what):
    err = maxerr(got, ref["logits"])
    print(f"las {name} {what}: |dlogits| = {err:.3e}")
    assert err < 5e-5, (name, what, err)              # tests/gru_util.py's bound on logits


def check_loss(name, got_logits, labels, ref):
    loss = float(F.cross_entropy(torch.as_tensor(got_logits).float(), labels))
    err = abs(loss - float(ref["loss"]))
    print(f"las {name}: loss {loss:.6f}, |dloss| = {err:.3e}")
    assert err < 1e-4 * max(1.0, abs(float(ref["loss"]))), (name, err)


def check_grads(name, grads, r64, r32):
    """tests/gru_util.py's noise idiom: maxerr(g, g64) < 4 noise + 2e-5 max(1, |g64|max), noise = the fp32 CPU model's error; the
    three identically zero gradients are exact zeros."""
    bad = []
    for k, g in zip(PARAMS, grads):
        g64 = r64["grads"][k]
        noise = maxerr(r32["grads"][k], g64)
        bound = 4 * noise + 2e-5 * max(1.0, float(g64.abs().max()))
        err = maxerr(torch.as_tensor(g).reshape(g64.shape), g64)
        print(f"las {name} grad {k}: err {err:.3e}  noise {noise:.3e}  bound {bound:.3e}  |g|max {float(g64.abs().max()):.3e}")
        if not err < bound:
            bad.append((k, err, bound))
        if k in ZERO_GRADS and not bool((torch.as_tensor(g) == 0).all()):
            bad.append((k, "not exactly zero", float(torch.as_tensor(g).abs().max())))
    assert not bad, (name, bad)


def check_buffers(name, got, ref):
    for k in BUFFERS:
        a, b = torch.as_tensor(got[k]), ref["buffers"][k]
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b), (name, k, int(a), int(b))
        else:
            err = maxerr(a.reshape(b.shape), b)
            print(f"las {name} {k}: err {err:.3e}")
            assert err < 2e-6 * max(1.0, float(b.abs().max())), (name, k, err)      # a few fp32 roundings of O(1) numbers


# ---- the C ABI on any build ---------------------------------------------------------------------------------------------------------

def _putter(al):
    def put(t, tag):
        a = np.ascontiguousarray(torch.as_tensor(t).numpy())
        return al.buf(tag, a.shape if a.ndim else (1,), a.dtype, fill=a)
    return put


def run_library(lib, al, state, x, lengths, training, mask=None, dlogits=None, x_time_major=False, stream=None):
    """howl_las_fwd (and howl_las_bwd when ``dlogits`` is given) on the buffers of allocator ``al`` -> dict(logits, grads list in
    PARAMS order, buffers).  The features are handed over as the (B, 3, 40, T) tensor (time fastest), or as (B, 3, T, 40) (mel
    fastest) through the strides.  The workspace is exactly howl_las_workspace_bytes long and starts out as NaN, like every output:
    whatever a kernel reads, an earlier launch of the call has written."""
    from howl_amd import lib as L
    B, CH, M, T = x.shape
    C = state["fc.3.bias"].numel()
    put = _putter(al)

    def get(v):
        return torch.from_numpy(np.array(al.get(v)))
    if x_time_major:
        xd = put(x.permute(0, 1, 3, 2).contiguous(), "x")
        sb, sc, sm, st = CH * T * M, T * M, 1, M
    else:
        xd = put(x, "x")
        sb, sc, sm, st = CH * M * T, M * T, T, 1
    ps = [put(state[k], k) for k in PARAMS]
    bs = [put(state[k], k) for k in BUFFERS]
    ld = None if lengths is None else put(torch.as_tensor(lengths, dtype=torch.int64), "lengths")
    md = None if mask is None else put(mask, "mask")
    n = lib.cdll.howl_las_workspace_bytes(B, T)
    ws = al.buf("workspace", n // 4, np.float32, fill="sentinel")
    logits = al.buf("logits", (B, C), np.float32, fill="sentinel", promised="all")
    prm = L.HowlLasParams(*[al.ptr(p) for p in ps])
    buf = L.HowlLasBuffers(*[al.ptr(b) for b in bs])
    scale = 1.0 / KEEP if mask is not None else 1.0
    lib.call("howl_las_fwd", ctypes.byref(prm), ctypes.byref(buf), al.ptr(xd), sb, sc, sm, st, B, M, T, C, al.ptr(ld), int(training),
             al.ptr(md), scale, al.ptr(logits), al.ptr(ws), n, stream)
    out = {"logits": get(logits), "grads": None}
    if dlogits is not None:
        dl = put(dlogits, "dlogits")
        gs = [al.buf("grad " + k, tuple(state[k].shape), np.float32, fill="sentinel", promised="all") for k in PARAMS]
        gr = L.HowlLasGrads(*[al.ptr(g) for g in gs])
        lib.call("howl_las_bwd", ctypes.byref(prm), al.ptr(xd), sb, sc, sm, st, B, M, T, C, al.ptr(ld), scale, al.ptr(dl), ctypes.byref(gr),
                 al.ptr(ws), n, stream)
        out["grads"] = [get(g) for g in gs]
    out["buffers"] = {k: get(b).reshape(state[k].shape) for k, b in zip(BUFFERS, bs)}
    out["params"] = {k: get(p) for k, p in zip(PARAMS, ps)}
    if ld is not None:
        out["lengths"] = get(ld)
    return out


def check_refusals(lib, al, stream=None):
    """Every refusal of include/howl_hip_las.h on a (B=2, T=6, 4 labels) problem: the code, a message that names the entry point and
    the reason, nothing launched (logits, gradients, workspace and BatchNorm buffers keep their bytes) -- and the next valid call
    succeeds, so no refusal leaves an error pending."""
    from howl_amd import lib as L
    B, T, C, M = 2, 6, 4, 40
    state = make_state(C, 5)
    g = torch.Generator().manual_seed(5)
    put = _putter(al)
    x = put(torch.randn(B, 3, M, T, generator=g), "x")
    ps = [put(state[k], k) for k in PARAMS]
    bs = [put(state[k], k) for k in BUFFERS]
    dl = put(torch.randn(B, C, generator=g), "dlogits")
    n = lib.cdll.howl_las_workspace_bytes(B, T)
    ws = al.buf("workspace", n // 4, np.float32, fill="sentinel")
    logits = al.buf("logits", (B, C), np.float32, fill="sentinel")
    gs = [al.buf("grad " + k, tuple(state[k].shape), np.float32, fill="sentinel") for k in PARAMS]
    watched = [ws, logits] + gs + bs

    def snapshot():
        return [np.array(al.get(v)).tobytes() for v in watched]

    def call(which, null=None, M=M, T=T, C=C, B=B, short=False, training=1):
        pp = [None if null == k else al.ptr(p) for k, p in zip(PARAMS, ps)]
        prm = None if null == "params" else ctypes.byref(L.HowlLasParams(*pp))
        buf = None if null == "buffers" else ctypes.byref(L.HowlLasBuffers(*[al.ptr(b) for b in bs]))
        gr = None if null == "grads" else ctypes.byref(L.HowlLasGrads(*[None if null == "grad " + k else al.ptr(v) for k, v in zip(PARAMS, gs)]))
        xp = None if null == "x" else al.ptr(x)
        wp = None if null == "ws" else al.ptr(ws)
        nb = n - 4 if short else n
        if which == "howl_las_fwd":
            return lib.cdll.howl_las_fwd(prm, buf, xp, 3 * M * T, M * T, T, 1, B, M, T, C, None, training, None, 1.0,
                                         None if null == "logits" else al.ptr(logits), wp, nb, stream)
        return lib.cdll.howl_las_bwd(prm, xp, 3 * M * T, M * T, T, 1, B, M, T, C, None, 1.0, None if null == "dlogits" else al.ptr(dl), gr, wp, nb,
                                     stream)
    common = [(dict(null="x"), -1, "null pointer"), (dict(null="params"), -1, "null pointer"), (dict(null="ws"), -1, "null pointer"),
              (dict(null=_L + "weight_hh_l0_reverse"), -1, "null pointer"), (dict(M=80), -1, "M=80"), (dict(T=0), -1, "T=0"),
              (dict(T=8193), -1, "T=8193"), (dict(C=0), -1, "num_labels=0"), (dict(C=65), -1, "num_labels=65"), (dict(B=0), -1, "B=0"),
              (dict(short=True), -3, "workspace too small")]
    only = {"howl_las_fwd": [(dict(null="logits"), -1, "null pointer"), (dict(null="buffers"), -1, "null pointer")],
            "howl_las_bwd": [(dict(null="dlogits"), -1, "null pointer"), (dict(null="grads"), -1, "null pointer"),
                             (dict(null="grad fc.3.bias"), -1, "null pointer")]}
    for which in ("howl_las_fwd", "howl_las_bwd"):
        for kw, code, text in common + only[which]:
            before = snapshot()
            rc = call(which, **kw)
            msg = lib.cdll.howl_last_error().decode()
            assert rc == code, (which, kw, rc, msg)
            assert msg.startswith(which + ":") and text in msg, (which, kw, msg)
            if hasattr(al, "sync"):
                al.sync()
            assert snapshot() == before, (which, kw, "a refused call wrote something")
        assert call(which) == 0, lib.cdll.howl_last_error().decode()      # the next valid call succeeds
    if hasattr(al, "sync"):
        al.sync()
    assert np.isfinite(np.array(al.get(logits))).all() and all(np.isfinite(np.array(al.get(v))).all() for v in gs)
    assert lib.cdll.howl_las_supported(B, M, T, C) == 1
    for bad in ((0, M, T, C), (B, 80, T, C), (B, M, 0, C), (B, M, 8193, C), (B, M, T, 0), (B, M, T, 65)):
        assert lib.cdll.howl_las_supported(*bad) == 0, bad
    assert lib.cdll.howl_las_workspace_bytes(B, 0) == 0 and lib.cdll.howl_las_workspace_bytes(B, 8192) > lib.cdll.howl_las_workspace_bytes(B, T) > 0


def load_golden():
    """-> (arrays dict of every G17 part, state dict of 35 keys with the aliases restored)."""
    g = {}
    for part in GOLDEN_PARTS:
        with np.load(GOLDEN_DIR / part) as f:
            g.update({k: f[k] for k in f.files})
    state = {k[6:]: torch.from_numpy(g[k]) for k in g if k.startswith("state/")}
    for a, k in ALIASES.items():
        state[a] = state[k]
    order = list(RefLas(4).state_dict())
    return g, {k: state[k] for k in order}
