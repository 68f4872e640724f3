"""Yardstick and runners of the small-cnn / seq-cnn tests (tests/test_emu_cnn.py on the hipemu emulator, tests/test_gpu_cnn.py on the
device).

``RefCnn`` restates both models of include/howl_hip_cnn.h on torch CPU layers -- the two conv stages with ReLU, MaxPool and
BatchNorm, Linear - ReLU - mask - Linear -- with the reference's module names, so a ``state_dict`` loads into it unchanged.
``reference()`` runs it in float64 (the yardstick) or float32 (the noise of the same model in the kernels' precision) with an
explicit keep mask and returns scores, loss, every parameter gradient and the updated running statistics.  small-cnn's loss is the
cross-entropy, seq-cnn's ``log_softmax`` + ``CTCLoss`` on the model's output lengths.  ``run_library()`` drives the C ABI of any
build on the buffers of an allocator with tests/guard_mem.py's interface.
"""
import ctypes
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SMALL, SEQ = 0, 1
GOLDEN = {SMALL: Path(__file__).resolve().parent / "golden" / "g19_small_cnn.npz", SEQ: Path(__file__).resolve().parent / "golden" / "g20_seq_cnn.npz"}
PARAMS = ["encoder1.0.weight", "encoder1.0.bias", "encoder1.3.weight", "encoder1.3.bias", "encoder2.0.weight", "encoder2.0.bias",
          "encoder2.3.weight", "encoder2.3.bias", "output.0.weight", "output.0.bias", "output.3.weight", "output.3.bias"]
BUFFERS = ["encoder1.3.running_mean", "encoder1.3.running_var", "encoder1.3.num_batches_tracked", "encoder2.3.running_mean",
           "encoder2.3.running_var", "encoder2.3.num_batches_tracked"]
KEEP = 0.9
BLANK = 0
# name -> (kind, B, T, labels, lengths or None, seed).  small-cnn: both ends of the valid range (7 and 10 pooled rows, 4 and 5 conv1
# rows) and the converted window, B of 1 and 5, 2 / 4 / 12 labels.  seq-cnn: the shortest clip (one output row), an odd pooled row
# count, and the 1 s clip with ragged lengths: 41 pooled rows = six conv0 tiles, three data-gradient tiles and three conv1 tiles,
# each with a remainder.  GPU only: "q150", ten conv0 tiles (the weight gradient's eight workgroups along time loop), and
# "s26b", more utterances than either weight gradient has utterance groups (32 and 16).
CASES = {"s26": (SMALL, 5, 26, 4, None, 21), "s40": (SMALL, 1, 40, 2, None, 22), "s41": (SMALL, 5, 41, 12, None, 33),
         "q5": (SEQ, 5, 5, 4, None, 24), "q22": (SEQ, 1, 22, 2, None, 25), "q81": (SEQ, 5, 81, 12, [78, 61, 30, 9, 5], 46),
         "q150": (SEQ, 2, 150, 4, None, 27), "s26b": (SMALL, 40, 26, 4, None, 448)}
MARGIN = 1e-5      # smallest distance of a ReLU / max-pool decision from its tie in the committed cases (decision_margin)


def compute_length(T):
    """``SequentialCnn.compute_length`` (reference cnn.py:90-95)."""
    n = int((T + 2 * 10 - (20 - 1) - 1) / 1 + 1) // 2
    return int((n + 2 * 2 - (5 - 1) - 1) / 2 + 1) // 2


class RefCnn(nn.Module):
    def __init__(self, kind, num_labels):
        super().__init__()
        self.kind = kind
        conv0 = nn.Conv2d(1, 48, (8, 16), padding=(4, 0), stride=(2, 2)) if kind == SMALL else nn.Conv2d(1, 48, (20, 16), padding=(10, 0), stride=(1, 2))
        self.encoder1 = nn.Sequential(conv0, nn.ReLU(), nn.MaxPool2d(2), nn.BatchNorm2d(48))
        self.encoder2 = nn.Sequential(nn.Conv2d(48, 64, (5, 5), padding=2, stride=(2, 1)), nn.ReLU(), nn.MaxPool2d(2), nn.BatchNorm2d(64))
        self.output = nn.Sequential(nn.Linear(384 if kind == SMALL else 192, 128), nn.ReLU(), nn.Dropout(0.1), nn.Linear(128, num_labels))

    def forward(self, x, keep_mask=None, taps=None):
        """x (B, C, 40, T); keep_mask (B, 128) / (T', B, 128) of 0/1 or None (no dropout).  ``taps``: a list that receives the
        pre-ReLU tensors (decision_margin)."""
        x = x[:, :1].permute(0, 1, 3, 2)
        z0 = self.encoder1[0](x)
        x1 = self.encoder1[3](self.encoder1[2](self.encoder1[1](z0)))
        z1 = self.encoder2[0](x1)
        x2 = self.encoder2[3](self.encoder2[2](self.encoder2[1](z1)))
        if self.kind == SMALL:
            h = x2.reshape(x2.size(0), -1)
        else:
            h = x2.permute(2, 0, 1, 3).contiguous()
            h = h.view(h.size(0), h.size(1), -1)
        a1 = self.output[0](h)
        if taps is not None:
            taps.extend([z0, z1, a1])
        y1 = self.output[1](a1)
        if keep_mask is not None:
            y1 = y1 * keep_mask.to(y1.dtype) * (1.0 / KEEP)
        return self.output[3](y1)


def make_state(kind, num_labels, seed):
    """A seeded float32 state with every BatchNorm tensor away from its initial value."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in RefCnn(kind, num_labels).state_dict().items()}
    for name, n in (("encoder1.3", 48), ("encoder2.3", 64)):
        sd[f"{name}.weight"] = 0.5 + torch.rand(n, generator=g)
        sd[f"{name}.bias"] = 0.6 * torch.rand(n, generator=g) - 0.3
        sd[f"{name}.running_mean"] = 0.4 * torch.rand(n, generator=g) - 0.2
        sd[f"{name}.running_var"] = 0.5 + torch.rand(n, generator=g)
        sd[f"{name}.num_batches_tracked"] = torch.tensor(3)
    return sd


def make_targets(kind, B, T, C, lengths, g):
    """small-cnn: class labels (B,).  seq-cnn: dict(targets (B, 3), target_lengths, input_lengths = the model's output lengths);
    at most 3 distinct labels, never more than the output rows: no loss is infinite."""
    if kind == SMALL:
        return torch.randint(0, C, (B,), generator=g)
    frames = [T] * B if lengths is None else lengths
    il = torch.tensor([compute_length(n) for n in frames], dtype=torch.int64)
    tl = torch.tensor([min(3, int(n), C - 1) for n in il], dtype=torch.int64)
    targets = torch.tensor([[1 + (j + b) % (C - 1) for j in range(3)] for b in range(B)], dtype=torch.int64)
    return dict(targets=targets, target_lengths=tl, input_lengths=il)


def make_case(name):
    """-> (kind, state, x (B,3,40,T) float32, lengths, targets, keep mask)."""
    kind, B, T, C, lengths, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, 40, T, generator=g)
    targets = make_targets(kind, B, T, C, lengths, g)
    shape = (B, 128) if kind == SMALL else (compute_length(T), B, 128)
    mask = (torch.rand(*shape, generator=g) < KEEP).float()
    return kind, make_state(kind, C, seed), x, lengths, targets, mask


def loss_of(kind, scores, targets):
    if kind == SMALL:
        return F.cross_entropy(scores, targets)
    return F.ctc_loss(torch.log_softmax(scores, -1), targets["targets"], targets["input_lengths"], targets["target_lengths"], blank=BLANK)


def reference(kind, state, x, targets=None, mask=None, train=False, dtype=torch.float64, taps=None):
    """-> dict(logits, loss, grads {name: tensor}, buffers {name: tensor}) of the restated model in ``dtype`` on the CPU.  seq-cnn's
    ``logits`` are the (T', B, L) scores."""
    C = state["output.3.bias"].numel()
    m = RefCnn(kind, C).to(dtype)
    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()})
    m.train(train)
    logits = m(x.to(dtype), mask if train else None, taps)
    out = {"logits": logits.detach(), "loss": None, "grads": None}
    if targets is not None:
        loss = loss_of(kind, logits, targets)
        out["loss"] = loss.detach()
        if train:
            loss.backward()
            named = dict(m.named_parameters())
            out["grads"] = {k: named[k].grad.detach() for k in PARAMS}
    out["buffers"] = {k: v.detach().clone() for k, v in m.state_dict().items() if k in BUFFERS}
    return out


def decision_margin(kind, state, x, mask):
    """The smallest distance of any ReLU or max-pool decision of the training forward from its tie, in float64: the winner of every
    pool window from zero and from the runner-up (where the winner is positive: otherwise no gradient passes either way), and
    the head's hidden pre-activations from zero."""
    taps = []
    reference(kind, state, x, None, mask, train=True, taps=taps)
    z0, z1, a1 = [t.detach() for t in taps]
    worst = float(a1.detach().abs().min())
    for z in (z0, z1):
        H, W = z.shape[2] // 2 * 2, z.shape[3] // 2 * 2
        win = z[:, :, :H, :W].unfold(2, 2, 2).unfold(3, 2, 2).reshape(z.shape[0], z.shape[1], H // 2, W // 2, 4)
        top = win.topk(2, dim=-1).values
        worst = min(worst, float(top[..., 0].abs().min()))
        live = top[..., 0] > 0
        if live.any():
            worst = min(worst, float((top[..., 0] - top[..., 1])[live].min()))
    return worst


_REF = {}


def case_reference(name):
    """fp64 and fp32 results of a case in training mode, the fp64 and fp32 eval scores, and d loss / d scores at the fp64 scores
    (what the library's backward is fed) -- computed once per process and shared."""
    if name not in _REF:
        kind, state, x, lengths, targets, mask = make_case(name)
        r64 = reference(kind, state, x, targets, mask, train=True)
        r32 = reference(kind, state, x, targets, mask, train=True, dtype=torch.float32)
        e64 = reference(kind, state, x, targets)
        e32 = reference(kind, state, x, targets, dtype=torch.float32)
        z = r64["logits"].clone().requires_grad_(True)
        loss_of(kind, z, targets).backward()
        _REF[name] = dict(kind=kind, state=state, x=x, lengths=lengths, targets=targets, mask=mask, train64=r64, train32=r32, eval64=e64,
                          eval32=e32, dlogits=z.grad.float())
    return _REF[name]


def maxerr(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def check_logits(name, got, ref, what):
    err = maxerr(got, ref["logits"])
    print(f"cnn {name} {what}: |dlogits| = {err:.3e}")
    assert err < 5e-5, (name, what, err)


def check_loss(name, kind, got_logits, targets, ref):
    loss = float(loss_of(kind, torch.as_tensor(got_logits).float(), targets))
    err = abs(loss - float(ref["loss"]))
    print(f"cnn {name}: loss {loss:.6f}, |dloss| = {err:.3e}")
    assert err < 1e-4 * max(1.0, abs(float(ref["loss"]))), (name, err)


def check_grads(name, grads, r64, r32):
    """maxerr(g, g64) < 4 noise + 2e-5 max(1, |g64|max), noise = the fp32 CPU model's error (tests/gru_util.py's idiom)."""
    bad = []
    for k, g in zip(PARAMS, grads):
        g64 = r64["grads"][k]
        noise = maxerr(r32["grads"][k], g64)
        bound = 4 * noise + 2e-5 * max(1.0, float(g64.abs().max()))
        err = maxerr(torch.as_tensor(g).reshape(g64.shape), g64)
        print(f"cnn {name} grad {k}: err {err:.3e}  noise {noise:.3e}  bound {bound:.3e}  |g|max {float(g64.abs().max()):.3e}")
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
            print(f"cnn {name} {k}: err {err:.3e}")
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


def run_library(lib, al, kind, state, x, training, mask=None, dlogits=None, x_time_major=False, stream=None):
    """howl_cnn_fwd (and howl_cnn_bwd when ``dlogits`` is given, in the scores' shape) on the buffers of allocator ``al`` ->
    dict(logits in the model's shape, grads list in PARAMS order, buffers).  The features are handed over as channel 0 of the
    (B, 3, 40, T) tensor in place (strides), or time-major (B, T, 40) as the fused frontend leaves them.  The workspace is
    exactly howl_cnn_workspace_bytes long and starts out as NaN, like every output."""
    from howl_amd import lib as L
    B, _, M, T = x.shape
    C = state["output.3.bias"].numel()
    H = int(lib.cdll.howl_cnn_out_rows(kind, T))

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
    md = None if mask is None else put(mask, "mask")
    n = lib.cdll.howl_cnn_workspace_bytes(kind, B, T, C)
    ws = al.buf("workspace", n // 4, np.float32, fill="sentinel")
    logits = al.buf("logits", (B, C) if kind == SMALL else (B, H, C), np.float32, fill="sentinel", promised="all")
    prm = L.HowlCnnParams(*[al.ptr(p) for p in ps])
    buf = L.HowlCnnBuffers(*[al.ptr(b) for b in bs])
    scale = 1.0 / KEEP if mask is not None else 1.0
    lib.call("howl_cnn_fwd", kind, ctypes.byref(prm), ctypes.byref(buf), al.ptr(xd), sb, sm, st, B, M, T, C, int(training), al.ptr(md),
             scale, al.ptr(logits), al.ptr(ws), n, stream)
    shaped = (lambda t: t) if kind == SMALL else (lambda t: t.permute(1, 0, 2))
    out = {"logits": shaped(get(logits)), "grads": None}
    if dlogits is not None:
        dl = put(shaped(torch.as_tensor(dlogits)).contiguous(), "dlogits")      # (T', B, L) -> the (B, T', L) buffer
        gs = [al.buf("grad " + k, tuple(state[k].shape), np.float32, fill="sentinel", promised="all") for k in PARAMS]
        gr = L.HowlCnnGrads(*[al.ptr(g) for g in gs])
        lib.call("howl_cnn_bwd", kind, ctypes.byref(prm), al.ptr(xd), sb, sm, st, B, M, T, C, scale, al.ptr(dl), ctypes.byref(gr),
                 al.ptr(ws), n, stream)
        out["grads"] = [get(g) for g in gs]
    out["buffers"] = {k: get(b).reshape(state[k].shape) for k, b in zip(BUFFERS, bs)}
    out["params"] = {k: get(p) for k, p in zip(PARAMS, ps)}
    return out


def check_refusals(lib, al, kind, stream=None):
    """Every refusal of include/howl_hip_cnn.h on a small problem: the code, a message that names the entry point and the reason,
    nothing launched (scores, gradients, workspace and BatchNorm buffers keep their bytes) -- and the next valid call succeeds,
    so no refusal leaves an error pending."""
    from howl_amd import lib as L
    B, C, M = 2, 4, 40
    T = 30 if kind == SMALL else 9
    lo, hi = (26, 41) if kind == SMALL else (5, 8192)
    H = int(lib.cdll.howl_cnn_out_rows(kind, T))
    state = make_state(kind, C, 5)
    g = torch.Generator().manual_seed(5)

    def put(t, tag):
        a = np.ascontiguousarray(torch.as_tensor(t).numpy())
        return al.buf(tag, a.shape if a.ndim else (1,), a.dtype, fill=a)
    x = put(torch.randn(B, 1, M, T, generator=g), "x")
    ps = [put(state[k], k) for k in PARAMS]
    bs = [put(state[k], k) for k in BUFFERS]
    shape = (B, C) if kind == SMALL else (B, H, C)
    dl = put(torch.randn(*shape, generator=g), "dlogits")
    mk = put(torch.ones(B * H * 128), "mask")
    n = lib.cdll.howl_cnn_workspace_bytes(kind, B, T, C)
    ws = al.buf("workspace", n // 4, np.float32, fill="sentinel")
    logits = al.buf("logits", shape, np.float32, fill="sentinel")
    gs = [al.buf("grad " + k, tuple(state[k].shape), np.float32, fill="sentinel") for k in PARAMS]
    watched = [ws, logits] + gs + bs

    def snapshot():
        return [np.array(al.get(v)).tobytes() for v in watched]

    def call(which, null=None, M=M, T=T, C=C, B=B, short=False, training=1, kind=kind, mask=False):
        pp = [None if null == k else al.ptr(p) for k, p in zip(PARAMS, ps)]
        prm = None if null == "params" else ctypes.byref(L.HowlCnnParams(*pp))
        buf = None if null == "buffers" else ctypes.byref(L.HowlCnnBuffers(*[al.ptr(b) for b in bs]))
        gr = None if null == "grads" else ctypes.byref(L.HowlCnnGrads(*[None if null == "grad " + k else al.ptr(v) for k, v in zip(PARAMS, gs)]))
        xp = None if null == "x" else al.ptr(x)
        wp = None if null == "ws" else al.ptr(ws)
        nb = n - 4 if short else n
        if which == "howl_cnn_fwd":
            return lib.cdll.howl_cnn_fwd(kind, prm, buf, xp, M * T, T, 1, B, M, T, C, training, al.ptr(mk) if mask else None, 1.0,
                                         None if null == "logits" else al.ptr(logits), wp, nb, stream)
        return lib.cdll.howl_cnn_bwd(kind, prm, xp, M * T, T, 1, B, M, T, C, 1.0, None if null == "dlogits" else al.ptr(dl), gr, wp, nb, stream)
    common = [(dict(null="x"), -1, "null pointer"), (dict(null="params"), -1, "null pointer"), (dict(null="ws"), -1, "null pointer"),
              (dict(null="encoder2.0.weight"), -1, "null pointer"), (dict(kind=2), -1, "kind=2"), (dict(M=80), -1, "M=80"),
              (dict(T=lo - 1), -1, f"T={lo - 1}"), (dict(T=hi + 1), -1, f"T={hi + 1}"), (dict(C=0), -1, "num_labels=0"),
              (dict(C=65), -1, "num_labels=65"), (dict(B=0), -1, "B=0"), (dict(short=True), -3, "workspace too small")]
    only = {"howl_cnn_fwd": [(dict(null="logits"), -1, "null pointer"), (dict(null="buffers"), -1, "null pointer"),
                             (dict(training=0, mask=True), -1, "dropout mask in eval mode")],
            "howl_cnn_bwd": [(dict(null="dlogits"), -1, "null pointer"), (dict(null="grads"), -1, "null pointer"),
                             (dict(null="grad output.3.bias"), -1, "null pointer")]}
    for which in ("howl_cnn_fwd", "howl_cnn_bwd"):
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
    assert lib.cdll.howl_cnn_supported(kind, B, M, T, C) == 1
    for bad in ((2, B, M, T, C), (kind, 0, M, T, C), (kind, B, 80, T, C), (kind, B, M, lo - 1, C), (kind, B, M, hi + 1, C), (kind, B, M, T, 0),
                (kind, B, M, T, 65)):
        assert lib.cdll.howl_cnn_supported(*bad) == 0, bad
    assert lib.cdll.howl_cnn_workspace_bytes(kind, B, lo - 1, C) == 0 and lib.cdll.howl_cnn_workspace_bytes(kind, B, hi, C) >= n > 0
    assert lib.cdll.howl_cnn_out_rows(kind, lo - 1) == 0 and lib.cdll.howl_cnn_out_rows(kind, hi + 1) == 0
