"""Shared by tests/test_emu_lstm_stream.py (hipemu, guarded host buffers) and tests/test_gpu_lstm_stream.py (device, sentinel
bands): the streaming seq-lstm / lstm entry point of include/howl_hip_lstm_stream.h called through an allocator of
tests/guard_mem.py, the eager chain (howl_logmel_fwd -> howl_lstm_fwd -> howl_head_fwd) on the same library, the float64 oracle,
and the module-level checks (session, engines) that run unchanged on either side.

Tolerances (the project's precedent for a fused kernel against its launch chain, tests/stream_util.py): with e = max |logits -
fp64 oracle| over the valid rows, e_fused <= 2 e_eager + 1e-6, where e_eager is the existing chain on the same inputs; the factor
2 covers the head's other summation order, the recurrence is meant to be the same bits.  The same form for the returned (h, c).
|probs - softmax64(own logits)| <= 1e-6 and row sums within 1e-6 of 1."""
import ctypes
from pathlib import Path

import numpy as np
import torch

from howl_amd.lib import HowlHeadParams, HowlLstmParams, HowlLstmSaved
from oracle import frontend as fe
from oracle import models as om

W = 16                     # the kernel's window (howl_amd/csrc/lstm_stream.hip: LS_W)
HOP, WIN = 200, 512
LSTM_KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0")
HEAD_KEYS = ("dnn.0.weight", "dnn.0.bias", "dnn.2.weight", "dnn.2.bias")


def g4_pair():
    """[mean, std] of golden G4's ZMUV statistics."""
    g = np.load(Path(__file__).resolve().parent / "golden" / "g4_zmuv.npz")
    mean, mean2 = float(g["mean"][0]), float(g["mean2"][0])
    return np.array([mean, np.sqrt(mean2 - mean * mean)], np.float32)


def num_frames(n):
    return 1 + n // HOP


def compute_lengths(n):
    """StandardAudioTransform.compute_lengths: the frames of an uncentred 512-sample transform, three fewer than the centred one has
    (38 for 8000 samples, 318 for 64000); 512 samples give one frame, fewer none."""
    return (n - WIN) // HOP + 1


def random_state(C, seed):
    """Seeded random weights at nn.LSTM / nn.Linear's default scales."""
    g = torch.Generator().manual_seed(seed)
    sd = om.lstm_init(C)
    return {k: (v.abs().max() * (2 * torch.rand(v.shape, generator=g) - 1)).float() for k, v in sd.items()}


def softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def pack_fb(al, lib, fb, tag=""):
    src = al.buf(tag + "fb", fb.shape, np.float32, np.ascontiguousarray(fb, np.float32))
    fbp = al.buf(tag + "fbp", int(lib.cdll.howl_fb_packed_floats(fb.shape[1])), np.float32, "sentinel", promised="all")
    lib.call("howl_fb_pack", al.ptr(src), fb.shape[1], al.ptr(fbp), None)
    return fbp


class Model:
    """One model's parameters (every tensor in a buffer of its own), the packed filterbank and the ZMUV pair."""

    def __init__(self, al, lib, sd, tag=""):
        self.al, self.lib, self.sd, self.tag = al, lib, sd, tag
        self.C = sd["dnn.2.weight"].shape[0]
        self.p = {k: al.buf(tag + k, v.shape, np.float32, v.numpy()) for k, v in sd.items()}
        self.lstm = HowlLstmParams(*[al.ptr(self.p[k]) for k in LSTM_KEYS])
        self.head = HowlHeadParams(*[al.ptr(self.p[k]) for k in HEAD_KEYS])
        self.fbp = pack_fb(al, lib, fe.mel_fb(40).numpy(), tag)
        self.pair = g4_pair()
        self.zm = al.buf(tag + "zmuv", 2, np.float32, self.pair)

    def chunks(self, clips, frames=None, state=None, last_only=False, zmuv=True, tag="", want_logits=True, n_samples=True, L_max=None,
               ld=None):
        """clips: list of 1-D float32 arrays (ragged) -> (probs, logits, (h, c) or None), outputs of exactly the promised shape:
        (N, T_max, C) with every element promised, or (N, C) with ``last_only``.  The PCM buffer is (N, L_max) with the rows ending
        at the buffer's end (ld == L_max)."""
        al, C = self.al, self.C
        N = len(clips)
        ns = np.array([len(c) for c in clips], np.int64)
        L_max = int(ns.max()) if L_max is None else L_max
        ld = L_max if ld is None else ld
        rows = np.zeros((N, ld), np.float32)
        for i, c in enumerate(clips):
            rows[i, :len(c)] = c
        flat = rows.reshape(-1)[:(N - 1) * ld + L_max]
        pcm = al.buf(tag + "pcm", flat.size, np.float32, flat)
        nsb = al.buf(tag + "n_samples", N, np.int64, ns) if n_samples else None
        frb = None if frames is None else al.buf(tag + "frames", N, np.int64, np.asarray(frames, np.int64))
        T_max = num_frames(L_max)
        shape = (N, C) if last_only else (N, T_max, C)
        probs = al.buf(tag + "probs", shape, np.float32, "sentinel", promised="all")
        logits = al.buf(tag + "logits", shape, np.float32, "sentinel", promised="all") if want_logits else None
        h = c = None
        if state is not None:
            h = al.buf(tag + "h", (N, 128), np.float32, np.ascontiguousarray(state[0], np.float32))
            c = al.buf(tag + "c", (N, 128), np.float32, np.ascontiguousarray(state[1], np.float32))
        self.lib.call("howl_lstm_stream_chunks", ctypes.byref(self.lstm), ctypes.byref(self.head), al.ptr(pcm), ld, N, L_max, al.ptr(nsb),
                      al.ptr(frb), al.ptr(self.fbp), 40, 1e-7, al.ptr(self.zm) if zmuv else None, al.ptr(h), al.ptr(c), C,
                      1 if last_only else 0, al.ptr(probs), al.ptr(logits), int(np.prod(shape[1:])), None)
        al.sync()
        out_state = None if state is None else (al.get(h).copy(), al.get(c).copy())
        return al.get(probs).copy(), None if logits is None else al.get(logits).copy(), out_state

    def eager(self, clip, frames=None, state=None, last_only=False, zmuv=True, tag="eager."):
        """The launch chain of today on ONE clip: howl_logmel_fwd (layout (1, T, M), ZMUV fused) -> howl_lstm_fwd (B = 1: the
        four-sequence kernel with the input projection in the step) -> howl_head_fwd -> (logits (frames, C) or (C,), hT, cT)."""
        al, lib, C = self.al, self.lib, self.C
        L = len(clip)
        T = num_frames(L)
        fr = T if frames is None else int(frames)
        pcm = al.buf(tag + "pcm", L, np.float32, np.ascontiguousarray(clip, np.float32))
        feat = al.buf(tag + "feat", (1, T, 40), np.float32, "sentinel", promised="all")
        lib.call("howl_logmel_fwd", al.ptr(pcm), 1, L, L, al.ptr(self.fbp), 40, 1e-7, al.ptr(self.zm) if zmuv else None, al.ptr(feat), 1, None)
        lnb = al.buf(tag + "lengths", 1, np.int64, np.array([fr], np.int64))
        gx = al.buf(tag + "gx", (1, fr, 512), np.float32, "sentinel")
        gates = al.buf(tag + "gates", (1, fr, 512), np.float32, "sentinel")
        cc = al.buf(tag + "c_saved", (1, fr, 128), np.float32, "sentinel")
        hseq = al.buf(tag + "hseq", (1, fr + 1, 128), np.float32, "sentinel")
        sv = HowlLstmSaved(al.ptr(gx), al.ptr(gates), al.ptr(cc), al.ptr(hseq), None, fr, T)
        hT = al.buf(tag + "hT", (1, 128), np.float32, "sentinel", promised="all")
        cT = al.buf(tag + "cT", (1, 128), np.float32, "sentinel", promised="all")
        h0 = c0 = None
        if state is not None:
            h0 = al.buf(tag + "h0", (1, 128), np.float32, np.ascontiguousarray(state[0], np.float32))
            c0 = al.buf(tag + "c0", (1, 128), np.float32, np.ascontiguousarray(state[1], np.float32))
        nws = int(lib.cdll.howl_lstm_workspace_bytes(1, fr))
        ws = al.buf(tag + "ws", nws, np.uint8, "sentinel")
        lib.call("howl_lstm_fwd", ctypes.byref(self.lstm), al.ptr(feat), 1, fr, 40, al.ptr(lnb), al.ptr(h0), al.ptr(c0), ctypes.byref(sv),
                 al.ptr(hT), al.ptr(cT), al.ptr(ws), nws, None)
        rows = 1 if last_only else fr
        y1 = al.buf(tag + "y1", (rows, 256), np.float32, "sentinel", promised="all")
        y2 = al.buf(tag + "y2", (rows, C), np.float32, "sentinel", promised="all")
        if last_only:
            lib.call("howl_head_fwd", ctypes.byref(self.head), al.ptr(hT), 1, 0, 128, 1, 128, 256, C, al.ptr(y1), al.ptr(y2), None)
        else:
            h1 = ctypes.c_void_p(al.ptr(hseq).value + 128 * 4)          # rows t = hseq[0][t + 1]
            lib.call("howl_head_fwd", ctypes.byref(self.head), h1, fr, (fr + 1) * 128, 128, fr, 128, 256, C, al.ptr(y1), al.ptr(y2), None)
        al.sync()
        y = al.get(y2).copy()
        return (y[0] if last_only else y), al.get(hT)[0].copy(), al.get(cT)[0].copy()

    def oracle(self, clip, frames=None, state=None, last_only=False, zmuv=True):
        """oracle.frontend + oracle.models in float64 -> (logits (frames, C) or (C,), h (128,), c (128,))."""
        return oracle64(self.sd, clip, self.pair if zmuv else None, frames, state, last_only)


def oracle64(sd, clip, pair, frames=None, state=None, last_only=False):
    x = fe.standard_audio_transform(torch.from_numpy(np.ascontiguousarray(clip, np.float32)).double().unsqueeze(0),
                                    fe.mel_fb(40).double(), mels_only=True)
    if pair is not None:
        x = (x - float(pair[0])) / float(pair[1])
    fr = x.shape[-1] if frames is None else int(frames)
    sd64 = {k: v.double() for k, v in sd.items()}
    hx = None
    if state is not None:
        hx = (torch.from_numpy(np.asarray(state[0], np.float64)).reshape(1, 1, 128), torch.from_numpy(np.asarray(state[1], np.float64)).reshape(1, 1, 128))
    fwd = om.lstm_forward if last_only else om.seq_lstm_forward
    y, (h, c) = fwd(sd64, x.unsqueeze(1), torch.tensor([fr]), hx)
    y = y[0] if last_only else y[:, 0]
    return y.numpy(), h[0, 0].numpy(), c[0, 0].numpy()


def check_case(al, lib, lengths, C, state=False, zmuv=True, last_only=False, seed=0, what="", model=None):
    """Item 1: N ragged clips in one launch against the fp64 oracle, with the eager chain's own error as the yardstick -- on the
    logits of the valid rows and on the returned (h, c); rows past a stream's frame count exactly zero; probs == softmax of the
    launch's own logits."""
    from howl_amd.utils.synth import synthetic_pcm
    N = len(lengths)
    m = model or Model(al, lib, random_state(C, 1000 + 17 * C + seed))
    pcm = synthetic_pcm(N, max(lengths), seed=seed + N).numpy().astype(np.float32)
    clips = [pcm[i, :n].copy() for i, n in enumerate(lengths)]
    frames = [compute_lengths(n) for n in lengths] if last_only else None
    rng = np.random.default_rng(seed)
    st = (0.5 * rng.standard_normal((N, 128)).astype(np.float32), 0.5 * rng.standard_normal((N, 128)).astype(np.float32)) if state else None
    # the returned state is always asked for: a zero start is the NULL pair's meaning spelled out
    st_in = st if st is not None else (np.zeros((N, 128), np.float32), np.zeros((N, 128), np.float32))
    probs, logits, (h, c) = m.chunks(clips, frames=frames, state=st_in, last_only=last_only, zmuv=zmuv, tag=what)
    e_fused = e_eager = s_fused = s_eager = 0.0
    for i, clip in enumerate(clips):
        fr = frames[i] if last_only else num_frames(len(clip))
        sti = None if st is None else (st[0][i], st[1][i])
        ey, eh, ec = m.eager(clip, frames[i] if last_only else None, sti, last_only, zmuv, tag=f"{what}eager{i}.")
        oy, oh, oc = m.oracle(clip, frames[i] if last_only else None, sti, last_only, zmuv)
        mine = logits[i] if last_only else logits[i, :fr]
        e_fused, e_eager = max(e_fused, np.abs(mine - oy).max()), max(e_eager, np.abs(ey - oy).max())
        s_fused = max(s_fused, np.abs(h[i] - oh).max(), np.abs(c[i] - oc).max())
        s_eager = max(s_eager, np.abs(eh - oh).max(), np.abs(ec - oc).max())
        if not last_only:
            assert not probs[i, fr:].any() and not logits[i, fr:].any(), f"stream {i}: rows past frame {fr} are not zero"
        p = probs[i] if last_only else probs[i, :fr]
        assert np.abs(p - softmax64(mine)).max() <= 1e-6, np.abs(p - softmax64(mine)).max()
        assert np.abs(p.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    print(f"lstm stream vs oracle: {what} N={N} lengths={list(lengths)} C={C} state={state} zmuv={zmuv} last_only={last_only}: "
          f"logits e_fused={e_fused:.3e} e_eager={e_eager:.3e}; (h, c) e_fused={s_fused:.3e} e_eager={s_eager:.3e}")
    assert e_fused <= 2 * e_eager + 1e-6, f"logits: e_fused={e_fused:.3e} > 2 * e_eager ({e_eager:.3e}) + 1e-6"
    assert s_fused <= 2 * s_eager + 1e-6, f"(h, c): e_fused={s_fused:.3e} > 2 * e_eager ({s_eager:.3e}) + 1e-6"
    al.check()
    return e_fused, e_eager, s_fused, s_eager


def check_state_carry(al, lib, golden, C=5):
    """Item 2: G15's sequence clips cut 32000 + the rest: chunk A from a zero state, chunk B from the returned state, from PCM,
    against the eager chain carrying its own (hT, cT) the same way (what model.streaming() does) and against the fp64 oracle."""
    audio = np.asarray(golden("g15_whole_clips_seq_lstm")["audio"], np.float32)
    N = audio.shape[0]
    m = Model(al, lib, random_state(C, 515))
    A, B = [a[:32000].copy() for a in audio], [a[32000:].copy() for a in audio]
    zero = (np.zeros((N, 128), np.float32), np.zeros((N, 128), np.float32))
    _, la, sa = m.chunks(A, state=zero, tag="A.")
    pb, lb, sb = m.chunks(B, state=sa, tag="B.")
    e_fused = e_eager = s_fused = s_eager = 0.0
    for i in range(N):
        ea, eh, ec = m.eager(A[i], tag=f"eagerA{i}.")
        eb, eh2, ec2 = m.eager(B[i], state=(eh, ec), tag=f"eagerB{i}.")
        oa, oh, oc = m.oracle(A[i])
        ob, oh2, oc2 = m.oracle(B[i], state=(oh, oc))
        e_fused = max(e_fused, np.abs(la[i] - oa).max(), np.abs(lb[i] - ob).max())
        e_eager = max(e_eager, np.abs(ea - oa).max(), np.abs(eb - ob).max())
        s_fused = max(s_fused, np.abs(sb[0][i] - oh2).max(), np.abs(sb[1][i] - oc2).max())
        s_eager = max(s_eager, np.abs(eh2 - oh2).max(), np.abs(ec2 - oc2).max())
    print(f"lstm stream state carry (G15, 32000 + 32000): logits e_fused={e_fused:.3e} e_eager={e_eager:.3e}; "
          f"(h, c) e_fused={s_fused:.3e} e_eager={s_eager:.3e}")
    assert e_fused <= 2 * e_eager + 1e-6 and s_fused <= 2 * s_eager + 1e-6, (e_fused, e_eager, s_fused, s_eager)
    assert np.abs(pb - softmax64(lb)).max() <= 1e-6
    al.check()
    return e_fused, e_eager, s_fused, s_eager


def check_independence(al, lib, C=5):
    """Item 3: a stream's outputs and carried state are the same bits launched alone, as any of the four rows of a workgroup and
    at another index of a 9-stream batch; a repeated launch repeats them."""
    from howl_amd.utils.synth import synthetic_pcm
    m = Model(al, lib, random_state(C, 33))
    lengths = [4321, 3200, 8000, 400, 6600, 1000, 3400, 7000, 5000]
    pcm = synthetic_pcm(9, 8000, seed=5).numpy().astype(np.float32)
    clips = [pcm[i, :n].copy() for i, n in enumerate(lengths)]
    rng = np.random.default_rng(3)
    st = (0.3 * rng.standard_normal((9, 128)).astype(np.float32), 0.3 * rng.standard_normal((9, 128)).astype(np.float32))
    probs, logits, (h, c) = m.chunks(clips, state=st, tag="all.")
    again = m.chunks(clips, state=st, tag="again.")
    assert np.array_equal(probs, again[0]) and np.array_equal(logits, again[1]) and np.array_equal(h, again[2][0]) and np.array_equal(c, again[2][1])
    target, fr = clips[0], num_frames(lengths[0])
    s0 = (st[0][:1], st[1][:1])

    def same(p, l, hc, k, what):
        assert np.array_equal(p[k, :fr], probs[0, :fr]) and np.array_equal(l[k, :fr], logits[0, :fr]), what
        assert np.array_equal(hc[0][k], h[0]) and np.array_equal(hc[1][k], c[0]), what
    p1, l1, hc1 = m.chunks([target], state=s0, tag="solo.")
    same(p1, l1, hc1, 0, "alone")
    for row in range(1, 4):      # as row `row` of one workgroup, among other clips
        group = [clips[1 + j] for j in range(row)] + [target]
        stg = (np.concatenate([st[0][1:1 + row], s0[0]]), np.concatenate([st[1][1:1 + row], s0[1]]))
        pg, lg, hcg = m.chunks(group, state=stg, tag=f"row{row}.")
        same(pg, lg, hcg, row, f"row {row} of a workgroup")
    order = list(range(1, 9)) + [0]      # index 8 of a 9-stream batch: alone in the third workgroup
    pm, lm, hcm = m.chunks([clips[i] for i in order], state=(st[0][order], st[1][order]), tag="moved.")
    same(pm, lm, hcm, 8, "index 8 of 9")
    assert np.isfinite(probs).all() and np.abs(logits[0, :3] - logits[1, :3]).max() > 0      # the streams differ
    al.check()


def check_out_of_contract(al, lib, C=3):
    """Item 7: n_samples / frames outside their contract are clamped inside the kernel (400 .. L_max, 1 .. T_n): nothing outside
    the stream's rows is read or written, every promised element is written."""
    from howl_amd.utils.synth import synthetic_pcm
    m = Model(al, lib, random_state(C, 77))
    L_max, N = 4321, 5
    pcm = synthetic_pcm(N, L_max, seed=9).numpy().astype(np.float32)
    clips = [pcm[i].copy() for i in range(N)]
    ns = np.array([100, 10 ** 6, -5, 400, L_max], np.int64)
    fr = np.array([0, 10 ** 4, 2, -1, 7], np.int64)
    nsb = al.buf("bad.n_samples", N, np.int64, ns)
    frb = al.buf("bad.frames", N, np.int64, fr)
    flat = pcm.reshape(-1)
    pb = al.buf("bad.pcm", flat.size, np.float32, flat)
    T_max = num_frames(L_max)
    probs = al.buf("bad.probs", (N, T_max, C), np.float32, "sentinel", promised="all")
    logits = al.buf("bad.logits", (N, T_max, C), np.float32, "sentinel", promised="all")
    h = al.buf("bad.h", (N, 128), np.float32, 0.0)
    c = al.buf("bad.c", (N, 128), np.float32, 0.0)
    lib.call("howl_lstm_stream_chunks", ctypes.byref(m.lstm), ctypes.byref(m.head), al.ptr(pb), L_max, N, L_max, al.ptr(nsb), al.ptr(frb),
             al.ptr(m.fbp), 40, 1e-7, al.ptr(m.zm), al.ptr(h), al.ptr(c), C, 0, al.ptr(probs), al.ptr(logits), T_max * C, None)
    al.sync()
    got = al.get(probs)
    want_ns = np.clip(ns, 400, L_max)
    want_fr = np.clip(fr, 1, 1 + want_ns // HOP)
    ref, _, _ = m.chunks([clips[i][:want_ns[i]] for i in range(N)], frames=want_fr, tag="clamped.", L_max=L_max,
                         state=(np.zeros((N, 128), np.float32), np.zeros((N, 128), np.float32)))
    assert np.array_equal(got, ref)
    for i in range(N):
        assert got[i, :want_fr[i]].all() and not got[i, want_fr[i]:].any(), i
    al.check()


# ---- module level: the same code on the device and, inside emu_util.emulated_package(), on the emulator -------------------------

def _zmuv(golden, dev):
    from howl_amd.data.transform.operator import ZmuvTransform
    g4 = golden("g4_zmuv")
    zmuv = ZmuvTransform().to(dev)
    for k in ("mean", "mean2", "total"):
        getattr(zmuv, k).copy_(torch.from_numpy(np.asarray(g4[k])))
    return zmuv


def seq_engine(golden, dev, sd, words=("hey", "fire", "fox"), fused=None):
    from howl_amd.context import InferenceContext
    from howl_amd.model import RegisteredModel
    from howl_amd.model.inference import InferenceEngine
    ctx = InferenceContext(list(words), token_type="word", use_blank=True)
    model = RegisteredModel.find_registered_class("seq-lstm")(ctx.num_labels)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model = model.to(dev).eval().streaming()
    engine = InferenceEngine(model, _zmuv(golden, dev), ctx)
    if fused is not None:
        engine.fused_chunks = fused
    engine.std = engine.std.to(dev)
    return engine


def top2_margin(sd, clip, pair):
    """Smallest gap between the two largest fp64 oracle probabilities over the frames of a clip."""
    y, _, _ = oracle64(sd, clip, pair)
    p = np.sort(softmax64(y), -1)
    return float((p[:, -1] - p[:, -2]).min())


CHAIN = ("howl_logmel_fwd", "howl_lstm_fwd", "howl_head_fwd")


def check_g8_history(golden, dev, library):
    """Item 4: with fused_chunks on, InferenceEngine.infer reproduces golden g8_seq_engine's label history (81 frames, all label
    0; the fp64 oracle's smallest top-2 probability gap is 7.48e-3, five orders above the fp32 paths' error: a plumbing check) as exactly ONE howl_lstm_stream_chunks and nothing of the launch chain."""
    from stream_util import CallLog
    from howl_amd.settings import SETTINGS
    g = golden("g8_seq_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    SETTINGS.inference_engine.smoothing_window_ms = 0
    try:
        sd = om.lstm_init(int(g["num_labels"]))
        clip = np.asarray(g["clip"], np.float32)
        margin = top2_margin(sd, clip, g4_pair())
        print(f"g8_seq_engine: fp64 top-2 margin {margin:.3e}")
        assert margin >= 7e-3, margin      # (7.48e-3 on the oracle; what matters is that it dwarfs the ~1e-7 error of either path)
        engine = seq_engine(golden, dev, sd, fused=True)
        with CallLog(library) as log:
            present = engine.infer(torch.from_numpy(clip).to(dev))
        assert bool(present) == bool(g["present"])
        hist = np.array(engine.label_history, dtype=np.float64)
        assert hist.shape == g["label_history"].shape
        assert np.array_equal(hist[:, 1], g["label_history"][:, 1])
        assert np.abs(hist[:, 0] - g["label_history"][:, 0]).max() < 1e-6
        assert log.names.count("howl_lstm_stream_chunks") == 1 and not any(n in log.names for n in CHAIN), log.names
        assert engine.model.streaming_state is not None and tuple(engine.model.streaming_state[0].shape) == (1, 1, 128)
        # fused and eager calls alternate on one engine: the eager call starts from the state the fused one left, and the other way
        engine.fused_chunks = False
        with CallLog(library) as log:
            engine.infer(torch.from_numpy(clip[:8000]).to(dev))
        assert [n for n in log.names if n in CHAIN] == list(CHAIN) and "howl_lstm_stream_chunks" not in log.names, log.names
        engine.fused_chunks = True
        with CallLog(library) as log:
            engine.infer(torch.from_numpy(clip[8000:]).to(dev))
        assert log.names.count("howl_lstm_stream_chunks") == 1 and not any(n in log.names for n in CHAIN), log.names
    finally:
        SETTINGS.reset()


def infer_many_inputs():
    """The issue's inputs: seeded default initialisation with the recurrence and the last layer scaled up (decisive, varied
    argmax), 5 labels with blank 4, eight clips of 48000 .. 400 samples."""
    from howl_amd.utils.synth import synthetic_pcm
    from howl_amd.model import RegisteredModel
    torch.manual_seed(2024)
    model = RegisteredModel.find_registered_class("seq-lstm")(5)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd["lstm.weight_ih_l0"] *= 3
    sd["lstm.weight_hh_l0"] *= 3
    sd["dnn.2.weight"] *= 60
    pcm = synthetic_pcm(8, 48000, seed=77)
    sizes = [48000, 40000, 33333, 16000, 8000, 4321, 1000, 400]
    return sd, [pcm[i, :n].clone() for i, n in enumerate(sizes)]


def check_infer_many(golden, dev, library):
    """Item 4: infer_many(clips) gives the results and the per-clip label_history of the eager [reset(); infer(clip)], exactly, with
    no frame left out -- after asserting on the fp64 oracle that the inputs do provide the >= 1e-4 top-2 margin that makes exact
    equality a fair demand -- as ONE launch."""
    from stream_util import CallLog
    sd, clips = infer_many_inputs()
    pair = g4_pair()
    frames, labels, worst = 0, set(), 1.0
    for c in clips:
        y, _, _ = oracle64(sd, c.numpy(), pair)
        p = np.sort(softmax64(y), -1)
        worst = min(worst, float((p[:, -1] - p[:, -2]).min()))
        frames += len(y)
        labels |= set(y.argmax(-1).tolist())
    print(f"infer_many inputs: {frames} frames, fp64 top-2 margin {worst:.3e}, argmax labels {sorted(labels)}")
    assert frames == 762 and worst >= 1e-4 and len(labels) >= 3, (frames, worst, labels)
    engine = seq_engine(golden, dev, sd, fused=False)
    assert engine.blank_idx == 4 and engine.context.num_labels == 5
    dclips = [c.to(dev) for c in clips]
    want, hists = [], []
    for c in dclips:
        engine.reset()
        want.append(bool(engine.infer(c)))
        hists.append(list(engine.label_history))
    engine.reset()
    engine.fused_chunks = True
    with CallLog(library) as log:
        got = engine.infer_many(dclips)
    assert log.names.count("howl_lstm_stream_chunks") == 1 and not any(n in log.names for n in CHAIN), log.names
    assert got == want, (got, want)
    assert len(engine.clip_histories) == len(hists)
    for i, (a, b) in enumerate(zip(engine.clip_histories, hists)):
        assert a == b, f"clip {i}: label history differs"
    assert sum(len(h) for h in hists) > 0
    assert engine.model.streaming_state is None and engine.label_history == []      # left reset
    # a clip outside the kernel's range (fewer than 400 samples) makes the call the plain loop of infer: clip by clip, each on the
    # path that applies to it
    with CallLog(library) as log:
        engine.infer_many([dclips[-1], dclips[-1][:300]])
    assert log.names.count("howl_lstm_stream_chunks") == 1 and [n for n in log.names if n in CHAIN] == list(CHAIN), log.names


def check_switch_default(golden, dev, library, monkeypatch):
    """Item 4: with the switch unset fused_chunks is False and the call log of infer is today's."""
    from stream_util import CallLog
    from howl_amd.model.inference import InferenceEngine
    monkeypatch.delenv("HOWL_STREAM_FUSED", raising=False)
    e = seq_engine(golden, dev, om.lstm_init(5))
    assert e.fused_chunks is False
    with CallLog(library) as log:
        e.infer(torch.from_numpy(np.asarray(golden("g8_seq_engine")["clip"], np.float32)).to(dev))
    # (the first call of a fresh engine also builds the filterbank and the ZMUV pair, as it always did)
    assert [n for n in log.names if n in CHAIN or "stream" in n] == list(CHAIN), log.names
    monkeypatch.setenv("HOWL_STREAM_FUSED", "1")
    assert InferenceEngine(e.model, e.zmuv, e.context).fused_chunks is True
    monkeypatch.setenv("HOWL_STREAM_FUSED", "0")
    assert InferenceEngine(e.model, e.zmuv, e.context).fused_chunks is False


def check_frame_engine_lstm(golden, dev, library, C=4, windows=4):
    """Item 5: FrameInferenceEngine.ingest_frame on an `lstm` model: the fused window against the eager one, window by window, with
    the fp64 oracle's probabilities as the reference (e_fused <= 2 e_eager + 1e-6), one launch per window."""
    from stream_util import CallLog
    from howl_amd.context import InferenceContext
    from howl_amd.model import RegisteredModel
    from howl_amd.model.inference import FrameInferenceEngine
    from howl_amd.utils.synth import synthetic_pcm
    sd = random_state(C, 91)
    ctx = InferenceContext(["hey", "fire", "fox"], token_type="word")
    assert ctx.num_labels == C
    model = RegisteredModel.find_registered_class("lstm")(C)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model = model.to(dev).eval().streaming()
    engine = FrameInferenceEngine(500, 63, model, _zmuv(golden, dev), ctx)
    engine.std = engine.std.to(dev)
    clip = synthetic_pcm(1, 8000 + 1008 * windows, seed=21)[0]
    seen = []
    real = engine._append_probability_frame

    def record(prediction, curr_time=None):
        seen.append(np.array(prediction, np.float64))
        return real(prediction, curr_time=curr_time)
    engine._append_probability_frame = record
    pair = g4_pair()
    assert int(engine.std.compute_lengths(torch.tensor([8000]))) == compute_lengths(8000) == 38
    e_fused = e_eager = 0.0
    for i in range(windows):
        w = clip[i * 1008: i * 1008 + 8000]
        y, _, _ = oracle64(sd, w.numpy(), pair, frames=compute_lengths(8000), last_only=True)
        ref = softmax64(y)
        engine.fused_windows = False
        with CallLog(library) as log:
            engine.ingest_frame(w.to(dev), curr_time=63.0 * i)
        assert [n for n in log.names if n in CHAIN] == list(CHAIN), log.names
        engine.fused_windows = True
        with CallLog(library) as log:
            engine.ingest_frame(w.to(dev), curr_time=63.0 * i)
        assert log.names.count("howl_lstm_stream_chunks") == 1 and not any(n in log.names for n in CHAIN), log.names
        e_eager, e_fused = max(e_eager, np.abs(seen[-2] - ref).max()), max(e_fused, np.abs(seen[-1] - ref).max())
    print(f"frame engine with lstm: probabilities e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
    assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
    # with the switch off nothing changes; training mode keeps the chain
    assert engine._fused_session(clip[:8000].to(dev)) is not None
    # a window inside the kernel's range but without one whole 512-sample frame (compute_lengths < 1) is the chain's business
    assert engine._fused_session(clip[:500].to(dev)) is None and engine._fused_session(clip[:512].to(dev)) is not None
    model.train()
    assert engine._fused_session(clip[:8000].to(dev)) is None
    model.eval()


def check_streaming_alternation(golden, dev, clips=2, C=5):
    """Item 2 through the Python plumbing: G15's sequence clips cut 32000 + the rest on a `seq-lstm` in .eval().streaming().  The
    eager model on chunk A then chunk B is the yardstick; against it and the fp64 oracle: (i) session.probabilities(A) then
    probabilities(B, state=returned) -- the session's own pair, advanced in place; (ii) eager A, then fused B from
    model.streaming_state -- a foreign pair, copied; (iii) fused A, its state assigned to model.streaming_state, then eager B.
    Logits of both chunks and the final state within e_fused <= 2 e_eager + 1e-6; the final state bit-equal to the eager one's (the
    eager chain at B = 1 runs the same recurrence step).  Then the same two hand-overs through InferenceEngine.infer with the
    switch flipped between the chunks: model.streaming_state afterwards is the eager engine's, bit for bit."""
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    audio = np.asarray(golden("g15_whole_clips_seq_lstm")["audio"], np.float32)[:clips]
    sd = random_state(C, 515)
    model = RegisteredModel.find_registered_class("seq-lstm")(C)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model = model.to(dev).eval().streaming()
    std = StandardAudioTransform().to(dev).eval()
    zmuv = _zmuv(golden, dev)
    session = model.stream_session(std, zmuv)
    pair = g4_pair()

    def eager(chunk):
        with torch.no_grad():
            y = model(std.log_mel_for_model(chunk.unsqueeze(0), zmuv), None)      # reads and assigns model.streaming_state
        return y[:, 0].cpu().numpy()

    def fused(chunk, state):
        T = num_frames(chunk.numel())
        logits = torch.empty((1, T, C), dtype=torch.float32, device=dev)
        probs, state = session.probabilities(chunk.reshape(1, -1), state=state, logits=logits)
        assert np.abs(probs.cpu().numpy() - softmax64(logits.cpu().numpy())).max() <= 1e-6
        return logits[0].cpu().numpy(), state

    def host(state):
        assert tuple(state[0].shape) == (1, 1, 128) and tuple(state[1].shape) == (1, 1, 128)
        return state[0].cpu().numpy().reshape(128).copy(), state[1].cpu().numpy().reshape(128).copy()

    worst = {}
    for i in range(clips):
        A, B = torch.from_numpy(audio[i, :32000].copy()).to(dev), torch.from_numpy(audio[i, 32000:].copy()).to(dev)
        oa, oh, oc = oracle64(sd, audio[i, :32000], pair)
        ob, oh2, oc2 = oracle64(sd, audio[i, 32000:], pair, state=(oh, oc))
        runs = {}
        model.streaming_state = None
        ea, mid = eager(A), host(model.streaming_state)
        eb = eager(B)
        runs["eager"] = (ea, eb, host(model.streaming_state))
        la, st = fused(A, None)                                        # (i)
        mid_i = host(st)
        lb, st2 = fused(B, st)
        assert st2[0] is st[0] and st2[1] is st[1]
        runs["i"] = (la, lb, host(st2))
        model.streaming_state = None                                   # (ii)
        ea2 = eager(A)
        lb2, st = fused(B, model.streaming_state)
        runs["ii"] = (ea2, lb2, host(st))
        la3, st = fused(A, None)                                       # (iii)
        model.streaming_state = st
        eb3 = eager(B)
        runs["iii"] = (la3, eb3, host(model.streaming_state))
        assert np.array_equal(mid_i[0], mid[0]) and np.array_equal(mid_i[1], mid[1]), "state behind chunk A differs from the eager one"
        assert np.abs(mid[0] - mid[1]).max() > 1e-3      # h and c are different things: a swap would show
        for name, (ya, yb, (h, c)) in runs.items():
            e = max(np.abs(ya - oa).max(), np.abs(yb - ob).max())
            se = max(np.abs(h - oh2).max(), np.abs(c - oc2).max())
            worst[name] = (max(worst.get(name, (0, 0))[0], e), max(worst.get(name, (0, 0))[1], se))
            if name != "eager":
                assert np.array_equal(h, runs["eager"][2][0]) and np.array_equal(c, runs["eager"][2][1]), f"path ({name}): final state"
    print("streaming alternation (G15, 32000 + 32000): " + "; ".join(f"{k}: logits e={v[0]:.3e} (h, c) e={v[1]:.3e}" for k, v in worst.items()))
    for name in ("i", "ii", "iii"):
        assert worst[name][0] <= 2 * worst["eager"][0] + 1e-6 and worst[name][1] <= 2 * worst["eager"][1] + 1e-6, (name, worst)
    # the same hand-overs through the engine
    engine = seq_engine(golden, dev, sd, fused=False)
    engine.sequence = [0, 1, 2, 0, 1, 2]      # never present: every call walks all of its frames
    A, B = torch.from_numpy(audio[0, :32000].copy()).to(dev), torch.from_numpy(audio[0, 32000:].copy()).to(dev)
    finals, hists = {}, {}
    for name, switches in (("eager", (False, False)), ("fused", (True, True)), ("eager-fused", (False, True)), ("fused-eager", (True, False))):
        engine.reset()
        for chunk, on in zip((A, B), switches):
            engine.fused_chunks = on
            engine.infer(chunk)
        finals[name], hists[name] = host(engine.model.streaming_state), list(engine.label_history)
    for name in ("fused", "eager-fused", "fused-eager"):
        assert np.array_equal(finals[name][0], finals["eager"][0]) and np.array_equal(finals[name][1], finals["eager"][1]), name
        assert len(hists[name]) == len(hists["eager"]), name
    return worst


def check_session(golden, dev, C=5):
    """The session's own contract: shapes, the carried state in model.streaming_state's shape, refusal of training mode and of a
    train-mode (VTLP) frontend."""
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.utils.synth import synthetic_pcm
    model = RegisteredModel.find_registered_class("seq-lstm")(C)
    model.load_state_dict({k: v.clone() for k, v in random_state(C, 12).items()})
    model = model.to(dev).eval()
    std = StandardAudioTransform().to(dev).eval()
    session = model.stream_session(std, _zmuv(golden, dev))
    assert session.supported(8000) and session.supported(400) and not session.supported(399) and not session.supported(1638400)
    pcm = synthetic_pcm(3, 4321).to(dev)
    probs, state = session.probabilities(pcm)
    assert tuple(probs.shape) == (3, 22, C) and tuple(state[0].shape) == (1, 3, 128) and tuple(state[1].shape) == (1, 3, 128)
    probs2, state2 = session.probabilities(pcm, state=state)      # advanced in place: the session's own tensors
    assert state2[0] is state[0] and not torch.equal(probs, probs2)
    none_probs, none_state = session.probabilities(pcm, return_state=False)
    assert none_state is None and torch.equal(none_probs, probs)
    model.train()
    try:
        session.probabilities(pcm)
    except RuntimeError as e:
        assert "eval" in str(e)
    else:
        raise AssertionError("training mode must raise")
    model.eval()
    std.train()
    if std.augment_params[0].enabled:
        assert not session.supported(8000)
    std.augment_params[0].enabled = True
    assert not session.supported(8000)
    try:
        session.probabilities(pcm)
    except ValueError as e:
        assert "range" in str(e)
    else:
        raise AssertionError("a train-mode (VTLP) frontend must be refused")
