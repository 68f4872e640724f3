"""Shared by tests/test_emu_gru_stream.py (hipemu, guarded host buffers) and tests/test_gpu_gru_stream.py (device, sentinel bands):
the streaming gru entry points of include/howl_hip_gru_stream.h called through an allocator of tests/guard_mem.py, the eager chain
(howl_logmel_fwd with the ZMUV pair + howl_gru_fwd in eval mode) on the same library, the float64 oracle (oracle.frontend +
tests/gru_util.py's RefGru), and the module-level checks (session, engine) that run unchanged on either side."""
import ctypes

import numpy as np
import torch

import gru_util
import stream_util
from stream_util import ZMUV_PAIR, CallLog, softmax64  # noqa: F401
from oracle import frontend as fe

# (N, L, C, variant) of check 1, chosen for the geometry's edges: T = 3 (the halos are wider than the data, 2 steps of 3); T + 4
# even; the client's window (T = 41: the pool drops a column, 21 steps of 22); T = 42 (no column dropped, 21 steps of 23), also run
# to the end (23 of 23); `frames` alone sets the stop (2 steps of 22); 1 s; the largest window and label count (T = 83, 42 steps
# of 43); no ZMUV.  variant: frames = "T" (all T frames) or a number; zmuv = False (zmuv_pair = NULL)
CASES = [(1, 512, 4, {}), (3, 1000, 4, {}), (3, 8000, 12, {}), (2, 8200, 4, {}), (2, 8200, 4, {"frames": "T"}), (3, 8000, 12, {"frames": 1}),
         (3, 8600, 5, {}), (2, 16000, 12, {}), (3, 16599, 64, {}), (2, 8000, 4, {"zmuv": False})]
CASE_IDS = [f"N{N}-L{L}-C{C}" + "".join(f"-{k}{v}" for k, v in var.items()) for N, L, C, var in CASES]
# Not free choices: with seeds 5, 7 or 27 conv2's single output channel is below zero everywhere on synthetic_pcm, the ReLU clamps
# it, and the logits do not depend on the audio at all -- an encoder bug would pass every check.  check_against_oracle asserts on
# the oracle that this is not the case.
SEEDS = {4: 21, 5: 21, 12: 23, 64: 33}
SHARPEN = {"dnn.0.weight": 3.0, "dnn.3.weight": 6.0, "lstm_encoder.weight_ih_l0": 2.0, "lstm_encoder.weight_hh_l0": 2.0}
LIVE = 1e-2      # the oracle's logits must move by more than this with the audio


def frames_of(L):
    """compute_lengths of a window of L samples."""
    return (L - 512) // 200 + 1


def case_frames(L, variant):
    f = variant.get("frames")
    return frames_of(L) if f is None else (1 + L // 200 if f == "T" else int(f))


def sharp_state(C, seed=None):
    """gru_util.make_state with the head and the recurrent weights scaled up, so that the logits spread with the audio."""
    sd = gru_util.make_state(C, SEEDS[C] if seed is None else seed)
    for k, f in SHARPEN.items():
        sd[k] = sd[k] * f
    return sd


def gru_params(al, sd, tag=""):
    """Every parameter and running buffer in a buffer of its own -> (buffers by name, HowlGruParams, HowlGruBuffers)."""
    from howl_amd import lib as L
    bufs = {}
    for k in gru_util.PARAMS + gru_util.BUFFERS:
        a = np.ascontiguousarray(sd[k].numpy())
        bufs[k] = al.buf(tag + k, a.shape if a.ndim else (1,), a.dtype, a)
    prm = L.HowlGruParams(*[al.ptr(bufs[k]) for k in gru_util.PARAMS])
    buf = L.HowlGruBuffers(*[al.ptr(bufs[k]) for k in gru_util.BUFFERS])
    return bufs, prm, buf


class Fused:
    """The streaming entry point on one model: any number of `windows` launches; there is no prepared state."""

    def __init__(self, al, lib, sd, C, tag=""):
        self.al, self.lib, self.C, self.tag = al, lib, C, tag
        self.p, self.prm, self.bnb = gru_params(al, sd, tag)
        self.fbp = stream_util.pack_fb(al, lib, fe.mel_fb(40).numpy())
        self.zm = al.buf(tag + "zmuv", 2, np.float32, ZMUV_PAIR)

    def windows(self, flat, N, L, ld, tag="", want_logits=True, frames=None, zmuv=True, stream=None):
        """`flat`: the samples, window n = flat[n * ld : n * ld + L]; the buffer ends with the last window."""
        al, C = self.al, self.C
        assert flat.size == (N - 1) * ld + L
        pcm = al.buf(tag + "pcm", flat.size, np.float32, flat)
        probs = al.buf(tag + "probs", (N, C), np.float32, "sentinel", promised="all")
        logits = al.buf(tag + "logits", (N, C), np.float32, "sentinel", promised="all") if want_logits else None
        nws = int(self.lib.cdll.howl_gru_stream_workspace_bytes(N, L))
        assert nws > 0 and nws % 16 == 0
        ws = al.buf(tag + "ws", nws // 4, np.float32, "sentinel")      # exactly the size the query returns
        self.lib.call("howl_gru_stream_windows", ctypes.byref(self.prm), ctypes.byref(self.bnb), al.ptr(pcm), ld, N, L,
                      frames_of(L) if frames is None else frames, al.ptr(self.fbp), 40, 1e-7, al.ptr(self.zm) if zmuv else None, C,
                      al.ptr(probs), al.ptr(logits), al.ptr(ws), nws, stream)
        al.sync()
        return al.get(probs).copy(), None if logits is None else al.get(logits).copy()


def eager_logits(al, lib, sd, rows, fbp, zm, frames, tag="eager."):
    """The chain the engine runs today on the same library: howl_logmel_fwd with the ZMUV pair (`zm` None: without) + howl_gru_fwd
    in eval mode (gru_util.run_library)."""
    B, L = rows.shape
    T = 1 + L // 200
    pcm = al.buf(tag + "pcm", rows.shape, np.float32, rows)
    lm = al.buf(tag + "logmel", (B, 40, T), np.float32, "sentinel", promised="all")
    lib.call("howl_logmel_fwd", al.ptr(pcm), B, L, L, al.ptr(fbp), 40, 1e-7, al.ptr(zm), al.ptr(lm), 0, None)
    al.sync()
    x = torch.from_numpy(np.array(al.get(lm))).reshape(B, 1, 40, T)
    out = gru_util.run_library(lib, al, sd, x, [frames] * B, 0, x_time_major=True)
    al.sync()
    return out["logits"].numpy()


_ORACLE = {}


def oracle_logits64(sd, rows, frames, pair=ZMUV_PAIR, key=None):
    """oracle.frontend + ZMUV + tests/gru_util.py's RefGru in float64: (N, L) PCM -> (N, C) logits.  `key`: computed once per process
    and shared."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    x = fe.standard_audio_transform(torch.from_numpy(np.ascontiguousarray(rows)).double(), fe.mel_fb(40).double())
    if pair is not None:
        x = (x - float(pair[0])) / float(pair[1])
    out = gru_util.reference(sd, x, [frames] * rows.shape[0], dtype=torch.float64)["logits"].numpy()
    if key is not None:
        _ORACLE[key] = out
    return out


def oracle_liveness(sd, N, L, C, frames, pair, key):
    """How far the oracle's logits move with the audio: between synthetic_pcm(N, L) and synthetic_pcm(N, L, seed=3), and between the
    windows of the first.  Both must exceed LIVE, or the case could not tell a broken encoder from a working one."""
    from howl_amd.utils.synth import synthetic_pcm
    rows = synthetic_pcm(N, L).numpy().astype(np.float32)
    ref = oracle_logits64(sd, rows, frames, pair, key=key)
    other = oracle_logits64(sd, synthetic_pcm(N, L, seed=3).numpy().astype(np.float32), frames, pair, key=key + ("seed3",))
    moved = float(np.abs(ref - other).max(axis=1).min())
    spread = float(np.abs(ref - ref[:1]).max()) if N > 1 else None
    return rows, ref, moved, spread


def check_against_oracle(al, lib, N, L, C, variant=None):
    """Checks 1 and 3: fused logits against the fp64 oracle, bounded by the EAGER chain's own error against the same oracle:
    e_fused <= 2 e_eager + 1e-6 (both are exact-fp32 chains in another summation order); probs = softmax64(logits) and rows summing
    to 1 within 1e-6; every operand's guards intact and exactly [N, C] written (the allocator's check)."""
    variant = variant or {}
    sd = sharp_state(C)
    frames = case_frames(L, variant)
    zmuv = variant.get("zmuv", True)
    pair = ZMUV_PAIR if zmuv else None
    rows, ref, moved, spread = oracle_liveness(sd, N, L, C, frames, pair, key=(N, L, C, frames, zmuv))
    print(f"gru stream oracle: N={N} L={L} C={C} frames={frames} zmuv={zmuv}: moved by {moved:.3e} with the audio, spread over the "
          f"windows {spread if spread is None else format(spread, '.3e')}")
    assert moved > LIVE and (spread is None or spread > LIVE), (moved, spread)
    f = Fused(al, lib, sd, C)
    probs, logits = f.windows(rows.reshape(-1), N, L, L, frames=frames, zmuv=zmuv)
    eager = eager_logits(al, lib, sd, rows, f.fbp, f.zm if zmuv else None, frames)
    e_fused, e_eager = np.abs(logits - ref).max(), np.abs(eager - ref).max()
    print(f"gru stream vs oracle: N={N} L={L} C={C} frames={frames} zmuv={zmuv}: e_fused={e_fused:.3e} e_eager={e_eager:.3e} "
          f"|logits|max={np.abs(ref).max():.3f}")
    assert e_fused <= 2 * e_eager + 1e-6, f"N={N} L={L} C={C}: e_fused={e_fused:.3e} > 2 * e_eager ({e_eager:.3e}) + 1e-6"
    sm = softmax64(logits)
    assert np.abs(probs - sm).max() <= 1e-6, np.abs(probs - sm).max()
    assert np.abs(probs.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    al.check()
    return e_fused, e_eager


def check_independence(al, lib, L=8000, C=4, N=5, ld=1008, many=257):
    """Check 2: window n alone (N = 1) and as row n of N windows, and a repeated launch: the same bits; `many` windows in one launch
    (more workgroups than compute units): rows 0, 1 and many - 1 equal their N = 1 bits and everything is finite."""
    from howl_amd.utils.synth import synthetic_pcm
    sd = sharp_state(C)
    flat = synthetic_pcm(1, (N - 1) * ld + L).numpy().astype(np.float32).reshape(-1)
    f = Fused(al, lib, sd, C)
    probs, logits = f.windows(flat, N, L, ld, "all.")
    probs2, logits2 = f.windows(flat, N, L, ld, "again.")
    assert np.array_equal(probs, probs2) and np.array_equal(logits, logits2)
    assert np.isfinite(probs).all() and np.abs(logits[0] - logits[-1]).max() > 0      # the windows differ
    for n in range(N):
        p1, l1 = f.windows(flat[n * ld:n * ld + L].copy(), 1, L, L, f"solo{n}.")
        assert np.array_equal(p1[0], probs[n]) and np.array_equal(l1[0], logits[n]), n
    if many:
        rows = synthetic_pcm(many, L, seed=3).numpy().astype(np.float32)
        pm, lm = f.windows(rows.reshape(-1), many, L, L, "many.")
        assert np.isfinite(pm).all() and np.isfinite(lm).all()
        for n in (0, 1, many - 1):
            p1, l1 = f.windows(rows[n].copy(), 1, L, L, f"many.solo{n}.")
            assert np.array_equal(p1[0], pm[n]) and np.array_equal(l1[0], lm[n]), n
    al.check()


def check_refusals(al, lib):
    """Check 4: every refusal of include/howl_hip_gru_stream.h on a (N = 2, L = 1000, C = 4) problem: the code, a message that names
    the entry point, nothing launched (probs, logits and the workspace keep their bytes) -- and the next valid call succeeds; the
    `supported` and `workspace_bytes` tables with the zeros at and outside the edges."""
    from howl_amd import lib as LL
    N, L, C = 2, 1000, 4
    T = 1 + L // 200
    sd = sharp_state(C)
    f = Fused(al, lib, sd, C)
    pcm = al.buf("pcm", N * L, np.float32, np.zeros(N * L, np.float32))
    probs = al.buf("probs", (N, C), np.float32, "sentinel")
    logits = al.buf("logits", (N, C), np.float32, "sentinel")
    nws = int(lib.cdll.howl_gru_stream_workspace_bytes(N, L))
    ws = al.buf("ws", nws // 4, np.float32, "sentinel")
    watched = [probs, logits, ws]

    def snapshot():
        al.sync()
        return [np.array(al.get(v)).tobytes() for v in watched]

    def windows(null=None, L=L, M=40, C=C, N=N, frames=frames_of(L), short=False):
        g = lambda name, v: None if null == name else al.ptr(v)      # noqa: E731
        pp = [None if null == k else al.ptr(f.p[k]) for k in gru_util.PARAMS]
        bb = [None if null == k else al.ptr(f.p[k]) for k in gru_util.BUFFERS]
        prm = None if null == "params" else ctypes.byref(LL.HowlGruParams(*pp))
        buf = None if null == "buffers" else ctypes.byref(LL.HowlGruBuffers(*bb))
        return lib.cdll.howl_gru_stream_windows(prm, buf, g("pcm", pcm), L, N, L, frames, g("fbp", f.fbp), M, 1e-7, al.ptr(f.zm), C,
                                                g("probs", probs), al.ptr(logits), g("ws", ws), nws - 4 if short else nws, None)

    stats = [k for k in gru_util.BUFFERS if not k.endswith("num_batches_tracked")]
    cases = [(dict(L=511), -1, "L=511"), (dict(L=16600), -1, "L=16600"), (dict(M=80), -1, "M=80"), (dict(C=0), -1, "C=0"),
             (dict(C=65), -1, "C=65"), (dict(N=0), -1, "N=0"), (dict(N=8193), -1, "N=8193"), (dict(frames=0), -1, "frames=0"),
             (dict(frames=T + 1), -1, f"frames={T + 1}"), (dict(short=True), -3, "workspace too small")] + \
            [(dict(null=k), -1, "null pointer") for k in ["params", "buffers", "pcm", "fbp", "probs", "ws"] + gru_util.PARAMS + stats]
    for kw, code, text in cases:
        before = snapshot()
        rc = windows(**kw)
        msg = lib.cdll.howl_last_error().decode()
        assert rc == code, (kw, rc, msg)
        assert msg.startswith("howl_gru_stream_windows:") and text in msg, (kw, msg)
        assert snapshot() == before, (kw, "a refused call wrote something")
    assert windows() == 0, lib.cdll.howl_last_error().decode()      # the next valid call succeeds
    # bn*_batches is not read: NULL is fine
    assert all(windows(null=k) == 0 for k in gru_util.BUFFERS if k.endswith("num_batches_tracked")), lib.cdll.howl_last_error().decode()
    al.sync()
    assert np.isfinite(np.array(al.get(probs))).all() and np.isfinite(np.array(al.get(logits))).all()
    for Lq, M, Cq, ok in [(8000, 40, 4, 1), (512, 40, 1, 1), (16599, 40, 64, 1), (511, 40, 4, 0), (16600, 40, 4, 0), (8000, 80, 4, 0),
                          (8000, 40, 0, 0), (8000, 40, 65, 0)]:
        assert lib.cdll.howl_gru_stream_supported(Lq, M, Cq) == ok, (Lq, M, Cq)
    for Nq, Lq in [(0, 8000), (8193, 8000), (1, 511), (1, 16600), (-1, 8000)]:
        assert lib.cdll.howl_gru_stream_workspace_bytes(Nq, Lq) == 0, (Nq, Lq)
    for Nq, Lq in [(1, 512), (1, 8000), (8192, 8000), (1, 16599), (3, 16599)]:
        nb = lib.cdll.howl_gru_stream_workspace_bytes(Nq, Lq)
        assert nb > 0 and nb % 16 == 0 and nb == Nq * lib.cdll.howl_gru_stream_workspace_bytes(1, Lq), (Nq, Lq, nb)


# ---- module level: the same code on the device and, inside emu_util.emulated_package(), on the emulator -------------------------

ENGINE_VOCAB = ["hey", "fire", "fox", "one", "two", "three", "four", "five", "six", "seven", "eight"]      # + [OOV]: 12 labels


def gru_engine(golden, dev, fused):
    """A FrameInferenceEngine (500 ms windows, 63 ms stride) over a gru model with the sharpened state for C = 12, seed 23, and the
    ZMUV statistics of golden G4."""
    from howl_amd.context import InferenceContext
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.model.inference import FrameInferenceEngine
    g4 = golden("g4_zmuv")
    ctx = InferenceContext(ENGINE_VOCAB, token_type="word")
    assert ctx.num_labels == 12
    model = RegisteredModel.find_registered_class("gru")(ctx.num_labels)
    model.load_state_dict({k: v.clone() for k, v in sharp_state(12).items()})
    model = model.to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    for k in ("mean", "mean2", "total"):
        getattr(zmuv, k).copy_(torch.from_numpy(np.asarray(g4[k])))
    engine = FrameInferenceEngine(500, 63, model, zmuv, ctx)
    engine.fused_windows = fused
    engine.std = engine.std.to(dev)
    return engine


def windows_of(clip, engine):
    from howl_amd.utils import audio_utils
    starts, chunk = audio_utils.stride_starts(clip.size(-1), engine.max_window_size_ms, engine.eval_stride_size_ms, engine.sample_rate)
    return clip.as_strided((len(starts), chunk), (starts[1] - starts[0], 1)), starts, chunk


def check_engine(golden, dev, library, first=None):
    """Check 5: the G8 clip's 37 windows through ingest_frame, fused and eager: the same label history, exactly one
    howl_gru_stream_windows per window and no frontend / gru launch on the fused path; every window's top-two gap in the fp64
    oracle exceeds 1e-3 (no window is left out of the comparison) and the oracle's labels are not constant; all windows in one
    probabilities() call against window_probabilities(clip): check 1's bound, argmax identical.  `first`: the emulator's form, the
    clip cut behind its first `first` windows (the oracle's conditions still cover all 37)."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        whole = torch.from_numpy(np.asarray(g["clip"]))
        engine = gru_engine(golden, dev, False)
        all_windows, all_starts, chunk = windows_of(whole, engine)
        assert len(all_starts) == 37 and chunk == 8000
        sd = {k: v.detach().cpu() for k, v in engine.model.state_dict().items()}
        pair = engine.zmuv.pair().cpu().numpy()
        ref = softmax64(oracle_logits64(sd, all_windows.numpy(), frames_of(chunk), pair, key="g8"))
        top = np.sort(ref, axis=1)
        gap = (top[:, -1] - top[:, -2]).min()
        labels = ref.argmax(1)
        print(f"G8 clip: smallest top-two gap {gap:.3e}, oracle labels {labels.tolist()}")
        assert gap > 1e-3, gap
        assert len(set(labels.tolist())) > 1      # the history is not constant
        W = 37 if first is None else first
        clip = whole[:all_starts[W - 1] + chunk].contiguous().to(dev)
        ref, labels = ref[:W], labels[:W]
        hist = {}
        for fused in (False, True):
            engine = gru_engine(golden, dev, fused)
            windows, starts, chunk = windows_of(clip, engine)
            assert len(starts) == W
            with CallLog(library) as log:
                for i, s in enumerate(starts):
                    engine.ingest_frame(clip[s:s + chunk], curr_time=float(engine.eval_stride_size_ms * i))
            hist[fused] = np.array(engine.label_history, dtype=np.float64)
            if fused:
                assert log.names.count("howl_gru_stream_windows") == W, log.names
                assert not {"howl_logmel_fwd", "howl_gru_fwd"} & set(log.names), log.names
            else:
                assert log.names.count("howl_gru_fwd") == W and "howl_gru_stream_windows" not in log.names, log.names
        assert hist[True].shape[0] == W and np.array_equal(hist[True], hist[False]), (hist[True], hist[False])
        with CallLog(library) as log:
            fusedp = engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
        assert log.names.count("howl_gru_stream_windows") == 1, log.names
        engine.fused_windows = False
        eager = engine.window_probabilities(clip)
        e_fused, e_eager = np.abs(fusedp - ref).max(), np.abs(eager - ref).max()
        print(f"G8 clip, {W} windows in one launch: e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
        assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
        assert np.array_equal(fusedp.argmax(1), eager.argmax(1)) and np.array_equal(fusedp.argmax(1), labels)
    finally:
        SETTINGS.reset()


def check_session(dev, L=2000, C=4, N=2):
    """Check 6: the session reads the model in place, so the next call answers for the new weights with no refresh, after
    load_state_dict and after an in-place write that torch's version counters do not see (check 1's criterion, the eager module
    path as the yardstick); training mode raises; supported() follows the range, 80 mel bins and a train-mode VTLP frontend."""
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.utils.synth import synthetic_pcm
    first, other = sharp_state(C, 21), sharp_state(C, 23)
    model = RegisteredModel.find_registered_class("gru")(C)
    model.load_state_dict({k: v.clone() for k, v in first.items()})
    model = model.to(dev).eval()
    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    rows = synthetic_pcm(N, L)
    pcm = rows.to(dev)
    zmuv.update(std(pcm))
    pair = zmuv.pair().cpu().numpy()
    session = model.stream_session(std, zmuv)
    assert not hasattr(session, "refresh")
    assert session.supported(L) and session.supported(512) and session.supported(16599)
    assert not session.supported(511) and not session.supported(16600)
    frames = frames_of(L)
    lengths = torch.full((N,), frames, dtype=torch.int64)

    def both():
        logits = torch.empty((N, C), dtype=torch.float32, device=dev)
        probs = session.probabilities(pcm, logits=logits)
        with torch.no_grad():
            eager = model(std.log_mel_for_model(pcm, zmuv), lengths)
        return probs.cpu().numpy(), logits.cpu().numpy(), eager.cpu().numpy()

    def verdict(sd, what):
        probs, logits, eager = both()
        ref = oracle_logits64(sd, rows.numpy(), frames, pair)
        e_fused, e_eager = np.abs(logits - ref).max(), np.abs(eager - ref).max()
        print(f"gru session vs oracle ({what}): e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
        assert e_fused <= 2 * e_eager + 1e-6, (what, e_fused, e_eager)
        assert np.abs(probs - softmax64(logits)).max() <= 1e-6
        return ref

    ref1 = verdict(first, "first state")
    model.load_state_dict({k: v.clone() for k, v in other.items()})
    ref2 = verdict(other, "after load_state_dict")
    assert np.abs(ref1 - ref2).max() > 1e-2      # the two models do differ
    model.dnn[3].bias.data.add_(0.5)             # `.data` shares the storage, not the version counter
    third = {k: v.clone() for k, v in other.items()}
    third["dnn.3.bias"] = third["dnn.3.bias"] + 0.5
    ref3 = verdict(third, "after an in-place write")
    assert np.abs(ref3 - ref2).max() > 0.4
    # 80 mel bins and a train-mode frontend that would draw a VTLP filterbank are outside the session
    from howl_amd.settings import SETTINGS
    SETTINGS.audio_transform.num_mels = 80
    try:
        std80 = StandardAudioTransform().to(dev).eval()
    finally:
        SETTINGS.reset()
    assert std80.n_mels == 80 and not model.stream_session(std80, zmuv).supported(L)
    std.augment_params[0].enabled = True
    try:
        std.train()
        assert not session.supported(L)
        std.eval()
        assert session.supported(L)
    finally:
        std.augment_params[0].enabled = False
        std.eval()
    model.train()
    try:
        session.probabilities(pcm)
    except RuntimeError as e:
        assert "eval" in str(e)
    else:
        raise AssertionError("training mode must raise")
    finally:
        model.eval()
