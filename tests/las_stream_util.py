"""Shared by tests/test_emu_las_stream.py (hipemu, guarded host buffers) and tests/test_gpu_las_stream.py (device, sentinel bands):
the streaming las entry points of include/howl_hip_las_stream.h called through an allocator of tests/guard_mem.py, the eager chain
(howl_logmel_fwd + howl_deltas_fwd + howl_las_fwd in eval mode) on the same library, the float64 oracle (oracle.frontend +
tests/las_util.py's RefLas), and the module-level checks (session, engine) that run unchanged on either side."""
import ctypes

import numpy as np
import torch

import las_util
import stream_util
from stream_util import ZMUV_PAIR, CallLog, softmax64  # noqa: F401
from oracle import frontend as fe

# (N, L, C) of check 1, chosen for the geometry's edges: T = 3 with one step of two; two steps of three; the client's window (both
# pools drop a column); neither pool drops; only the second drops; 1 s; the largest window (T = 83, 21 steps of 22) and label count
CASES = [(1, 512, 4), (3, 1000, 4), (3, 8000, 12), (2, 8200, 4), (3, 8600, 5), (2, 16000, 12), (3, 16599, 64)]
SEEDS = {4: 21, 12: 27, 64: 5, 5: 23}
SHARPEN = {"attn.context_vec": 8.0, "attn.k_proj.weight": 3.0, "attn.v_proj.weight": 3.0, "fc.0.weight": 3.0, "fc.3.weight": 6.0}


def frames_of(L):
    """compute_lengths of a window of L samples."""
    return (L - 512) // 200 + 1


def sharp_state(C, seed=None):
    """las_util.make_state with the attention, the head and the recurrent weights scaled up: the plain state's logits differ
    between windows by 1e-4 .. 1e-3 only, under which an encoder bug could hide; this one spreads them by 3e-2 .. 2e-1."""
    sd = las_util.make_state(C, SEEDS[C] if seed is None else seed)
    for k in list(sd):
        if k in SHARPEN:
            sd[k] = sd[k] * SHARPEN[k]
        elif k.startswith("encoder.lstm_encoder.weight_"):
            sd[k] = sd[k] * 2.0
    return sd


def las_params(al, sd, tag=""):
    """Every parameter and running buffer in a buffer of its own -> (buffers by name, HowlLasParams, HowlLasBuffers)."""
    from howl_amd import lib as L
    bufs = {}
    for k in las_util.PARAMS + las_util.BUFFERS:
        a = np.ascontiguousarray(sd[k].numpy())
        bufs[k] = al.buf(tag + k, a.shape if a.ndim else (1,), a.dtype, a)
    prm = L.HowlLasParams(*[al.ptr(bufs[k]) for k in las_util.PARAMS])
    buf = L.HowlLasBuffers(*[al.ptr(bufs[k]) for k in las_util.BUFFERS])
    return bufs, prm, buf


class Fused:
    """The streaming entry points on one model: prepare once, then any number of `windows` launches."""

    def __init__(self, al, lib, sd, C, tag=""):
        self.al, self.lib, self.C, self.tag = al, lib, C, tag
        self.p, self.prm, self.bnb = las_params(al, sd, tag)
        self.fbp = stream_util.pack_fb(al, lib, fe.mel_fb(40).numpy())
        self.zm = al.buf(tag + "zmuv", 2, np.float32, ZMUV_PAIR)
        self.state_bytes = int(lib.cdll.howl_las_stream_state_bytes(C))
        assert self.state_bytes > 4 * (2 * 384 * (352 + 96) + 2 * 192 * 192 + 192 * 256) and self.state_bytes % 4 == 0
        # exactly the size the query returns, NaN sentinels: whatever the window kernel reads, prepare has written
        self.state = al.buf(tag + "state", self.state_bytes // 4, np.float32, "sentinel", promised="all")
        lib.call("howl_las_stream_prepare", ctypes.byref(self.prm), ctypes.byref(self.bnb), C, al.ptr(self.state), self.state_bytes, None)

    def windows(self, flat, N, L, ld, tag="", want_logits=True, frames=None, stream=None):
        """`flat`: the samples, window n = flat[n * ld : n * ld + L]; the buffer ends with the last window."""
        al, C = self.al, self.C
        assert flat.size == (N - 1) * ld + L
        pcm = al.buf(tag + "pcm", flat.size, np.float32, flat)
        probs = al.buf(tag + "probs", (N, C), np.float32, "sentinel", promised="all")
        logits = al.buf(tag + "logits", (N, C), np.float32, "sentinel", promised="all") if want_logits else None
        nws = int(self.lib.cdll.howl_las_stream_workspace_bytes(N, L))
        assert nws > 0 and nws % 4 == 0
        ws = al.buf(tag + "ws", nws // 4, np.float32, "sentinel")
        self.lib.call("howl_las_stream_windows", al.ptr(self.state), al.ptr(pcm), ld, N, L, frames_of(L) if frames is None else frames,
                      al.ptr(self.fbp), 40, 1e-7, al.ptr(self.zm), C, al.ptr(probs), al.ptr(logits), al.ptr(ws), nws, stream)
        al.sync()
        return al.get(probs).copy(), None if logits is None else al.get(logits).copy()


def eager_logits(al, lib, sd, rows, fbp, zm, frames, tag="eager."):
    """The chain the engine runs today on the same library: howl_logmel_fwd (layout (B, M, T), no ZMUV) + howl_deltas_fwd (ZMUV in
    its epilogue) + howl_las_fwd in eval mode."""
    B, L = rows.shape
    T = 1 + L // 200
    pcm = al.buf(tag + "pcm", rows.shape, np.float32, rows)
    lm = al.buf(tag + "logmel", (B, 40, T), np.float32, "sentinel", promised="all")
    lib.call("howl_logmel_fwd", al.ptr(pcm), B, L, L, al.ptr(fbp), 40, 1e-7, None, al.ptr(lm), 0, None)
    x3 = al.buf(tag + "x3", (B, 3, 40, T), np.float32, "sentinel", promised="all")
    lib.call("howl_deltas_fwd", al.ptr(lm), B, 40, T, al.ptr(zm), al.ptr(x3), None)
    al.sync()
    x = torch.from_numpy(np.array(al.get(x3)))
    return las_util.run_library(lib, al, sd, x, [frames] * B, 0)["logits"].numpy()


_ORACLE = {}


def oracle_logits64(sd, rows, frames, pair=ZMUV_PAIR, key=None):
    """oracle.frontend (three channels) + ZMUV + tests/las_util.py's RefLas in float64: (N, L) PCM -> (N, C) logits.  `key`: computed
    once per process and shared."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    x = fe.standard_audio_transform(torch.from_numpy(np.ascontiguousarray(rows)).double(), fe.mel_fb(40).double())
    if pair is not None:
        x = (x - float(pair[0])) / float(pair[1])
    out = las_util.reference(sd, x, [frames] * rows.shape[0], dtype=torch.float64)["logits"].numpy()
    if key is not None:
        _ORACLE[key] = out
    return out


def check_against_oracle(al, lib, N, L, C, placement_tag=""):
    """Checks 1 and 3: fused logits against the fp64 oracle, bounded by the EAGER chain's own error against the same oracle:
    e_fused <= 2 e_eager + 1e-6 (both are exact-fp32 chains in another summation order); probs = softmax64(logits) and rows summing
    to 1 within 1e-6; every operand's guards intact and exactly [N, C] written (the allocator's check)."""
    from howl_amd.utils.synth import synthetic_pcm
    sd = sharp_state(C)
    rows = synthetic_pcm(N, L).numpy().astype(np.float32)
    frames = frames_of(L)
    f = Fused(al, lib, sd, C)
    probs, logits = f.windows(rows.reshape(-1), N, L, L)
    eager = eager_logits(al, lib, sd, rows, f.fbp, f.zm, frames)
    ref = oracle_logits64(sd, rows, frames, key=(N, L, C))
    e_fused, e_eager = np.abs(logits - ref).max(), np.abs(eager - ref).max()
    print(f"las stream vs oracle: N={N} L={L} C={C}: e_fused={e_fused:.3e} e_eager={e_eager:.3e} |logits|max={np.abs(ref).max():.3f} "
          f"spread={np.abs(ref - ref[:1]).max():.3e}")
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
    """Check 4: every refusal of include/howl_hip_las_stream.h on a (N = 2, L = 1000, C = 4) problem: the code, a message that names
    the entry point, nothing launched (probs, logits, workspace and state keep their bytes) -- and the next valid call succeeds."""
    from howl_amd import lib as LL
    N, L, C = 2, 1000, 4
    T = 1 + L // 200
    sd = sharp_state(C)
    f = Fused(al, lib, sd, C)
    pcm = al.buf("pcm", N * L, np.float32, np.zeros(N * L, np.float32))
    probs = al.buf("probs", (N, C), np.float32, "sentinel")
    logits = al.buf("logits", (N, C), np.float32, "sentinel")
    nws = int(lib.cdll.howl_las_stream_workspace_bytes(N, L))
    ws = al.buf("ws", nws // 4, np.float32, "sentinel")
    state2 = al.buf("state2", f.state_bytes // 4, np.float32, "sentinel")
    watched = [probs, logits, ws, state2, f.state]

    def snapshot():
        al.sync()
        return [np.array(al.get(v)).tobytes() for v in watched]

    def windows(null=None, L=L, M=40, C=C, N=N, frames=frames_of(L), short=False):
        g = lambda name, v: None if null == name else al.ptr(v)      # noqa: E731
        return lib.cdll.howl_las_stream_windows(g("state", f.state), g("pcm", pcm), L, N, L, frames, g("fbp", f.fbp), M, 1e-7, al.ptr(f.zm), C,
                                                g("probs", probs), al.ptr(logits), g("ws", ws), nws - 4 if short else nws, None)

    def prepare(null=None, C=C, short=False):
        pp = [None if null == k else al.ptr(f.p[k]) for k in las_util.PARAMS]
        prm = None if null == "params" else ctypes.byref(LL.HowlLasParams(*pp))
        buf = None if null == "buffers" else ctypes.byref(f.bnb)
        return lib.cdll.howl_las_stream_prepare(prm, buf, C, None if null == "state" else al.ptr(state2),
                                                f.state_bytes - 4 if short else f.state_bytes, None)

    cases = [(windows, dict(L=511), -1, "L=511"), (windows, dict(L=16600), -1, "L=16600"), (windows, dict(M=80), -1, "M=80"),
             (windows, dict(C=0), -1, "C=0"), (windows, dict(C=65), -1, "C=65"), (windows, dict(N=0), -1, "N=0"),
             (windows, dict(N=8193), -1, "N=8193"), (windows, dict(frames=0), -1, "frames=0"),
             (windows, dict(frames=T + 1), -1, f"frames={T + 1}"), (windows, dict(short=True), -3, "workspace too small")] + \
            [(windows, dict(null=k), -1, "null pointer") for k in ("state", "pcm", "fbp", "probs", "ws")] + \
            [(prepare, dict(null=k), -1, "null pointer") for k in ("params", "buffers", "state", "attn.context_vec")] + \
            [(prepare, dict(C=0), -1, "C=0"), (prepare, dict(C=65), -1, "C=65"), (prepare, dict(short=True), -1, "state of")]
    for fn, kw, code, text in cases:
        which = "howl_las_stream_" + fn.__name__
        before = snapshot()
        rc = fn(**kw)
        msg = lib.cdll.howl_last_error().decode()
        assert rc == code, (which, kw, rc, msg)
        assert msg.startswith(which + ":") and text in msg, (which, kw, msg)
        assert snapshot() == before, (which, kw, "a refused call wrote something")
    assert prepare() == 0 and windows() == 0, lib.cdll.howl_last_error().decode()      # the next valid calls succeed
    al.sync()
    assert np.isfinite(np.array(al.get(probs))).all() and np.isfinite(np.array(al.get(logits))).all()
    for Lq, M, Cq, ok in [(8000, 40, 4, 1), (512, 40, 1, 1), (16599, 40, 64, 1), (511, 40, 4, 0), (16600, 40, 4, 0), (8000, 80, 4, 0),
                          (8000, 40, 0, 0), (8000, 40, 65, 0)]:
        assert lib.cdll.howl_las_stream_supported(Lq, M, Cq) == ok, (Lq, M, Cq)
    assert lib.cdll.howl_las_stream_state_bytes(0) == 0 and lib.cdll.howl_las_stream_state_bytes(65) == 0
    for Nq, Lq in [(0, 8000), (8193, 8000), (1, 511), (1, 16600)]:
        assert lib.cdll.howl_las_stream_workspace_bytes(Nq, Lq) == 0, (Nq, Lq)


# ---- module level: the same code on the device and, inside emu_util.emulated_package(), on the emulator -------------------------

ENGINE_VOCAB = ["hey", "fire", "fox", "one", "two", "three", "four", "five", "six", "seven", "eight"]      # + [OOV]: 12 labels


def las_engine(golden, dev, fused):
    """A FrameInferenceEngine (500 ms windows, 63 ms stride) over a las model with the sharpened state for C = 12, seed 27."""
    from howl_amd.context import InferenceContext
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.model.inference import FrameInferenceEngine
    g4 = golden("g4_zmuv")
    ctx = InferenceContext(ENGINE_VOCAB, token_type="word")
    assert ctx.num_labels == 12
    model = RegisteredModel.find_registered_class("las")(ctx.num_labels)
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
    howl_las_stream_windows per window and no frontend / las launch on the fused path; every window's top-two gap in the fp64
    oracle exceeds 1e-3 (no window is left out of the comparison) and the oracle's labels are not constant; all windows in one
    probabilities() call against window_probabilities(clip): check 1's bound, argmax identical.  `first`: the emulator's form, the
    clip cut behind its first `first` windows (an emulated window costs a second; the oracle's conditions still cover all 37)."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        whole = torch.from_numpy(np.asarray(g["clip"]))
        engine = las_engine(golden, dev, False)
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
            engine = las_engine(golden, dev, fused)
            windows, starts, chunk = windows_of(clip, engine)
            assert len(starts) == W
            with CallLog(library) as log:
                for i, s in enumerate(starts):
                    engine.ingest_frame(clip[s:s + chunk], curr_time=float(engine.eval_stride_size_ms * i))
            hist[fused] = np.array(engine.label_history, dtype=np.float64)
            if fused:
                assert log.names.count("howl_las_stream_windows") == W and log.names.count("howl_las_stream_prepare") == 1, log.names
                assert not {"howl_logmel_fwd", "howl_deltas_fwd", "howl_las_fwd"} & set(log.names), log.names
            else:
                assert log.names.count("howl_las_fwd") == W and "howl_las_stream_windows" not in log.names, log.names
        assert hist[True].shape[0] == W and np.array_equal(hist[True], hist[False]), (hist[True], hist[False])
        with CallLog(library) as log:
            fusedp = engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
        assert log.names.count("howl_las_stream_windows") == 1, log.names
        engine.fused_windows = False
        eager = engine.window_probabilities(clip)
        e_fused, e_eager = np.abs(fusedp - ref).max(), np.abs(eager - ref).max()
        print(f"G8 clip, {W} windows in one launch: e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
        assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
        assert np.array_equal(fusedp.argmax(1), eager.argmax(1)) and np.array_equal(fusedp.argmax(1), labels)
    finally:
        SETTINGS.reset()


def check_staleness(dev, L=2000, C=4, N=2):
    """Check 6: after load_state_dict the next call answers for the NEW weights (check 1's criterion, the eager module path as the
    yardstick); after a write torch cannot see, refresh() does; training mode raises; supported() follows the range and VTLP."""
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.utils.synth import synthetic_pcm
    first, other = sharp_state(C, 31), sharp_state(C, 32)
    model = RegisteredModel.find_registered_class("las")(C)
    model.load_state_dict({k: v.clone() for k, v in first.items()})
    model = model.to(dev).eval()
    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    rows = synthetic_pcm(N, L)
    pcm = rows.to(dev)
    zmuv.update(std(pcm))
    pair = zmuv.pair().cpu().numpy()
    session = model.stream_session(std, zmuv)
    assert session.supported(L) and session.supported(512) and session.supported(16599)
    assert not session.supported(511) and not session.supported(16600)
    frames = frames_of(L)
    lengths = torch.full((N,), frames, dtype=torch.int64)

    def both():
        logits = torch.empty((N, C), dtype=torch.float32, device=dev)
        probs = session.probabilities(pcm, logits=logits)
        with torch.no_grad():
            eager = model(std.log_mel_for_model(pcm, zmuv, channels=3), lengths)
        return probs.cpu().numpy(), logits.cpu().numpy(), eager.cpu().numpy()

    def verdict(sd, what):
        probs, logits, eager = both()
        ref = oracle_logits64(sd, rows.numpy(), frames, pair)
        e_fused, e_eager = np.abs(logits - ref).max(), np.abs(eager - ref).max()
        print(f"las session vs oracle ({what}): e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
        assert e_fused <= 2 * e_eager + 1e-6, (what, e_fused, e_eager)
        assert np.abs(probs - softmax64(logits)).max() <= 1e-6
        return ref, logits

    ref1, _ = verdict(first, "first state")
    model.load_state_dict({k: v.clone() for k, v in other.items()})
    ref2, _ = verdict(other, "after load_state_dict")
    assert np.abs(ref1 - ref2).max() > 1e-2      # the two models do differ
    # a write torch cannot see (`.data` shares the storage, not the version counter: what an in-kernel optimiser step looks like
    # from here): the session keeps answering for the state it prepared until refresh()
    stale_key = tuple((t.data_ptr(), t._version) for t in session._watched())
    model.fc[3].bias.data.add_(0.5)
    assert tuple((t.data_ptr(), t._version) for t in session._watched()) == stale_key
    third = {k: v.clone() for k, v in other.items()}
    third["fc.3.bias"] = third["fc.3.bias"] + 0.5
    assert np.abs(both()[1] - ref2).max() < 1e-3      # still the prepared state's answer
    session.refresh()
    ref3, _ = verdict(third, "after refresh()")
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
