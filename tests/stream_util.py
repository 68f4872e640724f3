"""Shared by tests/test_emu_res8_stream.py (hipemu, guarded host buffers) and tests/test_gpu_res8_stream.py (device, sentinel
bands): the streaming res8 entry points of include/howl_hip_stream.h called through an allocator of tests/guard_mem.py, the eager
chain (howl_logmel_fwd + howl_res8_fwd, eval mode) on the same library, the float64 oracle, and the module-level checks (session,
engine) that run unchanged on either side."""
import ctypes

import numpy as np
import torch

from howl_amd.lib import HowlRes8Params, HowlRes8Saved
from oracle import frontend as fe
from oracle import models as om

ZMUV_PAIR = np.array([-4.5, 3.25], np.float32)      # [mean, std] of the order the log-mels of speech-level PCM have


def random_state(C, seed):
    """Seeded random res8 weights at the closed-form scales, with non-trivial BatchNorm running buffers."""
    g = torch.Generator().manual_seed(seed)
    sd = om.res8_init(C)
    for k, v in sd.items():
        if k.endswith("weight") or k.endswith("bias"):
            sd[k] = (v.abs().max() * (2 * torch.rand(v.shape, generator=g) - 1)).float()
    for i in range(1, 7):
        sd[f"bn{i}.running_mean"] = (0.2 * torch.randn(45, generator=g)).float()
        sd[f"bn{i}.running_var"] = (0.4 + torch.rand(45, generator=g)).float()
    return sd


def params(al, sd, tag=""):
    """Every parameter and running buffer in a buffer of its own -> (buffers, HowlRes8Params)."""
    p = {k: al.buf(tag + k, v.shape, np.float32 if v.dtype == torch.float32 else np.int64, v.numpy()) for k, v in sd.items()}
    prm = HowlRes8Params()
    prm.conv0_w = al.ptr(p["conv0.weight"])
    for i in range(6):
        prm.conv_w[i] = al.ptr(p[f"conv{i+1}.weight"]).value
        prm.bn_running_mean[i] = al.ptr(p[f"bn{i+1}.running_mean"]).value
        prm.bn_running_var[i] = al.ptr(p[f"bn{i+1}.running_var"]).value
        prm.bn_num_batches[i] = al.ptr(p[f"bn{i+1}.num_batches_tracked"]).value
    prm.out_w, prm.out_b = al.ptr(p["output.weight"]), al.ptr(p["output.bias"])
    return p, prm


def pack_fb(al, lib, fb):
    src = al.buf("fb", fb.shape, np.float32, np.ascontiguousarray(fb, np.float32))
    fbp = al.buf("fbp", int(lib.cdll.howl_fb_packed_floats(fb.shape[1])), np.float32, "sentinel", promised="all")
    lib.call("howl_fb_pack", al.ptr(src), fb.shape[1], al.ptr(fbp), None)
    return fbp


class Fused:
    """The streaming entry points on one model: prepare once, then any number of `windows` launches."""

    def __init__(self, al, lib, sd, C, tag=""):
        self.al, self.lib, self.C, self.tag = al, lib, C, tag
        self.p, self.prm = params(al, sd, tag)
        self.fbp = pack_fb(al, lib, fe.mel_fb(40).numpy())
        self.zm = al.buf(tag + "zmuv", 2, np.float32, ZMUV_PAIR)
        nbytes = int(lib.cdll.howl_res8_stream_state_bytes(C))
        assert nbytes > 0
        assert nbytes % 4 == 0      # (as floats: the NaN sentinel cannot be mistaken for data the way a byte pattern can)
        self.state = al.buf(tag + "state", nbytes // 4, np.float32, "sentinel", promised="all")      # exactly the size the query returns
        lib.call("howl_res8_stream_prepare", ctypes.byref(self.prm), C, al.ptr(self.state), nbytes, None)

    def windows(self, flat, N, L, ld, tag="", want_logits=True):
        """`flat`: the samples, window n = flat[n * ld : n * ld + L]; the buffer ends with the last window."""
        al, C = self.al, self.C
        assert flat.size == (N - 1) * ld + L
        pcm = al.buf(tag + "pcm", flat.size, np.float32, flat)
        probs = al.buf(tag + "probs", (N, C), np.float32, "sentinel", promised="all")
        logits = al.buf(tag + "logits", (N, C), np.float32, "sentinel", promised="all") if want_logits else None
        self.lib.call("howl_res8_stream_windows", al.ptr(self.state), al.ptr(pcm), ld, N, L, al.ptr(self.fbp), 40, 1e-7, al.ptr(self.zm),
                      C, al.ptr(probs), al.ptr(logits), None)
        al.sync()
        return al.get(probs).copy(), None if logits is None else al.get(logits).copy()


def eager_logits(al, lib, sd, rows, C, fbp, zm, tag="eager."):
    """The chain the engine runs today on the same library: howl_logmel_fwd (layout (B, T, M), ZMUV fused) + howl_res8_fwd in eval
    mode on three rotating activation buffers."""
    B, L = rows.shape
    T = 1 + L // 200
    p, prm = params(al, sd, tag)
    pcm = al.buf(tag + "pcm", rows.shape, np.float32, rows)
    feat = al.buf(tag + "feat", (B, T, 40), np.float32, "sentinel", promised="all")
    lib.call("howl_logmel_fwd", al.ptr(pcm), B, L, L, al.ptr(fbp), 40, 1e-7, al.ptr(zm), al.ptr(feat), 1, None)
    ns = int(lib.cdll.howl_res8_saved_floats(B, T, 40))
    rot = [al.buf(f"{tag}rot{i}", ns, np.float32, "sentinel") for i in range(3)]
    saved = HowlRes8Saved()
    for i in range(7):
        saved.s[i] = al.ptr(rot[i % 3]).value
    saved.bn_stats = al.ptr(al.buf(tag + "bn_stats", (6, 2, 48), np.float32, "sentinel"))
    saved.pooled = al.ptr(al.buf(tag + "pooled", (B, 48), np.float32, "sentinel"))
    saved.mask0 = al.ptr(al.buf(tag + "mask0", ns, np.uint16, "sentinel"))
    nws = int(lib.cdll.howl_res8_eval_workspace_bytes_mels(B, T, 40))
    ws = al.buf(tag + "ws", nws, np.uint8, "sentinel")
    logits = al.buf(tag + "logits", (B, C), np.float32, "sentinel", promised="all")
    lib.call("howl_res8_fwd", ctypes.byref(prm), al.ptr(feat), T * 40, 40, 1, B, T, 40, C, 0, ctypes.byref(saved), al.ptr(logits), al.ptr(ws),
             nws, None)
    al.sync()
    return al.get(logits).copy()


def oracle_logits64(sd, rows, pair=ZMUV_PAIR):
    """oracle.frontend + oracle.models in float64: (N, L) PCM -> (N, C) logits."""
    x = fe.standard_audio_transform(torch.from_numpy(np.ascontiguousarray(rows)).double(), fe.mel_fb(40).double(), mels_only=True)
    if pair is not None:
        x = (x - float(pair[0])) / float(pair[1])
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return om.res8_forward(sd64, x.unsqueeze(1), False).numpy()


def softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def check_against_oracle(al, lib, L, C, N=3, seed=0):
    """Item 1: fused logits against the fp64 oracle, bounded by the EAGER chain's own error against the same oracle:
    e_fused <= 2 e_eager + 1e-6 (both are exact-fp32 MFMA chains over the same K = 405 in another summation order)."""
    from howl_amd.utils.synth import synthetic_pcm
    sd = random_state(C, 100 + seed + C)
    rows = synthetic_pcm(N, L).numpy().astype(np.float32)
    f = Fused(al, lib, sd, C)
    probs, logits = f.windows(rows.reshape(-1), N, L, L)
    eager = eager_logits(al, lib, sd, rows, C, f.fbp, f.zm)
    ref = oracle_logits64(sd, rows)
    e_fused, e_eager = np.abs(logits - ref).max(), np.abs(eager - ref).max()
    print(f"stream vs oracle: L={L} C={C} N={N}: e_fused={e_fused:.3e} e_eager={e_eager:.3e} |logits|max={np.abs(ref).max():.3f}")
    assert e_fused <= 2 * e_eager + 1e-6, f"L={L} C={C}: e_fused={e_fused:.3e} > 2 * e_eager ({e_eager:.3e}) + 1e-6"
    sm = softmax64(logits)
    assert np.abs(probs - sm).max() <= 1e-6, np.abs(probs - sm).max()
    assert np.abs(probs.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    al.check()
    return e_fused, e_eager


def check_independence(al, lib, L=8000, C=4, N=5, ld=1008):
    """Item 2: window n alone (N = 1) and as row n of N windows, and a repeated launch: the same bits."""
    from howl_amd.utils.synth import synthetic_pcm
    sd = random_state(C, 7)
    flat = synthetic_pcm(1, (N - 1) * ld + L).numpy().astype(np.float32).reshape(-1)
    f = Fused(al, lib, sd, C)
    probs, logits = f.windows(flat, N, L, ld, "all.")
    probs2, logits2 = f.windows(flat, N, L, ld, "again.")
    assert np.array_equal(probs, probs2) and np.array_equal(logits, logits2)
    assert np.isfinite(probs).all() and np.abs(logits[0] - logits[-1]).max() > 0      # the windows differ
    for n in range(N):
        p1, l1 = f.windows(flat[n * ld:n * ld + L].copy(), 1, L, L, f"solo{n}.")
        assert np.array_equal(p1[0], probs[n]) and np.array_equal(l1[0], logits[n]), n
    al.check()


# ---- module level: the same code on the device and, inside emu_util.emulated_package(), on the emulator -------------------------

def g8_engine(golden, dev, fused):
    from howl_amd.context import InferenceContext
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.model.inference import FrameInferenceEngine
    g4 = golden("g4_zmuv")
    ctx = InferenceContext(["hey", "fire", "fox"], token_type="word")
    model = RegisteredModel.find_registered_class("res8")(ctx.num_labels)
    model.load_state_dict({k: v.clone() for k, v in om.res8_init(ctx.num_labels).items()})
    model = model.to(dev).eval().streaming()
    zmuv = ZmuvTransform().to(dev)
    for k in ("mean", "mean2", "total"):
        getattr(zmuv, k).copy_(torch.from_numpy(np.asarray(g4[k])))
    engine = FrameInferenceEngine(500, 63, model, zmuv, ctx)
    engine.fused_windows = fused
    engine.std = engine.std.to(dev)      # (the engine does this on its first call; some tests reach for its session before that)
    return engine


class CallLog:
    """Records the entry points a Library is asked for while active."""

    def __init__(self, library):
        self.library, self.names = library, []

    def __enter__(self):
        self._real = self.library.call

        def call(name, *args):
            self.names.append(name)
            return self._real(name, *args)
        self.library.call = call
        return self

    def __exit__(self, *exc):
        del self.library.call
        return False


def check_g8_labels(golden, dev, library):
    """Item 3: the first five windows of the G8 clip through the fused ingest_frame and the engine's smoother give the labels the
    reference's engine recorded -- and each of them was ONE windows launch, with no frontend / res8 launch beside it."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        engine = g8_engine(golden, dev, fused=True)
        clip = torch.from_numpy(np.asarray(g["clip"])).to(dev)
        with CallLog(library) as log:
            labels = [engine.ingest_frame(clip[i * 1008: i * 1008 + 8000], curr_time=63.0 * i) for i in range(5)]
        assert labels == [int(x) for x in g["label_history"][:5, 1]], (labels, g["label_history"][:5, 1])
        assert log.names.count("howl_res8_stream_windows") == 5 and log.names.count("howl_res8_stream_prepare") == 1, log.names
        assert "howl_res8_fwd" not in log.names and "howl_logmel_fwd" not in log.names, log.names
    finally:
        SETTINGS.reset()


def check_staleness(dev, L=8000, C=4, N=2):
    """Item 6: after load_state_dict the next call answers for the NEW weights (same criterion as item 1, the eager module path
    as the yardstick), not for the ones the state was prepared from."""
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.utils.synth import synthetic_pcm
    first, other = random_state(C, 31), random_state(C, 32)
    model = RegisteredModel.find_registered_class("res8")(C)
    model.load_state_dict({k: v.clone() for k, v in first.items()})
    model = model.to(dev).eval()
    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    rows = synthetic_pcm(N, L)
    pcm = rows.to(dev)
    zmuv.update(std(pcm))
    pair = zmuv.pair().cpu().numpy()
    session = model.stream_session(std, zmuv)
    assert session.supported(L) and not session.supported(200) and not session.supported(20000)

    def both():
        logits = torch.empty((N, C), dtype=torch.float32, device=dev)
        probs = session.probabilities(pcm, logits=logits)
        with torch.no_grad():
            eager = model(std.log_mel_for_model(pcm, zmuv), None)
        return probs.cpu().numpy(), logits.cpu().numpy(), eager.cpu().numpy()

    for sd in (first, other):
        if sd is other:
            model.load_state_dict({k: v.clone() for k, v in other.items()})
        probs, logits, eager = both()
        ref = oracle_logits64(sd, rows.numpy(), pair)
        e_fused, e_eager = np.abs(logits - ref).max(), np.abs(eager - ref).max()
        print(f"session vs oracle: e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
        assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
        assert np.abs(probs - softmax64(logits)).max() <= 1e-6
    assert np.abs(oracle_logits64(first, rows.numpy(), pair) - ref).max() > 1e-2      # the two models do differ
    model.train()
    try:
        session.probabilities(pcm)
    except RuntimeError as e:
        assert "eval" in str(e)
    else:
        raise AssertionError("training mode must raise")
