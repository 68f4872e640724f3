"""Shared by tests/test_emu_cnn_stream.py (hipemu, guarded host buffers) and tests/test_gpu_cnn_stream.py (device, sentinel bands):
the streaming small-cnn / seq-cnn entry points of include/howl_hip_cnn_stream.h called through an allocator of tests/guard_mem.py,
the eager chain (howl_logmel_fwd with the ZMUV pair + howl_cnn_fwd in eval mode) on the same library, the float64 oracle
(oracle.frontend + tests/cnn_util.py's RefCnn), and the module-level checks (session, engines) that run unchanged on either side."""
import ctypes
import re
from pathlib import Path

import numpy as np
import torch

import cnn_util
import stream_util
from cnn_util import SEQ, SMALL
from stream_util import ZMUV_PAIR, CallLog, softmax64  # noqa: F401
from oracle import frontend as fe

ROOT = Path(__file__).resolve().parent.parent
# the output rows one workgroup of the seq-cnn kernel produces, read from the header: the cases below sit on its seams
R = int(re.search(r"#define\s+HOWL_CNN_STREAM_TILE_ROWS\s+(\d+)", (ROOT / "include" / "howl_hip_cnn_stream.h").read_text()).group(1))
# cnn_util.make_state with the head scaled up: with the plain state the oracle's logits move by 1e-3 .. 1e-2 with the audio, and a
# dead encoder would pass every check; with these factors the smallest movement over the cases below is 2.1e-2 (asserted per case)
SHARPEN = {"output.0.weight": 3.0, "output.3.weight": 6.0}
LIVE = 1e-2      # the oracle's logits must move by more than this with the audio
SEEDS = {SMALL: {2: 22, 4: 21, 12: 33, 64: 33}, SEQ: {2: 25, 4: 24, 5: 27, 12: 46, 64: 27}}

# small-cnn (N, L, C, variant): T = 26 (7 pooled rows, the smallest window); T = 28 (the pool drops a row; L no multiple of 200);
# the client's window; the largest window and label count; no ZMUV; overlapping rows.  variant: zmuv = False, ld = the row stride
SMALL_CASES = [(1, 5000, 2, {}), (3, 5599, 12, {}), (3, 8000, 12, {}), (3, 8199, 64, {}), (2, 8000, 4, {"zmuv": False}),
               (3, 8000, 4, {"ld": 1008})]


def seq_span(r):
    """The shortest and the longest clip with r output rows."""
    return 1600 * r - 800, 1600 * r + 799


def _seq_cases():
    """Clips with r rows for r on the tile's seams, each at both ends of its length range, N = 1 (N = 2 for the shortest clip), the
    label counts spread over them; one ragged launch with n_samples given, one with n_samples = NULL, one without ZMUV."""
    cases, labels = [], [2, 5, 12, 64]
    for i, r in enumerate([1, 2, R - 1, R, R + 1, 2 * R, 2 * R + 1]):
        for j, L in enumerate(seq_span(r)):
            cases.append(([L] * (2 if L == 800 else 1), labels[(2 * i + j) % 4], {}))
    ragged = [seq_span(2 * R + 1)[1], seq_span(R)[0] + 333, seq_span(1)[0] + 77, seq_span(R + 1)[1], seq_span(2)[0] + 1]
    cases.append((ragged, 5, {}))
    cases.append(([seq_span(R + 1)[0]] * 2, 4, {"null": True}))
    cases.append(([seq_span(2)[1], seq_span(R)[1]], 12, {"zmuv": False}))
    return cases


SEQ_CASES = _seq_cases()


def small_id(case):
    N, L, C, var = case
    return f"N{N}-L{L}-C{C}" + "".join(f"-{k}{v}" for k, v in var.items())


def seq_id(case):
    sizes, C, var = case
    return "L" + "_".join(str(n) for n in sizes) + f"-C{C}" + "".join(f"-{k}{v}" for k, v in var.items())


def rows_of(L):
    """Output rows of a seq-cnn clip of L samples."""
    return cnn_util.compute_length(1 + L // 200)


def sharp_state(kind, C, seed=None):
    sd = cnn_util.make_state(kind, C, SEEDS[kind][C] if seed is None else seed)
    for k, f in SHARPEN.items():
        sd[k] = sd[k] * f
    return sd


def cnn_params(al, sd, tag=""):
    """Every parameter and running buffer in a buffer of its own -> (buffers by name, HowlCnnParams, HowlCnnBuffers)."""
    from howl_amd import lib as L
    bufs = {}
    for k in cnn_util.PARAMS + cnn_util.BUFFERS:
        a = np.ascontiguousarray(sd[k].numpy())
        bufs[k] = al.buf(tag + k, a.shape if a.ndim else (1,), a.dtype, a)
    prm = L.HowlCnnParams(*[al.ptr(bufs[k]) for k in cnn_util.PARAMS])
    buf = L.HowlCnnBuffers(*[al.ptr(bufs[k]) for k in cnn_util.BUFFERS])
    return bufs, prm, buf


class Fused:
    """The streaming entry points on one model: any number of launches; there is no prepared state."""

    def __init__(self, al, lib, kind, sd, C, tag=""):
        self.al, self.lib, self.kind, self.C, self.tag = al, lib, kind, C, tag
        self.p, self.prm, self.bnb = cnn_params(al, sd, tag)
        self.fbp = stream_util.pack_fb(al, lib, fe.mel_fb(40).numpy())
        self.zm = al.buf(tag + "zmuv", 2, np.float32, ZMUV_PAIR)

    def _ws(self, tag, N, L):
        nws = int(self.lib.cdll.howl_cnn_stream_workspace_bytes(self.kind, N, L))
        assert nws > 0 and nws % 16 == 0
        return self.al.buf(tag + "ws", nws // 4, np.float32, "sentinel"), nws      # exactly the size the query returns

    def windows(self, flat, N, L, ld, tag="", want_logits=True, zmuv=True, stream=None):
        """small-cnn.  `flat`: the samples, window n = flat[n * ld : n * ld + L]; the buffer ends with the last window."""
        al, C = self.al, self.C
        assert flat.size == (N - 1) * ld + L
        pcm = al.buf(tag + "pcm", flat.size, np.float32, flat)
        probs = al.buf(tag + "probs", (N, C), np.float32, "sentinel", promised="all")
        logits = al.buf(tag + "logits", (N, C), np.float32, "sentinel", promised="all") if want_logits else None
        ws, nws = self._ws(tag, N, L)
        self.lib.call("howl_cnn_stream_windows", ctypes.byref(self.prm), ctypes.byref(self.bnb), al.ptr(pcm), ld, N, L, al.ptr(self.fbp), 40,
                      1e-7, al.ptr(self.zm) if zmuv else None, C, al.ptr(probs), al.ptr(logits), al.ptr(ws), nws, stream)
        al.sync()
        return al.get(probs).copy(), None if logits is None else al.get(logits).copy()

    def clips(self, flat, sizes, L_max, ld, tag="", want_logits=True, zmuv=True, null=False, stream=None):
        """seq-cnn.  `flat`: the samples, clip n = flat[n * ld : n * ld + sizes[n]]; the buffer ends with row N - 1's L_max samples.
        `null`: n_samples = NULL (every clip has L_max samples).  -> (probs, logits) of shape (N, rows(L_max), C): exactly that
        is promised (the rows behind a clip's own as zeros)."""
        al, C, N = self.al, self.C, len(sizes)
        assert flat.size == (N - 1) * ld + L_max and max(sizes) <= L_max
        rows = rows_of(L_max)
        assert rows == int(self.lib.cdll.howl_cnn_stream_rows(SEQ, L_max))
        pcm = al.buf(tag + "pcm", flat.size, np.float32, flat)
        ns = None if null else al.buf(tag + "n_samples", N, np.int64, np.asarray(sizes, np.int64))
        probs = al.buf(tag + "probs", (N, rows, C), np.float32, "sentinel", promised="all")
        logits = al.buf(tag + "logits", (N, rows, C), np.float32, "sentinel", promised="all") if want_logits else None
        ws, nws = self._ws(tag, N, L_max)
        self.lib.call("howl_cnn_stream_clips", ctypes.byref(self.prm), ctypes.byref(self.bnb), al.ptr(pcm), ld, N, L_max, al.ptr(ns),
                      al.ptr(self.fbp), 40, 1e-7, al.ptr(self.zm) if zmuv else None, C, al.ptr(probs), al.ptr(logits), rows * C, al.ptr(ws),
                      nws, stream)
        al.sync()
        return al.get(probs).copy(), None if logits is None else al.get(logits).copy()


def eager_logits(al, lib, kind, sd, rows, fbp, zm, tag="eager."):
    """The chain the engines run today on the same library: howl_logmel_fwd with the ZMUV pair (`zm` None: without) + howl_cnn_fwd
    in eval mode (cnn_util.run_library).  rows (B, L) -> (B, C) or (B, rows, C)."""
    B, L = rows.shape
    T = 1 + L // 200
    pcm = al.buf(tag + "pcm", rows.shape, np.float32, rows)
    lm = al.buf(tag + "logmel", (B, 40, T), np.float32, "sentinel", promised="all")
    lib.call("howl_logmel_fwd", al.ptr(pcm), B, L, L, al.ptr(fbp), 40, 1e-7, al.ptr(zm), al.ptr(lm), 0, None)
    al.sync()
    x = torch.from_numpy(np.array(al.get(lm))).reshape(B, 1, 40, T)
    out = cnn_util.run_library(lib, al, kind, sd, x, 0, x_time_major=True)
    al.sync()
    z = out["logits"]
    return (z if kind == SMALL else z.permute(1, 0, 2)).contiguous().numpy()


_ORACLE = {}


def oracle_logits64(kind, sd, rows, pair=ZMUV_PAIR, key=None):
    """oracle.frontend + ZMUV + tests/cnn_util.py's RefCnn in float64, eval mode: (N, L) PCM -> (N, C) or (N, rows, C) logits.
    `key`: computed once per process and shared."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    x = fe.standard_audio_transform(torch.from_numpy(np.ascontiguousarray(rows)).double(), fe.mel_fb(40).double())
    if pair is not None:
        x = (x - float(pair[0])) / float(pair[1])
    z = cnn_util.reference(kind, sd, x)["logits"]
    out = (z if kind == SMALL else z.permute(1, 0, 2)).contiguous().numpy()
    if key is not None:
        _ORACLE[key] = out
    return out


def _pcm(N, L, seed=None):
    from howl_amd.utils.synth import synthetic_pcm
    return (synthetic_pcm(N, L) if seed is None else synthetic_pcm(N, L, seed=seed)).numpy().astype(np.float32)


def _verdict(what, logits, probs, eager, ref):
    """e_fused <= 2 e_eager + 1e-6 on the logits over every row of every clip (tile seams included); probs = softmax64(logits) and
    rows summing to 1 within 1e-6."""
    e_fused, e_eager = float(np.abs(logits - ref).max()), float(np.abs(eager - ref).max())
    print(f"cnn stream vs oracle: {what}: e_fused={e_fused:.3e} e_eager={e_eager:.3e} |logits|max={np.abs(ref).max():.3f}")
    assert e_fused <= 2 * e_eager + 1e-6, f"{what}: e_fused={e_fused:.3e} > 2 * e_eager ({e_eager:.3e}) + 1e-6"
    sm = softmax64(logits)
    assert np.abs(probs - sm).max() <= 1e-6, np.abs(probs - sm).max()
    assert np.abs(probs.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    return e_fused, e_eager


def check_small(al, lib, N, L, C, variant=None):
    """Fused logits of N windows against the fp64 oracle, bounded by the EAGER chain's own error against the same oracle; every
    operand's guards intact and exactly [N, C] written (the allocator's check)."""
    variant = variant or {}
    zmuv, ld = variant.get("zmuv", True), variant.get("ld", L)
    pair = ZMUV_PAIR if zmuv else None
    sd = sharp_state(SMALL, C)
    flat = _pcm(1, (N - 1) * ld + L).reshape(-1) if ld != L else _pcm(N, L).reshape(-1)
    other = _pcm(1, (N - 1) * ld + L, seed=3).reshape(-1) if ld != L else _pcm(N, L, seed=3).reshape(-1)
    rows = np.stack([flat[n * ld:n * ld + L] for n in range(N)])
    rows3 = np.stack([other[n * ld:n * ld + L] for n in range(N)])
    ref = oracle_logits64(SMALL, sd, rows, pair, key=("small", N, L, C, zmuv, ld))
    ref3 = oracle_logits64(SMALL, sd, rows3, pair, key=("small", N, L, C, zmuv, ld, "seed3"))
    moved = float(np.abs(ref - ref3).max(axis=1).min())
    print(f"cnn stream oracle: small N={N} L={L} C={C} zmuv={zmuv} ld={ld}: moved by {moved:.3e} with the audio")
    assert moved > LIVE, moved
    f = Fused(al, lib, SMALL, sd, C)
    probs, logits = f.windows(flat, N, L, ld, zmuv=zmuv)
    eager = eager_logits(al, lib, SMALL, sd, rows, f.fbp, f.zm if zmuv else None)
    res = _verdict(f"small N={N} L={L} C={C} zmuv={zmuv} ld={ld}", logits, probs, eager, ref)
    al.check()
    return res


def seq_inputs(sizes, seed=None):
    """One (N, L_max) buffer of audio; clip n is the first sizes[n] samples of row n (what follows them in the row is audio too: a
    kernel that read behind a clip's end would not get zeros)."""
    L_max = max(sizes)
    return _pcm(len(sizes), L_max, seed), L_max


def seq_oracle(sd, buf, sizes, pair, key):
    """Per clip (eval mode couples nothing): [(rows(n), C)] fp64 logits."""
    return [oracle_logits64(SEQ, sd, buf[n:n + 1, :L], pair, key=None if key is None else key + (n, L))[0] for n, L in enumerate(sizes)]


def check_seq(al, lib, sizes, C, variant=None):
    """Fused logits of ragged clips against the fp64 oracle per clip, bounded by the eager chain's own error (one eager call per
    clip, as the engine's loop runs them); rows behind a clip's own read back as zeros; exactly (N, rows(L_max), C) written."""
    variant = variant or {}
    zmuv, null = variant.get("zmuv", True), variant.get("null", False)
    pair = ZMUV_PAIR if zmuv else None
    sd = sharp_state(SEQ, C)
    N = len(sizes)
    buf, L_max = seq_inputs(sizes)
    buf3, _ = seq_inputs(sizes, seed=3)
    key = ("seq", tuple(sizes), C, zmuv)
    refs = seq_oracle(sd, buf, sizes, pair, key)
    refs3 = seq_oracle(sd, buf3, sizes, pair, key + ("seed3",))
    moved = min(float(np.abs(a - b).max()) for a, b in zip(refs, refs3))
    print(f"cnn stream oracle: seq L={sizes} C={C} zmuv={zmuv}: moved by {moved:.3e} with the audio")
    assert moved > LIVE, moved
    f = Fused(al, lib, SEQ, sd, C)
    probs, logits = f.clips(buf.reshape(-1), sizes, L_max, L_max, zmuv=zmuv, null=null)
    worst = (0.0, 0.0)
    for n, L in enumerate(sizes):
        r = rows_of(L)
        assert refs[n].shape == (r, C)
        eager = eager_logits(al, lib, SEQ, sd, buf[n:n + 1, :L], f.fbp, f.zm if zmuv else None, tag=f"eager{n}.")[0]
        res = _verdict(f"seq clip {n} of L={sizes} ({r} rows) C={C} zmuv={zmuv}", logits[n, :r], probs[n, :r], eager, refs[n])
        worst = max(worst, res)
        assert not probs[n, r:].any() and not logits[n, r:].any(), (n, "rows behind the clip's own must be zeros")
    al.check()
    return worst


# ---- independence ----------------------------------------------------------------------------------------------------------------

def check_small_independence(al, lib, L=8000, C=4, N=5, ld=1008, many=257):
    """Window n alone (N = 1) and as row n of N overlapping windows, and a repeated launch: the same bits; `many` windows in one
    launch (more workgroups than compute units): rows 0, 1 and many - 1 equal their N = 1 bits and everything is finite."""
    sd = sharp_state(SMALL, C)
    flat = _pcm(1, (N - 1) * ld + L).reshape(-1)
    f = Fused(al, lib, SMALL, sd, C)
    probs, logits = f.windows(flat, N, L, ld, "all.")
    probs2, logits2 = f.windows(flat, N, L, ld, "again.")
    assert np.array_equal(probs, probs2) and np.array_equal(logits, logits2)
    assert np.isfinite(probs).all() and np.abs(logits[0] - logits[-1]).max() > 0      # the windows differ
    for n in range(N):
        p1, l1 = f.windows(flat[n * ld:n * ld + L].copy(), 1, L, L, f"solo{n}.")
        assert np.array_equal(p1[0], probs[n]) and np.array_equal(l1[0], logits[n]), n
    if many:
        rows = _pcm(many, L, seed=3)
        pm, lm = f.windows(rows.reshape(-1), many, L, L, "many.")
        assert np.isfinite(pm).all() and np.isfinite(lm).all()
        for n in (0, 1, many - 1):
            p1, l1 = f.windows(rows[n].copy(), 1, L, L, f"many.solo{n}.")
            assert np.array_equal(p1[0], pm[n]) and np.array_equal(l1[0], lm[n]), n
    al.check()


def check_seq_independence(al, lib, C=5):
    """The ragged launch of SEQ_CASES twice: the same bits; each of its clips alone (N = 1, L_max = its own length, another row
    stride and so another alignment of its samples): the bits of its rows in the ragged launch."""
    sizes = [c for c in SEQ_CASES if len(c[0]) == 5][0][0]
    sd = sharp_state(SEQ, C)
    buf, L_max = seq_inputs(sizes)
    f = Fused(al, lib, SEQ, sd, C)
    ld = L_max + 3      # rows 1 and 3 start on an odd sample: the per-sample load path
    flat = np.zeros((len(sizes) - 1) * ld + L_max, np.float32)
    for n in range(len(sizes)):
        flat[n * ld:n * ld + L_max] = buf[n]
    probs, logits = f.clips(flat, sizes, L_max, ld, "all.")
    probs2, logits2 = f.clips(flat, sizes, L_max, ld, "again.")
    assert np.array_equal(probs, probs2) and np.array_equal(logits, logits2)
    assert np.isfinite(probs).all() and np.isfinite(logits).all()
    for n, L in enumerate(sizes):
        r = rows_of(L)
        p1, l1 = f.clips(buf[n, :L].copy(), [L], L, L, f"solo{n}.")
        assert p1.shape == (1, r, C)
        assert np.array_equal(p1[0], probs[n, :r]) and np.array_equal(l1[0], logits[n, :r]), n
        assert np.abs(l1[0]).max() > 0
    al.check()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def check_refusals(al, lib, kind):
    """Every refusal of include/howl_hip_cnn_stream.h on a (N = 2, C = 4) problem of `kind`: the code, a message that names the entry
    point, nothing launched (probs, logits and the workspace keep their bytes) -- and the next valid call succeeds; the
    `supported`, `workspace_bytes` and `rows` tables with the zeros at and outside the edges."""
    from howl_amd import lib as LL
    N, C = 2, 4
    L = 5200 if kind == SMALL else 4000
    name = "howl_cnn_stream_windows" if kind == SMALL else "howl_cnn_stream_clips"
    lo, hi = (5000, 8199) if kind == SMALL else (800, 1638399)
    rows = 1 if kind == SMALL else rows_of(L)
    sd = sharp_state(kind, C)
    f = Fused(al, lib, kind, sd, C)
    pcm = al.buf("pcm", N * L, np.float32, np.zeros(N * L, np.float32))
    ns = al.buf("n_samples", N, np.int64, np.asarray([L, L - 900], np.int64))
    probs = al.buf("probs", (N, rows, C), np.float32, "sentinel")
    logits = al.buf("logits", (N, rows, C), np.float32, "sentinel")
    nws = int(lib.cdll.howl_cnn_stream_workspace_bytes(kind, N, L))
    assert nws > 0 and nws % 16 == 0
    ws = al.buf("ws", nws // 4, np.float32, "sentinel")
    watched = [probs, logits, ws]

    def snapshot():
        al.sync()
        return [np.array(al.get(v)).tobytes() for v in watched]

    def launch(null=None, L=L, M=40, C=C, N=N, ld=L, out_ld=rows * C, short=False, other=False):
        g = lambda key, v: None if null == key else al.ptr(v)      # noqa: E731
        pp = [None if null == k else al.ptr(f.p[k]) for k in cnn_util.PARAMS]
        bb = [None if null == k else al.ptr(f.p[k]) for k in cnn_util.BUFFERS]
        prm = None if null == "params" else ctypes.byref(LL.HowlCnnParams(*pp))
        buf = None if null == "buffers" else ctypes.byref(LL.HowlCnnBuffers(*bb))
        nb = nws - 4 if short else nws
        if (kind == SMALL) != other:
            return lib.cdll.howl_cnn_stream_windows(prm, buf, g("pcm", pcm), ld, N, L, g("fbp", f.fbp), M, 1e-7, al.ptr(f.zm), C,
                                                    g("probs", probs), al.ptr(logits), g("ws", ws), nb, None)
        return lib.cdll.howl_cnn_stream_clips(prm, buf, g("pcm", pcm), ld, N, L, al.ptr(ns), g("fbp", f.fbp), M, 1e-7, al.ptr(f.zm), C,
                                              g("probs", probs), al.ptr(logits), out_ld, g("ws", ws), nb, None)

    stats = [k for k in cnn_util.BUFFERS if not k.endswith("num_batches_tracked")]
    cases = [(dict(L=lo - 1), -1, f"L={lo - 1}"), (dict(L=hi + 1), -1, f"L={hi + 1}"), (dict(M=80), -1, "M=80"), (dict(C=0), -1, "C=0"),
             (dict(C=65), -1, "C=65"), (dict(N=0), -1, "N=0"), (dict(N=8193), -1, "N=8193"), (dict(ld=-1), -1, "negative"),
             (dict(short=True), -3, "workspace too small")] + \
            [(dict(null=k), -1, "null pointer") for k in ["params", "buffers", "pcm", "fbp", "probs", "ws"] + cnn_util.PARAMS + stats]
    if kind == SEQ:
        cases.append((dict(out_ld=rows * C - 1), -1, f"out_ld={rows * C - 1}"))
    for kw, code, text in cases:
        before = snapshot()
        rc = launch(**kw)
        msg = lib.cdll.howl_last_error().decode()
        assert rc == code, (kw, rc, msg)
        assert msg.startswith(name + ":") and text in msg, (kw, msg)
        assert snapshot() == before, (kw, "a refused call wrote something")
    # the other kind's launch refuses this kind's shape (its own range), and names itself
    if kind == SEQ:      # (4000 samples are no small-cnn window; a small-cnn window of 5200 samples IS a seq-cnn clip)
        before = snapshot()
        assert launch(other=True) == -1
        msg = lib.cdll.howl_last_error().decode()
        assert msg.startswith("howl_cnn_stream_windows:") and f"L={L}" in msg, msg
        assert snapshot() == before
    assert launch() == 0, lib.cdll.howl_last_error().decode()      # the next valid call succeeds
    # bn*_batches is not read: NULL is fine
    assert all(launch(null=k) == 0 for k in cnn_util.BUFFERS if k.endswith("num_batches_tracked")), lib.cdll.howl_last_error().decode()
    al.sync()
    assert np.isfinite(np.array(al.get(probs))).all() and np.isfinite(np.array(al.get(logits))).all()


def check_tables(lib):
    """`supported`, `workspace_bytes` and `rows`: ones / sizes / row counts inside the range, zeros at and just outside every edge
    and for the other kind's lengths."""
    c = lib.cdll
    for kind, L, M, C, ok in [(SMALL, 8000, 40, 4, 1), (SMALL, 5000, 40, 1, 1), (SMALL, 8199, 40, 64, 1), (SMALL, 4999, 40, 4, 0),
                              (SMALL, 8200, 40, 4, 0), (SMALL, 8000, 80, 4, 0), (SMALL, 8000, 40, 0, 0), (SMALL, 8000, 40, 65, 0),
                              (SEQ, 8000, 40, 4, 1), (SEQ, 800, 40, 1, 1), (SEQ, 1638399, 40, 64, 1), (SEQ, 799, 40, 4, 0),
                              (SEQ, 1638400, 40, 4, 0), (SEQ, 8000, 80, 4, 0), (SEQ, 8000, 40, 0, 0), (SEQ, 8000, 40, 65, 0),
                              (SMALL, 16000, 40, 4, 0), (SMALL, 800, 40, 4, 0), (2, 8000, 40, 4, 0), (-1, 8000, 40, 4, 0)]:
        assert c.howl_cnn_stream_supported(kind, L, M, C) == ok, (kind, L, M, C)
    for kind, N, L in [(SMALL, 0, 8000), (SMALL, 8193, 8000), (SMALL, 1, 4999), (SMALL, 1, 8200), (SMALL, -1, 8000), (SEQ, 0, 8000),
                       (SEQ, 8193, 8000), (SEQ, 1, 799), (SEQ, 1, 1638400), (2, 1, 8000), (SMALL, 1, 16000)]:
        assert c.howl_cnn_stream_workspace_bytes(kind, N, L) == 0, (kind, N, L)
    for kind, N, L in [(SMALL, 1, 5000), (SMALL, 8192, 8199), (SEQ, 1, 800), (SEQ, 8192, 1638399), (SEQ, 3, 16000)]:
        nb = c.howl_cnn_stream_workspace_bytes(kind, N, L)
        assert nb > 0 and nb % 16 == 0, (kind, N, L, nb)
    for kind, L in [(SMALL, 4999), (SMALL, 8200), (SEQ, 799), (SEQ, 1638400), (2, 8000), (SMALL, 16000)]:
        assert c.howl_cnn_stream_rows(kind, L) == 0, (kind, L)
    assert c.howl_cnn_stream_rows(SMALL, 5000) == c.howl_cnn_stream_rows(SMALL, 8199) == 2
    for r in (1, 2, R, R + 1, 2 * R + 1, 1024):
        lo, hi = seq_span(r)
        hi = min(hi, 1638399)
        assert c.howl_cnn_stream_rows(SEQ, lo) == c.howl_cnn_stream_rows(SEQ, hi) == r == c.howl_cnn_out_rows(SEQ, 1 + lo // 200), r
        assert c.howl_cnn_stream_rows(SEQ, lo - 1) == r - 1
    assert rows_of(1638399) == 1024


# ---- module level: the same code on the device and, inside emu_util.emulated_package(), on the emulator -------------------------

ENGINE_VOCAB = ["hey", "fire", "fox", "one", "two", "three", "four", "five", "six", "seven", "eight"]      # + [OOV]: 12 labels
# Model seeds of the engine checks, chosen on the float64 oracle so that every frame's decision is far from a tie (the margin
# below: the smallest of the top-two gap after reweighting, the smoothed maximum's distance from the threshold and the blank test's
# gap, over every frame) and the label history is not constant.  Found on the oracle (check_* print and assert them again):
#   small-cnn, C = 12, seed 21, the G8 clip's 37 windows:               margin 1.291e-02, 4 different labels (2 in the first five)
#   seq-cnn, C = 5, seed 25, 8000 + 16000 samples of synthetic_pcm 77:  margin 2.478e-03, 3 different labels
#   seq-cnn, C = 5, seed 25, the six clips of MANY_SIZES:               margin 3.451e-03, 3 different labels
# against an eager error of 1e-7 .. 1e-6 on the probabilities: three to four orders of magnitude.  Seeds tried and not taken:
# small-cnn 33 and seq-cnn 27, 23, 24, 46 decide one label everywhere; small-cnn 25 (1.6e-04) and seq-cnn 22 (4.0e-04) are closer.
ENGINE_SEED = {SMALL: 21, SEQ: 25}
MANY_SIZES = [27200, 9000, 5800, 2599, 1000, 800]      # 17 rows (three tiles) .. 1 row


def decision_margin(probs, stamps, mode, blank, weights=1, threshold=0.0, smoothing_ms=50.0):
    """The engines' per-frame decisions replayed in float64 on (frames, C) oracle probabilities -> (the smallest distance of any of
    them from its tie, the labels decided).  mode 0: InferenceEngine._run_frames (frames whose arg-max is `blank` are skipped: the
    blank test is a top-two gap); 1: FrameInferenceEngine's loop.  The quantities: the top-two gap of the reweighted frame, the
    top-two gap of the smoothed envelope, the envelope maximum's distance from the threshold."""
    margin, labels, frames = np.inf, [], []
    for now, p in zip(stamps, np.asarray(probs, np.float64)):
        p = p * weights
        p = p / p.sum()
        top = np.sort(p)
        margin = min(margin, top[-1] - top[-2])
        if mode == 0 and int(p.argmax()) == blank:
            continue
        frames.append((now, p))
        while now - frames[0][0] > smoothing_ms:
            frames.pop(0)
        env = np.max(np.vstack([q for _, q in frames]), axis=0)
        top = np.sort(env)
        margin = min(margin, top[-1] - top[-2], abs(top[-1] - threshold))
        labels.append(int(env.argmax()))
    return float(margin), labels


def _zmuv(golden, dev):
    from howl_amd.data.transform.operator import ZmuvTransform
    g4 = golden("g4_zmuv")
    zmuv = ZmuvTransform().to(dev)
    for k in ("mean", "mean2", "total"):
        getattr(zmuv, k).copy_(torch.from_numpy(np.asarray(g4[k])))
    return zmuv


def _model(kind, C, dev, sd=None):
    from howl_amd.model import CnnSettings, RegisteredModel
    model = RegisteredModel.find_registered_class("small-cnn" if kind == SMALL else "seq-cnn")(C, CnnSettings(num_labels=C))
    model.load_state_dict({k: v.clone() for k, v in (sd or sharp_state(kind, C, ENGINE_SEED[kind])).items()})
    return model.to(dev).eval()


def small_engine(golden, dev, fused, max_window_ms=500):
    """A FrameInferenceEngine (500 ms windows, 63 ms stride) over a small-cnn model with the sharpened state for C = 12 and the ZMUV
    statistics of golden G4."""
    from howl_amd.context import InferenceContext
    from howl_amd.model.inference import FrameInferenceEngine
    ctx = InferenceContext(ENGINE_VOCAB, token_type="word")
    assert ctx.num_labels == 12
    engine = FrameInferenceEngine(max_window_ms, 63, _model(SMALL, 12, dev), _zmuv(golden, dev), ctx)
    if fused is not None:
        engine.fused_windows = fused
    engine.std = engine.std.to(dev)
    return engine


def seq_engine(golden, dev, fused, decide=False):
    """An InferenceEngine over a seq-cnn model with the sharpened state for C = 5 (three words, OOV, blank = 4)."""
    from howl_amd.context import InferenceContext
    from howl_amd.model.inference import InferenceEngine
    ctx = InferenceContext(["hey", "fire", "fox"], token_type="word", use_blank=True)
    assert ctx.num_labels == 5 and ctx.blank_label == 4
    engine = InferenceEngine(_model(SEQ, 5, dev).streaming(), _zmuv(golden, dev), ctx)
    if fused is not None:
        engine.fused_chunks = fused
    engine.device_decisions = decide
    engine.std = engine.std.to(dev)
    return engine


def windows_of(clip, engine):
    from howl_amd.utils import audio_utils
    starts, chunk = audio_utils.stride_starts(clip.size(-1), engine.max_window_size_ms, engine.eval_stride_size_ms, engine.sample_rate)
    return clip.as_strided((len(starts), chunk), (starts[1] - starts[0], 1)), starts, chunk


SMALL_CHAIN = ("howl_logmel_fwd", "howl_cnn_fwd")


def check_small_engine(golden, dev, library, first=None):
    """The G8 clip's 37 windows through ingest_frame, fused and eager: the same label history, exactly one howl_cnn_stream_windows
    per window and no frontend / cnn launch on the fused path -- after asserting on the fp64 oracle that every window's decision
    is further than 100 e_eager from its tie and that the history holds at least two labels.  `first`: the emulator's form, the
    clip cut behind its first `first` windows (the oracle's conditions still cover all 37)."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        whole = torch.from_numpy(np.asarray(g["clip"]))
        engine = small_engine(golden, dev, False)
        all_windows, all_starts, chunk = windows_of(whole, engine)
        assert len(all_starts) == 37 and chunk == 8000
        sd = {k: v.detach().cpu() for k, v in engine.model.state_dict().items()}
        pair = engine.zmuv.pair().cpu().numpy()
        ref = softmax64(oracle_logits64(SMALL, sd, all_windows.numpy(), pair, key="g8"))
        margin, labels = decision_margin(ref, [63.0 * i for i in range(37)], 1, None, 1, engine.threshold, engine.smoothing_window_ms)
        W = 37 if first is None else first
        clip = whole[:all_starts[W - 1] + chunk].contiguous().to(dev)
        hist = {}
        for fused in (False, True):
            engine = small_engine(golden, dev, fused)
            windows, starts, chunk = windows_of(clip, engine)
            assert len(starts) == W
            with CallLog(library) as log:
                for i, s in enumerate(starts):
                    engine.ingest_frame(clip[s:s + chunk], curr_time=float(engine.eval_stride_size_ms * i))
            hist[fused] = np.array(engine.label_history, dtype=np.float64)
            if fused:
                assert log.names.count("howl_cnn_stream_windows") == W, log.names
                assert not set(SMALL_CHAIN) & set(log.names), log.names
            else:
                assert log.names.count("howl_cnn_fwd") == W and "howl_cnn_stream_windows" not in log.names, log.names
        with CallLog(library) as log:
            fusedp = engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
        assert log.names.count("howl_cnn_stream_windows") == 1, log.names
        engine.fused_windows = False
        eager = engine.window_probabilities(clip)
        e_fused, e_eager = np.abs(fusedp - ref[:W]).max(), np.abs(eager - ref[:W]).max()
        print(f"G8 clip, small-cnn: decision margin {margin:.3e} over 37 windows, oracle labels {labels}; {W} windows in one launch: "
              f"e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
        assert margin > 100 * e_eager, (margin, e_eager)
        assert len(set(labels)) >= 2 and len(set(hist[False][:, 1].tolist())) >= (2 if first is None else 1)
        assert hist[False][:, 1].tolist() == [float(v) for v in labels[:W]]
        assert hist[True].shape[0] == W and np.array_equal(hist[True], hist[False]), (hist[True], hist[False])
        assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
    finally:
        SETTINGS.reset()


def check_small_switch(golden, dev, monkeypatch):
    """The switch is opt-in, and a 1 s window (outside the kernel's range) keeps the chain."""
    from howl_amd.model.cnn import SmallCnnStreamSession
    from howl_amd.model.inference import FrameInferenceEngine
    monkeypatch.delenv("HOWL_STREAM_FUSED", raising=False)
    e = small_engine(golden, dev, fused=None)
    assert FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context).fused_windows is False
    monkeypatch.setenv("HOWL_STREAM_FUSED", "1")
    on = FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context)
    assert on.fused_windows is True
    on.std = on.std.to(dev)
    assert isinstance(on._fused_session(torch.zeros(8000, device=dev)), SmallCnnStreamSession)
    assert on._fused_session(torch.zeros(16000, device=dev)) is None


SEQ_CHAIN = ("howl_logmel_fwd", "howl_cnn_fwd")


def _seq_oracle_probs(engine, clip):
    sd = {k: v.detach().cpu() for k, v in engine.model.state_dict().items()}
    pair = engine.zmuv.pair().cpu().numpy()
    return softmax64(oracle_logits64(SEQ, sd, clip.numpy()[None], pair)[0])


def _seq_margin(engine, clips):
    """decision_margin over the frames of every clip (each from a reset engine, as infer_many runs them)."""
    margin, labels = np.inf, []
    for c in clips:
        p = _seq_oracle_probs(engine, c)
        delta = int(c.numel() / engine.sample_rate * 1000) / len(p)
        m, ls = decision_margin(p, [delta * (i + 1) for i in range(len(p))], 0, engine.blank_idx, 1, engine.threshold, engine.smoothing_window_ms)
        margin, labels = min(margin, m), labels + ls
    return margin, labels


def _eager_probability_error(engine, clips, dev):
    """The eager chain's error on the probabilities against the oracle (what the margins are measured in)."""
    worst = 0.0
    for c in clips:
        x = engine.std.log_mel_for_model(c.to(dev).unsqueeze(0), engine.zmuv)
        with torch.no_grad():
            p = engine.model(x, None).softmax(-1).squeeze(1).cpu().numpy()
        worst = max(worst, float(np.abs(p - _seq_oracle_probs(engine, c)).max()))
    return worst


def check_seq_infer(golden, dev, library):
    """InferenceEngine.infer on an 8000- and a 16000-sample chunk with fused_chunks off and on: identical label_history and return
    values, one howl_cnn_stream_clips per chunk and nothing of the chain -- after the oracle's margins."""
    from howl_amd.settings import SETTINGS
    from howl_amd.utils.synth import synthetic_pcm
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        pcm = synthetic_pcm(2, 16000, seed=77)
        chunks = [pcm[0, :8000].clone(), pcm[1].clone()]
        engine = seq_engine(golden, dev, False)
        margin, labels = _seq_margin(engine, chunks)
        e_eager = _eager_probability_error(engine, chunks, dev)
        print(f"seq-cnn infer: decision margin {margin:.3e} over {sum(rows_of(c.numel()) for c in chunks)} frames, oracle labels {labels}, "
              f"e_eager={e_eager:.3e}")
        assert margin > 100 * e_eager, (margin, e_eager)
        got = {}
        for fused in (False, True):
            engine = seq_engine(golden, dev, fused)
            with CallLog(library) as log:
                res = [bool(engine.infer(c.to(dev))) for c in chunks]
            got[fused] = (res, list(engine.label_history))
            if fused:
                assert log.names.count("howl_cnn_stream_clips") == 2 and not set(SEQ_CHAIN) & set(log.names), log.names
            else:
                assert log.names.count("howl_cnn_fwd") == 2 and "howl_cnn_stream_clips" not in log.names, log.names
        assert len({l for _, l in got[False][1]}) >= 2, got[False][1]
        assert got[True] == got[False], (got[True], got[False])
    finally:
        SETTINGS.reset()


def check_seq_infer_many(golden, dev, library):
    """infer_many over six ragged clips (one of them three tiles long) against the per-clip loop, with device_decisions off and on:
    identical results and clip_histories, ONE howl_cnn_stream_clips for all clips -- after the oracle's margins."""
    from howl_amd.settings import SETTINGS
    from howl_amd.utils.synth import synthetic_pcm
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        assert rows_of(MANY_SIZES[0]) > 2 * R
        pcm = synthetic_pcm(len(MANY_SIZES), max(MANY_SIZES), seed=77)
        clips = [pcm[i, :n].clone() for i, n in enumerate(MANY_SIZES)]
        engine = seq_engine(golden, dev, False)
        margin, labels = _seq_margin(engine, clips)
        e_eager = _eager_probability_error(engine, clips, dev)
        print(f"seq-cnn infer_many: decision margin {margin:.3e} over {sum(rows_of(n) for n in MANY_SIZES)} frames, oracle labels "
              f"{sorted(set(labels))}, e_eager={e_eager:.3e}")
        assert margin > 100 * e_eager, (margin, e_eager)
        dclips = [c.to(dev) for c in clips]
        with CallLog(library) as log:
            want = engine.infer_many(dclips)      # fused_chunks off: the per-clip loop
        hists = [list(h) for h in engine.clip_histories]
        assert log.names.count("howl_cnn_fwd") == len(clips) and "howl_cnn_stream_clips" not in log.names, log.names
        assert len({l for h in hists for _, l in h}) >= 2, hists
        for decide in (False, True):
            engine = seq_engine(golden, dev, True, decide=decide)
            with CallLog(library) as log:
                got = engine.infer_many(dclips)
            assert log.names.count("howl_cnn_stream_clips") == 1 and not set(SEQ_CHAIN) & set(log.names), log.names
            assert log.names.count("howl_decide_clips") == (1 if decide else 0), log.names
            assert got == want, (decide, got, want)
            assert [list(h) for h in engine.clip_histories] == hists, decide
            assert engine.label_history == []      # left reset
    finally:
        SETTINGS.reset()


def check_session(kind, dev, C=4):
    """The session reads the model in place: the next call answers for the new weights with no refresh, after load_state_dict,
    after an in-place parameter write and after a running-statistics write that torch's version counters do not see (the oracle
    bound, the eager module path as the yardstick); the training-mode refusal and the shape refusal leave std.rand where it was;
    supported() follows the range, 80 mel bins and a train-mode VTLP frontend."""
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.utils.synth import synthetic_pcm
    N, L = 2, (5400 if kind == SMALL else 4000)
    first, other = sharp_state(kind, C, 21), sharp_state(kind, C, 23)
    model = _model(kind, C, dev, first)
    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    rows = synthetic_pcm(N, L)
    pcm = rows.to(dev)
    zmuv.update(std(pcm))
    pair = zmuv.pair().cpu().numpy()
    session = model.stream_session(std, zmuv)
    assert not hasattr(session, "refresh")
    if kind == SMALL:
        assert session.supported(L) and session.supported(5000) and session.supported(8199)
        assert not session.supported(4999) and not session.supported(8200)
    else:
        assert session.supported(L) and session.supported(800) and session.supported(1638399)
        assert not session.supported(799) and not session.supported(1638400)
        assert [session.rows_of(n) for n in (800, 2399, 2400, 16000)] == [1, 1, 2, 10]

    def both():
        shape = (N, C) if kind == SMALL else (N, rows_of(L), C)
        logits = torch.empty(shape, dtype=torch.float32, device=dev)
        if kind == SMALL:
            probs = session.probabilities(pcm, logits=logits)
        else:
            probs, state = session.probabilities(pcm, logits=logits)
            assert state is None
        with torch.no_grad():
            eager = model(std.log_mel_for_model(pcm, zmuv), None)
        eager = eager if kind == SMALL else eager.permute(1, 0, 2)
        return probs.cpu().numpy(), logits.cpu().numpy(), eager.cpu().numpy()

    def verdict(sd, what):
        probs, logits, eager = both()
        ref = oracle_logits64(kind, sd, rows.numpy(), pair)
        _verdict(f"session ({what})", logits, probs, eager, ref)
        return ref

    ref1 = verdict(first, "first state")
    model.load_state_dict({k: v.clone() for k, v in other.items()})
    ref2 = verdict(other, "after load_state_dict")
    assert np.abs(ref1 - ref2).max() > 1e-2      # the two models do differ
    model.output[3].bias.data.add_(0.5)          # `.data` shares the storage, not the version counter
    third = {k: v.clone() for k, v in other.items()}
    third["output.3.bias"] = third["output.3.bias"] + 0.5
    ref3 = verdict(third, "after an in-place parameter write")
    assert np.abs(ref3 - ref2).max() > 0.4
    model.encoder2[3].running_mean.data.add_(0.25)
    fourth = {k: v.clone() for k, v in third.items()}
    fourth["encoder2.3.running_mean"] = fourth["encoder2.3.running_mean"] + 0.25
    ref4 = verdict(fourth, "after a running-statistics write")
    assert np.abs(ref4 - ref3).max() > 1e-2
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
        # the two refusals come before the frontend's draw
        state = std.rand.getstate()
        model.train()
        try:
            session.probabilities(pcm)
        except RuntimeError as e:
            assert "eval" in str(e)
        else:
            raise AssertionError("training mode must raise")
        finally:
            model.eval()
        try:
            session.probabilities(pcm[:, :700])
        except ValueError as e:
            assert "outside the streaming kernel's range" in str(e)
        else:
            raise AssertionError("a shape outside the range must raise")
        assert std.rand.getstate() == state
        session.probabilities(pcm)
        assert std.rand.getstate() != state      # a call that runs does draw
    finally:
        std.augment_params[0].enabled = False
        std.eval()
    if kind == SEQ:
        try:
            session.probabilities(pcm, state=(None, None))
        except ValueError as e:
            assert "no state" in str(e)
        else:
            raise AssertionError("a state must raise")
