"""Refused lstm / head calls through the raw C ABI (bodies shared by tests/test_emu_lstm.py and tests/test_gpu_lstm.py): a call
that returns an error must have launched nothing.  Every output buffer, saved tensor, gradient and workspace of a problem
(B=3, T=4, M=40, head 128 -> 256 -> 5) is filled with the sentinel of tests/guard_mem.py; a case asserts the status code, the
entry point named in the error text, and that the refused call changed none of those buffers.  ``al`` is guard_mem's allocator
interface: Arena on the emulator (guard pages), Banded on the device (sentinel bands)."""
import ctypes
import json
from pathlib import Path

import numpy as np

from guard_mem import sentinel_mask
from howl_amd.lib import (FB_PACKED_FLOATS, MAX_MELS, HowlHeadGrads, HowlHeadParams, HowlLogmelArgs, HowlLstmGrads, HowlLstmParams,
                          HowlLstmSaved)

E_ARG, E_WORKSPACE = -1, -3
B, T, C = 3, 4, 5
SIZES = json.loads((Path(__file__).resolve().parent / "golden" / "lstm_workspace_sizes.json").read_text())


class Problem:
    def __init__(self, al, lib, M=40, x_frames=0, t_out=T, gx=True):
        self.al, self.lib, self.M = al, lib, M
        rng = np.random.default_rng(3)
        rnd = lambda name, *shape: al.buf(name, shape, np.float32, (rng.standard_normal(shape) * 0.2).astype(np.float32))
        self.guarded = {}

        def out(name, shape, dtype=np.float32):
            self.guarded[name] = al.buf(name, shape, dtype, "sentinel")
            return self.guarded[name]

        self.x = rnd("x", B, x_frames or T, M)
        self.lengths = al.buf("lengths", B, np.int64, np.array([4, 3, 1], np.int64))
        w = [rnd("w_ih", 512, M), rnd("w_hh", 512, 128), rnd("b_ih", 512), rnd("b_hh", 512)]
        self.prm = HowlLstmParams(*[al.ptr(a) for a in w])
        saved = [out("gx", (B, T, 512)), out("gates", (B, T, 512)), out("c", (B, T, 128)), out("hseq", (B, T + 1, 128)), out("dgates", (B, T, 512))]
        self.sv = HowlLstmSaved(al.ptr(saved[0]) if gx else None, *[al.ptr(a) for a in saved[1:]], t_out, x_frames)
        self.hT, self.cT = out("hT", (B, 128)), out("cT", (B, 128))
        self.ws = out("ws", int(lib.cdll.howl_lstm_workspace_bytes(B, T)), np.uint8)
        self.grads = HowlLstmGrads(*[al.ptr(out("d" + n, a.shape)) for n, a in zip(("w_ih", "w_hh", "b_ih", "b_hh"), w)])
        self.dy = rnd("dy", B, T, 128)
        # the head, on hidden states of its own (an input here: howl_seq_lstm_bwd reads them from saved->hseq)
        hw = [rnd("w1", 256, 128), rnd("b1", 256), rnd("w2", C, 256), rnd("b2", C)]
        self.hp = HowlHeadParams(*[al.ptr(a) for a in hw])
        self.hgrads = HowlHeadGrads(*[al.ptr(out("d" + n, a.shape)) for n, a in zip(("w1", "b1", "w2", "b2"), hw)])
        self.dz1, self.dhs = out("dz1", (B * T, 256)), out("dhs", (B, T, 128))
        self.head_ws = out("head_ws", int(lib.cdll.howl_head_workspace_bytes(128, 256, C)), np.uint8)

    def snapshot(self):
        self.al.sync()
        return {k: np.array(self.al.get(v)) for k, v in self.guarded.items()}

    def refused(self, name, args, rc, who, untouched=True, exact=True):
        """Calls ``name``; asserts status, the whole error text ``who`` (``exact=False``: that it names ``who``), and that no
        guarded buffer changed (``untouched``: that each still holds only the sentinel)."""
        before = self.snapshot()
        got = getattr(self.lib.cdll, name)(*args)
        text = self.lib.cdll.howl_last_error().decode()
        after = self.snapshot()
        assert got == rc, (got, text)
        assert text == who if exact else who in text, text
        for k in before:
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), f"{name} was refused ({text}) but wrote {k}"
            if untouched:
                assert sentinel_mask(after[k]).all(), k
        return text

    def fwd_args(self):
        al = self.al
        return (ctypes.byref(self.prm), al.ptr(self.x), B, T, self.M, al.ptr(self.lengths), None, None, ctypes.byref(self.sv), al.ptr(self.hT),
                al.ptr(self.cT), al.ptr(self.ws), self.ws_bytes(self.ws), None)

    @staticmethod
    def ws_bytes(ws):
        return ws.nbytes if isinstance(ws, np.ndarray) else ws.numel()      # (the device allocator hands out byte views)

    def bwd_args(self, short=0):
        al = self.al
        return (ctypes.byref(self.prm), al.ptr(self.x), B, T, self.M, al.ptr(self.lengths), None, ctypes.byref(self.sv), al.ptr(self.dy), None,
                None, ctypes.byref(self.grads), al.ptr(self.ws), self.ws_bytes(self.ws) - short, None)

    def seq_bwd_args(self, y1, dy2, short=1):
        al = self.al
        return (ctypes.byref(self.hp), 256, C, al.ptr(y1), al.ptr(dy2), al.ptr(self.dz1), al.ptr(self.dhs), ctypes.byref(self.hgrads), None,
                al.ptr(self.head_ws), self.ws_bytes(self.head_ws), ctypes.byref(self.prm), al.ptr(self.x), B, T, self.M, al.ptr(self.lengths),
                None, ctypes.byref(self.sv), ctypes.byref(self.grads), al.ptr(self.ws), self.ws_bytes(self.ws) - short, None, None)


def check_fwd_x_frames(al, lib):
    p = Problem(al, lib, x_frames=T - 1)
    p.refused("howl_lstm_fwd", p.fwd_args(), E_ARG, f"howl_lstm_fwd: x_frames={T - 1} < T={T}")


def check_fwd_gx_null(al, lib, monkeypatch):
    monkeypatch.setenv("HOWL_LSTM_ROWS", "16")      # the 16-row recurrence needs the projection buffer (and a packing launch)
    p = Problem(al, lib, gx=False)
    assert lib.cdll.howl_lstm_needs_gx(ctypes.byref(p.prm), B, T, 40, 0) == 1
    p.refused("howl_lstm_fwd", p.fwd_args(), E_ARG,
              "howl_lstm_fwd: saved->gx is NULL but this shape runs the projection GEMM (howl_lstm_needs_gx)")


def check_bwd_too_many_features(al, lib):
    p = Problem(al, lib, M=MAX_MELS + 1)
    p.refused("howl_lstm_bwd", p.bwd_args(), E_ARG,
              f"howl_lstm_bwd: M={MAX_MELS + 1} input features exceed the workspace layout (max {MAX_MELS})")


def check_bwd_x_frames(al, lib):
    p = Problem(al, lib, x_frames=T - 1)
    p.refused("howl_lstm_bwd", p.bwd_args(), E_ARG, f"howl_lstm_bwd: x_frames={T - 1} < T={T}")


def check_bwd_t_out(al, lib):
    p = Problem(al, lib, t_out=T + 1)
    p.refused("howl_lstm_bwd", p.bwd_args(), E_ARG, f"howl_lstm_bwd: t_out={T + 1} outside 1..T")


def check_bwd_workspace(al, lib):
    p = Problem(al, lib)
    p.refused("howl_lstm_bwd", p.bwd_args(short=1), E_WORKSPACE, "howl_lstm_bwd: workspace too small")


def _finite_hidden_states(p):
    """saved->hseq as a forward would have left it (here: random): the head reads it as its input."""
    rng = np.random.default_rng(4)
    hseq = p.al.buf("hseq_in", (B, T + 1, 128), np.float32, (rng.standard_normal((B, T + 1, 128)) * 0.5).astype(np.float32))
    p.sv.hseq = p.al.ptr(hseq).value
    del p.guarded["hseq"]
    return hseq


def check_seq_bwd_workspace_with_dy2(al, lib):
    """The LSTM half refuses (its workspace is one byte short): the head half must not have run.  The text is the LSTM half's."""
    p = Problem(al, lib)
    _finite_hidden_states(p)
    rng = np.random.default_rng(5)
    y1 = al.buf("y1", (B * T, 256), np.float32, np.abs(rng.standard_normal((B * T, 256))).astype(np.float32))
    dy2 = al.buf("dy2", (B * T, C), np.float32, rng.standard_normal((B * T, C)).astype(np.float32))
    p.refused("howl_seq_lstm_bwd", p.seq_bwd_args(y1, dy2), E_WORKSPACE, "howl_lstm_bwd: workspace too small")


def check_seq_bwd_workspace_after_seq_head_ctc(al, lib, monkeypatch):
    """The same after a real howl_seq_head_ctc: dz1, dhs and the head workspace as that call left them, everything else untouched."""
    monkeypatch.setenv("HOWL_ROWGEMM_MIN_ROWS", "1")      # the fused launch covers B * T = 12 rows
    p = Problem(al, lib)
    hseq = _finite_hidden_states(p)
    assert lib.cdll.howl_seq_head_ctc_supported(B, T, 128, 256, C, 2) == 1
    targets = al.buf("targets", (B, 2), np.int64, np.array([[0, 1], [2, 0], [3, 3]], np.int64))
    tl = al.buf("tl", B, np.int64, np.array([2, 1, 0], np.int64))
    y2, nll = al.buf("y2", (B * T, C), np.float32, "sentinel"), al.buf("nll", B, np.float32, "sentinel")
    h1 = ctypes.c_void_p(al.ptr(hseq).value + 128 * 4)      # row (b, t) = hseq[b][t + 1]
    lib.call("howl_seq_head_ctc", ctypes.byref(p.hp), h1, (T + 1) * 128, 128, B, T, 128, 256, C, al.ptr(targets), 2, 2, al.ptr(p.lengths),
             al.ptr(tl), C - 1, al.ptr(y2), al.ptr(nll), al.ptr(p.dz1), al.ptr(p.dhs), al.ptr(p.head_ws), p.ws_bytes(p.head_ws), None)
    al.sync()
    assert not sentinel_mask(al.get(p.dz1)).any() and not sentinel_mask(al.get(p.dhs)).any()
    p.refused("howl_seq_lstm_bwd", p.seq_bwd_args(None, None), E_WORKSPACE, "howl_lstm_bwd: workspace too small", untouched=False)


def check_fwd_next_refused_frontend(al, lib):
    """howl_lstm_fwd_next with a next batch that howl_logmel_fwd refuses (too short for the reflect padding): nothing of the
    recurrence runs, and the text is the frontend's."""
    p = Problem(al, lib)
    pcm = al.buf("pcm", (2, 100), np.float32, 0.1)
    fbp = al.buf("fbp", FB_PACKED_FLOATS, np.float32, 0.0)
    feat = p.guarded["feat"] = al.buf("feat", (2, 1, 40), np.float32, "sentinel")
    nxt = HowlLogmelArgs(al.ptr(pcm), 2, 100, 100, al.ptr(fbp), 40, 1e-7, None, al.ptr(feat), 1)
    p.refused("howl_lstm_fwd_next", p.fwd_args()[:-1] + (ctypes.byref(nxt), None), E_ARG, "howl_logmel_fwd", exact=False)


def check_size_queries(lib):
    """The two workspace queries against the values recorded from the commit before the launch plans (tests/golden)."""
    for b, t, nbytes in SIZES["howl_lstm_workspace_bytes"]["rows"]:
        assert lib.cdll.howl_lstm_workspace_bytes(b, t) == nbytes, (b, t)
    for n_in, n_hid, n_out, nbytes in SIZES["howl_head_workspace_bytes"]["rows"]:
        assert lib.cdll.howl_head_workspace_bytes(n_in, n_hid, n_out) == nbytes, (n_in, n_hid, n_out)
