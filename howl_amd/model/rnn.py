"""``SequentialLstm`` ("seq-lstm") and ``SimpleLstm`` ("lstm") of ``howl/model/rnn.py:41-91`` on MI355X kernels
(``howl_amd/csrc/lstm.hip``): packed-sequence LSTM(40 -> 128) + Linear(128,256)-ReLU-Linear(256,C); ``SimpleGru`` ("gru") of
``howl/model/rnn.py:94-130`` on ``howl_amd/csrc/gru.hip``: conv encoder + GRU(40 -> 96) + Linear-ReLU-Dropout-Linear;
``LASClassifier`` ("las") of ``howl/model/rnn.py:133-215`` on ``howl_amd/csrc/las.hip``: conv encoder + bidirectional
LSTM(352 -> 96) + four-head fixed attention + Linear-ReLU-Dropout-Linear.

Same construction order / ``state_dict`` keys (``lstm.weight_ih_l0 ...``, ``dnn.0.*``, ``dnn.2.*``), same call protocol
``model(x: (B, C>=1, M, T), lengths)`` and streaming-state protocol as the reference; ``nn.LSTM`` / ``nn.Linear`` are
parameter containers only.  Like ``pack_padded_sequence`` the lengths must be sorted in decreasing order.
"""
import ctypes
from typing import Any

import torch
import torch.nn as nn

from howl_amd import lib as _lib
from howl_amd import ops, parallel
from howl_amd.settings import _EnvSettings

from .base import RegisteredModel
from .stream import PreparedStreamSession, StreamSession

__all__ = ["FixedAttentionModuleConfig", "GruStreamSession", "LASClassifier", "LASClassifierConfig", "LASEncoderConfig",
           "LasStreamSession", "LstmConfig", "LstmStreamSession", "SequentialLstm", "SimpleGru", "SimpleLstm"]

HID = 128


class LstmConfig(_EnvSettings):
    num_mels: int = 40
    hidden_size: int = 128
    num_labels: int = 2


class LASEncoderConfig(_EnvSettings):
    num_mels: int = 40
    num_spec_channels: int = 3
    num_latent_channels: int = 8
    hidden_size: int = 96
    num_layers: int = 1
    use_maxpool: bool = True


class FixedAttentionModuleConfig(_EnvSettings):
    num_heads: int = 4
    hidden_size: int = 96


class LASClassifierConfig(_EnvSettings):
    dnn_size: int = 256
    dropout: float = 0.1
    las_config: LASEncoderConfig = None              # None: the defaults
    fixed_attn_config: FixedAttentionModuleConfig = None

    def __init__(self, **overrides):
        super().__init__(**overrides)
        self.las_config = self.las_config or LASEncoderConfig()
        self.fixed_attn_config = self.fixed_attn_config or FixedAttentionModuleConfig()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _x_frames(x):
    """Frames per utterance of the buffer behind x (B,T,M): a leading-frames view of a longer (B,T_x,M) feature buffer is used in
    place (``HowlLstmSaved.x_frames``)."""
    M = x.shape[2]
    # (the stride of a one-frame time axis is never used to address anything -- and torch leaves it arbitrary, e.g. 1 after
    # permute(0, 2, 1).contiguous() of a (B, M, 1) tensor)
    if x.stride(2) != 1 or (x.shape[1] > 1 and x.stride(1) != M) or x.stride(0) % M or x.stride(0) < x.shape[1] * M:
        raise ValueError("LSTM input must be a (B,T,M) tensor with contiguous rows and a whole number of frames per utterance")
    return x.stride(0) // M


def _lstm_forward_raw(x, lengths, t_out, h0, c0, w_ih, w_hh, b_ih, b_hh, next_logmel=None):
    """``howl_lstm_fwd`` on x (B,T,M), contiguous or the leading frames of a longer contiguous buffer: returns (hs (B,t_out,128)
    view, hT, cT, saved buffers for the backward).  ``next_logmel``: a ``HowlLogmelArgs`` record -- the frontend of the NEXT batch
    runs with this call (``howl_lstm_fwd_next``: as rider blocks of the recurrence's launch where that leaves CUs idle)."""
    B, T, M = x.shape
    dev = x.device
    f32 = dict(dtype=torch.float32, device=dev)
    bufs = dict(gates=torch.empty((B, T, 4 * HID), **f32), c=torch.empty((B, T, HID), **f32),
                hseq=torch.empty((B, T + 1, HID), **f32))
    ws = torch.empty(_lib.get().cdll.howl_lstm_workspace_bytes(B, T), dtype=torch.uint8, device=dev)
    hT, cT = torch.empty((B, HID), **f32), torch.empty((B, HID), **f32)
    prm = _lib.HowlLstmParams(_vp(w_ih), _vp(w_hh), _vp(b_ih), _vp(b_hh))
    xf = _x_frames(x)
    # the (B, T, 512) projection buffer only where the library runs the projection GEMM (40 MB at 512 x 38 otherwise unused)
    gx = torch.empty((B, T, 4 * HID), **f32) if _lib.get().cdll.howl_lstm_needs_gx(ctypes.byref(prm), B, T, M, xf) else None
    sv = _lib.HowlLstmSaved(_vp(gx), _vp(bufs["gates"]), _vp(bufs["c"]), _vp(bufs["hseq"]), None, t_out, xf)
    if next_logmel is not None:
        _lib.get().call("howl_lstm_fwd_next", ctypes.byref(prm), _vp(x), B, T, M, _vp(lengths), _vp(h0), _vp(c0), ctypes.byref(sv),
                        _vp(hT), _vp(cT), _vp(ws), ws.numel(), ctypes.byref(next_logmel), ops._stream())
    else:
        _lib.get().call("howl_lstm_fwd", ctypes.byref(prm), _vp(x), B, T, M, _vp(lengths), _vp(h0), _vp(c0), ctypes.byref(sv),
                        _vp(hT), _vp(cT), _vp(ws), ws.numel(), ops._stream())
    saved = (x, lengths, c0, w_ih, w_hh, b_ih, b_hh, bufs["gates"], bufs["c"], bufs["hseq"], ws)
    return bufs["hseq"][:, 1:t_out + 1], hT, cT, saved


def _lstm_backward_raw(saved, t_out, d_hs, d_hT, d_cT, grads=None):
    """``howl_lstm_bwd``: gradients of (w_ih, w_hh, b_ih, b_hh), written into ``grads`` when given (flat-buffer views)."""
    x, lengths, c0, w_ih, w_hh, b_ih, b_hh, gates, cs, hseq, ws = saved
    B, T, M = x.shape
    dy = None
    if d_hs is not None:
        if t_out == T and d_hs.is_contiguous():
            dy = d_hs
        elif t_out == T:
            dy = d_hs.contiguous()
        else:
            dy = torch.zeros((B, T, HID), dtype=torch.float32, device=x.device)
            dy[:, :t_out].copy_(d_hs)
    d_hT = None if d_hT is None else d_hT.contiguous()
    d_cT = None if d_cT is None else d_cT.contiguous()
    dgates = torch.empty((B, T, 4 * HID), dtype=torch.float32, device=x.device)
    if grads is None:
        grads = [torch.empty_like(p) for p in (w_ih, w_hh, b_ih, b_hh)]
    prm = _lib.HowlLstmParams(_vp(w_ih), _vp(w_hh), _vp(b_ih), _vp(b_hh))
    sv = _lib.HowlLstmSaved(None, _vp(gates), _vp(cs), _vp(hseq), _vp(dgates), t_out, _x_frames(x))
    gr = _lib.HowlLstmGrads(*[_vp(g) for g in grads])
    _lib.get().call("howl_lstm_bwd", ctypes.byref(prm), _vp(x), B, T, M, _vp(lengths), _vp(c0), ctypes.byref(sv), _vp(dy),
                    _vp(d_hT), _vp(d_cT), ctypes.byref(gr), _vp(ws), ws.numel(), ops._stream())
    return grads


class _LstmFunction(torch.autograd.Function):
    """x (B,T,M) contiguous, lengths (B) int64 on the device or None -> (hs (B,t_out,128) view, hT (B,128), cT (B,128))."""

    @staticmethod
    def forward(ctx, x, lengths, t_out, h0, c0, w_ih, w_hh, b_ih, b_hh):
        hs, hT, cT, saved = _lstm_forward_raw(x, lengths, t_out, h0, c0, w_ih, w_hh, b_ih, b_hh)
        ctx.save_for_backward(*saved)
        ctx.t_out = t_out
        return hs, hT, cT

    @staticmethod
    def backward(ctx, d_hs, d_hT, d_cT):
        grads = _lstm_backward_raw(ctx.saved_tensors, ctx.t_out, d_hs, d_hT, d_cT)
        return (None, None, None, None, None) + tuple(grads)


def _row_geom(x):
    if x.dim() == 3:
        outer, inner = x.shape[0], x.shape[1]
        s_outer, s_inner = x.stride(0), x.stride(1)
    else:
        outer, inner, s_outer, s_inner = 1, x.shape[0], 0, x.stride(0)
    if x.stride(-1) != 1:
        raise ValueError("head: features must be unit-stride")
    return inner, s_outer, s_inner, outer * inner


def _head_forward_raw(x, w1, b1, w2, b2):
    """``howl_head_fwd``: (y1 = relu(x W1^T + b1), y2 = y1 W2^T + b2) for x (..., n_in) with unit-stride features."""
    n_hid, n_in = w1.shape
    n_out = w2.shape[0]
    inner, s_outer, s_inner, rows = _row_geom(x)
    f32 = dict(dtype=torch.float32, device=x.device)
    y1 = torch.empty(x.shape[:-1] + (n_hid,), **f32)
    y2 = torch.empty(x.shape[:-1] + (n_out,), **f32)
    prm = _lib.HowlHeadParams(_vp(w1), _vp(b1), _vp(w2), _vp(b2))
    _lib.get().call("howl_head_fwd", ctypes.byref(prm), _vp(x), inner, s_outer, s_inner, rows, n_in, n_hid, n_out, _vp(y1),
                    _vp(y2), ops._stream())
    return y1, y2


def _seq_head_ctc_supported(B, T, w1, w2, max_target):
    n_hid, n_in = w1.shape
    return bool(_lib.get().cdll.howl_seq_head_ctc_supported(int(B), int(T), n_in, n_hid, w2.shape[0], int(max_target)))


def _seq_head_ctc_raw(hs, w1, b1, w2, b2, targets, input_lengths, target_lengths, blank, max_target):
    """``howl_seq_head_ctc``: head forward + log_softmax / CTC + the head's backward over the rows in one launch.  hs (B, T, 128)
    view of the hidden states -> (y2 (B, T, n_out), nll (B,), dz1, dhs, head workspace holding the partial sums)."""
    n_hid, n_in = w1.shape
    n_out = w2.shape[0]
    B, T = hs.shape[:2]
    f32 = dict(dtype=torch.float32, device=hs.device)
    y2 = torch.empty((B, T, n_out), **f32)
    nll = torch.empty(B, **f32)
    dz1 = torch.empty((B, T, n_hid), **f32)
    dhs = torch.empty((B, T, n_in), **f32)
    head_ws = torch.empty(_lib.get().cdll.howl_head_workspace_bytes(n_in, n_hid, n_out), dtype=torch.uint8, device=hs.device)
    prm = _lib.HowlHeadParams(_vp(w1), _vp(b1), _vp(w2), _vp(b2))
    _lib.get().call("howl_seq_head_ctc", ctypes.byref(prm), _vp(hs), hs.stride(0), hs.stride(1), B, T, n_in, n_hid, n_out,
                    _vp(targets), targets.stride(0), int(max_target), _vp(input_lengths), _vp(target_lengths), int(blank), _vp(y2),
                    _vp(nll), _vp(dz1), _vp(dhs), _vp(head_ws), head_ws.numel(), ops._stream())
    return y2, nll, dz1, dhs, head_ws


def _head_backward_raw(x, y1, dy2, w1, b1, w2, b2, need_dx=True, grads=None, ctc_mean=None):
    """``howl_head_bwd``: dy2 (..., n_out) -> (dx or None, [dW1, db1, dW2, db2]), written into ``grads`` when given.
    ``ctc_mean`` = (nll, target_lengths, loss): the batch mean of a CTC loss taken by the same launch (``HowlCtcMean``)."""
    n_hid, n_in = w1.shape
    n_out = w2.shape[0]
    inner, s_outer, s_inner, rows = _row_geom(x)
    f32 = dict(dtype=torch.float32, device=x.device)
    dy2 = dy2.contiguous()
    dz1 = torch.empty_like(y1)
    dx = torch.empty(x.shape, **f32) if need_dx else None
    if grads is None:
        grads = [torch.empty_like(t) for t in (w1, b1, w2, b2)]
    ws = torch.empty(_lib.get().cdll.howl_head_workspace_bytes(n_in, n_hid, n_out), dtype=torch.uint8, device=x.device)
    prm = _lib.HowlHeadParams(_vp(w1), _vp(b1), _vp(w2), _vp(b2))
    gr = _lib.HowlHeadGrads(*[_vp(g) for g in grads])
    cm = None
    if ctc_mean is not None:
        nll, tl, loss = ctc_mean
        cm = ctypes.byref(_lib.HowlCtcMean(_vp(nll), _vp(tl), int(nll.numel()), _vp(loss)))
    _lib.get().call("howl_head_bwd", ctypes.byref(prm), _vp(x), inner, s_outer, s_inner, rows, n_in, n_hid, n_out, _vp(y1),
                    _vp(dy2), _vp(dz1), _vp(dx), ctypes.byref(gr), cm, _vp(ws), ws.numel(), ops._stream())
    return dx, grads


def _seq_backward_raw(saved, y1, dy2, head_params, grads, ctc_mean=None, adamw=None, head_rows_done=None):
    """``howl_seq_lstm_bwd``: head + LSTM backward of the sequence model in one call (t_out == T); ``grads`` = the eight flat-buffer
    views in ``hot_parameters()`` order.  ``adamw`` = (flat params, flat grads, m, v, lr, (beta1, beta2), eps, weight_decay, step,
    grad_scale): the optimiser step is part of the call (``HowlAdamW``).  ``head_rows_done`` = (dz1, dhs, head_ws) left by
    ``howl_seq_head_ctc`` (then ``y1`` / ``dy2`` are None: the call folds that launch's partial sums instead of running the rows)."""
    x, lengths, c0, w_ih, w_hh, b_ih, b_hh, gates, cs, hseq, ws = saved
    w1, b1, w2, b2 = head_params
    B, T, M = x.shape
    n_hid, n_in = w1.shape
    n_out = w2.shape[0]
    f32 = dict(dtype=torch.float32, device=x.device)
    dgates = torch.empty((B, T, 4 * HID), **f32)
    if head_rows_done is not None:
        dz1, dhs, head_ws = head_rows_done
        y1 = dy2 = None
    else:
        dy2 = dy2.contiguous()
        dz1 = torch.empty_like(y1)
        dhs = torch.empty((B, T, HID), **f32)
        head_ws = torch.empty(_lib.get().cdll.howl_head_workspace_bytes(n_in, n_hid, n_out), dtype=torch.uint8, device=x.device)
    hp = _lib.HowlHeadParams(_vp(w1), _vp(b1), _vp(w2), _vp(b2))
    hg = _lib.HowlHeadGrads(*[_vp(g) for g in grads[4:8]])
    cm = None
    if ctc_mean is not None:
        nll, tl, loss = ctc_mean
        cm = ctypes.byref(_lib.HowlCtcMean(_vp(nll), _vp(tl), int(nll.numel()), _vp(loss)))
    prm = _lib.HowlLstmParams(_vp(w_ih), _vp(w_hh), _vp(b_ih), _vp(b_hh))
    sv = _lib.HowlLstmSaved(None, _vp(gates), _vp(cs), _vp(hseq), _vp(dgates), T, _x_frames(x))
    gr = _lib.HowlLstmGrads(*[_vp(g) for g in grads[:4]])
    opt = None
    if adamw is not None:
        flat, fgrad, m, v, lr, betas, eps, wd, step, gscale = adamw
        opt = ctypes.byref(_lib.HowlAdamW(_vp(flat), _vp(fgrad), _vp(m), _vp(v), flat.numel(), lr, betas[0], betas[1], eps, wd, step, gscale))
    _lib.get().call("howl_seq_lstm_bwd", ctypes.byref(hp), n_hid, n_out, _vp(y1), _vp(dy2), _vp(dz1), _vp(dhs), ctypes.byref(hg), cm,
                    _vp(head_ws), head_ws.numel(), ctypes.byref(prm), _vp(x), B, T, M, _vp(lengths), _vp(c0), ctypes.byref(sv),
                    ctypes.byref(gr), _vp(ws), ws.numel(), opt, ops._stream())


class _HeadFunction(torch.autograd.Function):
    """Linear - ReLU - Linear (``self.dnn``, rnn.py:44-48) on the library's head kernels."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        y1, y2 = _head_forward_raw(x, w1, b1, w2, b2)
        ctx.save_for_backward(x, y1, w1, b1, w2, b2)
        return y2

    @staticmethod
    def backward(ctx, dy2):
        x, y1, w1, b1, w2, b2 = ctx.saved_tensors
        dx, grads = _head_backward_raw(x, y1, dy2, w1, b1, w2, b2, ctx.needs_input_grad[0])
        return (dx,) + tuple(grads)


class LstmStreamSession(StreamSession):
    """Streaming seq-lstm / lstm: ``probabilities(pcm, ...)`` takes N independent raw PCM chunks to their class probabilities in ONE
    kernel launch (``howl_lstm_stream_chunks``: log-mel + ZMUV, the recurrence, the head and the softmax, four streams per
    workgroup; no gate / cell / hidden-sequence stores, nothing of the head through HBM).  The weights are read in place on every
    call: nothing is prepared, nothing can go stale.  Eval mode only, standard filterbank only.  The kernel's range, which
    ``supported()`` answers for chunks of UP TO ``n_samples`` samples: 40 mel bins, 400 samples .. 8192 frames, <= 64 labels.

    ``seq-lstm``: probs (N, 1 + L_max // 200, C), rows behind a stream's last frame zero, and the carried state as the pair of
    (1, N, 128) tensors ``model.streaming_state`` holds.  ``lstm``: the head on the final hidden state only, probs (N, C), no state
    (``SimpleLstm`` is stateless between calls, rnn.py:89-90)."""
    RUNS = "the inference path (no saved activations)"
    UNIT = "chunks"
    in_range = staticmethod(ops.lstm_stream_supported)

    def __init__(self, model, std, zmuv):
        super().__init__(model, std, zmuv)
        self.last_only = isinstance(model, SimpleLstm)
        self._own = None      # the state pair this session returned last: handed back, it is advanced in place

    @staticmethod
    def rows_of(n_samples: int) -> int:
        """Rows of ``probs`` (the engine's frames) a chunk of ``n_samples`` samples has: one per frame."""
        return 1 + n_samples // 200

    @torch.no_grad()
    def probabilities(self, pcm: torch.Tensor, n_samples: torch.Tensor = None, frames: torch.Tensor = None, state=None,
                      return_state: bool = True, logits: torch.Tensor = None):
        """pcm: (N, L_max) fp32 on the device, unit sample stride; ``n_samples`` (N) int64 on the device, the samples of each chunk
        (None: L_max for all); ``frames`` (N) int64 on the device, the frames to run (None: all ``1 + n_samples // 200``); ``state``:
        the (h, c) pair to start from, (1, N, 128) each, None = zeros.  -> (probs, state).  The returned state tensors belong to the
        session: handed back as ``state`` of the next call they are advanced in place (no copy); any other pair is copied first.
        ``return_state=False`` with ``state=None``: no state is carried at all (a pass over whole clips)."""
        self._enter(pcm)
        N = pcm.size(0)
        h = c = None
        if not self.last_only and (state is not None or return_state):
            if state is not None and (tuple(state[0].shape) != (1, N, HID) or tuple(state[1].shape) != (1, N, HID)):
                raise RuntimeError(f"Expected hidden size (1, {N}, {HID}), got {tuple(state[0].shape)}")     # as nn.LSTM does
            own = self._own
            if state is not None and own is not None and state[0] is own[0] and state[1] is own[1]:
                h, c = own
            else:
                hc = torch.zeros((2, 1, N, HID), dtype=torch.float32, device=pcm.device)
                if state is not None:
                    hc[0].copy_(state[0])
                    hc[1].copy_(state[1])
                h, c = hc[0], hc[1]
        l, d = self.model.lstm, self.model.dnn
        lstm_prm = _lib.HowlLstmParams(_vp(l.weight_ih_l0), _vp(l.weight_hh_l0), _vp(l.bias_ih_l0), _vp(l.bias_hh_l0))
        head_prm = _lib.HowlHeadParams(_vp(d[0].weight), _vp(d[0].bias), _vp(d[2].weight), _vp(d[2].bias))
        pair = self._pair()
        probs = ops.lstm_stream_chunks(lstm_prm, head_prm, pcm, self.std._standard_fb(), self.std.n_mels, pair, self.model.num_labels,
                                       n_samples=n_samples, frames=frames, h=h, c=c, last_only=self.last_only, logits=logits)
        self._own = (h, c) if h is not None else None
        return probs, self._own


class _LstmBase(RegisteredModel):
    def stream_session(self, std, zmuv) -> LstmStreamSession:
        """One-launch inference from raw PCM for this model (see ``LstmStreamSession``)."""
        return LstmStreamSession(self, std, zmuv)

    def __init__(self, num_labels: int, config: LstmConfig = None):
        super().__init__(num_labels)
        config = config or LstmConfig()
        if config.hidden_size != HID:
            raise NotImplementedError("the MI355X LSTM kernels are specialised for hidden_size=128")
        self.lstm = nn.LSTM(config.num_mels, config.hidden_size)
        self.dnn = nn.Sequential(nn.Linear(config.hidden_size, int(2 * config.hidden_size)), nn.ReLU(),
                                 nn.Linear(int(2 * config.hidden_size), num_labels))
        self.hc = None

    def _lstm_inputs(self, x, lengths, t_out=None):
        """-> (xb (B, t_out, M) contiguous, device lengths or None, t_out, h0, c0).

        ``lengths`` follows ``pack_padded_sequence``: one entry per sequence, sorted in decreasing order, 1..T.  A host tensor
        (the reference's batches carry them on the host) is checked here.  A DEVICE tensor together with ``t_out`` = its
        maximum is trusted as already checked -- reading it back would stall the stream the step is queued on."""
        x0 = x[:, 0]                                   # (B, M, T), log-mels only (rnn.py:61,86)
        if not ops.on_device(x0):
            raise _lib.HowlHipError("LSTM input must be on a HIP device (no CPU fallback)")
        xb = x0.permute(0, 2, 1)
        B, T, _ = xb.shape
        if lengths is not None and t_out is not None and ops.on_device(lengths):
            if lengths.numel() != B or not 1 <= t_out <= T:
                raise RuntimeError("lengths must have one entry per sequence and t_out must be in 1..T")
            lengths = lengths.to(torch.int64)
        elif lengths is not None:
            lc = lengths.detach().cpu().long()
            if lc.numel() != B:
                raise RuntimeError("lengths must have one entry per sequence")
            if (lc[:-1] < lc[1:]).any():
                raise RuntimeError("`lengths` array must be sorted in decreasing order (pack_padded_sequence semantics)")
            if lc.min() <= 0 or lc.max() > T:
                raise RuntimeError("lengths must be in 1..T")
            t_out = int(lc.max())
            lengths = lc.to(xb.device)
        else:
            t_out = T
        if t_out < T:                                  # frames no sequence reaches: the kernels and the saved buffers only see
            xb = xb[:, :t_out]                         # t_out steps (a view: the library takes the buffer's frame stride)
        M = xb.shape[2]
        if (xb.stride(2) != 1 or (xb.shape[1] > 1 and xb.stride(1) != M) or xb.stride(0) % M       # the fused frontend already hands over a (B,T,M) buffer;
                or xb.stride(0) < xb.shape[1] * M):                            # expanded / overlapping batch views are copied
            xb = xb.contiguous()
        hx = self.streaming_state if self.is_streaming and self.streaming_state is not None else None
        if hx is not None and (tuple(hx[0].shape) != (1, B, HID) or tuple(hx[1].shape) != (1, B, HID)):
            raise RuntimeError(f"Expected hidden size (1, {B}, {HID}), got {tuple(hx[0].shape)}")     # as nn.LSTM does
        h0 = hx[0][0].contiguous() if hx is not None else None
        c0 = hx[1][0].contiguous() if hx is not None else None
        return xb, lengths, t_out, h0, c0

    def _run_lstm(self, x, lengths):
        xb, lengths, t_out, h0, c0 = self._lstm_inputs(x, lengths)
        l = self.lstm
        return _LstmFunction.apply(xb, lengths, t_out, h0, c0, l.weight_ih_l0, l.weight_hh_l0, l.bias_ih_l0, l.bias_hh_l0)

    def hot_parameters(self):
        """Parameters in the order the fused trainer lays them out (and ``_launch_backward`` fills their gradients)."""
        l = self.lstm
        return [l.weight_ih_l0, l.weight_hh_l0, l.bias_ih_l0, l.bias_hh_l0, self.dnn[0].weight, self.dnn[0].bias,
                self.dnn[2].weight, self.dnn[2].bias]

    def _head(self, h):
        return _HeadFunction.apply(h, self.dnn[0].weight, self.dnn[0].bias, self.dnn[2].weight, self.dnn[2].bias)


class SequentialLstm(_LstmBase, name="seq-lstm"):
    @property
    def streaming_state(self) -> Any:
        return self.hc

    @streaming_state.setter
    def streaming_state(self, x: Any):
        self.hc = x

    def forward(self, x, lengths):
        hs, hT, cT = self._run_lstm(x, lengths)
        if self.is_streaming:
            self.streaming_state = (hT.detach().clone().unsqueeze(0), cT.detach().clone().unsqueeze(0))
        return self._head(hs).permute(1, 0, 2)         # (T_len, B, num_labels), as dnn(rnn_seq) in rnn.py:71

    # --- training.fused.FusedTrainer hooks: the same launches as forward() / autograd, without the autograd graph -----
    TAKES_NEXT_LOGMEL = True      # FusedTrainer.step_sequence(next_audio=...): the next batch's frontend rides in the forward call
    TAKES_CTC = True              # ... and _launch_forward(ctc=...): head + CTC + head backward rows as one launch where covered

    def _launch_forward(self, feat, lengths, t_out=None, next_logmel=None, ctc=None):
        """feat (B, C>=1, M, T) -> scores (T_len, B, num_labels) view; keeps what ``_launch_backward`` needs.  ``t_out`` with
        device-resident ``lengths``: see ``_lstm_inputs``.  ``next_logmel``: see ``_lstm_forward_raw``.
        ``ctc`` = (targets (B, Lmax) int64, target_lengths, blank, max_target), all on the device: where the library's fused launch
        covers the batch (``howl_seq_head_ctc``: short windows, >= 2048 rows) the head, log_softmax + CTC and the head's backward
        over the rows run as ONE launch behind the recurrence; ``self.ctc_nll`` is then the (B,) negative log likelihoods and
        ``_launch_backward`` takes ``dscores=None``.  Otherwise ``self.ctc_nll`` is None and the caller runs the loss itself."""
        xb, lengths, t_out, h0, c0 = self._lstm_inputs(feat, lengths, t_out)
        ps = self.hot_parameters()
        hs, hT, cT, saved = _lstm_forward_raw(xb, lengths, t_out, h0, c0, *ps[:4], next_logmel=next_logmel)
        self.ctc_nll = None
        if self.is_streaming:                          # same carry as forward() (rnn.py:64-68)
            self.streaming_state = (hT.detach().clone().unsqueeze(0), cT.detach().clone().unsqueeze(0))
        if (ctc is not None and lengths is not None and t_out == xb.shape[1]
                and _seq_head_ctc_supported(xb.shape[0], t_out, ps[4], ps[6], ctc[3])):
            targets, target_lengths, blank, max_target = ctc
            y2, nll, dz1, dhs, head_ws = _seq_head_ctc_raw(hs, *ps[4:8], targets, lengths, target_lengths, blank, max_target)
            self._seq_saved = (saved, t_out, hs, None, (dz1, dhs, head_ws))
            self.ctc_nll = nll
            return y2.permute(1, 0, 2)
        y1, y2 = _head_forward_raw(hs, *ps[4:8])
        self._seq_saved = (saved, t_out, hs, y1, None)
        return y2.permute(1, 0, 2)

    def _launch_backward(self, dscores, out_grads=None, ctc_mean=None, adamw=None):
        """dscores: d loss / d scores as a (T_len, B, num_labels) view of a (B, T_len, num_labels) buffer (ops.ctc_loss_fwd_bwd);
        ``ctc_mean`` = (nll, target_lengths, loss) when the loss launch left its batch mean to the head's backward;
        ``adamw``: see ``_seq_backward_raw`` -- ``self.optimizer_step_done`` says whether the call took it."""
        saved, t_out, hs, y1, rows_done = self._seq_saved
        ps = self.hot_parameters()
        grads = out_grads if out_grads is not None else [torch.empty_like(p) for p in ps]
        x = saved[0]
        self.optimizer_step_done = False
        if rows_done is not None:    # howl_seq_head_ctc ran the head's rows behind the forward recurrence: fold, dW1, LSTM backward
            _seq_backward_raw(saved, None, None, ps[4:8], grads, ctc_mean, adamw, head_rows_done=rows_done)
            self.optimizer_step_done = adamw is not None
        elif t_out == x.shape[1]:      # whole buffer ran: one call, the wide weight gradients and the slab folds merged (12 launches)
            _seq_backward_raw(saved, y1, dscores.permute(1, 0, 2), ps[4:8], grads, ctc_mean, adamw)
            self.optimizer_step_done = adamw is not None
        else:
            dhs, _ = _head_backward_raw(hs, y1, dscores.permute(1, 0, 2), *ps[4:8], True, grads[4:8], ctc_mean)
            _lstm_backward_raw(saved, t_out, dhs, None, None, grads[:4])
        self._seq_saved = None
        return grads


class SimpleLstm(_LstmBase, name="lstm"):
    NEEDS_LENGTHS = True       # FusedTrainer.step passes the frame lengths through

    # --- training.fused.FusedTrainer hooks (cross-entropy on the last hidden state, pretrain_gsc.py:126-133) ---------
    def _launch_forward(self, feat, lengths, t_out=None):
        """feat (B, C>=1, M, T), frame lengths -> logits (B, num_labels); keeps what ``_launch_backward`` needs."""
        if lengths is None:
            raise TypeError("SimpleLstm needs lengths (rnn.py:88 packs unconditionally)")
        xb, lengths, t_out, h0, c0 = self._lstm_inputs(feat, lengths, t_out)
        ps = self.hot_parameters()
        _, hT, _, saved = _lstm_forward_raw(xb, lengths, t_out, h0, c0, *ps[:4])
        y1, y2 = _head_forward_raw(hT, *ps[4:8])
        self._cls_saved = (saved, t_out, hT, y1)
        return y2

    def _launch_backward(self, feat, dlogits, out_grads=None):
        saved, t_out, hT, y1 = self._cls_saved
        ps = self.hot_parameters()
        grads = out_grads if out_grads is not None else [torch.empty_like(p) for p in ps]
        dhT, _ = _head_backward_raw(hT, y1, dlogits, *ps[4:8], True, grads[4:8])
        _lstm_backward_raw(saved, t_out, None, dhT, None, grads[:4])
        self._cls_saved = None
        return grads

    def forward(self, x, lengths):
        if lengths is None:
            raise TypeError("SimpleLstm needs lengths (rnn.py:88 packs unconditionally)")
        hs, hT, cT = self._run_lstm(x, lengths)
        if self.is_streaming:
            # rnn.py:89-90 assigns streaming_state, which the base class setter drops (base.py:35-37): stays stateless
            self.streaming_state = (hT.unsqueeze(0), cT.unsqueeze(0))
        return self._head(hT)


class _GruFunction(torch.autograd.Function):
    """The whole gru model as one differentiable function of its sixteen parameters: ``howl_gru_fwd`` / ``howl_gru_bwd``."""

    @staticmethod
    def forward(ctx, model, feat, lengths, t_out, *params):
        logits = model._launch_forward(feat, lengths, t_out)
        ctx.model, ctx.feat, ctx.saved = model, feat, model._gru_saved
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        ctx.model._gru_saved = ctx.saved
        grads = ctx.model._launch_backward(ctx.feat, dlogits.contiguous())
        return (None, None, None, None) + tuple(grads)


class GruStreamSession(StreamSession):
    """Streaming gru: ``probabilities(pcm)`` takes (N, L) raw PCM windows to their (N, C) class probabilities in ONE kernel launch
    (``howl_gru_stream_windows``: log-mel and ZMUV, both convolutions, the recurrence, the head and the softmax, one workgroup per
    window).  The kernel reads the model's parameters and running statistics in place, so there is no prepared state and nothing
    to refresh: a ``load_state_dict``, an optimiser step or a write torch does not see is in the next call's answer.  The session
    owns its scratch, so two engines on two streams share nothing.  Eval mode only, standard filterbank only.  The kernel's range,
    which ``supported()`` answers for: 40 mel bins, 512 samples .. 83 frames, <= 64 labels."""
    RUNS = "eval-mode BatchNorm (running statistics) and no dropout"
    in_range = staticmethod(ops.gru_stream_supported)

    @torch.no_grad()
    def probabilities(self, pcm: torch.Tensor, frames: int = None, logits: torch.Tensor = None) -> torch.Tensor:
        """pcm: (N, L) fp32 on the device, unit sample stride (rows may be overlapping views of one clip); ``frames``: the frames the
        recurrence runs over (None: ``std.compute_lengths(L)``) -> (N, C) on the device."""
        self._enter(pcm)
        N, L = pcm.shape
        if frames is None:
            frames = self._frames_of(L)
        ws = self._workspace(ops.gru_stream_workspace_bytes(N, L), pcm.device)
        pair = self._pair()
        prm, buf = self.model._params_struct(), self.model._buffers_struct()
        return ops.gru_stream_windows(prm, buf, pcm, int(frames), self.std._standard_fb(), self.std.n_mels, pair, self.model.num_labels,
                                      ws, logits=logits)


class SimpleGru(RegisteredModel, name="gru"):
    """``SimpleGru`` of the reference (rnn.py:94-130) on the kernels of ``howl_amd/csrc/gru.hip``, the whole model one C-ABI call
    per direction: Conv2d(1,8,3,padding=(1,3)) - BatchNorm - ReLU - MaxPool(1,2) - Conv2d(8,1,3,padding=1) - ReLU - BatchNorm
    - GRU(40 -> 96) on the packed batch - Linear(96,192) - ReLU - Dropout(0.2) - Linear(192, num_labels) on the final states.
    Same construction order and ``state_dict`` keys (``conv_encoder.{0,1,4,6}.*``, ``lstm_encoder.*_l0``, ``dnn.{0,3}.*``): a
    reference workspace loads with ``strict=True``; the ``nn`` modules are parameter containers only.

    The whole (B, 40, T) buffer goes through the encoder, padded frames included (they count in the BatchNorm statistics, as in
    the reference); utterance b's recurrence runs ``(lengths[b] + 4) // 2`` steps.  Decided once:

    * the reference's ``lengths += 4`` mutates the caller's tensor; this class never writes to ``lengths`` (the entry points
      hand over a fresh tensor each batch, so nothing observable changes);
    * like ``pack_padded_sequence``, host ``lengths`` must be sorted in decreasing order (the ``RuntimeError`` of the LSTM
      models); device-resident lengths together with ``t_out`` are trusted, as there;
    * ``LASEncoderConfig`` other than ``num_mels=40, num_latent_channels=8, hidden_size=96, use_maxpool=True`` raises
      ``NotImplementedError`` at construction (``num_spec_channels`` and ``num_layers`` are not used by this model);
    * dropout draws one ``howl_dropout_mask`` launch per training forward, keyed from torch's CPU generator and salted by the
      replica rank, unless ``forced_keep_mask`` (B, 192 of 0/1) is set.
    """
    NEEDS_LENGTHS = True       # FusedTrainer.step passes the frame lengths through

    def __init__(self, num_labels: int, config: LASEncoderConfig = None):
        super().__init__(num_labels)
        config = config or LASEncoderConfig()
        for name, want in (("num_mels", 40), ("num_latent_channels", 8), ("hidden_size", 96), ("use_maxpool", True)):
            if getattr(config, name) != want:
                raise NotImplementedError(f"the MI355X gru kernels are specialised for {name}={want} (got {getattr(config, name)})")
        conv1 = nn.Conv2d(1, config.num_latent_channels, 3, padding=(1, 3))
        conv2 = nn.Conv2d(config.num_latent_channels, 1, 3, padding=1)
        self.conv_encoder = nn.Sequential(conv1, nn.BatchNorm2d(config.num_latent_channels), nn.ReLU(), nn.MaxPool2d((1, 2)), conv2,
                                          nn.ReLU(), nn.BatchNorm2d(1))
        self.use_maxpool = config.use_maxpool
        self.lstm_encoder = nn.GRU(config.num_mels, config.hidden_size, bidirectional=False)
        self.dnn = nn.Sequential(nn.Linear(config.hidden_size, int(2 * config.hidden_size)), nn.ReLU(), nn.Dropout(0.2),
                                 nn.Linear(int(2 * config.hidden_size), num_labels))
        self.dropout_p = 0.2
        self.forced_keep_mask = None     # tests: (B, 192) 0/1 mask used instead of a fresh draw
        self._gru_saved = None

    def hot_parameters(self):
        """Parameters in the library's gradient order (``HowlGruGrads``) = ``state_dict`` order."""
        e, r, d = self.conv_encoder, self.lstm_encoder, self.dnn
        return [e[0].weight, e[0].bias, e[1].weight, e[1].bias, e[4].weight, e[4].bias, e[6].weight, e[6].bias, r.weight_ih_l0,
                r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0, d[0].weight, d[0].bias, d[3].weight, d[3].bias]

    def _inputs(self, x, lengths, t_out):
        """-> (x0 (B, 40, T) view of the log-Mel channel, device int64 lengths or None).  Host lengths are checked as
        ``_LstmBase._lstm_inputs`` checks them; device lengths with ``t_out`` (their maximum) are trusted."""
        x0 = x[:, 0]
        if not ops.on_device(x0):
            raise _lib.HowlHipError("gru input must be on a HIP device (no CPU fallback)")
        B, _, T = x0.shape
        if lengths is not None and t_out is not None and ops.on_device(lengths):
            if lengths.numel() != B or not 1 <= t_out <= T:
                raise RuntimeError("lengths must have one entry per sequence and t_out must be in 1..T")
            lengths = lengths.to(torch.int64)
        elif lengths is not None:
            lc = lengths.detach().cpu().long()
            if lc.numel() != B:
                raise RuntimeError("lengths must have one entry per sequence")
            if (lc[:-1] < lc[1:]).any():
                raise RuntimeError("`lengths` array must be sorted in decreasing order (pack_padded_sequence semantics)")
            if lc.min() <= 0 or lc.max() > T:
                raise RuntimeError("lengths must be in 1..T")
            lengths = lc.to(x0.device)
        return x0, lengths

    def _draw_mask(self, B, device):
        if self.forced_keep_mask is not None:
            return self.forced_keep_mask.to(device=device, dtype=torch.float32).contiguous()
        if self.dropout_p <= 0:
            return None
        # one launch of the counter-based device generator; the key comes from torch's CPU generator (a host draw: reproducible
        # under torch.manual_seed, nothing read back from the device)
        mask = torch.empty((B, 192), dtype=torch.float32, device=device)
        key = int(torch.randint(0, 2 ** 62, (1,)).item())
        key ^= (parallel.world_info()[0] * 0x9E3779B97F4A7C15) & (2 ** 62 - 1)   # replicas share the CPU seed, not the mask
        _lib.get().call("howl_dropout_mask", _vp(mask), mask.numel(), float(self.dropout_p), ctypes.c_ulonglong(key), ops._stream())
        return mask

    def _launch_forward(self, feat, lengths, t_out=None):
        """feat (B, C>=1, 40, T), frame lengths (or None = all T) -> logits (B, num_labels); in training mode keeps what
        ``_launch_backward`` needs (the library's workspace)."""
        x0, lengths = self._inputs(feat, lengths, t_out)
        B, M, T = x0.shape
        cdll = _lib.get().cdll
        if not cdll.howl_gru_supported(B, M, T, self.num_labels):
            raise _lib.HowlHipError(f"gru: B={B}, {M} mel bins, T={T}, {self.num_labels} labels is outside the kernels' range "
                                    f"(40 mel bins, 1..8192 frames, 1..64 labels)")
        ps = self.hot_parameters()
        e = self.conv_encoder
        prm = _lib.HowlGruParams(*[_vp(p) for p in ps])
        buf = _lib.HowlGruBuffers(_vp(e[1].running_mean), _vp(e[1].running_var), _vp(e[1].num_batches_tracked), _vp(e[6].running_mean),
                                  _vp(e[6].running_var), _vp(e[6].num_batches_tracked))
        ws = torch.empty(cdll.howl_gru_workspace_bytes(B, T), dtype=torch.uint8, device=x0.device)
        logits = torch.empty((B, self.num_labels), dtype=torch.float32, device=x0.device)
        mask = self._draw_mask(B, x0.device) if self.training else None
        if mask is not None and tuple(mask.shape) != (B, 192):
            raise RuntimeError(f"forced_keep_mask must be ({B}, 192), got {tuple(mask.shape)}")
        scale = 1.0 / (1.0 - self.dropout_p) if mask is not None else 1.0
        _lib.get().call("howl_gru_fwd", ctypes.byref(prm), ctypes.byref(buf), _vp(x0), x0.stride(0), x0.stride(1), x0.stride(2), B, M, T,
                        self.num_labels, _vp(lengths), int(self.training), _vp(mask), scale, _vp(logits), _vp(ws), ws.numel(),
                        ops._stream())
        self._gru_saved = (x0, lengths, scale, ws, mask) if self.training else None
        return logits

    def _launch_backward(self, feat, dlogits, out_grads=None):
        if self._gru_saved is None:
            raise NotImplementedError("gru: the backward pass needs a training-mode forward (eval mode saves nothing)")
        x0, lengths, scale, ws, _ = self._gru_saved
        B, M, T = x0.shape
        ps = self.hot_parameters()
        grads = out_grads if out_grads is not None else [torch.empty_like(p) for p in ps]
        prm = _lib.HowlGruParams(*[_vp(p) for p in ps])
        gr = _lib.HowlGruGrads(*[_vp(g) for g in grads])
        dlogits = dlogits.contiguous()
        _lib.get().call("howl_gru_bwd", ctypes.byref(prm), _vp(x0), x0.stride(0), x0.stride(1), x0.stride(2), B, M, T, self.num_labels,
                        _vp(lengths), scale, _vp(dlogits), ctypes.byref(gr), _vp(ws), ws.numel(), ops._stream())
        self._gru_saved = None
        return grads

    def forward(self, x, lengths):
        return _GruFunction.apply(self, x, lengths, None, *self.hot_parameters())

    def _params_struct(self):
        return _lib.HowlGruParams(*[_vp(p) for p in self.hot_parameters()])

    def _buffers_struct(self):
        e = self.conv_encoder
        return _lib.HowlGruBuffers(_vp(e[1].running_mean), _vp(e[1].running_var), _vp(e[1].num_batches_tracked), _vp(e[6].running_mean),
                                   _vp(e[6].running_var), _vp(e[6].num_batches_tracked))

    def stream_session(self, std, zmuv) -> GruStreamSession:
        """The streaming path for this model behind ``std`` (``StandardAudioTransform``) and ``zmuv`` (``ZmuvTransform`` or None):
        raw PCM windows -> probabilities in one launch, with scratch of its own (``GruStreamSession``)."""
        return GruStreamSession(self, std, zmuv)


class _LasFunction(torch.autograd.Function):
    """The whole las model as one differentiable function of its twenty-five parameters: ``howl_las_fwd`` / ``howl_las_bwd``."""

    @staticmethod
    def forward(ctx, model, feat, lengths, t_out, *params):
        logits = model._launch_forward(feat, lengths, t_out)
        ctx.model, ctx.feat, ctx.saved = model, feat, model._las_saved
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        ctx.model._las_saved = ctx.saved
        grads = ctx.model._launch_backward(ctx.feat, dlogits.contiguous())
        return (None, None, None, None) + tuple(grads)


class LasStreamSession(PreparedStreamSession):
    """Streaming las: ``probabilities(pcm)`` takes (N, L) raw PCM windows to their (N, C) class probabilities in ONE kernel launch
    (``howl_las_stream_windows``: log-mel, deltas and ZMUV, both convolutions, the input projections, both recurrences, the
    attention, the head and the softmax, one workgroup per window).  The session owns its prepared state (W_ih and the V / K
    projections as MFMA fragments, W_hh in lane order, both BatchNorms folded from their running statistics) and its scratch, so
    two engines on two streams share nothing; the state is prepared again whenever a hot parameter, a BatchNorm weight or bias or
    a running buffer of the model was replaced or written through torch since the last launch (``data_ptr()`` / ``_version``:
    ``load_state_dict``, an optimiser step).  Writes that torch does not see need ``refresh()``.  Eval mode only, standard
    filterbank only.  The kernel's range, which ``supported()`` answers for: 40 mel bins, 512 samples .. 83 frames, <= 64 labels."""
    RUNS = "eval-mode BatchNorm (running statistics) and no dropout"
    in_range = staticmethod(ops.las_stream_supported)

    def _watched(self):
        bn1, bn2 = self.model.encoder.conv_encoder[1], self.model.encoder.conv_encoder[5]
        return self.model.hot_parameters() + [bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var]

    def _state_bytes(self):
        return ops.las_stream_state_bytes(self.model.num_labels)

    def _prepare(self, state):
        prm = _lib.HowlLasParams(*[_vp(p) for p in self.model.hot_parameters()])
        ops.las_stream_prepare(prm, self.model._bn_buffers(), self.model.num_labels, state)

    @torch.no_grad()
    def probabilities(self, pcm: torch.Tensor, frames: int = None, logits: torch.Tensor = None) -> torch.Tensor:
        """pcm: (N, L) fp32 on the device, unit sample stride (rows may be overlapping views of one clip); ``frames``: the frames the
        recurrences and the attention run over (None: ``std.compute_lengths(L)``) -> (N, C) on the device."""
        self._enter(pcm)
        N, L = pcm.shape
        if frames is None:
            frames = self._frames_of(L)
        state = self._prepared_state(pcm.device)
        ws = self._workspace(ops.las_stream_workspace_bytes(N, L), pcm.device)
        pair = self._pair()
        return ops.las_stream_windows(state, pcm, int(frames), self.std._standard_fb(), self.std.n_mels, pair, self.model.num_labels,
                                      ws, logits=logits)


class _LasEncoder(nn.Module):
    """Parameter container with the reference's names (rnn.py:133-153): conv1 and conv2 are registered twice, as attributes and
    inside ``conv_encoder``, so both key families appear in the ``state_dict`` and share one tensor each."""

    def __init__(self, config: LASEncoderConfig):
        super().__init__()
        c = config.num_latent_channels
        self.use_maxpool = config.use_maxpool
        self.conv1 = conv1 = nn.Conv2d(config.num_spec_channels, c, 3, padding=2)
        self.conv2 = conv2 = nn.Conv2d(c, c, 3, padding=2)
        self.conv_encoder = nn.Sequential(conv1, nn.BatchNorm2d(c), nn.ReLU(), nn.MaxPool2d((1, 2)), conv2, nn.BatchNorm2d(c), nn.ReLU(),
                                          nn.MaxPool2d((1, 2)))
        self.lstm_encoder = nn.LSTM(c * (config.num_mels + 4), config.hidden_size, config.num_layers, bias=True, bidirectional=True)


class _FixedAttention(nn.Module):
    """Parameter container of ``FixedAttentionModule`` (rnn.py:171-177)."""

    def __init__(self, config: FixedAttentionModuleConfig):
        super().__init__()
        self.context_vec = nn.Parameter(torch.Tensor(config.hidden_size * 2).uniform_(-0.25, 0.25), requires_grad=True)
        self.v_proj = nn.Linear(config.hidden_size * 2, config.hidden_size * 2)
        self.k_proj = nn.Linear(config.hidden_size * 2, config.hidden_size * 2)
        self.num_heads = config.num_heads


class LASClassifier(RegisteredModel, name="las"):
    """``LASClassifier`` of the reference (rnn.py:133-215) on the kernels of ``howl_amd/csrc/las.hip``, the whole model one C-ABI
    call per direction: Conv2d(3,8,3,padding=2) - BatchNorm - ReLU - MaxPool(1,2) - Conv2d(8,8,3,padding=2) - BatchNorm - ReLU
    - MaxPool(1,2) - bidirectional LSTM(352 -> 96) on the packed batch - ``FixedAttentionModule`` (4 heads; the scores come from
    ``v_proj``, the weighted sum runs over ``k_proj``'s output, as the reference's arithmetic has it) - Linear(192,256) - ReLU
    - Dropout(0.1) - Linear(256, num_labels).  Same construction order and ``state_dict`` keys, the double registration of conv1 /
    conv2 included (35 keys, 25 distinct parameters): a reference workspace loads with ``strict=True`` and a saved one loads in the
    reference; the ``nn`` modules are parameter containers only.

    The whole (B, 3, 40, T) buffer goes through the encoder, padded frames included (they count in the BatchNorm statistics, as
    in the reference); utterance b's recurrences and attention run ``n_b = (((lengths[b] + 2) // 2) + 2) // 2`` steps.  Decided once:

    * the reference keeps the batch's padded steps ``n_b <= t < max n_b`` in the softmax with an additive -100.  Their ``rnn_seq`` is
      zero, and their softmax weight is at most e^(-100 + spread) of the largest, which vanishes against 1 in fp32.  The kernels
      leave these steps out, so an utterance's result never depends on its batch neighbours (the float64 restatement of
      ``tests/las_util.py`` keeps them: the tests would show if it ever mattered);
    * this class never writes to ``lengths``;
    * like ``pack_padded_sequence``, host ``lengths`` must be sorted in decreasing order and lie in 1..T; device-resident lengths
      together with ``t_out`` are trusted;
    * any config other than ``num_mels=40, num_spec_channels=3, num_latent_channels=8, hidden_size=96, num_layers=1,
      use_maxpool=True``, 4 heads and ``dnn_size=256`` raises ``NotImplementedError`` at construction;
    * dropout draws one ``howl_dropout_mask`` launch per training forward, keyed from torch's CPU generator and salted by the
      replica rank, unless ``forced_keep_mask`` (B, 256 of 0/1) is set;
    * the gradients of ``conv1.bias``, ``conv2.bias`` (each in front of a batch-statistics BatchNorm) and ``attn.v_proj.bias`` (a
      constant under the softmax over time) are identically zero and come back as exact zeros.

    Not sequential; no streaming state."""
    NEEDS_LENGTHS = True       # FusedTrainer.step passes the frame lengths through
    FEATURE_CHANNELS = 3       # log-mels, deltas, accelerations: ``log_mel_for_model(channels=3)``

    def __init__(self, num_labels: int, config: LASClassifierConfig = None):
        super().__init__(num_labels)
        config = config or LASClassifierConfig()
        enc, att = config.las_config, config.fixed_attn_config
        for obj, name, want in ((enc, "num_mels", 40), (enc, "num_spec_channels", 3), (enc, "num_latent_channels", 8), (enc, "hidden_size", 96),
                                (enc, "num_layers", 1), (enc, "use_maxpool", True), (att, "num_heads", 4), (att, "hidden_size", 96),
                                (config, "dnn_size", 256)):
            if getattr(obj, name) != want:
                raise NotImplementedError(f"the MI355X las kernels are specialised for {name}={want} (got {getattr(obj, name)})")
        if not 0.0 <= config.dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1) (got {config.dropout})")
        self.encoder = _LasEncoder(enc)
        self.attn = _FixedAttention(att)
        self.fc = nn.Sequential(nn.Linear(enc.hidden_size * 2, config.dnn_size), nn.ReLU(), nn.Dropout(config.dropout),
                                nn.Linear(config.dnn_size, num_labels))
        self.dropout_p = config.dropout
        self.forced_keep_mask = None     # tests: (B, 256) 0/1 mask used instead of a fresh draw
        self._las_saved = None

    def hot_parameters(self):
        """The 25 distinct parameters in the library's gradient order (``HowlLasGrads``) = ``state_dict`` order without the aliases."""
        e, r, a, d = self.encoder, self.encoder.lstm_encoder, self.attn, self.fc
        bn1, bn2 = e.conv_encoder[1], e.conv_encoder[5]
        return [e.conv1.weight, e.conv1.bias, e.conv2.weight, e.conv2.bias, bn1.weight, bn1.bias, bn2.weight, bn2.bias,
                r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0, r.weight_ih_l0_reverse, r.weight_hh_l0_reverse,
                r.bias_ih_l0_reverse, r.bias_hh_l0_reverse, a.context_vec, a.v_proj.weight, a.v_proj.bias, a.k_proj.weight, a.k_proj.bias,
                d[0].weight, d[0].bias, d[3].weight, d[3].bias]

    def _inputs(self, x, lengths, t_out):
        """-> (x (B, 3, 40, T), device int64 lengths or None).  Host lengths are checked as ``SimpleGru._inputs`` checks them; device
        lengths with ``t_out`` (their maximum) are trusted."""
        if not ops.on_device(x):
            raise _lib.HowlHipError("las input must be on a HIP device (no CPU fallback)")
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"las reads three feature channels: x must be (B, 3, 40, T), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError("las input must be float32")
        B, T = x.shape[0], x.shape[3]
        if lengths is not None and t_out is not None and ops.on_device(lengths):
            if lengths.numel() != B or not 1 <= t_out <= T:
                raise RuntimeError("lengths must have one entry per sequence and t_out must be in 1..T")
            lengths = lengths.to(torch.int64)
        elif lengths is not None:
            lc = lengths.detach().cpu().long()
            if lc.numel() != B:
                raise RuntimeError("lengths must have one entry per sequence")
            if (lc[:-1] < lc[1:]).any():
                raise RuntimeError("`lengths` array must be sorted in decreasing order (pack_padded_sequence semantics)")
            if lc.min() <= 0 or lc.max() > T:
                raise RuntimeError("lengths must be in 1..T")
            lengths = lc.to(x.device)
        return x, lengths

    def _draw_mask(self, B, device):
        if self.forced_keep_mask is not None:
            return self.forced_keep_mask.to(device=device, dtype=torch.float32).contiguous()
        if self.dropout_p <= 0:
            return None
        # one launch of the counter-based device generator; the key comes from torch's CPU generator (a host draw: reproducible
        # under torch.manual_seed, nothing read back from the device)
        mask = torch.empty((B, 256), dtype=torch.float32, device=device)
        key = int(torch.randint(0, 2 ** 62, (1,)).item())
        key ^= (parallel.world_info()[0] * 0x9E3779B97F4A7C15) & (2 ** 62 - 1)   # replicas share the CPU seed, not the mask
        _lib.get().call("howl_dropout_mask", _vp(mask), mask.numel(), float(self.dropout_p), ctypes.c_ulonglong(key), ops._stream())
        return mask

    def _bn_buffers(self):
        bn1, bn2 = self.encoder.conv_encoder[1], self.encoder.conv_encoder[5]
        return _lib.HowlLasBuffers(_vp(bn1.running_mean), _vp(bn1.running_var), _vp(bn1.num_batches_tracked), _vp(bn2.running_mean),
                                   _vp(bn2.running_var), _vp(bn2.num_batches_tracked))

    def _launch_forward(self, feat, lengths, t_out=None):
        """feat (B, 3, 40, T) in any strides, frame lengths (or None = all T) -> logits (B, num_labels); in training mode keeps
        what ``_launch_backward`` needs (the library's workspace)."""
        x, lengths = self._inputs(feat, lengths, t_out)
        B, _, M, T = x.shape
        cdll = _lib.get().cdll
        if not cdll.howl_las_supported(B, M, T, self.num_labels):
            raise _lib.HowlHipError(f"las: B={B}, {M} mel bins, T={T}, {self.num_labels} labels is outside the kernels' range "
                                    f"(40 mel bins, 1..8192 frames, 1..64 labels)")
        prm = _lib.HowlLasParams(*[_vp(p) for p in self.hot_parameters()])
        buf = self._bn_buffers()
        ws = torch.empty(cdll.howl_las_workspace_bytes(B, T), dtype=torch.uint8, device=x.device)
        logits = torch.empty((B, self.num_labels), dtype=torch.float32, device=x.device)
        mask = self._draw_mask(B, x.device) if self.training else None
        if mask is not None and tuple(mask.shape) != (B, 256):
            raise RuntimeError(f"forced_keep_mask must be ({B}, 256), got {tuple(mask.shape)}")
        scale = 1.0 / (1.0 - self.dropout_p) if mask is not None else 1.0
        _lib.get().call("howl_las_fwd", ctypes.byref(prm), ctypes.byref(buf), _vp(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), B, M,
                        T, self.num_labels, _vp(lengths), int(self.training), _vp(mask), scale, _vp(logits), _vp(ws), ws.numel(),
                        ops._stream())
        self._las_saved = (x, lengths, scale, ws, mask) if self.training else None
        return logits

    def _launch_backward(self, feat, dlogits, out_grads=None):
        if self._las_saved is None:
            raise NotImplementedError("las: the backward pass needs a training-mode forward (eval mode saves nothing)")
        x, lengths, scale, ws, _ = self._las_saved
        B, _, M, T = x.shape
        ps = self.hot_parameters()
        grads = out_grads if out_grads is not None else [torch.empty_like(p) for p in ps]
        prm = _lib.HowlLasParams(*[_vp(p) for p in ps])
        gr = _lib.HowlLasGrads(*[_vp(g) for g in grads])
        dlogits = dlogits.contiguous()
        _lib.get().call("howl_las_bwd", ctypes.byref(prm), _vp(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), B, M, T,
                        self.num_labels, _vp(lengths), scale, _vp(dlogits), ctypes.byref(gr), _vp(ws), ws.numel(), ops._stream())
        self._las_saved = None
        return grads

    def forward(self, x, lengths):
        return _LasFunction.apply(self, x, lengths, None, *self.hot_parameters())

    def stream_session(self, std, zmuv) -> LasStreamSession:
        """A streaming session over this model, ``std`` (a ``StandardAudioTransform``) and ``zmuv`` (a ``ZmuvTransform`` or None):
        raw PCM windows -> probabilities in one launch, with buffers of its own (``LasStreamSession``)."""
        return LasStreamSession(self, std, zmuv)
