"""Thin torch-tensor front of the C ABI: pointer / stream plumbing only, no arithmetic.

Every function requires HIP-resident, contiguous fp32 tensors and enqueues on torch's current stream.  There is
deliberately no CPU branch: a CPU tensor raises.
"""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib

HOP = 200
N_FFT = 512


def on_device(t) -> bool:
    """The single residency check of the package: every tensor handed to the C ABI must live in HIP device memory."""
    return t.is_cuda


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, dtype=torch.float32, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError("tensor required")
    if not on_device(t):
        raise _lib.HowlHipError("howl_amd ops need HIP-device tensors (no CPU fallback); got a CPU tensor")
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return ctypes.c_void_p(t.data_ptr())


def num_frames(length: int) -> int:
    return 1 + length // HOP


def fb_pack(fb: torch.Tensor) -> torch.Tensor:
    """(257, M) filterbank on the device -> packed operand (one (260, 48) bank, two beyond 48 mel bins)."""
    out = torch.empty(_lib.fb_packed_floats(fb.shape[1]), dtype=torch.float32, device=fb.device)
    _lib.get().call("howl_fb_pack", _p(fb), fb.shape[1], _p(out), _stream())
    return out


def fb_from_points(f_pts, n_mels: int, nyquist: float, out: torch.Tensor) -> torch.Tensor:
    """M+2 corner frequencies (host floats) -> packed filterbank written into ``out`` (device, ``fb_packed_floats(M)`` floats)."""
    if out.numel() < _lib.fb_packed_floats(n_mels):
        raise ValueError(f"packed filterbank buffer holds {out.numel()} floats, {n_mels} mel bins need {_lib.fb_packed_floats(n_mels)}")
    pts = _lib.HowlMelPoints()
    vals = np.asarray(f_pts, dtype=np.float32)
    np.frombuffer(pts, dtype=np.float32)[:vals.size] = vals      # (one block copy: a Python loop over 42 floats cost 9 us)
    _lib.get().call("howl_fb_from_points", ctypes.byref(pts), n_mels, float(nyquist), _p(out), _stream())
    return out


def logmel(pcm: torch.Tensor, fbp: torch.Tensor, n_mels: int, zmuv_pair=None, layout: int = 0,
           log_eps: float = 1e-7) -> torch.Tensor:
    """(B, L) PCM -> log-mel (B, M, T) [layout 0] or (B, T, M) [layout 1]; optional fused ZMUV."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (B, L)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    B, L = pcm.shape
    T = num_frames(L)
    out = torch.empty((B, n_mels, T) if layout == 0 else (B, T, n_mels), dtype=torch.float32, device=pcm.device)
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    _lib.get().call("howl_logmel_fwd", ctypes.c_void_p(pcm.data_ptr()), B, L, pcm.stride(0), _p(fbp), n_mels,
                    log_eps, _p(zmuv_pair, allow_none=True), _p(out), layout, _stream())
    return out


def logmel_args(pcm: torch.Tensor, fbp: torch.Tensor, n_mels: int, zmuv_pair=None, layout: int = 0, log_eps: float = 1e-7):
    """``logmel``'s call as a ``HowlLogmelArgs`` record for entry points that run the frontend of the NEXT batch themselves
    (``howl_lstm_fwd_next``): returns (record, out tensor, tensors the record points into -- keep them alive until the call)."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (B, L)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    B, L = pcm.shape
    T = num_frames(L)
    out = torch.empty((B, n_mels, T) if layout == 0 else (B, T, n_mels), dtype=torch.float32, device=pcm.device)
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    rec = _lib.HowlLogmelArgs(ctypes.c_void_p(pcm.data_ptr()), B, L, pcm.stride(0), _p(fbp), n_mels, log_eps,
                              _p(zmuv_pair, allow_none=True), _p(out), layout)
    return rec, out, (pcm, fbp, zmuv_pair)


def deltas(logmel_bmt: torch.Tensor, zmuv_pair=None) -> torch.Tensor:
    B, M, T = logmel_bmt.shape
    out = torch.empty((B, 3, M, T), dtype=torch.float32, device=logmel_bmt.device)
    _lib.get().call("howl_deltas_fwd", _p(logmel_bmt), B, M, T, _p(zmuv_pair, allow_none=True), _p(out), _stream())
    return out


def zmuv_update(x, total, mean, mean2, scratch):
    _lib.get().call("howl_zmuv_update", _p(x), x.numel(), _p(total), _p(mean), _p(mean2),
                    _p(scratch, torch.float64), _stream())


def zmuv_update_masked(x, mask, total, mean, mean2, scratch, count_scale=1.0):
    """``mask`` already expanded to ``x``'s shape; ``count_scale`` = (unexpanded mask size) / x.numel()."""
    _lib.get().call("howl_zmuv_update_masked", _p(x), _p(mask), x.numel(), float(count_scale), _p(total), _p(mean), _p(mean2),
                    _p(scratch, torch.float64), _stream())


def zmuv_pair(mean, mean2, out):
    _lib.get().call("howl_zmuv_pair", _p(mean), _p(mean2), _p(out), _stream())
    return out


def zmuv_apply(x, pair):
    out = torch.empty_like(x)
    _lib.get().call("howl_zmuv_apply", _p(x), x.numel(), _p(pair), _p(out), _stream())
    return out


def collate_augment(bank, idx, src_len, shift, from_head, sigma, sp_prob, seed, lout, mix=None, dst_off=None):
    """``mix`` = (bg_bank (N, Lbg), bg_idx, bg_off, alpha) puts DatasetMixer in front of the chain; ``dst_off`` (int32 per
    row) places the samples that many columns into the zero row (frame batchifier's front padding)."""
    B = idx.numel()
    out = torch.empty((B, lout), dtype=torch.float32, device=bank.device)
    if mix is None:
        bg, bg_ld, bg_idx, bg_off, alpha = None, 0, None, None, None
    else:
        bg, bg_ld = _p(mix[0]), mix[0].stride(0)
        bg_idx, bg_off, alpha = _p(mix[1], torch.int32), _p(mix[2], torch.int32), _p(mix[3])
    _lib.get().call("howl_collate_augment_window", _p(bank), bank.stride(0), _p(idx, torch.int32), _p(src_len, torch.int32),
                    _p(shift, torch.int32), _p(from_head, torch.int32), _p(sigma), _p(sp_prob),
                    ctypes.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF), bg, bg_ld, bg_idx, bg_off, alpha,
                    _p(dst_off, torch.int32, allow_none=True), B, lout, _p(out), _stream())
    return out


def stretch_records(src_rows, lengths, rates, mix=None):
    """``HowlStretchClip`` records (a numpy record array, ``lib.STRETCH_CLIP_FIELDS``) for clips of ``lengths`` samples at bank
    rows ``src_rows`` stretched by ``rates``, their outputs back to back; returns (records, total output samples).
    ``mix`` = (bg_idx, bg_off, alpha) per clip (``DatasetMixer``'s draws)."""
    n = len(lengths)
    rec = np.zeros(n, dtype=np.dtype(_lib.STRETCH_CLIP_FIELDS))
    lens = np.asarray(lengths, dtype=np.int64)
    rec["rate"], rec["src_row"], rec["len"] = rates, src_rows, lens
    rec["out_len"] = np.rint(lens / rec["rate"])                                                # Python's round (half to even), as librosa
    rec["n_out"] = np.ceil((1 + lens // 512) / rec["rate"])                                     # len(np.arange(0, n_in, rate))
    rec["dst_off"] = np.cumsum(rec["out_len"], dtype=np.int64) - rec["out_len"]
    if mix is not None:
        rec["bg_idx"], rec["bg_off"], rec["alpha"] = mix
    return rec, int(rec["out_len"].sum(dtype=np.int64))


def time_stretch(bank, records, records_dev, total, bg=None, through_transform=False):
    """``TimestretchTransform`` for a batch of ragged clips in one launch: ``records`` (``stretch_records``) are read on the
    host, ``records_dev`` (the same bytes in device memory, e.g. an int64 tensor) by the kernel; returns the flat (``total``,)
    buffer of stretched clips, clip b at ``records["dst_off"][b]`` -- viewed (total, 1) it is a ragged bank for
    ``collate_augment``.  ``bank``: (N, Lmax), or the (total, 1) view of a flat buffer with ``src_row`` = sample offset.
    ``bg``: the background bank of the records' mix.  A clip of rate 1.0 is copied unless ``through_transform``."""
    records = np.ascontiguousarray(records)
    if records.dtype.itemsize != 48:
        raise TypeError("records must be HowlStretchClip records (ops.stretch_records)")
    if not on_device(records_dev):
        _p(records_dev)
    if records_dev.numel() * records_dev.element_size() < records.nbytes or records_dev.data_ptr() % 8:
        raise ValueError("records_dev must hold the records' bytes at an 8-byte aligned address")
    out = torch.empty(max(total, 1), dtype=torch.float32, device=bank.device)
    _lib.get().call("howl_timestretch_clips", _p(bank), bank.stride(0), bank.numel(), _p(bg, allow_none=True),
                    0 if bg is None else bg.stride(0), 0 if bg is None else bg.numel(), ctypes.c_void_p(records.ctypes.data),
                    ctypes.c_void_p(records_dev.data_ptr()), len(records), _p(out), total,
                    _lib.TIMESTRETCH_NO_COPY if through_transform else 0, _stream())
    return out[:total]


_RESAMPLE_PLANS = {}


def resample_plan(sr_in: int, sr_out: int):
    """``howl_resample_plan`` for a rate pair -> (``HowlResamplePlan``, the host bank as a (up, taps) float32 array), computed
    once per pair.  A pair outside the supported range raises ``HowlHipError`` with the pair in its message."""
    key = (int(sr_in), int(sr_out))
    if key not in _RESAMPLE_PLANS:
        plan = _lib.HowlResamplePlan()
        lib = _lib.get()
        lib.call("howl_resample_plan", key[0], key[1], ctypes.byref(plan))
        bank = np.empty((plan.up, plan.taps), dtype=np.float32)
        assert lib.cdll.howl_resample_bank_floats(ctypes.byref(plan)) == bank.size
        lib.call("howl_resample_bank", ctypes.byref(plan), ctypes.c_void_p(bank.ctypes.data))
        _RESAMPLE_PLANS[key] = (plan, bank)
    return _RESAMPLE_PLANS[key]


def resample_out_len(plan, length: int) -> int:
    """ceil(length * up / down): the full output length of a clip of ``length`` frames."""
    return (int(length) * plan.up + plan.down - 1) // plan.down


def resample_records(src_offs, lengths, dst_offs, out_lens):
    """``HowlResampleClip`` records (``lib.RESAMPLE_CLIP_FIELDS``): clip b is frames ``src_offs[b] .. + lengths[b]`` of the source
    and becomes ``out[dst_offs[b] .. + out_lens[b])``."""
    rec = np.zeros(len(lengths), dtype=np.dtype(_lib.RESAMPLE_CLIP_FIELDS))
    rec["src_off"], rec["dst_off"], rec["len"], rec["out_len"] = src_offs, dst_offs, lengths, out_lens
    return rec


def resample_clips(src, channels: int, plan, bank_dev, records, records_dev, out):
    """Channel mean + band-limited resampling of a batch of ragged clips in one launch (``howl_resample_clips``), written into
    ``out`` (a flat float32 device buffer: a dense (N, max_len) bank viewed flat, or a ragged flat bank) at the records'
    ``dst_off``; nothing else of ``out`` is touched.  ``src``: the raw interleaved samples on the device, int16 or float32, flat;
    ``bank_dev``: ``resample_plan``'s bank on the device; ``records`` (``resample_records``) are read on the host,
    ``records_dev`` (the same bytes in device memory, e.g. an int64 tensor) by the kernel."""
    records = np.ascontiguousarray(records)
    if records.dtype.itemsize != 24:
        raise TypeError("records must be HowlResampleClip records (ops.resample_records)")
    fmt = {torch.float32: _lib.RESAMPLE_F32, torch.int16: _lib.RESAMPLE_I16}.get(src.dtype)
    if fmt is None:
        raise TypeError(f"expected float32 or int16 samples, got {src.dtype}")
    if not on_device(records_dev):
        _p(records_dev)
    if records_dev.numel() * records_dev.element_size() < records.nbytes or records_dev.data_ptr() % 8:
        raise ValueError("records_dev must hold the records' bytes at an 8-byte aligned address")
    _lib.get().call("howl_resample_clips", _p(src, src.dtype), src.numel(), fmt, int(channels), _p(bank_dev), bank_dev.numel(),
                    ctypes.byref(plan), ctypes.c_void_p(records.ctypes.data), ctypes.c_void_p(records_dev.data_ptr()), len(records),
                    _p(out), out.numel(), _stream())
    return out


def gather_windows(bank, idx, start, length, dst_off, lout):
    """Rows ``bank[idx[b], start[b]:start[b]+length[b]]`` placed at column ``dst_off[b]`` of a zero (B, lout) batch."""
    B = idx.numel()
    out = torch.empty((B, lout), dtype=torch.float32, device=bank.device)
    _lib.get().call("howl_gather_windows", _p(bank), bank.stride(0), _p(idx, torch.int32), _p(start, torch.int32),
                    _p(length, torch.int32), _p(dst_off, torch.int32), B, lout, _p(out), _stream())
    return out


def specaug_mask(x, f0, f, t0, t):
    B, C, M, T = x.shape
    if not on_device(x) or x.dtype != torch.float32:
        _p(x)
    sb, sc, sm, st = x.stride()
    _lib.get().call("howl_specaug_mask", ctypes.c_void_p(x.data_ptr()), B, C, M, T, sb, sc, sm, st, _p(f0, torch.int32),
                    _p(f, torch.int32), _p(t0, torch.int32), _p(t, torch.int32), _stream())
    return x


def xent(logits, labels, want_grad=True):
    B, C = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    _lib.get().call("howl_xent_fwd_bwd", _p(logits), _p(labels, torch.int64), B, C, _p(loss),
                    _p(dlogits, allow_none=True), _stream())
    return loss, dlogits


def _ctc_launch(scores, targets, input_lengths, target_lengths, blank, max_target, want_grad, defer_mean=False, long_targets=False):
    T, B, C = scores.shape
    dev = scores.device
    # the gradient takes the memory layout of the model's (B, T, C) output buffer, handed back as a (T, B, C) view
    dlogits = torch.empty((B, T, C), dtype=torch.float32, device=dev).permute(1, 0, 2) if want_grad else None
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # strided views: strides are passed explicitly
    # whole clips (more than 128 frames): the alpha rows of the windows behind the last one wait in a workspace
    # (long_targets: howl_ctc_loss_long, include/howl_hip_ctc_long.h -- the window and the row width depend on the longest target)
    if long_targets:
        _ctc_long_check(T, C, max_target)
        ws_floats = int(_lib.get().cdll.howl_ctc_long_workspace_floats(T, B, max_target)) if want_grad else 0
    else:
        ws_floats = int(_lib.get().cdll.howl_ctc_workspace_floats(T, B)) if want_grad else 0
    ws = torch.empty(ws_floats, dtype=torch.float32, device=dev) if ws_floats else None
    _lib.get().call("howl_ctc_loss_long" if long_targets else "howl_ctc_loss", vp(scores), scores.stride(0), scores.stride(1), T, B, C, vp(targets),
                    targets.stride(0), max_target, _p(input_lengths, torch.int64), _p(target_lengths, torch.int64), blank,
                    _p(nll), None if defer_mean else _p(loss), vp(dlogits), 0 if dlogits is None else dlogits.stride(0),
                    0 if dlogits is None else dlogits.stride(1), vp(ws), ws_floats, _stream())
    if defer_mean:      # `loss` is filled by howl_head_bwd's HowlCtcMean rider
        return loss, dlogits, nll
    return loss, dlogits


class _CtcLoss(torch.autograd.Function):
    """loss = CTCLoss(blank)(log_softmax(scores, -1), targets, input_lengths, target_lengths), reduction "mean": the fused
    kernel returns the loss and d loss / d scores in one pass (``howl_ctc_loss``)."""

    @staticmethod
    def forward(ctx, scores, targets, input_lengths, target_lengths, blank, max_target, long_targets=False):
        loss, dlogits = _ctc_launch(scores, targets, input_lengths, target_lengths, blank, max_target,
                                    ctx.needs_input_grad[0], long_targets=long_targets)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dlogits,) = ctx.saved_tensors
        return dlogits * grad_out, None, None, None, None, None, None


def _ctc_args(scores, targets, input_lengths, target_lengths, max_target):
    if not on_device(scores):
        raise _lib.HowlHipError("ctc_loss: scores must be on a HIP device (no CPU fallback)")
    if scores.dim() != 3 or targets.dim() != 2:
        raise ValueError("ctc_loss: scores must be (T, B, C) and targets the padded (B, L) matrix")
    if max_target is None:
        max_target = int(target_lengths.max()) if target_lengths.numel() else 0
    if max_target > targets.shape[1]:
        raise ValueError("ctc_loss: a target length exceeds the width of the target matrix")
    dev = scores.device
    targets = targets.to(dev, torch.int64)
    if targets.shape[1] > 0 and (targets.stride(1) != 1 or (targets.shape[0] > 1 and targets.stride(0) < max_target)):
        targets = targets.contiguous()          # rows of max_target labels that do not overlap (an expanded matrix: stride 0)
    return (targets, input_lengths.to(dev, torch.int64).contiguous(), target_lengths.to(dev, torch.int64).contiguous(),
            max_target)


def ctc_supported(T: int, C: int, max_target: int) -> bool:
    return bool(_lib.get().cdll.howl_ctc_supported(int(T), int(C), int(max_target)))


CTC_LONG_MAX_LABELS = 255      # HOWL_CTC_LONG_MAX_LABELS


def ctc_long_supported(T: int, C: int, max_target: int) -> bool:
    """``howl_ctc_long_supported``: the range of ``ctc_loss(..., long_targets=True)``."""
    return bool(_lib.get().cdll.howl_ctc_long_supported(int(T), int(C), int(max_target)))


def _ctc_long_check(T, C, max_target):
    if not ctc_long_supported(T, C, max_target):
        raise _lib.HowlHipError(f"ctc_loss: T={T} frames, C={C} classes, the batch's longest target has {max_target} labels: outside "
                                f"howl_ctc_loss_long's range (T <= 8192, C <= 64, targets <= {CTC_LONG_MAX_LABELS} labels)")


def ctc_loss_fwd_bwd(scores, targets, input_lengths, target_lengths, blank: int, max_target=None, defer_mean=False,
                     long_targets: bool = False):
    """Loss and d loss / d scores without an autograd graph (training.fused.FusedTrainer.step_sequence): same kernel as
    ``ctc_loss``; the batch must be inside the kernel's range.  ``defer_mean``: returns (loss, dscores, nll, target_lengths)
    with ``loss`` still unwritten -- the batch mean is left to ``howl_head_bwd`` (``SequentialLstm._launch_backward(...,
    ctc_mean=(nll, target_lengths, loss))``), one launch fewer.  ``long_targets``: as for ``ctc_loss``."""
    targets, input_lengths, target_lengths, max_target = _ctc_args(scores, targets, input_lengths, target_lengths, max_target)
    if scores.stride(2) != 1 or scores.dtype != torch.float32:
        raise ValueError("ctc_loss_fwd_bwd: scores must be fp32 with unit stride over the classes")
    out = _ctc_launch(scores, targets, input_lengths, target_lengths, int(blank), max_target, True, defer_mean, long_targets)
    return out + (target_lengths,) if defer_mean else out


def ctc_loss(scores, targets, input_lengths, target_lengths, blank: int, long_targets: bool = False):
    """``nn.CTCLoss(blank)(torch.log_softmax(scores, -1), targets, input_lengths, target_lengths)`` of the reference's training
    loop (train.py:250-256, 291-296) for ``scores`` of shape (T, B, C) on the device, as ONE fused kernel.  ``targets`` is the
    padded (B, L) int64 matrix; the two length vectors may live on the host (as in the reference) or on the device.  Whole
    clips are inside the kernel's range (T <= 8192 frames, walked in 128-frame windows); a batch outside it (C > 64, a
    target longer than 31 labels -- 255 with ``long_targets=True``, scores that are not fp32) raises -- the training path has no
    vendor fallback.  ``long_targets=True`` takes ``howl_ctc_loss_long`` (include/howl_hip_ctc_long.h): the same bits for a batch
    of at most 31 labels, and 2, 4 or 8 states of the label sequence per lane beyond (up to 63, 127, 255 labels)."""
    targets_d, in_d, tl_d, max_target = _ctc_args(scores, targets, input_lengths, target_lengths, None)
    T, B, C = scores.shape
    if scores.dtype != torch.float32:
        raise _lib.HowlHipError(f"ctc_loss: scores must be fp32 (got {scores.dtype})")
    if long_targets:
        _ctc_long_check(T, C, max_target)
    elif not _lib.get().cdll.howl_ctc_supported(T, C, max_target):
        raise _lib.HowlHipError(f"ctc_loss: T={T} frames, C={C} classes, targets of {max_target} labels: outside howl_ctc_loss's "
                                "range (T <= 8192, C <= 64, targets <= 31)")
    if scores.stride(2) != 1:
        scores = scores.contiguous()
    return _CtcLoss.apply(scores, targets_d, in_d, tl_d, int(blank), max_target, bool(long_targets))


def adamw_step(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=1.0):
    _lib.get().call("howl_adamw_step", _p(p), _p(g), _p(m), _p(v), p.numel(), lr, betas[0], betas[1], eps,
                    weight_decay, step, grad_scale, _stream())


def _stream_query(symbol, result):
    """The streaming entry points' queries are one wrapper for every model: ``*_stream_supported(n_samples, n_mels, n_labels) -> bool``,
    ``*_stream_state_bytes(n_labels) -> int``, ``*_stream_workspace_bytes(n_windows, n_samples) -> int``."""
    def query(*values):
        return result(getattr(_lib.get().cdll, symbol)(*[int(v) for v in values]))
    return query


# ---- streaming res8 (include/howl_hip_stream.h): one launch from the windows' PCM to their probabilities ----------------------------

res8_stream_supported = _stream_query("howl_res8_stream_supported", bool)
res8_stream_state_bytes = _stream_query("howl_res8_stream_state_bytes", int)


def res8_stream_prepare(prm, n_labels: int, state: torch.Tensor) -> torch.Tensor:
    """``prm``: a ``HowlRes8Params`` record (``Res8._params_struct``) -> the prepared ``state`` (uint8, ``res8_stream_state_bytes``)."""
    _lib.get().call("howl_res8_stream_prepare", ctypes.byref(prm), int(n_labels), _p(state, torch.uint8), state.numel(), _stream())
    return state


def res8_stream_windows(state, pcm, fbp, n_mels, zmuv_pair, n_labels, probs=None, logits=None, log_eps: float = 1e-7):
    """(N, L) PCM windows (unit sample stride, any row stride: overlapping views of one clip are fine) -> (N, C) probabilities in one
    launch; ``logits`` (N, C), when given, receives the pre-softmax scores."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (N, L)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    N, L = pcm.shape
    if probs is None:
        probs = torch.empty((N, n_labels), dtype=torch.float32, device=pcm.device)
    _lib.get().call("howl_res8_stream_windows", _p(state, torch.uint8), ctypes.c_void_p(pcm.data_ptr()), pcm.stride(0), N, L, _p(fbp),
                    int(n_mels), log_eps, _p(zmuv_pair, allow_none=True), int(n_labels), _p(probs), _p(logits, allow_none=True),
                    _stream())
    return probs


# ---- streaming las (include/howl_hip_las_stream.h): one launch from the windows' PCM to their probabilities -------------------------

las_stream_supported = _stream_query("howl_las_stream_supported", bool)
las_stream_state_bytes = _stream_query("howl_las_stream_state_bytes", int)
las_stream_workspace_bytes = _stream_query("howl_las_stream_workspace_bytes", int)


def las_stream_prepare(prm, buffers, n_labels: int, state: torch.Tensor) -> torch.Tensor:
    """``prm`` / ``buffers``: ``HowlLasParams`` / ``HowlLasBuffers`` records -> the prepared ``state`` (uint8, ``las_stream_state_bytes``)."""
    _lib.get().call("howl_las_stream_prepare", ctypes.byref(prm), ctypes.byref(buffers), int(n_labels), _p(state, torch.uint8),
                    state.numel(), _stream())
    return state


def las_stream_windows(state, pcm, frames: int, fbp, n_mels, zmuv_pair, n_labels, ws, probs=None, logits=None, log_eps: float = 1e-7):
    """(N, L) PCM windows (unit sample stride, any row stride: overlapping views of one clip are fine) -> (N, C) probabilities in one
    launch; ``frames``: the windows' ``compute_lengths``; ``ws``: uint8 scratch of ``las_stream_workspace_bytes(N, L)``; ``logits``
    (N, C), when given, receives the pre-softmax scores."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (N, L)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    N, L = pcm.shape
    if probs is None:
        probs = torch.empty((N, n_labels), dtype=torch.float32, device=pcm.device)
    _lib.get().call("howl_las_stream_windows", _p(state, torch.uint8), ctypes.c_void_p(pcm.data_ptr()), pcm.stride(0), N, L, int(frames),
                    _p(fbp), int(n_mels), log_eps, _p(zmuv_pair, allow_none=True), int(n_labels), _p(probs),
                    _p(logits, allow_none=True), _p(ws, torch.uint8), ws.numel(), _stream())
    return probs


# ---- streaming gru (include/howl_hip_gru_stream.h): one launch from the windows' PCM to their probabilities -------------------------

gru_stream_supported = _stream_query("howl_gru_stream_supported", bool)
gru_stream_workspace_bytes = _stream_query("howl_gru_stream_workspace_bytes", int)


def gru_stream_windows(prm, buffers, pcm, frames: int, fbp, n_mels, zmuv_pair, n_labels, ws, probs=None, logits=None,
                       log_eps: float = 1e-7):
    """(N, L) PCM windows (unit sample stride, any row stride: overlapping views of one clip are fine) -> (N, C) probabilities in one
    launch; ``prm`` / ``buffers``: ``HowlGruParams`` / ``HowlGruBuffers`` records, read in place; ``frames``: the windows'
    ``compute_lengths``; ``ws``: uint8 scratch of ``gru_stream_workspace_bytes(N, L)``; ``logits`` (N, C), when given, receives
    the pre-softmax scores."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (N, L)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    N, L = pcm.shape
    if probs is None:
        probs = torch.empty((N, n_labels), dtype=torch.float32, device=pcm.device)
    _lib.get().call("howl_gru_stream_windows", ctypes.byref(prm), ctypes.byref(buffers), ctypes.c_void_p(pcm.data_ptr()), pcm.stride(0), N,
                    L, int(frames), _p(fbp), int(n_mels), log_eps, _p(zmuv_pair, allow_none=True), int(n_labels), _p(probs),
                    _p(logits, allow_none=True), _p(ws, torch.uint8), ws.numel(), _stream())
    return probs


# ---- streaming small-cnn / seq-cnn (include/howl_hip_cnn_stream.h): one launch from the PCM to the probabilities --------------------
# (the queries take the kind first: ``_lib.CNN_SMALL`` or ``_lib.CNN_SEQ``)

cnn_stream_supported = _stream_query("howl_cnn_stream_supported", bool)
cnn_stream_workspace_bytes = _stream_query("howl_cnn_stream_workspace_bytes", int)
cnn_stream_rows = _stream_query("howl_cnn_stream_rows", int)


def cnn_stream_windows(prm, buffers, pcm, fbp, n_mels, zmuv_pair, n_labels, ws, probs=None, logits=None, log_eps: float = 1e-7):
    """small-cnn: (N, L) PCM windows (unit sample stride, any row stride: overlapping views of one clip are fine) -> (N, C)
    probabilities in one launch; ``prm`` / ``buffers``: ``HowlCnnParams`` / ``HowlCnnBuffers`` records, read in place; ``ws``: uint8
    scratch of ``cnn_stream_workspace_bytes(CNN_SMALL, N, L)``; ``logits`` (N, C), when given, receives the pre-softmax scores."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (N, L)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    N, L = pcm.shape
    if probs is None:
        probs = torch.empty((N, n_labels), dtype=torch.float32, device=pcm.device)
    _lib.get().call("howl_cnn_stream_windows", ctypes.byref(prm), ctypes.byref(buffers), ctypes.c_void_p(pcm.data_ptr()), pcm.stride(0), N,
                    L, _p(fbp), int(n_mels), log_eps, _p(zmuv_pair, allow_none=True), int(n_labels), _p(probs),
                    _p(logits, allow_none=True), _p(ws, torch.uint8), ws.numel(), _stream())
    return probs


def cnn_stream_clips(prm, buffers, pcm, fbp, n_mels, zmuv_pair, n_labels, ws, n_samples=None, probs=None, logits=None,
                     log_eps: float = 1e-7):
    """seq-cnn: (N, L_max) PCM clips (unit sample stride, any row stride) -> (N, cnn_stream_rows(CNN_SEQ, L_max), C) probabilities
    in one launch, the rows behind a clip's own written as zeros.  ``n_samples``: (N) int64 on the device or None (L_max for every
    clip); ``ws``: uint8 scratch of ``cnn_stream_workspace_bytes(CNN_SEQ, N, L_max)``; ``logits``, when given, receives the
    pre-softmax scores in the layout of ``probs``."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (N, L_max)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    N, L = pcm.shape
    if probs is None:
        probs = torch.empty((N, cnn_stream_rows(_lib.CNN_SEQ, L), n_labels), dtype=torch.float32, device=pcm.device)
    _lib.get().call("howl_cnn_stream_clips", ctypes.byref(prm), ctypes.byref(buffers), ctypes.c_void_p(pcm.data_ptr()),
                    pcm.stride(0) if N > 1 else L, N, L, _p(n_samples, torch.int64, allow_none=True), _p(fbp), int(n_mels), log_eps,
                    _p(zmuv_pair, allow_none=True), int(n_labels), _p(probs), _p(logits, allow_none=True), probs.stride(0),
                    _p(ws, torch.uint8), ws.numel(), _stream())
    return probs


# ---- streaming seq-lstm / lstm (include/howl_hip_lstm_stream.h): one launch from N PCM chunks to their frame probabilities --------

lstm_stream_supported = _stream_query("howl_lstm_stream_supported", bool)


def lstm_stream_chunks(lstm_prm, head_prm, pcm, fbp, n_mels, zmuv_pair, n_labels, n_samples=None, frames=None, h=None, c=None,
                       last_only=False, probs=None, logits=None, log_eps: float = 1e-7):
    """(N, L_max) PCM chunks (unit sample stride, any row stride) -> probabilities in one launch: (N, 1 + L_max // 200, C), or (N, C)
    with ``last_only``.  ``lstm_prm`` / ``head_prm``: ``HowlLstmParams`` / ``HowlHeadParams`` records; ``n_samples`` / ``frames``: (N)
    int64 on the device or None; ``h`` / ``c``: (N, 128) start state, overwritten with the carried state (both or neither);
    ``logits``, when given, receives the pre-softmax scores in the layout of ``probs``."""
    if pcm.dim() != 2:
        raise ValueError("pcm must be (N, L_max)")
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    if not on_device(pcm) or pcm.dtype != torch.float32:
        _p(pcm)
    N, L = pcm.shape
    if probs is None:
        shape = (N, n_labels) if last_only else (N, num_frames(L), n_labels)
        probs = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    _lib.get().call("howl_lstm_stream_chunks", ctypes.byref(lstm_prm), ctypes.byref(head_prm), ctypes.c_void_p(pcm.data_ptr()),
                    pcm.stride(0) if N > 1 else L, N, L, _p(n_samples, torch.int64, allow_none=True), _p(frames, torch.int64, allow_none=True),
                    _p(fbp), int(n_mels), log_eps, _p(zmuv_pair, allow_none=True), _p(h, allow_none=True), _p(c, allow_none=True),
                    int(n_labels), 1 if last_only else 0, _p(probs), _p(logits, allow_none=True), probs.stride(0), _stream())
    return probs


def decide_supported(cfg, t_max: int) -> bool:
    return bool(_lib.get().cdll.howl_decide_supported(ctypes.byref(cfg), int(t_max)))


def decide_clips(cfg, probs, n_frames, delta_ms, t_max: int, weighted=None):
    """``howl_decide_clips`` on (N, >= t_max, C) probabilities (unit class stride, any clip / frame stride): ONE launch of the
    engines' decision logic.  ``cfg``: a ``HowlDecideConfig`` record; ``n_frames`` (N) int32 and ``delta_ms`` (N) float64 on the
    device.  -> (ints (4, N) int32: present, status, n_labels, first_kept; end_time (N) float64; hist_time (N, t_max) float64;
    hist_label (N, t_max) int32), all on the device; only the first n_labels entries of a history row are written.  The two history
    tensors are allocated in full for every call: 12 bytes x N x t_max (1 MB for 64 clips of 1300 frames; 805 MB at the range's corner of
    8192 x 8192, where a caller passes the clips in groups)."""
    if probs.dim() != 3 or probs.size(2) != cfg.C or probs.size(1) < t_max:
        raise ValueError(f"probs must be (N, >= {t_max}, {cfg.C}), got {tuple(probs.shape)}")
    if probs.stride(2) != 1:
        probs = probs.contiguous()
    if not on_device(probs) or probs.dtype != torch.float32:
        _p(probs)
    N, dev = probs.size(0), probs.device
    ints = torch.empty((4, N), dtype=torch.int32, device=dev)
    end_time = torch.empty(N, dtype=torch.float64, device=dev)
    ld = max(int(t_max), 1)
    hist_time = torch.empty((N, ld), dtype=torch.float64, device=dev)
    hist_label = torch.empty((N, ld), dtype=torch.int32, device=dev)
    _lib.get().call("howl_decide_clips", ctypes.byref(cfg), ctypes.c_void_p(probs.data_ptr()), probs.stride(0), probs.stride(1), N, int(t_max),
                    _p(n_frames, torch.int32), _p(delta_ms, torch.float64), _p(ints[0], torch.int32), _p(ints[1], torch.int32),
                    _p(ints[2], torch.int32), _p(ints[3], torch.int32), _p(end_time, torch.float64), _p(hist_time, torch.float64),
                    _p(hist_label, torch.int32), ld, _p(weighted, allow_none=True), _stream())
    return ints, end_time, hist_time, hist_label
