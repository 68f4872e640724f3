"""Streaming decision logic over model outputs: ``InferenceEngine`` / ``FrameInferenceEngine`` with the reference's
API and finite-state machine (``howl/model/inference.py:19-267``), running on the MI355X hot path.

``FrameInferenceEngine.infer`` evaluates ALL strided windows of a clip in one batched launch of the fused frontend +
model (instead of one launch and one device->host sync per 63 ms stride, ``inference.py:247-261``) and then replays
the reference's per-window loop on the host, so ``label_history`` / ``pred_history`` and the early exit are identical.
Models that carry streaming state between windows keep the sequential path.
"""
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from howl_amd.context import InferenceContext
from howl_amd.data.transform.operator import ZmuvTransform
from howl_amd.data.transform.transform import StandardAudioTransform
from howl_amd.settings import SETTINGS
from howl_amd.utils import audio_utils

from .base import RegisteredModel
from .cnn import Res8, SequentialCnn, SmallCnn
from .decision import DeviceDecider, ProbabilitySmoother, SequenceMatcher
from .rnn import LASClassifier, SequentialLstm, SimpleGru, SimpleLstm

__all__ = ["FrameInferenceEngine", "InferenceEngine"]


class InferenceEngine:
    """Sequential-model engine: one forward over the whole clip, then the frame-by-frame decision logic on the host."""

    MAX_CLIPS_PER_LAUNCH = 8192      # infer_many: clips per streaming launch

    def __init__(self, model: RegisteredModel, zmuv_transform: ZmuvTransform, context: InferenceContext,
                 time_provider=time.time):
        cfg = SETTINGS.inference_engine
        self.model, self.zmuv, self.context, self.settings = model, zmuv_transform, context, cfg
        self.std = StandardAudioTransform().eval()
        self.time_provider = time_provider
        self.sample_rate = SETTINGS.audio.sample_rate
        self.blank_idx = context.blank_label
        # per-class reweighting of the probabilities (missing entries count as 1)
        self.inference_weights = 1
        if cfg.inference_weights:
            w = np.ones(context.num_labels)
            w[:len(cfg.inference_weights)] = cfg.inference_weights
            self.inference_weights = w
        self.coloring = context.coloring
        negative = context.negative_label
        if self.coloring:
            negative = self.coloring.color_map[negative]
        self.negative_label = negative
        self.threshold = cfg.inference_threshold
        self.inference_window_ms = cfg.inference_window_ms
        self.smoothing_window_ms = cfg.smoothing_window_ms
        self.tolerance_window_ms = cfg.tolerance_window_ms
        self.sequence = cfg.inference_sequence
        self._smoother = ProbabilitySmoother(self.smoothing_window_ms, self.threshold, negative,
                                             self.coloring.color_map if self.coloring else None)
        self._matcher = SequenceMatcher(self.sequence, self.inference_window_ms, self.tolerance_window_ms)
        self.curr_time = 0
        self.label_history = []
        # infer as ONE launch (LstmStreamSession, SeqCnnStreamSession) instead of the frontend + model + softmax chain: off unless
        # asked for
        self.fused_chunks = os.environ.get("HOWL_STREAM_FUSED") == "1"
        self._stream_session = None      # (see _session)
        # infer_many: the frame-by-frame decision logic of all clips as ONE launch behind the probabilities (DeviceDecider) instead
        # of the host loops: off unless asked for
        self.device_decisions = os.environ.get("HOWL_DECIDE_DEVICE") == "1"
        self.clip_histories = []      # infer_many: each clip's label_history
        self.reset()

    # the reference exposes both histories as plain attributes; pred_history lives in the smoother
    @property
    def pred_history(self):
        return self._smoother.frames

    @pred_history.setter
    def pred_history(self, frames):
        self._smoother.frames = list(frames)

    def to(self, device: torch.device):
        self.model, self.zmuv = self.model.to(device), self.zmuv.to(device)
        return self

    def reset(self):
        self.model.streaming_state = None
        self.curr_time = 0
        self._smoother.clear()
        self.label_history = []

    def _now_ms(self, curr_time):
        return self.time_provider() * 1000 if curr_time is None else curr_time

    def append_label(self, label: int, curr_time: float = None):
        self.label_history.append((self._now_ms(curr_time), label))

    def sequence_present(self, curr_time: float = None) -> bool:
        # the matcher reads the settings through the engine so that tests / callers may retune them after construction
        self._matcher.sequence, self._matcher.window_ms = self.sequence, self.inference_window_ms
        self._matcher.tolerance_ms = self.tolerance_window_ms
        return self._matcher.present(self.label_history, self._now_ms(curr_time))

    def _append_probability_frame(self, prediction: np.ndarray, curr_time: float = None) -> int:
        now = self._now_ms(curr_time)
        self._smoother.window_ms, self._smoother.threshold = self.smoothing_window_ms, self.threshold
        label = self._smoother.push(now, prediction)
        self.label_history.append((now, label))
        return label

    def _weighted(self, prediction: np.ndarray) -> np.ndarray:
        # the reference multiplies in place (inference.py:200,263): the product is rounded back to the probabilities' own
        # dtype (fp32) before the renormalisation, which matters for comparisons right at the threshold
        prediction = (prediction * self.inference_weights).astype(prediction.dtype, copy=False)
        return prediction / prediction.sum()

    def _session(self, kinds, n_samples: int):
        """The engine's streaming session for rows of up to ``n_samples`` samples, or None when it does not apply (the model is none
        of ``kinds``, training mode, a length outside the kernel's range): the caller then takes the launch chain.  The session is
        the engine's own, made on first use and again when the model or a transform was replaced."""
        if not isinstance(self.model, kinds) or self.model.training:
            return None
        s = self._stream_session
        if s is None or s.model is not self.model or s.std is not self.std or s.zmuv is not self.zmuv:
            s = self._stream_session = self.model.stream_session(self.std, self.zmuv)
        return s if s.supported(n_samples) else None

    def _lstm_session(self, kind, n_samples: int):
        """``LstmStreamSession`` for chunks of up to ``n_samples`` samples where the model is a ``kind`` (see ``_session``)."""
        return self._session(kind, n_samples)

    # the sequential models with a chunk session (``probabilities(pcm, n_samples=, state=, return_state=)`` and ``rows_of``)
    CHUNK_MODELS = (SequentialLstm, SequentialCnn)

    def _device_decider(self, mode: int, t_max: int, min_delta_ms: float, n_clips: int):
        """The decision launch for clips of up to ``t_max`` frames with the settings as they are now, or None when the switch is off
        or the configuration is outside the kernel's range: the caller then replays the logic on the host."""
        if not self.device_decisions:
            return None
        decider = DeviceDecider.from_engine(self, mode)
        return decider if decider.supported(t_max, min_delta_ms, n_clips) else None

    def _run_frames(self, predictions: np.ndarray, delta_ms) -> bool:
        """The frame-by-frame decision logic of ``infer`` on the (frames, C) probabilities of one chunk."""
        sequence_present = False
        delta_ms /= len(predictions)
        for prediction in predictions:
            prediction = self._weighted(prediction)
            self.curr_time += delta_ms
            if np.argmax(prediction) == self.blank_idx:
                continue
            self._append_probability_frame(prediction, curr_time=self.curr_time)
            if self.sequence_present(self.curr_time):
                sequence_present = True
                break
        return sequence_present

    @torch.no_grad()
    def infer(self, audio_data: torch.Tensor) -> bool:
        """Whole clip as one batch through a sequential model (``inference.py:179-211``)."""
        delta_ms = int(audio_data.size(-1) / self.sample_rate * 1000)
        self.std = self.std.to(audio_data.device)
        session = None
        if self.fused_chunks and audio_data.dim() == 1 and audio_data.dtype == torch.float32:
            session = self._session(self.CHUNK_MODELS, audio_data.size(-1))
        if session is not None:      # one launch, one host copy; the carried state read and assigned as SequentialLstm.forward does
            streaming = self.model.is_streaming
            probs, state = session.probabilities(audio_data.reshape(1, -1), state=self.model.streaming_state if streaming else None,
                                                 return_state=streaming)
            if streaming:
                self.model.streaming_state = state
            return self._run_frames(probs[0].cpu().numpy(), delta_ms)
        transformed = self.std.log_mel_for_model(audio_data.unsqueeze(0), self.zmuv, channels=getattr(self.model, "FEATURE_CHANNELS", 1))
        predictions = self.model(transformed, lengths=None)
        predictions = F.softmax(predictions, -1).squeeze(1).cpu().numpy()   # one device->host copy for all frames
        return self._run_frames(predictions, delta_ms)

    @torch.no_grad()
    def infer_many(self, clips) -> list:
        """``[reset(); infer(clip) for clip in clips]``.  With ``fused_chunks`` on and every clip inside the streaming kernel's range:
        the ragged clips padded into one (N, L_max) buffer and scored by ONE launch (each from a zero state, at most
        ``MAX_CLIPS_PER_LAUNCH`` per launch) with one host copy, then the decision logic replayed per clip on the host exactly as
        ``infer`` runs it -- or, with ``device_decisions`` on, run by ONE more launch on the probabilities where they are, with the
        same results.  Otherwise the plain loop.  Leaves the engine reset; ``clip_histories`` keeps each clip's
        ``label_history``."""
        clips = list(clips)
        self.clip_histories = []
        session = None
        if self.fused_chunks and clips and all(c.dim() == 1 and c.dtype == torch.float32 for c in clips):
            self.std = self.std.to(clips[0].device)
            session = self._session(self.CHUNK_MODELS, max(c.size(-1) for c in clips))
            if session is not None and not session.supported(min(c.size(-1) for c in clips)):
                session = None
        res = []
        if session is None:
            for clip in clips:
                self.reset()
                res.append(bool(self.infer(clip)))
                self.clip_histories.append(list(self.label_history))
            self.reset()
            return res
        for lo in range(0, len(clips), self.MAX_CLIPS_PER_LAUNCH):
            group = clips[lo:lo + self.MAX_CLIPS_PER_LAUNCH]
            sizes = [c.size(-1) for c in group]
            pcm = torch.nn.utils.rnn.pad_sequence(group, batch_first=True)
            n_samples = torch.tensor(sizes, dtype=torch.int64).to(pcm.device)
            probs, _ = session.probabilities(pcm, n_samples=n_samples, return_state=False)
            frames = [session.rows_of(n) for n in sizes]
            deltas = [int(n / self.sample_rate * 1000) / f for n, f in zip(sizes, frames)]      # as _run_frames divides
            decider = self._device_decider(0, max(frames), min(deltas), len(group))
            if decider is not None:
                present, histories, _ = decider.run(probs, frames, deltas)
                res.extend(present)
                self.clip_histories.extend(histories)
                continue
            probs = probs.cpu().numpy()
            for n, f, row in zip(sizes, frames, probs):
                self.reset()
                res.append(self._run_frames(row[:f], int(n / self.sample_rate * 1000)))
                self.clip_histories.append(list(self.label_history))
        self.reset()
        return res


class FrameInferenceEngine(InferenceEngine):
    def __init__(self, max_window_size_ms: int, eval_stride_size_ms: int, *args):
        super().__init__(*args)
        self.max_window_size_ms, self.eval_stride_size_ms = max_window_size_ms, eval_stride_size_ms
        # ingest_frame as ONE launch (Res8StreamSession, LasStreamSession, GruStreamSession, SmallCnnStreamSession) instead of the
        # frontend + model + softmax chain: off unless asked for
        self.fused_windows = os.environ.get("HOWL_STREAM_FUSED") == "1"
        self._frames_cache = {}

    def _stateless(self) -> bool:
        return not self.model.is_streaming or type(self.model).streaming_state is RegisteredModel.streaming_state

    @torch.no_grad()
    def window_probabilities(self, audio_data: torch.Tensor) -> np.ndarray:
        """softmax(model(zmuv(std(window)))) for every complete strided window, one batched launch -> (W, C)."""
        starts, chunk = audio_utils.stride_starts(audio_data.size(-1), self.max_window_size_ms, self.eval_stride_size_ms,
                                                  self.sample_rate)
        if not starts or chunk < 1000:
            return np.zeros((0, self.context.num_labels), np.float32)
        self.std = self.std.to(audio_data.device)
        stride_sz = starts[1] - starts[0] if len(starts) > 1 else chunk
        flat = audio_data.reshape(-1).contiguous()
        windows = flat.as_strided((len(starts), chunk), (stride_sz, 1))   # overlapping views, no copy
        feats = self.std.log_mel_for_model(windows, self.zmuv, channels=getattr(self.model, "FEATURE_CHANNELS", 1))
        lengths = self.std.compute_lengths(torch.full((len(starts),), chunk, device=audio_data.device))
        return self.model(feats, lengths).softmax(-1).cpu().numpy()

    MAX_WINDOWS_PER_LAUNCH = 8192

    @torch.no_grad()
    def window_probabilities_many(self, clips) -> list:
        """``window_probabilities`` of several clips with ONE frontend launch, one model forward and one device->host copy for all
        of their windows (clips whose windows have the same length share a batch: every clip at least one window long does)."""
        out = [np.zeros((0, self.context.num_labels), np.float32) for _ in clips]
        for members, probs in self._window_probabilities_device(clips):
            probs = probs.cpu().numpy()
            lo = 0
            for i, n, _ in members:
                out[i] = probs[lo:lo + n]
                lo += n
        return out

    def _window_probabilities_device(self, clips) -> list:
        """The probabilities of ``window_probabilities_many`` left on the device: [(members, (windows, C) tensor)] per group of clips
        that share a batch, ``members`` = [(clip index, its windows, its stride in samples)] in the tensor's row order.  Clips
        without a window are in no group."""
        groups = {}
        for i, clip in enumerate(clips):
            starts, chunk = audio_utils.stride_starts(clip.size(-1), self.max_window_size_ms, self.eval_stride_size_ms, self.sample_rate)
            if not starts or chunk < 1000:
                continue
            stride_sz = starts[1] - starts[0] if len(starts) > 1 else chunk
            groups.setdefault((chunk, clip.device), []).append((i, len(starts), stride_sz))
        res = []
        for (chunk, device), members in groups.items():
            self.std = self.std.to(device)
            views = [clips[i].reshape(-1).contiguous().as_strided((n, chunk), (stride_sz, 1)) for i, n, stride_sz in members]
            # at most MAX_WINDOWS_PER_LAUNCH windows per forward: 64 clips of 30 s at a 63-ms stride are ~30 k windows, i.e. 1 GB of
            # window copies and as much again per activation tensor -- the pass stays O(cap), not O(dataset)
            pieces, held, parts = [], 0, []
            def flush():
                nonlocal pieces, held
                if not pieces:
                    return
                windows = pieces[0] if len(pieces) == 1 else torch.cat(pieces)      # (windows of this launch, chunk): the only copy
                feats = self.std.log_mel_for_model(windows, self.zmuv, channels=getattr(self.model, "FEATURE_CHANNELS", 1))
                lengths = self.std.compute_lengths(torch.full((windows.size(0),), chunk, device=device))
                parts.append(self.model(feats, lengths).softmax(-1))
                pieces, held = [], 0
            for v in views:
                lo = 0
                while lo < v.size(0):
                    take = min(v.size(0) - lo, self.MAX_WINDOWS_PER_LAUNCH - held)
                    pieces.append(v[lo:lo + take])
                    held += take
                    lo += take
                    if held == self.MAX_WINDOWS_PER_LAUNCH:
                        flush()
            flush()
            res.append((members, parts[0] if len(parts) == 1 else torch.cat(parts)))
        return res

    def _run_fsm(self, probs) -> bool:
        sequence_present = False
        for prediction in probs:
            self._append_probability_frame(self._weighted(prediction), curr_time=self.curr_time)
            self.curr_time += self.eval_stride_size_ms
            if self.sequence_present(self.curr_time):
                sequence_present = True
                break
        return sequence_present

    @torch.no_grad()
    def infer_many(self, clips) -> list:
        """``[reset(); infer(clip) for clip in clips]`` with the windows of ALL clips scored in one batch (an evaluation pass over a
        dataset, train.py:42-94, is host-bound clip by clip: one launch chain and one host copy per clip); the label
        histories, smoothing and sequence search run per clip exactly as ``infer`` runs them -- on the host, or, with
        ``device_decisions`` on, by ONE launch per batch on the probabilities where they are.  Leaves the engine reset;
        ``clip_histories`` keeps each clip's ``label_history``."""
        clips = list(clips)
        self.clip_histories = []
        if not self._stateless():
            res = []
            for clip in clips:
                self.reset()
                res.append(bool(self._infer_sequential(clip)))
                self.clip_histories.append(list(self.label_history))
            self.reset()
            return res
        if not self.device_decisions:
            res = []
            for probs in self.window_probabilities_many(clips):
                self.reset()
                res.append(self._run_fsm(probs))
                self.clip_histories.append(list(self.label_history))
            self.reset()
            return res
        res, histories = [False] * len(clips), [[] for _ in clips]      # (a clip without a window: no frame, no history)
        for members, probs in self._window_probabilities_device(clips):
            counts = [n for _, n, _ in members]
            decider = self._device_decider(1, max(counts), self.eval_stride_size_ms, len(members))
            rows = probs.split(counts)
            if decider is None:
                host = probs.cpu().numpy()
                lo = 0
                for i, n, _ in members:
                    self.reset()
                    res[i] = self._run_fsm(host[lo:lo + n])
                    histories[i] = list(self.label_history)
                    lo += n
                continue
            for lo in range(0, len(members), DeviceDecider.MAX_CLIPS):
                part = members[lo:lo + DeviceDecider.MAX_CLIPS]
                padded = torch.nn.utils.rnn.pad_sequence(list(rows[lo:lo + len(part)]), batch_first=True)
                present, hists, _ = decider.run(padded, counts[lo:lo + len(part)], [self.eval_stride_size_ms] * len(part))
                for (i, _, _), p, h in zip(part, present, hists):
                    res[i], histories[i] = p, h
        self.clip_histories = histories
        self.reset()
        return res

    @torch.no_grad()
    def infer(self, audio_data: torch.Tensor) -> bool:
        if not self._stateless():
            return self._infer_sequential(audio_data)
        return self._run_fsm(self.window_probabilities(audio_data))

    def _infer_sequential(self, audio_data: torch.Tensor) -> bool:
        sequence_present = False
        for window in audio_utils.stride(audio_data, self.max_window_size_ms, self.eval_stride_size_ms, self.sample_rate):
            if window.size(-1) < 1000:
                break
            self.ingest_frame(window.squeeze(0), self.curr_time)
            self.curr_time += self.eval_stride_size_ms
            if self.sequence_present(self.curr_time):
                sequence_present = True
                break
        return sequence_present

    def _window_frames(self, frame):
        """``compute_lengths`` of this window as a (1,) int64 device tensor, or None below one frame.  It depends on the window's size
        alone: computed on the host and copied once per (size, device), not once per window."""
        key = (frame.size(-1), frame.device)
        if key not in self._frames_cache:
            n = int(self.std.compute_lengths(torch.tensor([frame.size(-1)]))[0])
            self._frames_cache[key] = torch.tensor([n], dtype=torch.int64).to(frame.device) if n >= 1 else None
        return self._frames_cache[key]

    def _fused_session(self, frame):
        """The streaming session for this window, or None when it does not apply (another model, training mode, a window outside
        the kernel's range): ``ingest_frame`` then takes the launch chain."""
        if frame.dim() != 1 or frame.dtype != torch.float32:
            return None
        if isinstance(self.model, SimpleLstm) and self._window_frames(frame) is None:
            return None      # (a window with no whole 512-sample frame has compute_lengths < 1: the chain's business)
        return self._session((Res8, LASClassifier, SimpleGru, SimpleLstm, SmallCnn), frame.size(-1))

    @torch.no_grad()
    def ingest_frame(self, frame: torch.Tensor, curr_time: float = None) -> int:
        """One window, as the live client feeds it (``inference.py:247-267``)."""
        self.std = self.std.to(frame.device)
        session = self._fused_session(frame) if self.fused_windows else None
        if session is None:
            lengths = torch.tensor([frame.size(-1)]).to(frame.device)
            transformed_lengths = self.std.compute_lengths(lengths)
            transformed_frame = self.std.log_mel_for_model(frame.unsqueeze(0), self.zmuv, channels=getattr(self.model, "FEATURE_CHANNELS", 1))
            prediction = self.model(transformed_frame, transformed_lengths).softmax(-1)[0]
        elif isinstance(self.model, SimpleLstm):      # one launch, one host copy; frames as compute_lengths
            prediction = session.probabilities(frame.reshape(1, -1), frames=self._window_frames(frame))[0][0]
        else:      # one launch, one host copy
            prediction = session.probabilities(frame.reshape(1, -1))[0]
        return self._append_probability_frame(self._weighted(prediction.cpu().numpy()), curr_time=curr_time)
