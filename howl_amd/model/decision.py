"""Host-side decision logic of the inference engines, separated from the device work: temporal smoothing of class
probabilities and the wake-sequence matcher.  Behaviour follows ``howl/model/inference.py:91-161`` (label FSM over a
sliding time window, max-over-window smoothing with threshold and optional label colouring); the golden label histories
(tests/golden G8) pin it.  ``DeviceDecider`` runs the same decisions for N clips in one kernel launch (include/howl_hip_decide.h), bit for bit."""
from collections import deque
from typing import List, Optional, Sequence, Tuple

import numpy as np


def _drop_older_than(items: List[Tuple[float, object]], now: float, horizon_ms: float):
    """Removes the leading entries that are more than ``horizon_ms`` older than ``now`` (entries are time-ordered)."""
    keep_from = 0
    for stamp, _ in items:
        if now - stamp > horizon_ms:
            keep_from += 1
        else:
            break
    if keep_from:
        del items[:keep_from]


class ProbabilitySmoother:
    """Keeps (time, probability vector) frames of the last ``window_ms`` and turns them into one label per frame."""

    def __init__(self, window_ms: float, threshold: float, negative_label: int, color_map: Optional[dict] = None):
        self.window_ms, self.threshold = window_ms, threshold
        self.negative_label, self.color_map = negative_label, color_map
        self.frames: List[Tuple[float, np.ndarray]] = []

    def clear(self):
        self.frames = []

    def push(self, now: float, probs: np.ndarray) -> int:
        self.frames.append((now, probs))
        _drop_older_than(self.frames, now, self.window_ms)
        envelope = np.max(np.vstack([p for _, p in self.frames]), axis=0)   # per-class maximum over the window
        label = int(envelope.argmax())
        confident = envelope[label] >= self.threshold
        if self.color_map is not None:      # a colouring is configured (even an empty map recolours every label)
            label = self.color_map.get(label, self.negative_label)
        return label if confident else self.negative_label


class SequenceMatcher:
    """Looks for ``sequence`` (label indices, in order) in a time-stamped label history.  Repeats of the label matched last
    keep a partial match alive; any other label breaks it once ``tolerance_ms`` have passed since the last useful frame."""

    def __init__(self, sequence: Sequence[int], window_ms: float, tolerance_ms: float):
        self.sequence, self.window_ms, self.tolerance_ms = sequence, window_ms, tolerance_ms

    def present(self, history: List[Tuple[float, int]], now: float) -> bool:
        if not self.sequence:
            return False
        _drop_older_than(history, now, self.window_ms)
        matched = 0            # labels of the sequence seen so far
        anchor = 0.0           # time of the last frame that advanced or sustained the match
        holding = None         # label whose repetition sustains the match
        for stamp, label in history:
            if label == self.sequence[matched]:
                matched += 1
                if matched == len(self.sequence):
                    return True
                holding, anchor = label, stamp
            elif label == holding:
                anchor = stamp
            elif anchor + self.tolerance_ms < stamp:
                matched, anchor, holding = 0, 0.0, None
        return False


class DeviceDecider:
    """The same decisions on the device (``include/howl_hip_decide.h``): per-class reweighting, blank skip, smoothing, threshold,
    colouring, label history and sequence matcher of N clips in ONE launch, one wavefront per clip, with the host's arithmetic
    operation for operation -- flags, labels and fp64 stamps are the bits the loops of ``inference.py`` over the two classes above
    produce.  Built from an engine's settings as they are at the call (callers may retune an engine after construction).

    ``mode`` 0: the sequence engine's loop (``InferenceEngine._run_frames``: time advances before the frame, frames whose arg-max
    is ``blank`` are skipped); 1: the frame engine's (``FrameInferenceEngine._run_fsm``)."""

    RING_FRAMES = 32            # HOWL_DECIDE_RING_FRAMES: frames the smoothing window may hold at one time
    MAX_CLIPS = 8192            # HOWL_DECIDE_MAX_CLIPS

    def __init__(self, mode: int, num_labels: int, blank: int, negative: int, threshold: float, smoothing_ms: float, window_ms: float,
                 tolerance_ms: float, sequence: Sequence[int], weights=None, color_map: Optional[dict] = None):
        self.mode, self.num_labels, self.blank, self.negative = int(mode), int(num_labels), blank, negative
        self.threshold, self.smoothing_ms, self.window_ms, self.tolerance_ms = threshold, smoothing_ms, window_ms, tolerance_ms
        self.sequence = list(sequence or [])
        self.weights = None if weights is None or np.isscalar(weights) and weights == 1 else np.asarray(weights, np.float64)
        self.color_map = color_map

    @classmethod
    def from_engine(cls, engine, mode: int) -> "DeviceDecider":
        s = engine._smoother        # (the negative label and the colour map are the smoother's, fixed at construction)
        return cls(mode, engine.context.num_labels, engine.blank_idx, s.negative_label, engine.threshold, engine.smoothing_window_ms,
                   engine.inference_window_ms, engine.tolerance_window_ms, engine.sequence, engine.inference_weights, s.color_map)

    def _plain(self) -> bool:
        """Everything the C struct can carry: integer labels, a weight per class, a colour map with non-negative colours, and a
        threshold that is a Python number (NumPy compares an fp32 probability with those in fp32, as the kernel does; with an
        np.float64 it compares in fp64)."""
        if type(self.threshold) not in (int, float):
            return False
        ints = [self.negative, *self.sequence] + ([self.blank] if self.mode == 0 else [])
        if not all(isinstance(v, (int, np.integer)) and -2 ** 31 <= v < 2 ** 31 for v in ints):
            return False
        if self.weights is not None and (self.weights.ndim != 1 or self.weights.size != self.num_labels):
            return False
        if self.color_map is not None and not all(isinstance(v, (int, np.integer)) and 0 <= v < 2 ** 31 for v in self.color_map.values()):
            return False
        return len(self.sequence) <= 16 and 1 <= self.num_labels <= 64

    def _config(self, device=None):
        """-> (HowlDecideConfig, the device tensors it points to)."""
        import torch
        from howl_amd import lib
        cfg = lib.HowlDecideConfig(mode=self.mode, C=self.num_labels, blank=int(self.blank) if self.mode == 0 else -1, negative=int(self.negative),
                                   threshold=float(self.threshold), smoothing_ms=float(self.smoothing_ms), window_ms=float(self.window_ms),
                                   tolerance_ms=float(self.tolerance_ms), seq_len=len(self.sequence))
        for i, v in enumerate(self.sequence):
            cfg.sequence[i] = int(v)
        keep = []
        if device is not None and self.weights is not None:
            keep.append(torch.from_numpy(self.weights).to(device))
            cfg.weights = keep[-1].data_ptr()
        if device is not None and self.color_map is not None:
            table = np.full(self.num_labels, -1, np.int32)
            for k, v in self.color_map.items():
                if 0 <= k < self.num_labels:
                    table[k] = v
            keep.append(torch.from_numpy(table).to(device))
            cfg.color = keep[-1].data_ptr()
        return cfg, keep

    def supported(self, t_max: int, min_delta_ms: float, n_clips: int = 1) -> bool:
        """Inside the kernel's range: up to 64 classes, a sequence of up to 16 labels, up to 8192 frames per clip, and a smoothing
        window that holds at most ``RING_FRAMES`` frames of the shortest frame period at a time, up to ``MAX_CLIPS`` clips."""
        from howl_amd import ops
        if not self._plain() or not 1 <= n_clips <= self.MAX_CLIPS or not ops.decide_supported(self._config()[0], t_max):
            return False
        held = t_max if not min_delta_ms > 0 else min(t_max, int(self.smoothing_ms // min_delta_ms) + 1)
        return held <= self.RING_FRAMES

    def replay(self, probs: np.ndarray, delta_ms: float):
        """The host loops on one clip's (frames, C) probabilities -> (present, label history, end time).  A restatement: the source
        of truth is ``InferenceEngine._weighted`` / ``_run_frames`` (mode 0) and ``FrameInferenceEngine._run_fsm`` (mode 1) in
        ``inference.py`` -- whoever changes those changes this with them; ``tests/decide_util.py::check_ring_overflow`` holds the
        two together (both modes, weights, colour map)."""
        smoother = ProbabilitySmoother(self.smoothing_ms, self.threshold, self.negative, self.color_map)
        matcher = SequenceMatcher(self.sequence, self.window_ms, self.tolerance_ms)
        history, cur = [], 0
        for p in probs:
            if self.weights is not None:
                p = (p * self.weights).astype(p.dtype, copy=False)
            p = p / p.sum()
            if self.mode == 0:
                cur += delta_ms
                if np.argmax(p) == self.blank:
                    continue
            history.append((cur, smoother.push(cur, p)))
            if self.mode != 0:
                cur += delta_ms
            if matcher.present(history, cur):
                return True, history, cur
        return False, history, cur

    def run(self, probs, n_frames, delta_ms):
        """probs: (N, >= max(n_frames), C) fp32 on the device; ``n_frames`` / ``delta_ms``: N host numbers each.  ONE launch and one
        host copy of the small outputs (the histories up to the longest one) -> (present: list of bool, histories: list of
        [(stamp, label)], end_times: list of float).  A clip whose smoothing ring overflowed is replayed on the host."""
        import torch
        from howl_amd import ops
        N, dev = probs.size(0), probs.device
        t_max = max([int(f) for f in n_frames] + [0])
        if t_max == 0:      # no frame anywhere: nothing to launch
            return [False] * N, [[] for _ in range(N)], [0.0] * N
        cfg, keep = self._config(dev)
        nf = torch.tensor([int(f) for f in n_frames], dtype=torch.int32).to(dev)
        dl = torch.tensor([float(d) for d in delta_ms], dtype=torch.float64).to(dev)
        ints, end_time, hist_time, hist_label = ops.decide_clips(cfg, probs, nf, dl, t_max)
        ints = ints.cpu().numpy()
        present, status, n_labels, first_kept = ints
        longest = int(n_labels.max()) if N else 0
        end_time = end_time.cpu().numpy()
        hist_time, hist_label = hist_time[:, :longest].cpu().numpy(), hist_label[:, :longest].cpu().numpy()
        del keep
        res, histories, ends = [], [], []
        for i in range(N):
            if status[i]:
                p, h, e = self.replay(probs[i, :int(n_frames[i])].cpu().numpy(), float(delta_ms[i]))
            else:
                lo, hi = int(first_kept[i]), int(n_labels[i])
                p, e = bool(present[i]), float(end_time[i])
                h = list(zip(hist_time[i, lo:hi].tolist(), hist_label[i, lo:hi].tolist()))
            res.append(p)
            histories.append(h)
            ends.append(e)
        return res, histories, ends
