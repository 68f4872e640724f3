"""Regenerates tests/golden/g18_timestretch.npz from the reference's own ``TimestretchTransform`` / ``TimeshiftTransform`` /
``NoiseTransform`` (howl/data/transform/transform.py:120-196) and ``WakeWordClipExample.update_audio_data``
(howl/data/common/example.py:83-104).

Run by hand where a checkout of the reference is present, under the import shims of ``_reference_shims.py`` (as
``make_golden.py`` is): ``python tests/golden/make_golden_timestretch.py``.  ``librosa.effects.time_stretch`` is replaced by a
recorder that notes (length, rate) and returns ``round(length / rate)`` zeros -- the draws, the lengths and the label scaling are
what is pinned here, not librosa's samples.  Under ``set_random_seed(0)``, N_BATCHES batches of the same five
``WakeWordClipExample``s go through ``TimestretchTransform().train()``, ``TimeshiftTransform().train()`` (whose
``int(0.5 * len)`` bound sees the stretched length) and ``NoiseTransform().train()`` -- the chain of
``training/run/train.py:202-206``.  Recorded per batch: the Timestretch gate (did the recorder run), the rates, the stretched lengths, the scaled ``timestamp_label_map``s (keys and values, padded with NaN / -1), the lengths behind Timeshift;
and, behind the last batch, the next ``random.random()`` and ``np.random.random_sample()`` -- how far the two generators advanced.
Data only; nothing of the reference's text.
"""
import random
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import _reference_shims  # noqa: E402

_reference_shims.install()

from howl.data.common.example import WakeWordClipExample  # noqa: E402
from howl.data.common.label import FrameLabelData  # noqa: E402
from howl.data.transform import transform as rt  # noqa: E402
from howl.utils.random_utils import set_random_seed  # noqa: E402

LENGTHS = (16000, 9000, 2048, 1500, 12345)      # 1500: under one transform frame (the port keeps such a clip at rate 1.0)
LABEL_MAPS = ({310.0: 0, 655.5: 1, 930.0: 2}, {}, {100.0: 1}, {40.0: 0, 80.0: 2}, {512.25: 2, 700.0: 0})
N_BATCHES, MAX_WORDS = 6, 3


def main():
    calls = []

    def recorder(y, rate):
        calls.append((len(y), float(rate)))
        return np.zeros(int(round(len(y) / rate)), np.float32)

    rt.librosa.effects.time_stretch = recorder
    set_random_seed(0)
    stretch, shift, noise = rt.TimestretchTransform().train(), rt.TimeshiftTransform().train(), rt.NoiseTransform().train()
    n = len(LENGTHS)
    gate = np.zeros(N_BATCHES, np.int64)
    rates = np.ones((N_BATCHES, n))
    stretched = np.zeros((N_BATCHES, n), np.int64)
    shifted = np.zeros((N_BATCHES, n), np.int64)
    keys = np.full((N_BATCHES, n, MAX_WORDS), np.nan)
    vals = np.full((N_BATCHES, n, MAX_WORDS), -1, np.int64)
    for b in range(N_BATCHES):
        examples = [WakeWordClipExample(FrameLabelData(dict(m), [], []), None, torch.zeros(L), 16000) for L, m in zip(LENGTHS, LABEL_MAPS)]
        calls.clear()
        out = stretch(examples)
        gate[b] = 1 if calls else 0
        assert len(calls) in (0, n)
        for k, ex in enumerate(out):
            if calls:
                assert calls[k][0] == LENGTHS[k]
                rates[b, k] = calls[k][1]
            stretched[b, k] = ex.audio_data.size(-1)
            for j, (t, v) in enumerate(ex.label_data.timestamp_label_map.items()):
                keys[b, k, j], vals[b, k, j] = t, v
        out = shift(out)
        for k, ex in enumerate(out):
            shifted[b, k] = ex.audio_data.size(-1)
        noise(out)
    np.savez_compressed(HERE / "g18_timestretch.npz", lengths=np.asarray(LENGTHS), gate=gate, rates=rates, stretched=stretched,
                        shifted=shifted, map_keys=keys, map_vals=vals,
                        in_keys=np.asarray([list(m) + [np.nan] * (MAX_WORDS - len(m)) for m in LABEL_MAPS]),
                        in_vals=np.asarray([list(m.values()) + [-1] * (MAX_WORDS - len(m)) for m in LABEL_MAPS]),
                        next_random=np.float64(random.random()), next_np_random=np.float64(np.random.random_sample()))
    print("wrote", HERE / "g18_timestretch.npz", "gates", gate.tolist(), "rates", rates.round(3).tolist())


if __name__ == "__main__":
    main()
