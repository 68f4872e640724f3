"""-m gpu: time-stretch augmentation on the device (include/howl_hip_timestretch.h) -- the checks of
tests/test_emu_timestretch.py with every operand between sentinel bands (tests/guard_mem.py Banded): the ragged batch of 7 and the
rate-1.0 identity against the float64 restatement with the measured tolerance, the mix operands, a frame_batch and a
sequence_batch with timestretch=True on a bank of 16 synthetic clips, and `train.main --synthetic 64 --timestretch` for res8."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for _p in (str(HERE.parent), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import timestretch_util as u  # noqa: E402
from gpu_util import DEV  # noqa: E402

pytestmark = pytest.mark.gpu


def _banded():
    from guard_mem import Banded
    return Banded("cuda")


def _no_band_changed(al):
    torch.cuda.synchronize()
    bad = al.problems()
    if bad:
        al.describe()
    assert not bad, "; ".join(bad)


def _lib():
    from howl_amd import lib
    return lib.get()


def test_ragged_batch_of_7_against_the_float64_restatement():
    al = _banded()
    u.check_batch7(al, _lib())
    _no_band_changed(al)


def test_rate_one_through_the_transform_reproduces_the_input():
    al = _banded()
    u.check_identity(al, _lib())
    _no_band_changed(al)


def test_mix_operands_and_bank_layouts():
    al = _banded()
    u.check_mix(al, _lib())
    u.check_layouts(al, _lib())
    _no_band_changed(al)


# ---- the collate ------------------------------------------------------------------------------------------------------------------------

N_CLIPS = 16


@pytest.fixture(scope="module")
def bank16():
    """16 synthetic clips of 2048 .. 9000 samples (one under 2048) in a ragged device bank, and their restated stretches on demand."""
    rng = np.random.default_rng(16)
    lengths = [int(v) for v in rng.integers(2048, 9001, N_CLIPS)]
    lengths[5] = 1500
    clips = [(0.2 * np.sin(2 * np.pi * (180.0 + 70.0 * k) * np.arange(L) / 16000.0) + 0.04 * rng.uniform(-1, 1, L)).astype(np.float32)
             for k, L in enumerate(lengths)]
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(lengths)])[:-1]]
    flat = torch.from_numpy(np.concatenate(clips)).to(DEV).reshape(-1, 1)
    cache = {}

    def restated(k, rate):
        if (k, rate) not in cache:
            if rate == 1.0:
                cache[(k, rate)] = (clips[k].astype(np.float64), 0.0)
            else:
                ref = u.stretch_f64(clips[k], rate)
                cache[(k, rate)] = (ref, float(np.max(np.abs(u.stretch_f32_phasor(clips[k], rate) - ref))))
        return cache[(k, rate)]
    return lengths, flat, offs, restated


def _collate(bank16, seed):
    from howl_amd.data.collate import DeviceCollate
    lengths, flat, offs, _ = bank16
    return DeviceCollate(flat, torch.tensor(lengths), None, max_len=max(lengths), row_offsets=offs, seed=seed, timestretch=True)


def _probe_seed(bank16, ids):
    """A seed whose first batch opens the Timestretch gate and keeps both Noise gates shut (the content is then the stretched
    clip's, sample for sample); the draws of that batch."""
    for seed in range(400):
        c = _collate(bank16, seed)
        lens, shift, head, sigma, sp = c.draw(ids)
        if c.last_rates is not None and not any(sigma) and not any(sp):
            return seed, lens, shift, head, list(c.last_rates)
    raise AssertionError("no seed found")


def test_frame_batch_with_timestretch(bank16):
    from howl_amd.data.transform.batchifier import DeviceClip, WakeWordFrameBatchifier
    lengths, _, _, restated = bank16
    ids = list(range(N_CLIPS))
    seed, lens, shift, head, rates = _probe_seed(bank16, ids)
    examples = [DeviceClip(k, L, {0.4 * L / 16: 1 + k % 2, 0.8 * L / 16: 2} if k % 3 else {}, "a b") for k, L in enumerate(lengths)]
    batchifier = WakeWordFrameBatchifier(0, positive_sample_prob=1.0, window_size_ms=200, rand=random.Random(3))
    seen = {}
    real_plan = batchifier.plan

    def plan(cropped):
        seen["clips"], seen["plan"] = list(cropped), real_plan(cropped)
        return seen["plan"]
    batchifier.plan = plan
    batch = _collate(bank16, seed).frame_batch(examples, batchifier)
    pl = seen["plan"]
    assert rates[5] == 1.0 and sum(r != 1.0 for r in rates) == N_CLIPS - 1
    assert lens == [int(round(L / r)) for L, r in zip(lengths, rates)]
    assert [c.num_samples for c in seen["clips"]] == [l - w for l, w in zip(lens, shift)]
    for ex, c, r in zip(examples, seen["clips"], rates):
        assert c.timestamp_label_map == {(1 / r) * k: v for k, v in ex.timestamp_label_map.items()}
    audio = batch.audio_data.cpu().numpy()
    assert audio.shape == (N_CLIPS, 3200) and np.isfinite(audio).all()
    assert batch.lengths.tolist() == pl.length and batch.labels.cpu().tolist() == pl.labels
    for row, (k, start, n, d0) in enumerate(zip(pl.source, pl.start, pl.length, pl.dst_off)):
        ref, gap = restated(k, rates[k])
        first = (shift[k] if head[k] else 0) + start
        want = np.zeros(3200)
        want[d0:d0 + n] = ref[first:first + n]
        assert np.max(np.abs(audio[row] - want)) <= u.TOLERANCE_FACTOR * gap, (row, k, rates[k])
    assert sum(n >= 1000 for n in pl.length) >= N_CLIPS // 2


def test_sequence_batch_with_timestretch(bank16):
    from howl_amd.data.transform.batchifier import DeviceClip
    lengths, _, _, restated = bank16
    ids = list(range(N_CLIPS))
    seed, lens, shift, head, rates = _probe_seed(bank16, ids)

    class Batchifier:      # AudioSequenceBatchifier's interface: order by length, labels from the examples
        def order_and_labels(self, examples, out_len):
            order = [int(k) for k in np.argsort(-np.asarray(out_len))]
            return order, torch.zeros(len(order), 1, dtype=torch.long), torch.ones(len(order), dtype=torch.long)
    batch = _collate(bank16, seed).sequence_batch([DeviceClip(k, L) for k, L in enumerate(lengths)], Batchifier())
    out_len = [l - w for l, w in zip(lens, shift)]
    order = [int(k) for k in np.argsort(-np.asarray(out_len))]
    audio = batch.audio_data.cpu().numpy()
    assert batch.audio_lengths.tolist() == [out_len[k] for k in order] and audio.shape == (N_CLIPS, max(out_len))
    assert np.isfinite(audio).all()
    for row, k in enumerate(order):
        ref, gap = restated(k, rates[k])
        first = shift[k] if head[k] else 0
        assert np.max(np.abs(audio[row, :out_len[k]] - ref[first:first + out_len[k]])) <= u.TOLERANCE_FACTOR * gap, (row, k, rates[k])
        assert not audio[row, out_len[k]:].any()


def test_train_entry_point_with_timestretch(tmp_path, monkeypatch):
    """`train.main --model res8 --synthetic 64 --timestretch`, two epochs: the stretch launch runs on the batches whose gate opens,
    the logged loss is finite and does not rise."""
    from howl_amd import lib
    for k, v in dict(NUM_EPOCHS="2", BATCH_SIZE="48", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.01", LR_DECAY="0.9", WEIGHT_DECAY="0.00001",
                     NUM_MELS="40", DEVICE="cuda:0", OBJECTIVE="frame", TOKEN_TYPE="word", VOCAB='["hey","fire","fox"]',
                     INFERENCE_SEQUENCE="[0,1,2]", SEED="0").items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("HOWL_TIMESTRETCH", raising=False)
    from howl_amd.settings import SETTINGS
    SETTINGS.reset()
    names = []
    real_call = lib.Library.call

    def spy(self, name, *args):
        names.append(name)
        return real_call(self, name, *args)
    monkeypatch.setattr(lib.Library, "call", spy)
    try:
        from howl_amd.training.run import train
        ws = tmp_path / "ws"
        train.main(["--model", "res8", "--workspace", str(ws), "--synthetic", "64", "--eval-freq", "10", "--timestretch"])
        lines = [json.loads(l) for l in (ws / "logs" / "scalars.jsonl").read_text().splitlines()]
        losses = [l["value"] for l in lines if l["tag"] == "Training/Loss"]
        assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] <= losses[0], losses
        n_stretch, n_collate = names.count("howl_timestretch_clips"), names.count("howl_collate_augment_window")
        assert 1 <= n_stretch <= n_collate == 4, (n_stretch, n_collate)
    finally:
        SETTINGS.reset()
