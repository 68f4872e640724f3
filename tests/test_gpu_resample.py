"""-m gpu: the resampler on the device (include/howl_hip_resample.h) -- the checks of tests/test_emu_resample.py with every operand
between sentinel bands (tests/guard_mem.py Banded): the bank against the formula, the ragged batch of 7 per rate pair and sample
format against the float64 restatement within the derived bound, the two tones, the properties without tolerance, both banks'
``from_files``, and `train.main` for res8 on a Howl-format dataset of 44.1 kHz stereo clips."""
import json
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for _p in (str(HERE.parent), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import resample_util as u  # noqa: E402
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


@pytest.mark.parametrize("sr_in", u.RATES)
def test_bank_is_the_formula(sr_in):
    u.check_bank(None, _lib(), sr_in)


@pytest.mark.parametrize("fmt", list(u.FORMATS))
@pytest.mark.parametrize("sr_in", u.RATES)
def test_ragged_batch_against_the_float64_restatement(sr_in, fmt):
    al = _banded()
    u.check_kernel(al, _lib(), sr_in, fmt)
    _no_band_changed(al)


def test_tones_below_and_above_the_new_nyquist():
    al = _banded()
    u.check_tones(al, _lib())
    _no_band_changed(al)


def test_identity_mean_and_placement_give_the_same_bits():
    al = _banded()
    u.check_exact(al, _lib())
    _no_band_changed(al)


def test_from_files_fills_both_banks(tmp_path):
    u.check_banks(tmp_path, DEV, _lib())


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------

def _howl_dataset(root, vocab, n_clips=16, sr=44100):
    """A Howl-format dataset of short 44.1 kHz stereo int16 clips: tone bursts per word, per-character end timestamps in ms."""
    rng = np.random.default_rng(44)
    (root / "audio").mkdir(parents=True)
    records = {"training": [], "dev": [], "test": []}
    for i in range(n_clips):
        ids = [0, 1, 2] if i % 2 == 0 else [int(v) for v in rng.permutation(3)[:2]]
        parts, stamps, pos = [np.zeros(int(0.1 * sr))], [], int(0.1 * sr)
        words = [vocab[w] for w in ids]
        for k, (w, text) in enumerate(zip(ids, words)):
            n = int(0.25 * sr)
            parts += [0.3 * np.sin(2 * np.pi * (300.0 + 450.0 * w) * np.arange(n) / sr) * np.hanning(n), np.zeros(int(0.05 * sr))]
            start_ms, end_ms = pos / sr * 1000, (pos + n) / sr * 1000
            stamps += [start_ms + (end_ms - start_ms) * (c + 1) / len(text) for c in range(len(text))]
            if k + 1 < len(words):
                stamps.append(end_ms)
            pos += n + int(0.05 * sr)
        parts.append(np.zeros(int(0.1 * sr)))
        mono = np.concatenate(parts) + 0.01 * rng.standard_normal(sum(len(p) for p in parts))
        stereo = np.stack([mono, 0.8 * mono + 0.002 * rng.standard_normal(mono.size)], axis=1)
        u.write_wav(root / "audio" / f"c{i:02d}.wav", np.round(32767.0 * np.clip(stereo, -1, 1)).astype(np.int16).reshape(-1), sr, 2)
        records["training" if i < n_clips - 4 else "dev"].append(
            dict(path=f"c{i:02d}.wav", transcription=" ".join(words), end_timestamps=stamps))
    for name, recs in records.items():
        (root / f"aligned-metadata-{name}.jsonl").write_text("".join(json.dumps(r) + "\n" for r in recs))
    return sum(len(r) for r in records.values())


def test_train_entry_point_reads_44k_stereo(tmp_path, monkeypatch):
    """`train.main --model res8 -i <dataset of 44.1 kHz stereo wavs>`, one epoch: the banks come from one resample launch per split
    and the logged loss is finite.  (Without from_files the first file raises "expected 16 kHz mono int16".)"""
    from howl_amd import lib
    for k, v in dict(NUM_EPOCHS="1", BATCH_SIZE="8", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.01", LR_DECAY="0.9", WEIGHT_DECAY="0.00001",
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
        n = _howl_dataset(tmp_path / "ds", ["hey", "fire", "fox"])
        with wave.open(str(tmp_path / "ds" / "audio" / "c00.wav"), "rb") as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (44100, 2, 2)
        ws = tmp_path / "ws"
        train.main(["--model", "res8", "--workspace", str(ws), "-i", str(tmp_path / "ds"), "--eval-freq", "10"])
        lines = [json.loads(l) for l in (ws / "logs" / "scalars.jsonl").read_text().splitlines()]
        losses = [l["value"] for l in lines if l["tag"] == "Training/Loss"]
        assert len(losses) == 1 and np.isfinite(losses).all(), losses
        assert names.count("howl_resample_clips") == 2 and n == 16                 # one launch per split (training, dev)
    finally:
        SETTINGS.reset()
