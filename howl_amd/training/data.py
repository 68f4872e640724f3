"""Minimal data plumbing for the entry points: a Google-Speech-Commands reader that needs no librosa (GSC clips are
16 kHz mono int16 wav) with the split / label rules of ``howl/data/dataset/gsc_dataset_loader.py:19-47``, a synthetic
stand-in for boxes without a dataset, and a device-resident clip bank with ``batchify`` semantics
(``howl/data/transform/operator.py:77-86``: sort by length descending, zero-pad right)."""
import json
import wave
from pathlib import Path
from types import SimpleNamespace
from typing import List, Tuple

import numpy as np
import torch

from howl_amd.data.common.batch import ClassificationBatch
from howl_amd.utils.synth import synthetic_pcm


def read_wav16k(path) -> torch.Tensor:
    with wave.open(str(path), "rb") as w:
        if w.getframerate() != 16000 or w.getnchannels() != 1 or w.getsampwidth() != 2:
            raise ValueError(f"{path}: expected 16 kHz mono int16 (resampling is outside the MI355X hot path)")
        return torch.from_numpy(np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32) / 32768.0)


def read_wav(path):
    """Any PCM wav ``wave`` opens -> (raw interleaved samples as a flat array, sample rate, channels).  16-bit PCM stays int16 (the
    device converts it); 8-bit (unsigned), 24- and 32-bit PCM become float32 in [-1, 1) here.  No resampling, no channel mix:
    ``ops.resample_clips`` does both on the way into a bank."""
    try:
        with wave.open(str(path), "rb") as w:
            rate, channels, width, frames = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
            raw = w.readframes(frames)
    except (wave.Error, EOFError, OSError) as e:
        raise ValueError(f"{path}: not a PCM wav file this reader opens ({e or type(e).__name__})") from e
    raw = raw[:len(raw) - len(raw) % (width * channels)]
    if width == 2:
        samples = np.frombuffer(raw, dtype="<i2")
    elif width == 1:
        samples = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        samples = (((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8) >> 8).astype(np.float32) / 8388608.0
    elif width == 4:
        samples = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples unsupported (8, 16, 24 or 32-bit PCM)")
    return samples, rate, channels


def wav_header(path):
    """(sample rate, channels, sample width in bytes, frames) from the file's header alone."""
    try:
        with wave.open(str(path), "rb") as w:
            return w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
    except (wave.Error, EOFError, OSError) as e:
        raise ValueError(f"{path}: not a PCM wav file this reader opens ({e or type(e).__name__})") from e


UPLOAD_CHUNK_BYTES = 64 << 20     # raw sample bytes per upload and launch of ``resample_files`` (one larger file is a chunk of its own)


def resample_files(paths, headers, out_lens, dst_offs, out: torch.Tensor, sample_rate: int):
    """Fills a zero-initialised flat device bank from wav files of any rate, channel count and PCM width: the files are grouped by
    (rate, channels, sample format), each group's raw samples are uploaded in chunks of at most ``UPLOAD_CHUNK_BYTES`` (and at
    most 8192 clips), and ONE ``howl_resample_clips`` launch per chunk writes clip i to ``out[dst_offs[i] .. + out_lens[i])``.
    ``headers``: ``wav_header`` per file -- lengths and offsets are the caller's host arithmetic on them; nothing is read back."""
    from howl_amd import lib as _lib, ops
    groups = {}
    for i, (rate, channels, width, frames) in enumerate(headers):
        if frames > 0 and out_lens[i] > 0:
            groups.setdefault((rate, channels, width == 2), []).append(i)
    for (rate, channels, is_i16), members in groups.items():
        plan, bank = ops.resample_plan(rate, sample_rate)
        bank_dev = torch.from_numpy(bank).reshape(-1).to(out.device)
        elem = 2 if is_i16 else 4
        start = 0
        while start < len(members):
            stop, nbytes = start, 0
            while stop < len(members) and stop - start < _lib.RESAMPLE_MAX_CLIPS:
                more = headers[members[stop]][3] * channels * elem
                if stop > start and nbytes + more > UPLOAD_CHUNK_BYTES:
                    break
                nbytes, stop = nbytes + more, stop + 1
            chunk, parts, src_offs, at = members[start:stop], [], [], 0
            for i in chunk:
                samples, r, c = read_wav(paths[i])
                if (r, c, samples.size) != (rate, channels, headers[i][3] * channels):
                    raise ValueError(f"{paths[i]}: {samples.size // max(c, 1)} frames read, the header promised {headers[i][3]}")
                parts.append(samples)
                src_offs.append(at)
                at += headers[i][3]
            src = torch.from_numpy(np.concatenate(parts)).to(out.device)
            rec = ops.resample_records(src_offs, [headers[i][3] for i in chunk], [dst_offs[i] for i in chunk], [out_lens[i] for i in chunk])
            rec_dev = torch.from_numpy(rec.view(np.int64).copy()).to(out.device)
            ops.resample_clips(src, channels, plan, bank_dev, rec, rec_dev, out)
            start = stop


def resampled_lengths(headers, sample_rate: int):
    """ceil(frames * up / down) per file: librosa's length for ``load(path, sr=sample_rate)``."""
    from howl_amd import ops
    return [ops.resample_out_len(ops.resample_plan(h[0], sample_rate)[0], h[3]) for h in headers]


def load_gsc_splits(path: Path, vocab: List[str]):
    """-> (train, dev, test), each a list of (path, label); labels: index in vocab, else len(vocab)."""
    path = Path(path)
    split = {}
    for name, tag in (("testing_list.txt", "test"), ("validation_list.txt", "dev")):
        with (path / name).open() as f:
            split.update({k: tag for k in f.read().split("\n")})
    files = [p for p in sorted(path.glob("*/*.wav")) if "noise" not in str(p)]
    label_of = {k: i for i, k in enumerate(vocab)}
    out = {"train": [], "dev": [], "test": []}
    for p in files:
        key = str(Path(p.parent.name) / p.name)
        out[split.get(key, "train")].append((p, label_of.get(p.parent.name, len(vocab))))
    return out["train"], out["dev"], out["test"]


class ClipBank:
    """All clips of a split decoded once, truncated to ``max_len`` and kept on the device as one (N, max_len) matrix."""

    def __init__(self, clips: List[torch.Tensor], labels: List[int], max_len: int, device):
        n = len(clips)
        self.max_len = max_len
        audio = torch.zeros(n, max_len)
        lengths = torch.zeros(n, dtype=torch.long)
        for i, c in enumerate(clips):
            c = c[:max_len]                      # truncate_length (operator.py:73-74)
            audio[i, : c.numel()] = c
            lengths[i] = c.numel()
        self.audio = audio.to(device)
        self.lengths_host = lengths                      # batch maxima / sort orders are host decisions: no read-back per batch
        self.lengths = lengths.to(device)
        self.labels = torch.tensor(labels, dtype=torch.long).to(device)

    @classmethod
    def from_files(cls, paths, labels: List[int], max_len: int, device, sample_rate: int = 16000):
        """The bank of ``ClipBank([read_wav16k(p) ...], labels, max_len, device)`` for wav files of ANY rate, channel count and
        PCM width, resampled to ``sample_rate`` mono on the device straight into the rows (``resample_files``); for 16 kHz mono
        int16 files the two banks are equal bit for bit."""
        headers = [wav_header(p) for p in paths]
        lengths = [min(n, max_len) for n in resampled_lengths(headers, sample_rate)]         # truncate_length (operator.py:73-74)
        self = cls.__new__(cls)
        self.max_len = max_len
        self.audio = torch.zeros(len(paths), max_len, device=device)
        resample_files(paths, headers, lengths, [i * max_len for i in range(len(paths))], self.audio.view(-1), sample_rate)
        self.lengths_host = torch.tensor(lengths, dtype=torch.long)
        self.lengths = self.lengths_host.to(device)
        self.labels = torch.tensor(labels, dtype=torch.long).to(device)
        return self

    def __len__(self):
        return self.audio.size(0)

    def batch(self, idx: torch.Tensor) -> ClassificationBatch:
        """batchify: longest first, zero padded to the batch maximum."""
        idx_host = idx.cpu()
        lengths = self.lengths_host[idx_host]
        order = torch.argsort(lengths, descending=True, stable=True)
        idx_host, lengths = idx_host[order], lengths[order]
        lmax = int(lengths[0])     # the batch maximum, as batchify pads (res8's time-mean sees no extra pad frames)
        dev = self.audio.device
        idx = idx_host.to(dev)
        return ClassificationBatch(self.audio[idx, :lmax], self.labels[idx], lengths.to(dev))

    def index_batches(self, batch_size: int, shuffle: bool, drop_last: bool, generator=None):
        """Lists of clip ids per batch (for DeviceCollate, which gathers / augments / pads on the device)."""
        n = len(self)
        perm = (torch.randperm(n, generator=generator) if shuffle else torch.arange(n)).numpy()   # id arrays, not lists:
        end = n - (n % batch_size) if drop_last else n                                            # the collate indexes with them
        for i in range(0, end, batch_size):
            yield perm[i:i + batch_size]

    def batches(self, batch_size: int, shuffle: bool, drop_last: bool, generator=None):
        n = len(self)
        perm = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)      # host: batch() sorts on the host
        end = n - (n % batch_size) if drop_last else n
        for i in range(0, end, batch_size):
            yield self.batch(perm[i:i + batch_size])


def synthetic_bank(n: int, max_len: int, num_labels: int, device, seed=0) -> ClipBank:
    pcm = synthetic_pcm(n, max_len, seed=seed)
    labels = [(i % 64) % num_labels for i in range(n)]     # the tone frequency of clip i encodes its label
    return ClipBank([pcm[i] for i in range(n)], labels, max_len, device)


# ---- wake-word datasets (training.run.train) --------------------------------------------------------------------------
def load_howl_splits(path: Path, prefix: str = "aligned-"):
    """A Howl-format dataset directory (``howl/data/dataset/dataset_loader.py:34-70``, ``WakeWordDatasetLoader``):
    ``<prefix>metadata-{training,dev,test}.jsonl`` with one JSON object per line (``path``, ``transcription``,
    ``end_timestamps`` per character in ms) and the clips under ``audio/``.  -> three lists of metadata records."""
    path = Path(path)

    def load(name):
        out = []
        with (path / f"{prefix}metadata-{name}.jsonl").open() as f:
            for line in f:
                if line.strip():
                    d = json.loads(line)
                    out.append(SimpleNamespace(path=(path / "audio" / d["path"]).absolute(), transcription=d["transcription"],
                                               end_timestamps=d.get("end_timestamps")))
        return out

    return load("training"), load("dev"), load("test")


class WakeWordClipBank:
    """Clips of a wake-word split decoded once and kept on the device RAGGED: one flat sample buffer, clip i at
    ``offsets[i] .. offsets[i] + lengths[i]`` (each start 16-byte aligned), so a single long negative costs its own length
    and not a row of that width for every clip.  The collate / gather kernels address a clip as ``bank + idx * bank_ld``: the
    bank is handed to them as the (total, 1) view ``rows`` (``bank_ld`` = 1) with ``idx`` = the clip's offset
    (``DeviceCollate(row_offsets=...)``).  Each clip comes with the descriptor the batchifiers work on (``DeviceClip``: clip
    id, length, frame labels from the context's labeler, transcription)."""

    MAX_OFFSET = (1 << 31) - 1     # offsets travel as int32 (8 GiB of samples, ~37 h of 16 kHz audio per split)

    def __init__(self, clips: List[torch.Tensor], metadata: list, labeler, device):
        lengths = [int(c.numel()) for c in clips]
        offsets, total = self._layout(lengths)
        flat = torch.zeros(max(total, 1))
        for c, o, n in zip(clips, offsets, lengths):
            flat[o:o + n] = c
        self._finish(flat.to(device), offsets, lengths, metadata, labeler)

    @classmethod
    def from_files(cls, paths, metadata: list, labeler, device, sample_rate: int = 16000):
        """The bank of ``WakeWordClipBank([read_wav16k(p) ...], metadata, labeler, device)`` for wav files of ANY rate, channel
        count and PCM width, resampled to ``sample_rate`` mono on the device straight into the flat buffer (``resample_files``);
        for 16 kHz mono int16 files the two banks are equal bit for bit.  ``end_timestamps`` are milliseconds: the labels do not
        depend on a file's rate."""
        headers = [wav_header(p) for p in paths]
        lengths = resampled_lengths(headers, sample_rate)
        offsets, total = cls._layout(lengths)
        flat = torch.zeros(max(total, 1), device=device)
        resample_files(paths, headers, lengths, offsets, flat, sample_rate)
        self = cls.__new__(cls)
        self._finish(flat, offsets, lengths, metadata, labeler)
        return self

    @classmethod
    def _layout(cls, lengths):
        """Clip starts in the flat buffer (each 16-byte aligned) and its size."""
        offsets, total = [], 0
        for n in lengths:
            offsets.append(total)
            total += (n + 3) & ~3
        if total > cls.MAX_OFFSET:
            raise MemoryError(f"clip bank of {total} samples ({total * 4 / 2**30:.0f} GiB) exceeds the 32-bit offsets of the collate "
                              f"kernels: shard the split")
        return offsets, total

    def _finish(self, flat, offsets, lengths, metadata, labeler):
        from howl_amd.data.transform.batchifier import DeviceClip
        self.flat = flat
        self.rows = self.flat.unsqueeze(1)          # (total, 1): row stride 1, "row" index = sample offset
        self.offsets = offsets
        self.max_len = max(lengths) if lengths else 0
        self.lengths = torch.tensor(lengths)
        self.examples = []
        for i, (n, m) in enumerate(zip(lengths, metadata)):
            tl = labeler.compute_frame_labels(m).timestamp_label_map if m.end_timestamps is not None else {}
            self.examples.append(DeviceClip(i, n, tl, m.transcription))

    def __len__(self):
        return len(self.examples)

    def clip(self, i: int) -> torch.Tensor:
        return self.flat[self.offsets[i]: self.offsets[i] + self.examples[i].num_samples]

    def subset(self, keep) -> List[int]:
        return [i for i, ex in enumerate(self.examples) if keep(ex)]
