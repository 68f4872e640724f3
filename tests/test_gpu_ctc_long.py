"""-m gpu: CTC for targets beyond 31 labels (include/howl_hip_ctc_long.h; ops.ctc_loss(..., long_targets=True)) against the
reference's arithmetic -- torch's CPU log_softmax + ctc_loss + autograd in fp64, at the whole-clip tests' bounds --, the same
bits whichever kernel body runs an utterance, the per-utterance contract between sentinel bands, refusals, and the training
path (FusedTrainer.step_sequence, train.main) on transcripts of more than 31 words."""
import json
import wave

import numpy as np
import pytest
import torch

import ctc_long_util as u
from gpu_util import DEV, maxerr
from oracle import frontend as ofe
from oracle import models as om

pytestmark = pytest.mark.gpu


def ops_runner(device_lengths=False):
    from howl_amd import ops

    def run(logits, targets, in_len, tgt_len, blank, scale=1.0):
        z = logits.to(DEV).requires_grad_(True)
        if device_lengths:
            targets, in_len, tgt_len = targets.to(DEV), in_len.to(DEV), tgt_len.to(DEV)
        out = ops.ctc_loss(z.permute(1, 0, 2), targets, in_len, tgt_len, blank, long_targets=True)
        (out if scale == 1.0 else scale * out).backward()
        return out.item(), z.grad.cpu()
    return run


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(u.CASES))
def test_ctc_long_vs_torch_cpu(name):
    logits, targets, in_len, tgt_len, blank, loss64, grad64, noise = u.case(name)
    loss, grad = ops_runner()(logits, targets, in_len, tgt_len, blank)                   # host length vectors, as train.py has them
    u.check_parity(name, loss, grad, in_len, loss64, grad64, noise)
    loss_d, grad_d = ops_runner(True)(logits, targets, in_len, tgt_len, blank)           # device-resident ones; a repeat
    u.check_parity(name + " (device lengths)", loss_d, grad_d, in_len, loss64, grad64, noise)
    assert loss_d == loss and torch.equal(grad_d, grad)
    _, grad3 = ops_runner()(logits, targets, in_len, tgt_len, blank, scale=3.0)          # upstream gradient scaling
    assert torch.equal(grad3, 3.0 * grad)


# ---- 2. window edges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [32, 64, 255])
def test_ctc_long_window_edges(M):
    from howl_amd import lib
    assert lib.get().cdll.howl_ctc_long_window_rows(M) == u.window_rows(M)
    u.check_window_edges(ops_runner(), M)


# ---- 3. the same bits whichever body runs an utterance ------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,B,C,Lmax,seed", u.short_cases())
def test_ctc_long_bits_do_not_depend_on_the_instantiation(T, B, C, Lmax, seed):
    from guard_mem import Banded
    from howl_amd import lib
    u.check_independence(Banded(str(DEV)), lib.get(), T, B, C, Lmax, seed)


# ---- 4. contract ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["label", "length", "input"])
def test_ctc_long_contract(kind):
    from guard_mem import Banded
    from howl_amd import lib
    u.check_contract(Banded(str(DEV)), lib.get(), kind)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------

def test_ctc_long_refusals():
    from ctc_util import make_case
    from howl_amd import lib, ops
    from howl_amd.lib import HowlHipError
    logits, targets, in_len, tgt_len, blank = make_case(300, 2, 5, 3, 4)
    z = logits.to(DEV).permute(1, 0, 2)
    with pytest.raises(HowlHipError, match="range"):           # a 256-label target
        ops.ctc_loss(z, torch.zeros(2, 256, dtype=torch.int64), in_len, torch.tensor([256, 3]), blank, long_targets=True)
    lg70 = make_case(20, 4, 70, 3, 4)
    with pytest.raises(HowlHipError, match="range"):           # C = 70
        ops.ctc_loss(lg70[0].to(DEV).permute(1, 0, 2), *lg70[1:], long_targets=True)
    with pytest.raises(HowlHipError, match="range"):           # T = 8193
        ops.ctc_loss(torch.zeros(8193, 1, 5, device=DEV), torch.zeros(1, 3, dtype=torch.int64), torch.tensor([8193]), torch.tensor([3]), 4,
                     long_targets=True)
    # a workspace that is too small: the message names the size
    from guard_mem import Banded
    need = int(lib.get().cdll.howl_ctc_long_workspace_floats(300, 2, 100))
    assert need == 2 * 300 * 64 * 4
    with pytest.raises(HowlHipError, match=rf"howl_ctc_loss_long: .* = {need} floats \(got {need - 64}\)"):
        u.call(Banded(str(DEV)), lib.get(), "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank, max_target=100, ws_floats=need - 64)
    # the next valid call succeeds; the default still stops at 31 labels
    loss, grad = ops_runner()(logits, targets, in_len, tgt_len, blank)
    _, loss64, grad64 = u.reference(logits.double(), targets, in_len, tgt_len, blank)
    assert abs(loss - float(loss64)) < 2e-5 * max(1.0, abs(float(loss64))) and np.isfinite(grad.numpy()).all()
    with pytest.raises(HowlHipError, match="range"):
        ops.ctc_loss(z[:40], torch.zeros(2, 40, dtype=torch.int64), torch.tensor([40, 40]), torch.tensor([40, 3]), blank)


# ---- 6. FusedTrainer.step_sequence ------------------------------------------------------------------------------------------------------------

def test_seq_lstm_long_target_ctc_step_vs_oracle(monkeypatch):
    """test_seq_lstm_whole_clip_ctc_step_vs_oracle's comparison (same tolerances) on clips of about 1 s whose targets have up to 48
    labels: the step completes on the library's kernels (torch's ctc_loss raises on the training path) and agrees with the oracle."""
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.training.fused import FusedTrainer
    from howl_amd.utils.synth import synthetic_pcm
    B, L, C = 8, 16000, 5
    pcm = synthetic_pcm(B, L)
    samples = torch.sort(torch.linspace(12000, L, B).long(), descending=True).values
    for b in range(B):
        pcm[b, samples[b]:] = 0.0
    std = StandardAudioTransform().to(DEV).eval()
    zmuv = ZmuvTransform().to(DEV)
    zmuv.update(std(pcm[:4].to(DEV)))
    flen = std.compute_lengths(samples)
    tl = torch.tensor([48, 40, 33, 32, 31, 12, 3, 0])
    assert int(flen.min()) > 48
    targets = torch.stack([(torch.arange(48) + b) % 4 for b in range(B)])        # no label twice in a row: L frames align it
    refs = {}
    fb = ofe.mel_fb(40)
    z = ofe.Zmuv()
    z.update(ofe.standard_audio_transform(pcm[:4], fb))
    x_ref = z(ofe.standard_audio_transform(pcm, fb))
    for dt in (torch.float32, torch.float64):
        sd = {k: v.clone().to(dt).requires_grad_(True) for k, v in om.lstm_init(C).items()}
        ref, _ = om.seq_lstm_forward(sd, x_ref.to(dt), flen)
        ref_loss = torch.nn.CTCLoss(4)(torch.log_softmax(ref, -1), targets, flen, tl)
        ref_loss.backward()
        refs[dt] = (ref.detach(), ref_loss.detach(), {k: v.grad for k, v in sd.items()})

    def no_vendor_ctc(*a, **k):
        raise AssertionError("torch.nn.functional.ctc_loss on the training path")
    monkeypatch.setattr(torch.nn.functional, "ctc_loss", no_vendor_ctc)

    def make():
        m = RegisteredModel.find_registered_class("seq-lstm")(C)
        m.load_state_dict({k: v.clone() for k, v in om.lstm_init(C).items()})
        return m.to(DEV).train()
    tr = FusedTrainer(make(), std, zmuv, lr=1e-3, weight_decay=1e-5)
    loss = tr.step_sequence(pcm.to(DEV), flen, targets, tl, 4)
    grads = [gg.clone() for gg in tr.fp.grad_views]
    ref, ref_loss, g64 = refs[torch.float64]
    assert tr.last_logits.shape == ref.shape and maxerr(tr.last_logits, ref) < 1e-3
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * max(1.0, ref_loss.item())
    for n, gg in zip(om.lstm_param_names(), grads):
        noise = maxerr(refs[torch.float32][2][n], g64[n])
        assert maxerr(gg, g64[n]) < 4.0 * noise + 2e-5 * max(1.0, g64[n].abs().max().item()), (n, maxerr(gg, g64[n]), noise)
    tr2 = FusedTrainer(make(), std, zmuv, lr=1e-3, weight_decay=1e-5)          # bit-repeatable
    loss_b = tr2.step_sequence(pcm.to(DEV), flen, targets, tl, 4)
    assert torch.equal(loss_b, loss) and all(torch.equal(a, b) for a, b in zip(grads, tr2.fp.grad_views))
    # beyond 255 labels the step still raises, naming the batch's longest target and the limit
    from howl_amd.lib import HowlHipError
    with pytest.raises(HowlHipError, match=r"longest target has 300 labels.*255"):
        tr2.step_sequence(pcm.to(DEV), flen, torch.zeros(B, 300, dtype=torch.int64), torch.tensor([300] + [3] * (B - 1)), 4)


# ---- 7. train.main end to end ----------------------------------------------------------------------------------------------------------------

def test_train_entry_point_with_a_42_word_transcript(tmp_path, monkeypatch):
    """test_train_entry_point_on_a_howl_format_dataset[seq-lstm-ctc]'s dataset (its builder, copied) with four training clips whose
    transcription is "hey fire fox" fourteen times -- 42 labels on 4 s of audio: the run finishes with finite epoch losses, no
    vendor loss kernel anywhere, and the library's long-target entry sees the 42 labels."""
    env = dict(NUM_EPOCHS="2", BATCH_SIZE="16", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.002", LR_DECAY="0.955",
               WEIGHT_DECAY="0.00001", NUM_MELS="40", DEVICE="cuda:0", OBJECTIVE="ctc", TOKEN_TYPE="word",
               VOCAB='["hey","fire","fox"]', INFERENCE_SEQUENCE="[0,1,2]", INFERENCE_THRESHOLD="0", SMOOTHING_WINDOW_MS="0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from howl_amd.settings import SETTINGS
    SETTINGS.reset()
    from howl_amd import lib
    from howl_amd.training.run import train

    def no_vendor_ctc(*a, **k):
        raise AssertionError("torch.nn.functional.ctc_loss on the training path")
    monkeypatch.setattr(torch.nn.functional, "ctc_loss", no_vendor_ctc)
    seen = []
    real_call = lib.Library.call

    def spy(self, name, *args):
        if name.startswith("howl_ctc_loss"):
            seen.append((name, args[8]))
        return real_call(self, name, *args)
    monkeypatch.setattr(lib.Library, "call", spy)
    ds = tmp_path / "ds"
    (ds / "audio").mkdir(parents=True)
    rng = np.random.default_rng(0)
    vocab = ["hey", "fire", "fox"]

    def long_clip():
        """42 words in 4 s: one short tone burst per word, the characters' end stamps spread evenly over it."""
        ids = [0, 1, 2] * 14
        n = 4 * 16000 // len(ids)
        tt = np.arange(n) / 16000
        parts, stamps = [], []
        for k, w in enumerate(ids):
            parts.append((0.3 * np.sin(2 * np.pi * (300.0 + 450.0 * w) * tt) * np.hanning(n)).astype(np.float32))
            start_ms, end_ms = k * n / 16.0, (k + 1) * n / 16.0
            text = vocab[w]
            stamps += [start_ms + (end_ms - start_ms) * (c + 1) / (len(text) + 1) for c in range(len(text))]
            if k + 1 < len(ids):
                stamps.append(end_ms)
        pcm = np.concatenate(parts)
        pcm = pcm + 0.01 * rng.standard_normal(pcm.size).astype(np.float32)
        return torch.from_numpy(pcm), " ".join(vocab[w] for w in ids), stamps

    for split, n in (("training", 48), ("dev", 12), ("test", 4)):
        with (ds / f"aligned-metadata-{split}.jsonl").open("w") as f:
            for i in range(n):
                if split == "training" and i % 12 == 5:
                    pcm, transcription, stamps = long_clip()
                else:
                    ids = [0, 1, 2] if i % 2 == 0 else [int(v) for v in rng.permutation(3)[: 1 + i % 3]]
                    if ids == [0, 1, 2] and i % 2:
                        ids = [2, 1, 0]
                    pcm, meta = train.make_clip(ids, vocab, rng)
                    tail = int(rng.integers(int(2.0 * 16000), int(4.0 * 16000))) - pcm.numel()
                    pcm = torch.cat([pcm, 0.01 * torch.from_numpy(rng.standard_normal(max(tail, 0)).astype(np.float32))])
                    transcription, stamps = meta.transcription, meta.end_timestamps
                name = f"{split}_{i}.wav"
                with wave.open(str(ds / "audio" / name), "wb") as w:
                    w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                    w.writeframes((pcm.numpy().clip(-1, 1) * 32767).astype("<i2").tobytes())
                f.write(json.dumps(dict(path=name, transcription=transcription, end_timestamps=stamps,
                                        phone_strings=None, words=None, phone_end_timestamps=None)) + "\n")
    ws = tmp_path / "ws"
    try:
        train.main(["--model", "seq-lstm", "--workspace", str(ws), "-i", str(ds), "--eval-freq", "1"])
    finally:
        SETTINGS.reset()
    lines = [json.loads(l) for l in (ws / "logs" / "scalars.jsonl").read_text().splitlines()]
    losses = [l["value"] for l in lines if l["tag"] == "Training/Loss"]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses), losses
    assert any(name == "howl_ctc_loss_long" and m >= 42 for name, m in seen), seen
    assert all(name == "howl_ctc_loss_long" for name, _ in seen)
