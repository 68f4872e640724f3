"""The phase loops of the 3x3 kernels (staging bursts under the K loop, the one-step-ahead operand pipeline) at the smallest shapes
at which they can go wrong: one fused training step of res8 through FusedRes8Trainer against the oracle, at the tolerances of
test_gpu_res8.py's baseline-size test, twice in one process (bit-identical), and with the data / weight gradient as two launches
(HOWL_RES8_BWD_PAIR=0: the same bits, as test_gpu_res8.py asserts for the merged launch).

  un-sliced instances (HOWL_RES8_SLICES=0, what the large-batch step runs), B = 5: odd, fewer utterances than workgroups, the
      `more == false` tail on a workgroup's first pass;  B = 300: some workgroups loop twice, others once
  81 frames (H = 27): waves with five and with four position tiles, both k_tail paths;  21 frames (H = 7): waves with 2, 1 and 0 tiles
  the default slicing at B = 5 (four workgroups per utterance in the forward pass and the data gradient)

B = 300 is not crossed with 21 frames: the bound on the gradients (5e-5, set for the baseline sizes) does not hold against the
oracle there for a reason outside the kernels.  A ReLU decision at a pre-activation within fp32 rounding (~1e-6) of zero falls
by summation order; 300 x 45 x 70 activations per layer have about one such tie per layer and step, and one flipped position
moves a weight gradient by |ds| |x| ~ 1 / (B P) x O(1) = 5e-5 x O(1) at P = 70 positions (4 x less at 81 frames; at B = 5 a
tie has a chance of 1 %).  Measured at B = 300, 21 frames: conv6.weight 7.5e-5, the same with and without this change (the
outputs are bit-identical); the oracle's own float32-vs-float64 difference there is 6e-9.
"""
import pytest
import torch

from gpu_util import DEV, make_res8, maxerr
from oracle import frontend as ofe
from oracle import models as om

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3      # test_gpu_res8.py
C = 12
_REF = {}


def _inputs(B, L):
    from howl_amd.utils.synth import synthetic_pcm
    return synthetic_pcm(B, L), torch.arange(B) % C


def _oracle(B, L):
    """The oracle's training step for (B, L), computed once and shared by the cases of that shape."""
    if (B, L) not in _REF:
        pcm, labels = _inputs(B, L)
        fb = ofe.mel_fb(40)
        z = ofe.Zmuv()
        z.update(ofe.standard_audio_transform(pcm[:4], fb))
        x = z(ofe.standard_audio_transform(pcm, fb))
        sd = om.res8_init(C)
        names = om.res8_param_names()
        opt = om.AdamWState([sd[n] for n in names], 0.01, 1e-5)
        loss, logits, grads = om.train_step(lambda s, xx: om.res8_forward(s, xx, True), sd, names, opt, x, labels)
        _REF[(B, L)] = (x.shape[-1], loss, logits, grads, sd, names)
    return _REF[(B, L)]


def _step(B, L):
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.training.fused import FusedRes8Trainer
    pcm, labels = _inputs(B, L)
    std = StandardAudioTransform().to(DEV).eval()
    zmuv = ZmuvTransform().to(DEV)
    zmuv.update(std(pcm[:4].to(DEV)))
    model = make_res8(C)
    trainer = FusedRes8Trainer(model, std, zmuv, lr=0.01, weight_decay=1e-5)
    loss = trainer.step(pcm.to(DEV), labels.to(DEV))
    torch.cuda.synchronize()
    return model, trainer, loss


@pytest.mark.parametrize("slices,B,L", [("0", 5, 16000), ("0", 5, 4000), ("0", 300, 16000),
                                        (None, 5, 16000)])      # (21 frames have too few position tiles to slice)
def test_phase_loops_fused_step_vs_oracle(monkeypatch, slices, B, L):
    if slices is None:
        monkeypatch.delenv("HOWL_RES8_SLICES", raising=False)
    else:
        monkeypatch.setenv("HOWL_RES8_SLICES", slices)
    monkeypatch.delenv("HOWL_RES8_BWD_PAIR", raising=False)
    frames, ref_loss, ref_logits, ref_grads, sd, names = _oracle(B, L)
    assert frames == (81 if L == 16000 else 21)
    model, trainer, loss = _step(B, L)
    grads = [g.clone() for g in trainer.fp.grad_views]
    err = {n: maxerr(g, ref_grads[n]) / max(1.0, ref_grads[n].abs().max().item()) for n, g in zip(names, grads)}
    print(f"slices={slices} B={B} frames={frames}: |dlogits|={maxerr(trainer.last_logits, ref_logits):.2e} "
          f"|dloss|={abs(loss.item() - ref_loss.item()):.2e} max |dgrad|/scale={max(err.values()):.2e} ({max(err, key=err.get)})")
    assert maxerr(trainer.last_logits, ref_logits) < LOGIT_TOL
    assert abs(loss.item() - ref_loss.item()) < 1e-4
    for n in names:
        assert err[n] < 5e-5, n
    for n, p in zip(names, model.hot_parameters()):
        # first AdamW step moves every weight by ~lr * sign(g): compare where the gradient is not rounding noise
        solid = ref_grads[n].abs() > 1e-5
        assert maxerr(p.detach().cpu()[solid], sd[n][solid]) < 2e-4, n
    for i in range(1, 7):
        assert maxerr(getattr(model, f"bn{i}").running_var, sd[f"bn{i}.running_var"]) < 1e-4

    # the same step from the same state a second time in this process: the same bits
    model2, trainer2, loss2 = _step(B, L)
    assert torch.equal(trainer2.fp.grad, trainer.fp.grad) and torch.equal(trainer2.fp.flat, trainer.fp.flat)
    assert torch.equal(trainer2.last_logits, trainer.last_logits) and torch.equal(loss2, loss)
    # ... and with the data and the weight gradient of a layer as two launches
    monkeypatch.setenv("HOWL_RES8_BWD_PAIR", "0")
    model3, trainer3, loss3 = _step(B, L)
    assert torch.equal(trainer3.fp.grad, trainer.fp.grad) and torch.equal(trainer3.fp.flat, trainer.fp.flat)
