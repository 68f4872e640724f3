"""The small-cnn and seq-cnn models on the device (howl_amd/csrc/cnn.hip through include/howl_hip_cnn.h, ``SmallCnn`` and
``SequentialCnn``): the parity set of tests/test_emu_cnn.py plus the two cases that loop the weight-gradient kernels, with canaries
around every buffer; the reference's golden numbers through the model classes; the fused training steps against the autograd path;
the dropout draw; ``ConvertedStaticModel`` over small-cnn; the refusals; both training entry points."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import cnn_util as u  # noqa: E402
from gpu_util import DEV, maxerr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = {u.SMALL: "small-cnn", u.SEQ: "seq-cnn"}


def _lib():
    from howl_amd import lib
    return lib.get()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make(kind, C, state=None):
    from howl_amd.model import CnnSettings, RegisteredModel
    m = RegisteredModel.find_registered_class(NAMES[kind])(C, CnnSettings(num_labels=C))
    if state is not None:
        m.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    return m.to(DEV)


def load_golden(kind):
    g = np.load(u.GOLDEN[kind])
    return g, {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}


def golden_targets(kind, g):
    if kind == u.SMALL:
        return torch.from_numpy(g["a/labels"])
    return dict(targets=torch.from_numpy(g["a/targets"]), target_lengths=torch.from_numpy(g["a/target_lengths"]),
                input_lengths=torch.from_numpy(g["a/input_lengths"]))


# ---- parity through the C ABI, every buffer between canary bands ----------------------------------------------------------------------

@pytest.mark.parametrize("time_major", (False, True))
@pytest.mark.parametrize("name", tuple(u.CASES))
def test_cnn_vs_fp64_with_canaries(name, time_major):
    from guard_mem import Banded
    r = u.case_reference(name)
    kind = r["kind"]
    al = Banded(DEV, log=open("/dev/null", "w"))
    ev = u.run_library(_lib(), al, kind, r["state"], r["x"], False, x_time_major=time_major, stream=_stream())
    u.check_logits(name, ev["logits"], r["eval64"], "eval")
    for k in u.BUFFERS:
        assert torch.equal(ev["buffers"][k], r["state"][k]), k
    tr = u.run_library(_lib(), al, kind, r["state"], r["x"], True, r["mask"], r["dlogits"], x_time_major=time_major, stream=_stream())
    al.check()                                                         # nothing outside any buffer, every output element written
    u.check_logits(name, tr["logits"], r["train64"], "train")
    u.check_loss(name, kind, tr["logits"], r["targets"], r["train64"])
    u.check_grads(name, tr["grads"], r["train64"], r["train32"])
    u.check_buffers(name, tr["buffers"], r["train64"])
    for k in u.PARAMS:
        assert torch.equal(tr["params"][k], r["state"][k]), k
    # repeated calls, and the other stride order, give the same bits
    again = u.run_library(_lib(), Banded(DEV, log=open("/dev/null", "w")), kind, r["state"], r["x"], True, r["mask"], r["dlogits"],
                          x_time_major=not time_major, stream=_stream())
    assert torch.equal(again["logits"], tr["logits"]) and all(torch.equal(a, b) for a, b in zip(again["grads"], tr["grads"]))


@pytest.mark.parametrize("name", ("s26", "q22"))
def test_eval_logits_do_not_depend_on_the_batch(name):
    from guard_mem import Banded
    r = u.case_reference(name)
    kind = r["kind"]
    run = lambda x: u.run_library(_lib(), Banded(DEV, log=open("/dev/null", "w")), kind, r["state"], x, False, stream=_stream())["logits"]
    pick = (lambda t, i: t[i]) if kind == u.SMALL else (lambda t, i: t[:, i])
    alone = pick(run(r["x"][:1]), 0)
    g = torch.Generator().manual_seed(77)
    for pos in range(3):
        x = torch.randn(7, 3, 40, r["x"].shape[-1], generator=g)
        x[pos] = r["x"][0]
        assert torch.equal(pick(run(x), pos), alone), pos


@pytest.mark.parametrize("kind", (u.SMALL, u.SEQ))
def test_cnn_refusals_on_the_device(kind):
    from guard_mem import Banded
    u.check_refusals(_lib(), Banded(DEV, log=open("/dev/null", "w")), kind, _stream())


# ---- the model classes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", (u.SMALL, u.SEQ))
def test_golden_state_loads_strictly_and_reproduces_the_reference(kind):
    g, state = load_golden(kind)
    m = make(kind, 4, state).eval()
    xa = torch.from_numpy(g["a/x"]).to(DEV)
    with torch.no_grad():
        assert maxerr(m(xa, None), g["a/eval_logits"]) < 5e-5
        assert maxerr(m(torch.from_numpy(g["b/x"]).to(DEV), None), g["b/eval_logits"]) < 5e-5
    with pytest.raises(ValueError, match="valid T is"):
        m(xa[..., :4], None)
    with pytest.raises(NotImplementedError, match="training-mode forward"):
        m(xa, None).sum().backward()
    targets, keep = golden_targets(kind, g), torch.from_numpy(g["a/keep_mask"]).float()
    m.train()
    m.forced_keep_mask = keep
    logits = m(xa, None)
    # the loss on the host in float64, as the reference computes it: d loss / d scores goes back through the model's backward
    z = logits.detach().cpu().double().requires_grad_(True)
    loss = u.loss_of(kind, z, targets)
    loss.backward()
    logits.backward(z.grad.float().to(DEV))
    assert maxerr(logits, g["a/train_logits"]) < 5e-5
    assert abs(loss.item() - float(g["a/loss"])) < 1e-4 * max(1.0, float(g["a/loss"]))
    r64 = u.reference(kind, state, xa.cpu(), targets, keep, train=True)
    r32 = u.reference(kind, state, xa.cpu(), targets, keep, train=True, dtype=torch.float32)
    grads = [p.grad.cpu() for p in m.hot_parameters()]
    u.check_grads(NAMES[kind] + " golden", grads, r64, r32)
    for k, got in zip(u.PARAMS, grads):      # the reference's own gradients (fp32 there, 16 mantissa bits recorded)
        ref = g["a/grad/" + k]
        assert maxerr(got.reshape(ref.shape), ref) < 4e-5 * max(1.0, float(np.abs(ref).max())), k
    u.check_buffers(NAMES[kind] + " golden", {k: v.cpu() for k, v in m.state_dict().items()},
                    {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})


class _LibraryXent(torch.autograd.Function):
    """The trainer's own loss launch (``ops.xent``) as a differentiable function, so that the autograd path hands the model the
    same d loss / d logits bits as ``FusedTrainer.step`` does."""

    @staticmethod
    def forward(ctx, logits, labels):
        from howl_amd import ops
        loss, dlogits = ops.xent(logits, labels)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return ctx.saved_tensors[0] * dloss, None


@pytest.mark.parametrize("kind", (u.SMALL, u.SEQ))
def test_fused_step_matches_autograd_path(kind):
    """FusedTrainer.step (small-cnn) / step_sequence (seq-cnn, CTC on the model's output lengths) with a forced mask against the
    autograd path through the same launches + torch.optim.AdamW, three steps.  On the first step both start from the same bits and
    the gradients are bit-identical; afterwards the parameters differ by the rounding of the two AdamW implementations and by
    what AdamW makes of the gradients' rounding."""
    from howl_amd import ops
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.training.fused import FusedTrainer
    from howl_amd.utils.synth import synthetic_pcm
    B, C = 10, 5
    L = 8000 if kind == u.SMALL else 16000
    pcm = synthetic_pcm(B, L).to(DEV)
    std = StandardAudioTransform().to(DEV).eval()
    zmuv = ZmuvTransform().to(DEV)
    zmuv.update(std(pcm[:4]))
    feats = std.log_mel_for_model(pcm, zmuv)
    T = feats.shape[-1]
    state = u.make_state(kind, C, 21)
    fused_model, ref_model = make(kind, C, state).train(), make(kind, C, state).train()
    H = fused_model.out_rows(T)
    assert H == (2 if kind == u.SMALL else u.compute_length(T)) and H >= 2
    shape = (B, 128) if kind == u.SMALL else (H, B, 128)
    keep = (torch.rand(*shape, generator=torch.Generator().manual_seed(3)) < 0.9).float()
    fused_model.forced_keep_mask = ref_model.forced_keep_mask = keep
    trainer = FusedTrainer(fused_model, std, zmuv, lr=1e-3, weight_decay=1e-5)
    opt = torch.optim.AdamW(ref_model.parameters(), 1e-3, weight_decay=1e-5)
    labels = (torch.arange(B) % C).to(DEV)
    frame_lengths = torch.sort(T - torch.arange(B) * 3, descending=True).values
    targets = torch.tensor([[1 + (b + j) % (C - 1) for j in range(3)] for b in range(B)])
    target_lengths = torch.tensor([1 + b % 3 for b in range(B)])
    losses, live = [], {}
    for step in range(3):
        opt.zero_grad()
        if kind == u.SMALL:
            loss_f = trainer.step(pcm, labels)
            loss_a = _LibraryXent.apply(ref_model(feats, None), labels)
        else:
            loss_f = trainer.step_sequence(pcm, frame_lengths, targets, target_lengths, 0)
            out_lengths = ref_model.output_lengths(frame_lengths)
            assert out_lengths.tolist() == [u.compute_length(int(n)) for n in frame_lengths] and int(out_lengths.min()) >= 3
            loss_a = ops.ctc_loss(ref_model(feats, frame_lengths), targets, out_lengths, target_lengths, 0, long_targets=True)
        loss_a.backward()
        assert np.isfinite(loss_f.item())
        assert abs(loss_f.item() - loss_a.item()) < 1e-6 * max(1.0, abs(loss_a.item())) and (step > 0 or loss_f.item() == loss_a.item())
        for k, p, gf in zip(u.PARAMS, ref_model.hot_parameters(), trainer.fp.grad_views):
            err = maxerr(p.grad, gf)
            print(f"step {step} {k}: fused vs autograd gradient {err:.3e}")
            assert err <= 2e-6 * max(1.0, gf.abs().max().item()), (step, k, err)
            assert step > 0 or torch.equal(p.grad, gf), (k, err)
            live[k] = live.get(k, True) & (gf.abs() > 1e-4)
        opt.step()
        # torch AdamW vs the flat kernel.  After the first step (bit-identical gradients): rounding only.  Later the two paths'
        # gradients differ by dg <= 2e-6 max(1, |g|max) (asserted above), and AdamW divides by the gradient's own magnitude: an
        # element with |g| > 1e-4 on every step so far moves by at most ~2 lr dg / 1e-4 more; an element whose gradient is a rounding
        # residue (a conv bias of a channel no ReLU clips sits in front of a training-mode BatchNorm, which absorbs it) steps by
        # the residue's sign in either implementation and is not compared.
        for k, p, q, gf in zip(u.PARAMS, ref_model.hot_parameters(), fused_model.hot_parameters(), trainer.fp.grad_views):
            if step == 0:
                assert maxerr(p, q) < 1e-6, (step, k)
            elif bool(live[k].any()):
                bound = 1e-6 + 2 * 1e-3 * 2e-6 * max(1.0, gf.abs().max().item()) / 1e-4
                assert maxerr(p[live[k]], q[live[k]]) < bound, (step, k)
        for a, b in zip(ref_model.buffers(), fused_model.buffers()):      # the same bits from the same bits; rounding afterwards
            assert torch.equal(a, b) if step == 0 or not a.is_floating_point() else maxerr(a, b) < 1e-5 * max(1.0, a.abs().max().item())
        losses.append(loss_f.item())
    assert losses[-1] < losses[0]


def test_dropout_draw():
    """Without a forced mask: one howl_dropout_mask launch per training forward; the keep rate of a (512, 128) mask is 0.9 within
    0.015 (more than 10 sigma of a fair draw, sigma = 0.0012); two replicas' salts give different masks."""
    from howl_amd import parallel
    m = make(u.SMALL, 4, u.make_state(u.SMALL, 4, 3)).train()
    x = torch.randn(512, 1, 40, 26, device=DEV)
    torch.manual_seed(1234)
    m._launch_forward(x)
    mask0 = m._cnn_saved[3].clone()
    assert tuple(mask0.shape) == (512, 128) and bool(((mask0 == 0) | (mask0 == 1)).all())
    assert abs(mask0.mean().item() - 0.9) < 0.015
    real = parallel.world_info
    try:
        parallel.world_info = lambda group=None: (1, 2)
        torch.manual_seed(1234)
        m._launch_forward(x)
        mask1 = m._cnn_saved[3].clone()
    finally:
        parallel.world_info = real
    assert abs(mask1.mean().item() - 0.9) < 0.015 and not torch.equal(mask0, mask1)
    torch.manual_seed(1234)
    m._launch_forward(x)
    assert torch.equal(m._cnn_saved[3], mask0)                         # reproducible under torch.manual_seed
    q = make(u.SEQ, 4, u.make_state(u.SEQ, 4, 3)).train()
    q._launch_forward(torch.randn(64, 1, 40, 81, device=DEV))
    assert tuple(q._cnn_saved[3].shape) == (10, 64, 128) and abs(q._cnn_saved[3].mean().item() - 0.9) < 0.015


def test_converted_static_model_slides_small_cnn():
    """``ConvertedStaticModel(small_cnn, 40, 10)`` in eval mode on T = 81: five rows, the first the model on ``x[..., 40:]`` (the
    reference's quirk), the others on the regular windows at 10, 20, 30, 40."""
    from howl_amd.model import ConvertedStaticModel
    g, state = load_golden(u.SMALL)
    m = make(u.SMALL, 4, state).eval()
    conv = ConvertedStaticModel(m, 40, 10).eval()
    x = torch.randn(3, 1, 40, 81, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        out = conv(x, None)
        assert tuple(out.shape) == (5, 3, 4)
        assert torch.equal(out[0], m(x[..., 40:], None))
        for k in range(1, 5):
            assert torch.equal(out[k], m(x[..., 10 * k:10 * k + 40], None)), k
        ref = u.reference(u.SMALL, state, x[..., 10:50].cpu())["logits"]
    assert maxerr(out[1], ref) < 5e-5


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------

def test_pretrain_gsc_entry_point_trains_small_cnn(tmp_path, monkeypatch):
    """`MAX_WINDOW_SIZE_SECONDS=0.5 NUM_LABELS=30 pretrain_gsc --model small-cnn --synthetic`: a handful of fused steps and one
    evaluation; the loss is finite, the workspace reloads and the reloaded model reproduces its logits.  Without NUM_LABELS the
    entry point raises before the first batch."""
    for k, v in dict(NUM_EPOCHS="1", BATCH_SIZE="16", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.002", LR_DECAY="0.8", DEVICE="cuda:0",
                     NUM_MELS="40", NUM_LABELS="30").items():
        monkeypatch.setenv(k, v)
    from howl_amd.settings import SETTINGS
    SETTINGS.reset()
    from howl_amd.workspace import Workspace
    x = torch.randn(3, 1, 40, 41, generator=torch.Generator().manual_seed(9)).to(DEV)
    seen = {}
    real_save = Workspace.save_model

    def save_model(self, model, best=False):      # the trained model's own logits at the moment it is written
        with torch.no_grad():
            seen["logits"] = model(x, None).clone()
        return real_save(self, model, best=best)
    monkeypatch.setattr(Workspace, "save_model", save_model)
    try:
        from howl_amd.training.run import pretrain_gsc
        ws = tmp_path / "ws"
        pretrain_gsc.main(["--model", "small-cnn", "--workspace", str(ws), "--synthetic", "64"])
        lines = [json.loads(l) for l in (ws / "logs" / "scalars.jsonl").read_text().splitlines()]
        losses = [l["value"] for l in lines if l["tag"] == "Training/Loss"]
        accs = [l["value"] for l in lines if l["tag"] == "Dev/Metric/acc"]
        assert len(losses) == 4 and all(np.isfinite(losses)) and len(accs) == 1
        sd = torch.load(ws / "model.pt.bin")
        assert list(sd) == list(u.RefCnn(u.SMALL, 30).state_dict())
        assert int(sd["encoder1.3.num_batches_tracked"]) == 4 and int(sd["encoder2.3.num_batches_tracked"]) == 4
        reloaded = make(u.SMALL, 30, sd).eval()
        with torch.no_grad():
            assert torch.equal(reloaded(x, None), seen["logits"]) and bool(torch.isfinite(seen["logits"]).all())
        monkeypatch.delenv("NUM_LABELS")
        with pytest.raises(ValueError, match="NUM_LABELS"):
            pretrain_gsc.main(["--model", "small-cnn", "--workspace", str(tmp_path / "ws2"), "--synthetic", "64"])
    finally:
        SETTINGS.reset()


def test_train_entry_point_trains_seq_cnn_with_ctc(tmp_path, monkeypatch):
    """`train --model seq-cnn` with the CTC objective on generated wake-word clips (five labels: three words, the negative and the
    blank): runs end to end on the fused step with no vendor loss kernel, the loss is finite, the workspace reloads."""
    env = dict(NUM_EPOCHS="2", BATCH_SIZE="16", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.002", LR_DECAY="0.955", WEIGHT_DECAY="0.00001",
               NUM_MELS="40", DEVICE="cuda:0", OBJECTIVE="ctc", TOKEN_TYPE="word", VOCAB='["hey","fire","fox"]', INFERENCE_SEQUENCE="[0,1,2]",
               INFERENCE_THRESHOLD="0", SMOOTHING_WINDOW_MS="0", NUM_LABELS="5")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from howl_amd.settings import SETTINGS
    SETTINGS.reset()

    def no_vendor_ctc(*a, **k):
        raise AssertionError("torch.nn.functional.ctc_loss on the training path")
    monkeypatch.setattr(torch.nn.functional, "ctc_loss", no_vendor_ctc)
    try:
        from howl_amd.training.run import train
        ws = tmp_path / "ws"
        pos, neg = train.main(["--model", "seq-cnn", "--workspace", str(ws), "--synthetic", "48"])
        assert pos["tp"] + pos["fn"] == 32 and neg["fp"] + neg["tn"] == 32
        lines = [json.loads(l) for l in (ws / "logs" / "scalars.jsonl").read_text().splitlines()]
        losses = [l["value"] for l in lines if l["tag"] == "Training/Loss"]
        assert len(losses) == 2 and all(np.isfinite(losses))
        sd = torch.load(ws / "model.pt.bin")
        assert list(sd) == list(u.RefCnn(u.SEQ, 5).state_dict())
        reloaded = make(u.SEQ, 5, sd).eval()
        with torch.no_grad():
            out = reloaded(torch.randn(2, 1, 40, 81, device=DEV), None)
        assert tuple(out.shape) == (10, 2, 5) and bool(torch.isfinite(out).all())
        monkeypatch.setenv("NUM_LABELS", "2")
        with pytest.raises(ValueError, match="NUM_LABELS"):
            train.main(["--model", "seq-cnn", "--workspace", str(tmp_path / "ws2"), "--synthetic", "48"])
    finally:
        SETTINGS.reset()
