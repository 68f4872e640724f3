"""The las model on the device (howl_amd/csrc/las.hip through include/howl_hip_las.h and ``LASClassifier``): the parity set of
tests/test_emu_las.py plus the 1 s window, the reference's golden numbers through the model class, the three-channel frontend
path, the fused training step against the autograd path, canaries around every buffer, the refusals, the training entry point,
the dropout draw and a frame-engine pass."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import las_util as u  # noqa: E402
from gpu_util import DEV, maxerr  # noqa: E402
from test_emu_las import check_golden_grads, golden_case_a  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from howl_amd import lib
    return lib.get()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make(C, state=None):
    from howl_amd.model import RegisteredModel
    m = RegisteredModel.find_registered_class("las")(C)
    if state is not None:
        m.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def g17():
    return u.load_golden()


# ---- parity through the C ABI, every buffer between canary bands ----------------------------------------------------------------------

@pytest.mark.parametrize("time_major", (False, True))
@pytest.mark.parametrize("name", tuple(u.CASES))
def test_las_vs_fp64_with_canaries(name, time_major):
    from guard_mem import Banded
    r = u.case_reference(name)
    al = Banded(DEV, log=open("/dev/null", "w"))
    ev = u.run_library(_lib(), al, r["state"], r["x"], r["lengths"], False, x_time_major=time_major, stream=_stream())
    u.check_logits(name, ev["logits"], r["eval64"], "eval")
    for k in u.BUFFERS:
        assert torch.equal(ev["buffers"][k], r["state"][k]), k
    tr = u.run_library(_lib(), al, r["state"], r["x"], r["lengths"], True, r["mask"], r["dlogits"], x_time_major=time_major, stream=_stream())
    al.check()                                                         # nothing outside any buffer, every output element written
    u.check_logits(name, tr["logits"], r["train64"], "train")
    u.check_loss(name, tr["logits"], r["labels"], r["train64"])
    u.check_grads(name, tr["grads"], r["train64"], r["train32"])       # (the three zero gradients are == 0 exactly)
    u.check_buffers(name, tr["buffers"], r["train64"])
    for k in u.PARAMS:
        assert torch.equal(tr["params"][k], r["state"][k]), k
    again = u.run_library(_lib(), Banded(DEV, log=open("/dev/null", "w")), r["state"], r["x"], r["lengths"], True, r["mask"], r["dlogits"],
                          x_time_major=time_major, stream=_stream())
    assert torch.equal(again["logits"], tr["logits"]) and all(torch.equal(a, b) for a, b in zip(again["grads"], tr["grads"]))


def test_eval_logits_do_not_depend_on_the_batch():
    from guard_mem import Banded
    r = u.case_reference("A")
    run = lambda x, lengths: u.run_library(_lib(), Banded(DEV, log=open("/dev/null", "w")), r["state"], x, lengths, False, stream=_stream())["logits"]
    whole = run(r["x"], r["lengths"])
    assert torch.equal(run(r["x"][2:3], [9])[0], whole[2])
    g = torch.Generator().manual_seed(77)
    for pos in range(4):
        x = torch.randn(6, 3, 40, 21, generator=g)
        x[pos] = r["x"][2]
        lengths = [21] * 6                                             # longer neighbours: three steps more than the utterance runs
        lengths[pos] = 9
        assert torch.equal(run(x, lengths)[pos], whole[2]), pos


def test_las_refusals_on_the_device():
    from guard_mem import Banded
    u.check_refusals(_lib(), Banded(DEV, log=open("/dev/null", "w")), _stream())


# ---- the model class ---------------------------------------------------------------------------------------------------------------------

def test_golden_state_loads_strictly_and_reproduces_the_reference(g17):
    g, state = g17
    assert len(state) == 35
    m = make(4, state).eval()
    xa, la_list, labels, keep = golden_case_a(g)
    xa, la = xa.to(DEV), torch.tensor(la_list)
    with torch.no_grad():
        assert maxerr(m(xa, la), g["a/eval_logits"]) < 5e-5
        assert maxerr(m(torch.from_numpy(g["b/x"]).to(DEV), None), g["b/eval_logits"]) < 5e-5
    assert la.tolist() == la_list                                      # the caller's lengths are not written
    m.train()
    m.forced_keep_mask = keep
    logits = m(xa, la)
    loss = torch.nn.functional.cross_entropy(logits, labels.to(DEV))
    loss.backward()
    assert maxerr(logits, g["a/train_logits"]) < 5e-5
    assert abs(loss.item() - float(g["a/loss"])) < 1e-4 * max(1.0, float(g["a/loss"]))
    r64 = u.reference(state, xa.cpu(), la_list, labels, keep, train=True)
    r32 = u.reference(state, xa.cpu(), la_list, labels, keep, train=True, dtype=torch.float32)
    grads = [p.grad.cpu() for p in m.hot_parameters()]
    u.check_grads("LASClassifier G17", grads, r64, r32)
    check_golden_grads(dict(zip(u.PARAMS, grads)), g)
    u.check_buffers("LASClassifier G17", {k: v.cpu() for k, v in m.state_dict().items()},
                    {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})
    sd = m.state_dict()                                                # a saved state has the reference's keys again
    assert list(sd) == list(u.RefLas(4).state_dict())


def test_model_refusals(g17):
    from howl_amd.model import LASClassifier, LASClassifierConfig, LASEncoderConfig
    g, state = g17
    with pytest.raises(NotImplementedError, match="hidden_size"):
        LASClassifier(4, LASClassifierConfig(las_config=LASEncoderConfig(hidden_size=128)))
    m = make(4, state).eval()
    xa = torch.from_numpy(g["a/x"]).to(DEV)
    with pytest.raises(RuntimeError, match="sorted in decreasing order"):
        m(xa, torch.tensor([3, 21, 17, 9, 1]))
    with pytest.raises(RuntimeError, match="1..T"):
        m(xa, torch.tensor([22, 17, 9, 3, 1]))
    with pytest.raises(RuntimeError, match="three feature channels"):
        m(xa[:, :1], None)
    with pytest.raises(NotImplementedError, match="training-mode forward"):
        m(xa, torch.tensor([21, 17, 9, 3, 1])).sum().backward()


# ---- the three-channel frontend path -------------------------------------------------------------------------------------------------------

def _frontend(B=6, L=8000):
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.utils.synth import synthetic_pcm
    pcm = synthetic_pcm(B, L).to(DEV)
    std = StandardAudioTransform().to(DEV).eval()
    zmuv = ZmuvTransform().to(DEV)
    zmuv.update(std(pcm[:4]))
    return pcm, std, zmuv


def test_three_channel_features_are_zmuv_of_std():
    """``log_mel_for_model(channels=3)`` is ``zmuv(std(audio))`` bit for bit (contiguous (B, 3, M, T)), ``channels=1`` is today's
    view bit for bit, and any other channel count is refused."""
    pcm, std, zmuv = _frontend()
    three = std.log_mel_for_model(pcm, zmuv, channels=3)
    assert three.is_contiguous() and tuple(three.shape[:3]) == (pcm.size(0), 3, std.n_mels)
    assert torch.equal(three, zmuv(std(pcm)))
    one = std.log_mel_for_model(pcm, zmuv, channels=1)
    default = std.log_mel_for_model(pcm, zmuv)
    assert torch.equal(one, default) and one.stride() == default.stride() and tuple(one.shape) == (pcm.size(0), 1, std.n_mels, three.size(3))
    assert maxerr(one[:, 0], three[:, 0]) < 1e-5                       # the same log-mels through the two launches
    with pytest.raises(ValueError, match="channels"):
        std.log_mel_for_model(pcm, zmuv, channels=2)


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


def test_fused_step_matches_autograd_path():
    """FusedTrainer.step (three-channel features, explicit launches, gradients straight into the flat buffer, flat AdamW) with a
    forced mask against the autograd path through the same launches + torch.optim.AdamW, three steps.  On the first step both start
    from the same bits and the gradients are bit-identical; afterwards the parameters differ by the rounding of the two AdamW
    implementations (and with them the later steps' gradients and running statistics)."""
    from howl_amd.training.fused import FusedTrainer
    B, C = 10, 5
    pcm, std, zmuv = _frontend(B)
    lengths = torch.sort(24 + torch.arange(B) % 15, descending=True).values
    labels = (torch.arange(B) % C).to(DEV)
    state = u.make_state(C, 31)
    keep = (torch.rand(B, 256, generator=torch.Generator().manual_seed(3)) < 0.9).float()
    fused_model, ref_model = make(C, state).train(), make(C, state).train()
    fused_model.forced_keep_mask = ref_model.forced_keep_mask = keep
    trainer = FusedTrainer(fused_model, std, zmuv, lr=1e-3, weight_decay=1e-5)
    feats = trainer.features(pcm)
    assert tuple(feats.shape[:3]) == (B, 3, 40) and torch.equal(feats, zmuv(std(pcm)))
    opt = torch.optim.AdamW(ref_model.hot_parameters(), 1e-3, weight_decay=1e-5)
    losses = []
    for step in range(3):
        loss_f = trainer.step(pcm, labels, lengths)
        opt.zero_grad()
        loss_a = _LibraryXent.apply(ref_model(feats, lengths), labels)
        loss_a.backward()
        assert abs(loss_f.item() - loss_a.item()) < 1e-6 and (step > 0 or loss_f.item() == loss_a.item())
        for k, p, gf in zip(u.PARAMS, ref_model.hot_parameters(), trainer.fp.grad_views):
            err = maxerr(p.grad, gf)
            print(f"step {step} {k}: fused vs autograd gradient {err:.3e}")
            assert err <= 2e-6 * max(1.0, gf.abs().max().item()), (step, k, err)
            assert step > 0 or torch.equal(p.grad, gf), (k, err)
        opt.step()
        for k, p, q in zip(u.PARAMS, ref_model.hot_parameters(), fused_model.hot_parameters()):
            assert maxerr(p, q) < 1e-6, (step, k)                      # torch AdamW vs the flat kernel: rounding only
        # the running statistics: the same bits after the first step (same parameters, same launches); afterwards the two models'
        # parameters differ by AdamW's rounding and the statistics follow (tests/las_util.py's bound on running statistics)
        for a, b in zip(ref_model.buffers(), fused_model.buffers()):
            assert torch.equal(a, b) if step == 0 or not a.is_floating_point() else maxerr(a, b) < 2e-6 * max(1.0, a.abs().max().item())
        losses.append(loss_f.item())
    assert losses[-1] < losses[0]


def test_dropout_draw():
    """Without a forced mask: one howl_dropout_mask launch per training forward; the keep rate of a (512, 256) mask is 0.9 within
    0.02 (more than 20 sigma of a fair draw, sigma = 0.0008); two replicas' salts give different masks."""
    from howl_amd import parallel
    m = make(4, u.make_state(4, 3)).train()
    x = torch.randn(512, 3, 40, 5, device=DEV)
    torch.manual_seed(1234)
    m._launch_forward(x, None)
    mask0 = m._las_saved[4].clone()
    assert tuple(mask0.shape) == (512, 256) and bool(((mask0 == 0) | (mask0 == 1)).all())
    assert abs(mask0.mean().item() - 0.9) < 0.02
    real = parallel.world_info
    try:
        parallel.world_info = lambda group=None: (1, 2)
        torch.manual_seed(1234)
        m._launch_forward(x, None)
        mask1 = m._las_saved[4].clone()
    finally:
        parallel.world_info = real
    assert abs(mask1.mean().item() - 0.9) < 0.02 and not torch.equal(mask0, mask1)
    torch.manual_seed(1234)
    m._launch_forward(x, None)
    assert torch.equal(m._las_saved[4], mask0)                         # reproducible under torch.manual_seed


def test_pretrain_gsc_entry_point_trains_las(tmp_path, monkeypatch):
    """`pretrain_gsc --model las --synthetic`: four epochs of four fused steps over 64 generated clips (the tone of a clip encodes
    its label) and an evaluation after each; the loss is finite and decreases -- a step's loss is that of a fresh batch of 16 with
    a fresh dropout draw, so epochs are compared: the mean of the last below the mean of the first (the float32 torch restatement
    of the model under the same optimiser settings falls from 3.44 to 3.35, 3.22 and 3.0 over these four epochs, whatever the
    seed); the workspace reloads with the reference's keys and the reloaded model reproduces its logits."""
    import json
    for k, v in dict(NUM_EPOCHS="4", BATCH_SIZE="16", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.002", LR_DECAY="0.8", DEVICE="cuda:0",
                     NUM_MELS="40").items():
        monkeypatch.setenv(k, v)
    from howl_amd.settings import SETTINGS
    SETTINGS.reset()
    from howl_amd.workspace import Workspace
    x = torch.randn(3, 3, 40, 51, generator=torch.Generator().manual_seed(9)).to(DEV)
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
        pretrain_gsc.main(["--model", "las", "--workspace", str(ws), "--synthetic", "64"])
        lines = [json.loads(l) for l in (ws / "logs" / "scalars.jsonl").read_text().splitlines()]
        losses = [l["value"] for l in lines if l["tag"] == "Training/Loss"]
        accs = [l["value"] for l in lines if l["tag"] == "Dev/Metric/acc"]
        print("las pretrain_gsc losses", losses)
        assert len(losses) == 16 and all(np.isfinite(losses)) and len(accs) == 4
        assert np.mean(losses[-4:]) < np.mean(losses[:4])
        sd = torch.load(ws / "model.pt.bin")
        assert list(sd) == list(u.RefLas(30).state_dict())
        assert int(sd["encoder.conv_encoder.1.num_batches_tracked"]) == 16 and int(sd["encoder.conv_encoder.5.num_batches_tracked"]) == 16
        reloaded = make(30, sd).eval()
        with torch.no_grad():
            assert torch.equal(reloaded(x, None), seen["logits"]) and bool(torch.isfinite(seen["logits"]).all())
    finally:
        SETTINGS.reset()


def test_frame_engine_pass_with_a_las_model():
    """``FrameInferenceEngine.window_probabilities`` with a las model: the engine hands the model the three-channel features of
    every strided window and gets the probabilities of the model called directly; ``infer`` runs to a decision."""
    from howl_amd.context import InferenceContext
    from howl_amd.model.inference import FrameInferenceEngine
    pcm, std, zmuv = _frontend(1, 24000)
    ctx = InferenceContext(["hey", "fire", "fox"], token_type="word")
    model = make(ctx.num_labels, u.make_state(ctx.num_labels, 41)).eval()
    engine = FrameInferenceEngine(500, 63, model, zmuv, ctx)
    clip = pcm[0]
    probs = engine.window_probabilities(clip)
    chunk, stride = 8000, int(63 / 1000 * 16000)
    n = (clip.numel() - chunk) // stride + 1
    assert probs.shape == (n, ctx.num_labels) and np.isfinite(probs).all()
    windows = torch.stack([clip[i * stride:i * stride + chunk] for i in range(probs.shape[0])])
    feats = engine.std.log_mel_for_model(windows, zmuv, channels=3)
    lengths = engine.std.compute_lengths(torch.full((windows.size(0),), chunk, device=DEV))
    with torch.no_grad():
        direct = model(feats, lengths).softmax(-1).cpu().numpy()
    assert np.abs(direct - probs).max() < 1e-6
    assert np.allclose(probs.sum(1), 1.0, atol=1e-5)
    assert engine.infer(clip) in (True, False)
