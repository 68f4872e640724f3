"""The gru model on the device (howl_amd/csrc/gru.hip through include/howl_hip_gru.h and ``SimpleGru``): the parity set of
tests/test_emu_gru.py plus the 1 s window, the reference's golden numbers through the model class, the fused training step against
the autograd path, canaries around every buffer, the refusals, the training entry point and the dropout draw."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import gru_util as u  # noqa: E402
from gpu_util import DEV, maxerr  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from howl_amd import lib
    return lib.get()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make(C, state=None):
    from howl_amd.model import RegisteredModel
    m = RegisteredModel.find_registered_class("gru")(C)
    if state is not None:
        m.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def g16():
    g = np.load(u.GOLDEN)
    return g, {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}


# ---- parity through the C ABI, every buffer between canary bands ----------------------------------------------------------------------

@pytest.mark.parametrize("time_major", (False, True))
@pytest.mark.parametrize("name", tuple(u.CASES))
def test_gru_vs_fp64_with_canaries(name, time_major):
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
    u.check_grads(name, tr["grads"], r["train64"], r["train32"])
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
        lengths = [21] * 6
        lengths[pos] = 9
        assert torch.equal(run(x, lengths)[pos], whole[2]), pos


def test_gru_refusals_on_the_device():
    from guard_mem import Banded
    u.check_refusals(_lib(), Banded(DEV, log=open("/dev/null", "w")), _stream())


# ---- the model class ---------------------------------------------------------------------------------------------------------------------

def test_golden_state_loads_strictly_and_reproduces_the_reference(g16):
    g, state = g16
    m = make(4, state).eval()
    xa, la = torch.from_numpy(g["a/x"]).to(DEV), torch.from_numpy(g["a/lengths"]).clone()
    with torch.no_grad():
        assert maxerr(m(xa, la), g["a/eval_logits"]) < 5e-5
        assert maxerr(m(torch.from_numpy(g["b/x"]).to(DEV), None), g["b/eval_logits"]) < 5e-5
    assert la.tolist() == g["a/lengths"].tolist()                      # the caller's lengths are not written
    labels, keep = torch.from_numpy(g["a/labels"]), torch.from_numpy(g["a/keep_mask"])
    m.train()
    m.forced_keep_mask = keep
    logits = m(xa, la)
    loss = torch.nn.functional.cross_entropy(logits, labels.to(DEV))
    loss.backward()
    assert maxerr(logits, g["a/train_logits"]) < 5e-5
    assert abs(loss.item() - float(g["a/loss"])) < 1e-4 * max(1.0, float(g["a/loss"]))
    r64 = u.reference(state, xa.cpu(), la.tolist(), labels, keep, train=True)
    r32 = u.reference(state, xa.cpu(), la.tolist(), labels, keep, train=True, dtype=torch.float32)
    u.check_grads("SimpleGru G16", [p.grad.cpu() for p in m.hot_parameters()], r64, r32)
    u.check_buffers("SimpleGru G16", {k: v.cpu() for k, v in m.state_dict().items()},
                    {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})


def test_model_refusals(g16):
    from howl_amd.model import LASEncoderConfig, SimpleGru
    g, state = g16
    with pytest.raises(NotImplementedError, match="hidden_size"):
        SimpleGru(4, LASEncoderConfig(hidden_size=128))
    m = make(4, state).eval()
    xa = torch.from_numpy(g["a/x"]).to(DEV)
    with pytest.raises(RuntimeError, match="sorted in decreasing order"):
        m(xa, torch.tensor([3, 21, 17, 9, 1]))
    with pytest.raises(NotImplementedError, match="training-mode forward"):
        m(xa, torch.tensor([21, 17, 9, 3, 1])).sum().backward()


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
    """FusedTrainer.step (explicit launches, gradients straight into the flat buffer, flat AdamW) with a forced mask against the
    autograd path through the same launches + torch.optim.AdamW, three steps.  On the first step both start from the same bits
    and the gradients are bit-identical; afterwards the parameters differ by the rounding of the two AdamW implementations."""
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.training.fused import FusedTrainer
    from howl_amd.utils.synth import synthetic_pcm
    B, L, C = 10, 8000, 5
    pcm = synthetic_pcm(B, L).to(DEV)
    std = StandardAudioTransform().to(DEV).eval()
    zmuv = ZmuvTransform().to(DEV)
    zmuv.update(std(pcm[:4]))
    lengths = torch.sort(24 + torch.arange(B) % 15, descending=True).values
    labels = (torch.arange(B) % C).to(DEV)
    feats = std.log_mel_for_model(pcm, zmuv)
    state = u.make_state(C, 21)
    keep = (torch.rand(B, 192, generator=torch.Generator().manual_seed(3)) < 0.8).float()
    fused_model, ref_model = make(C, state).train(), make(C, state).train()
    fused_model.forced_keep_mask = ref_model.forced_keep_mask = keep
    trainer = FusedTrainer(fused_model, std, zmuv, lr=1e-3, weight_decay=1e-5)
    opt = torch.optim.AdamW(ref_model.parameters(), 1e-3, weight_decay=1e-5)
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
        for a, b in zip(ref_model.buffers(), fused_model.buffers()):
            assert torch.equal(a, b)
        losses.append(loss_f.item())
    assert losses[-1] < losses[0]


def test_dropout_draw():
    """Without a forced mask: one howl_dropout_mask launch per training forward; the keep rate of a (512, 192) mask is 0.8 within
    0.02 (more than 6 sigma of a fair draw, sigma = 0.0013); two replicas' salts give different masks."""
    from howl_amd import parallel
    m = make(4, u.make_state(4, 3)).train()
    x = torch.randn(512, 1, 40, 5, device=DEV)
    torch.manual_seed(1234)
    m._launch_forward(x, None)
    mask0 = m._gru_saved[4].clone()
    assert tuple(mask0.shape) == (512, 192) and bool(((mask0 == 0) | (mask0 == 1)).all())
    assert abs(mask0.mean().item() - 0.8) < 0.02
    real = parallel.world_info
    try:
        parallel.world_info = lambda group=None: (1, 2)
        torch.manual_seed(1234)
        m._launch_forward(x, None)
        mask1 = m._gru_saved[4].clone()
    finally:
        parallel.world_info = real
    assert abs(mask1.mean().item() - 0.8) < 0.02 and not torch.equal(mask0, mask1)
    torch.manual_seed(1234)
    m._launch_forward(x, None)
    assert torch.equal(m._gru_saved[4], mask0)                         # reproducible under torch.manual_seed


def test_pretrain_gsc_entry_point_trains_gru(tmp_path, monkeypatch):
    """`pretrain_gsc --model gru --synthetic`: a handful of fused steps and one evaluation; the loss is finite, the workspace
    reloads and the reloaded model reproduces its logits."""
    import json
    for k, v in dict(NUM_EPOCHS="1", BATCH_SIZE="16", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.002", LR_DECAY="0.8", DEVICE="cuda:0",
                     NUM_MELS="40").items():
        monkeypatch.setenv(k, v)
    from howl_amd.settings import SETTINGS
    SETTINGS.reset()
    from howl_amd.workspace import Workspace
    x = torch.randn(3, 1, 40, 51, generator=torch.Generator().manual_seed(9)).to(DEV)
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
        pretrain_gsc.main(["--model", "gru", "--workspace", str(ws), "--synthetic", "64"])
        lines = [json.loads(l) for l in (ws / "logs" / "scalars.jsonl").read_text().splitlines()]
        losses = [l["value"] for l in lines if l["tag"] == "Training/Loss"]
        accs = [l["value"] for l in lines if l["tag"] == "Dev/Metric/acc"]
        assert len(losses) == 4 and all(np.isfinite(losses)) and len(accs) == 1
        sd = torch.load(ws / "model.pt.bin")
        assert list(sd) == list(u.RefGru(30).state_dict())
        assert int(sd["conv_encoder.1.num_batches_tracked"]) == 4 and int(sd["conv_encoder.6.num_batches_tracked"]) == 4
        reloaded = make(30, sd).eval()
        with torch.no_grad():
            assert torch.equal(reloaded(x, None), seen["logits"]) and bool(torch.isfinite(seen["logits"]).all())
    finally:
        SETTINGS.reset()
