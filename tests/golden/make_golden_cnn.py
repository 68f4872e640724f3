"""Regenerates tests/golden/g19_small_cnn.npz and g20_seq_cnn.npz from the reference's own ``SmallCnn`` / ``SequentialCnn``
(howl/model/cnn.py:32-104), constructed with ``CnnSettings(num_labels=4)``.

Run by hand where a checkout of the reference is present, under the import shims of ``_reference_shims.py`` (as
``make_golden.py`` is): ``python tests/golden/make_golden_cnn.py``.  Each file records, with seeded weights and every BatchNorm
tensor moved away from its initial value:

* ``state/<key>``: the full ``state_dict``;
* case A: x (5, 1, 40, T), T = 41 (small-cnn) or 81 (seq-cnn) -- eval scores, then ONE training-mode forward / backward: its scores,
  loss, every gradient, the dropout keep mask that draw used (captured by a forward hook on ``output.2``: output != 0 where the
  input is; where the input is 0 the mask cannot matter and is recorded as kept) and the running statistics afterwards.
  small-cnn: nn.CrossEntropyLoss on ``labels``.  seq-cnn: ``log_softmax`` + ``nn.CTCLoss(blank=0)`` with ``lengths`` [81, 70, 60,
  50, 45] turned into input lengths by the model's own ``compute_length`` (10, 9, 8, 6, 6: every one >= 5) and targets of at most 3
  labels: no loss is infinite;
* case B: x (2, 1, 40, T), T = 40 or 22 -- eval scores.

To keep each file at g16 / g17's size although a state has 133 000 numbers and every one of them a gradient, the numbers are chosen
or kept compressible: the weights and inputs are rounded to a grid (2^-10, 2^-6) BEFORE the reference runs -- they are the exact
state and input of everything recorded -- and the recorded gradients are rounded to 16 mantissa bits (relative error 2^-17,
three orders below the tests' bound).  Data only; nothing of the reference's text.
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import _reference_shims  # noqa: E402

_reference_shims.install()

from howl.model import RegisteredModel  # noqa: E402
from howl.model.cnn import CnnSettings  # noqa: E402


def grid(t, step):
    return torch.round(t / step) * step


def short_mantissa(a):
    """float32 rounded to 16 mantissa bits (the low byte zero: it compresses away)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (((b + np.uint32(0x80)) & np.uint32(0xFFFFFF00)).view(np.float32)).reshape(np.shape(a))


def record(name, path, seed, Ta, Tb):
    torch.manual_seed(seed)
    model = RegisteredModel.find_registered_class(name)(4, CnnSettings(num_labels=4))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for bn in (model.encoder1[3], model.encoder2[3]):
            n = bn.weight.numel()
            bn.weight.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.copy_(0.6 * torch.rand(n, generator=g) - 0.3)
            bn.running_mean.copy_(0.4 * torch.rand(n, generator=g) - 0.2)
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
            bn.num_batches_tracked.fill_(3)
        for p in model.parameters():
            p.copy_(grid(p, 2.0 ** -10))
    out = {f"state/{k}": v.detach().clone().numpy() for k, v in model.state_dict().items()}
    xa = grid(torch.randn(5, 1, 40, Ta, generator=g), 2.0 ** -6)
    xb = grid(torch.randn(2, 1, 40, Tb, generator=g), 2.0 ** -6)
    out.update({"a/x": xa.numpy(), "b/x": xb.numpy()})
    seq = name == "seq-cnn"
    if seq:
        lengths = torch.tensor([81, 70, 60, 50, 45])
        il = torch.tensor([model.compute_length(int(n)) for n in lengths])
        targets = torch.tensor([[1, 2, 3], [2, 1, 2], [3, 1, 0], [1, 0, 0], [2, 3, 1]])
        tl = torch.tensor([3, 3, 2, 1, 3])
        out.update({"a/lengths": lengths.numpy(), "a/input_lengths": il.numpy(), "a/targets": targets.numpy(), "a/target_lengths": tl.numpy()})
    else:
        lengths = None
        labels = torch.tensor([1, 3, 0, 2, 1])
        out["a/labels"] = labels.numpy()
    model.eval()
    with torch.no_grad():
        out["a/eval_logits"] = model(xa, lengths).numpy()
        out["b/eval_logits"] = model(xb, None).numpy()
    seen = {}
    hook = model.output[2].register_forward_hook(lambda mod, inp, res: seen.update(inp=inp[0].detach().clone(), out=res.detach().clone()))
    model.train()
    logits = model(xa, lengths)
    if seq:
        loss = torch.nn.CTCLoss(blank=0)(torch.log_softmax(logits, -1), targets, il, tl)
    else:
        loss = torch.nn.CrossEntropyLoss()(logits, labels)
    assert torch.isfinite(loss)
    loss.backward()
    hook.remove()
    keep = ((seen["out"] != 0) | (seen["inp"] == 0)).float()
    assert torch.allclose(seen["out"], seen["inp"] * keep / 0.9)
    out.update({"a/keep_mask": keep.numpy().astype(np.uint8), "a/train_logits": logits.detach().numpy(), "a/loss": loss.detach().numpy()})
    for k, p in model.named_parameters():
        out[f"a/grad/{k}"] = short_mantissa(p.grad.detach().numpy())
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"a/after/{k}"] = v.detach().clone().numpy()
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes", {k: v.shape for k, v in out.items() if k[:2] in ("a/", "b/") and "grad" not in k})


if __name__ == "__main__":
    record("small-cnn", HERE / "g19_small_cnn.npz", 1900, 41, 40)
    record("seq-cnn", HERE / "g20_seq_cnn.npz", 2000, 81, 22)
