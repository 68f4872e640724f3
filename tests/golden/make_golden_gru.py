"""Regenerates tests/golden/g16_gru.npz from the reference's own ``SimpleGru`` (howl/model/rnn.py:94-130).

Run by hand where a checkout of the reference is present, under the import shims of ``_reference_shims.py`` (as
``make_golden.py`` is): ``python tests/golden/make_golden_gru.py``.  Records, with seeded weights and every BatchNorm tensor moved
away from its initial value:

* ``state/<key>``: the full ``state_dict``;
* case A: x (5, 3, 40, 21), lengths [21, 17, 9, 3, 1], 4 labels -- eval logits, then ONE training-mode forward / backward with
  nn.CrossEntropyLoss: its logits, loss, every gradient, the dropout keep mask that draw used (captured by a forward hook on
  ``dnn.2``: output != 0 where the input is; where the input is 0 the mask cannot matter and is recorded as kept) and the running
  statistics afterwards;
* case B: x (4, 3, 40, 22), lengths None -- eval logits.

The reference adds 4 to ``lengths`` in place, so every call gets a clone.  Data only; nothing of the reference's text.
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


def main():
    torch.manual_seed(1600)
    model = RegisteredModel.find_registered_class("gru")(4)
    g = torch.Generator().manual_seed(1601)
    with torch.no_grad():
        for i in (1, 6):
            bn = model.conv_encoder[i]
            n = bn.weight.numel()
            bn.weight.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.copy_(0.6 * torch.rand(n, generator=g) - 0.3)
            bn.running_mean.copy_(0.4 * torch.rand(n, generator=g) - 0.2)
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
            bn.num_batches_tracked.fill_(3)
    out = {f"state/{k}": v.detach().clone().numpy() for k, v in model.state_dict().items()}

    xa = torch.randn(5, 3, 40, 21, generator=g)
    la = torch.tensor([21, 17, 9, 3, 1])
    labels = torch.tensor([1, 3, 0, 2, 1])
    xb = torch.randn(4, 3, 40, 22, generator=g)
    out.update({"a/x": xa.numpy(), "a/lengths": la.numpy(), "a/labels": labels.numpy(), "b/x": xb.numpy()})

    model.eval()
    with torch.no_grad():
        out["a/eval_logits"] = model(xa, la.clone()).numpy()
        out["b/eval_logits"] = model(xb, None).numpy()

    seen = {}
    hook = model.dnn[2].register_forward_hook(lambda mod, inp, res: seen.update(inp=inp[0].detach().clone(), out=res.detach().clone()))
    model.train()
    logits = model(xa, la.clone())
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    loss.backward()
    hook.remove()
    keep = ((seen["out"] != 0) | (seen["inp"] == 0)).float()
    assert torch.allclose(seen["out"], seen["inp"] * keep / 0.8)
    out.update({"a/keep_mask": keep.numpy(), "a/train_logits": logits.detach().numpy(), "a/loss": loss.detach().numpy()})
    for k, p in model.named_parameters():
        out[f"a/grad/{k}"] = p.grad.detach().numpy()
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"a/after/{k}"] = v.detach().clone().numpy()
    np.savez_compressed(HERE / "g16_gru.npz", **out)
    print("wrote", HERE / "g16_gru.npz", {k: v.shape for k, v in out.items() if k.startswith("a/") and "grad" not in k})


if __name__ == "__main__":
    main()
