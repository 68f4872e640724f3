"""Regenerates golden G17 (tests/golden/g17_las*.npz) from the reference's own ``LASClassifier`` (howl/model/rnn.py:133-215).

Run by hand where a checkout of the reference is present, under the import shims of ``_reference_shims.py`` (as
``make_golden.py`` is): ``python tests/golden/make_golden_las.py``.  Records, with the reference's default initialisation under a
seed and every BatchNorm tensor moved away from its initial value:

* ``state/<key>``: the ``state_dict``, split over three files so that none outgrows the limit for a committed file
  (``g17_las_lstm_fwd.npz``: the forward direction's LSTM tensors, ``g17_las_lstm_rev.npz``: the reverse direction's,
  ``g17_las.npz``: everything else and the cases).  The reference registers conv1 and conv2 twice; the aliased tensors
  (``encoder.conv_encoder.{0,4}.*``) are stored once, under ``encoder.conv{1,2}.*``;
* case A: x (5, 3, 40, 21), lengths [21, 17, 9, 3, 1], 4 labels -- eval logits, then ONE training-mode forward / backward with
  nn.CrossEntropyLoss: its logits, loss, the dropout keep mask that draw used (captured by a forward hook on ``fc.2``: output != 0
  where the input is; where the input is 0 the mask cannot matter and is recorded as kept), the running statistics afterwards and
  the gradients: in full for tensors of up to 4096 elements, for the larger matrices their row sums, column sums and every 97th
  element of the flattened tensor (``a/gradrow/``, ``a/gradcol/``, ``a/gradsample/``), which pins layout and transposition;
* case B: x (4, 3, 40, 22), lengths None -- eval logits.

Data only; nothing of the reference's text.
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

FULL_GRAD_MAX = 4096
SAMPLE_STRIDE = 97


def main():
    torch.manual_seed(1700)
    model = RegisteredModel.find_registered_class("las")(4)
    g = torch.Generator().manual_seed(1701)
    with torch.no_grad():
        for i in (1, 5):
            bn = model.encoder.conv_encoder[i]
            n = bn.weight.numel()
            bn.weight.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.copy_(0.6 * torch.rand(n, generator=g) - 0.3)
            bn.running_mean.copy_(0.4 * torch.rand(n, generator=g) - 0.2)
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
            bn.num_batches_tracked.fill_(3)
    sd = model.state_dict()
    assert len(sd) == 35
    fwd, rev, out = {}, {}, {}
    for k, v in sd.items():
        if k.startswith("encoder.conv_encoder.0.") or k.startswith("encoder.conv_encoder.4."):
            assert v.data_ptr() == sd[k.replace("conv_encoder.0", "conv1").replace("conv_encoder.4", "conv2")].data_ptr()
            continue
        part = rev if k.endswith("_reverse") else fwd if "lstm_encoder" in k else out
        part[f"state/{k}"] = v.detach().clone().numpy()

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
    hook = model.fc[2].register_forward_hook(lambda mod, inp, res: seen.update(inp=inp[0].detach().clone(), out=res.detach().clone()))
    model.train()
    logits = model(xa, la.clone())
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    loss.backward()
    hook.remove()
    keep = ((seen["out"] != 0) | (seen["inp"] == 0)).float()
    assert torch.allclose(seen["out"], seen["inp"] * keep / 0.9)
    out.update({"a/keep_mask": keep.numpy(), "a/train_logits": logits.detach().numpy(), "a/loss": loss.detach().numpy()})
    for k, p in model.named_parameters():          # (named_parameters lists a shared tensor once, under its first name)
        gr = p.grad.detach()
        if gr.numel() <= FULL_GRAD_MAX:
            out[f"a/grad/{k}"] = gr.numpy()
        else:
            out[f"a/gradrow/{k}"] = gr.sum(1).numpy()
            out[f"a/gradcol/{k}"] = gr.sum(0).numpy()
            out[f"a/gradsample/{k}"] = gr.reshape(-1)[::SAMPLE_STRIDE].clone().numpy()
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"a/after/{k}"] = v.detach().clone().numpy()
    for name, part in (("g17_las.npz", out), ("g17_las_lstm_fwd.npz", fwd), ("g17_las_lstm_rev.npz", rev)):
        np.savez_compressed(HERE / name, **part)
        print("wrote", HERE / name, (HERE / name).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
