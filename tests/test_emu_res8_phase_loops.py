"""The shapes of test_gpu_res8_phase_loops.py at B = 5 on the hipemu build of the same kernels: one training step (forward,
fused cross-entropy, backward) against the oracle.  81 frames (H = 27: waves with five and four position tiles) and 21 frames
(H = 7: waves with 2, 1 and 0 tiles); five utterances on the emulator's four CUs: the first workgroup loops twice, the others once
and take the `more == false` tail on their first pass.  The default slicing (four workgroups per utterance) needs a device of
at least 20 CUs, which the emulator takes from HIPEMU_CUS when it is loaded: that case runs in a process of its own.

Input seed: with five utterances every ReLU decision carries a fifth of the gradient, and a pre-activation within fp32 rounding of
zero is decided by the summation order, not by the arithmetic under test.  Seed 11 has one in layer 4 at 81 frames (the kernels
and the oracle take different sides: conv4's weight gradient is then off by 1.2e-3, the layers above it and the logits agree to
1e-7 -- before and after the phase loops were changed); seed 12 has none (every tensor within 2e-7)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from emu_util import emu_lib, ptr
from oracle import models as om
from test_emu_res8 import Res8Harness, feats

B, C, SEED = 5, 12, 12


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def _emu_step(lib, T):
    x = feats(B, T, SEED)
    h = Res8Harness(lib, B, T, C)
    logits = h.fwd(x[:, 0].permute(0, 2, 1).numpy(), training=True)
    loss, dlogits = np.zeros(1, np.float32), np.zeros((B, C), np.float32)
    lab = np.ascontiguousarray((torch.arange(B) % C).numpy(), np.int64)
    lib.call("howl_xent_fwd_bwd", ptr(h.logits), ptr(lab), B, C, ptr(loss), ptr(dlogits), None)
    return logits, float(loss[0]), h.bwd(dlogits)


_REF = {}


def _oracle(T):
    if T not in _REF:
        x = feats(B, T, SEED)
        sd = om.res8_init(C)
        names = om.res8_param_names()
        params = {n: sd[n].clone().requires_grad_(True) for n in names}
        sd_ref = dict(sd)
        sd_ref.update(params)
        logits = om.res8_forward(sd_ref, x, True)
        loss = torch.nn.functional.cross_entropy(logits, torch.arange(B) % C)
        grads = torch.autograd.grad(loss, [params[n] for n in names])
        _REF[T] = (logits.detach().numpy(), loss.item(), {n: g.numpy() for n, g in zip(names, grads)})
    return _REF[T]


def _check(T, logits, loss, grads):
    # tolerances: test_emu_res8.py test_res8_train_step
    ref_logits, ref_loss, ref_grads = _oracle(T)
    np.testing.assert_allclose(logits, ref_logits, rtol=0, atol=2e-5)
    assert abs(loss - ref_loss) < 1e-5
    for n, g in ref_grads.items():
        np.testing.assert_allclose(np.asarray(grads[n]).reshape(g.shape), g, rtol=0, atol=2e-5 * max(1.0, float(np.abs(g).max())),
                                   err_msg=n)


@pytest.mark.parametrize("T", [81, 21])
def test_phase_loops_unsliced_on_the_emulator(lib, monkeypatch, T):
    monkeypatch.setenv("HOWL_RES8_SLICES", "0")
    logits, loss, grads = _emu_step(lib, T)
    _check(T, logits, loss, grads)


def test_phase_loops_default_slicing_on_the_emulator():
    here = Path(__file__).resolve().parent
    code = r"""
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
os.environ.setdefault("NUM_MELS", "40")
os.environ.pop("HOWL_RES8_SLICES", None)
import test_emu_res8_phase_loops as P
logits, loss, grads = P._emu_step(P.emu_lib(), 81)
print("RESULT" + json.dumps({"logits": logits.tolist(), "loss": loss, "grads": {k: v.reshape(-1).tolist() for k, v in grads.items()}}))
""" % (str(here.parent), str(here))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HIPEMU_CUS="32"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.split("RESULT", 1)[1])
    _check(81, np.asarray(res["logits"], np.float32), res["loss"], {k: np.asarray(v, np.float32) for k, v in res["grads"].items()})
