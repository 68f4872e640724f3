"""MobileNetClassifier kernels (howl_amd/csrc/mobilenet.hip) on the hipemu CPU emulator vs the oracle restatement
(oracle/mobilenet.py; parity unpinned against torchvision -- see its header): layer table, forward in training and
eval mode, BatchNorm buffer updates, every parameter gradient."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from emu_util import emu_lib, ptr
from howl_amd.lib import HowlHipError, HowlMbLayer
import mb_layerwise as ml
from mb_util import check_grads, oracle_step
from oracle import mobilenet as om


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def layer_table(lib):
    out = []
    for i in range(lib.cdll.howl_mobilenet_num_layers()):
        d = HowlMbLayer()
        lib.call("howl_mobilenet_layer", i, ctypes.byref(d))
        out.append(d)
    return out


def flat_params(lib, sd, C):
    names = om.mobilenet_param_names()
    flat = np.concatenate([sd[n].numpy().reshape(-1) for n in names]).astype(np.float32)
    assert flat.size == lib.cdll.howl_mobilenet_param_floats(C)
    return flat, names


def flat_buffers(sd):
    out = []
    for l in om.layer_table():
        out += [sd[l["bn"] + ".running_mean"].numpy(), sd[l["bn"] + ".running_var"].numpy()]
    return np.concatenate(out).astype(np.float32)


def test_layer_table_matches_oracle(lib):
    tab, otab = layer_table(lib), om.layer_table()
    assert len(tab) == len(otab) == 53
    kinds = {"dense": 0, "pw": 1, "dw": 2}
    acts = {"none": 0, "relu6": 1, "relu": 2}
    off = 0
    for d, o in zip(tab, otab):
        assert (d.kind, d.cin, d.cout, d.stride, d.pad_h, d.pad_w, d.act, d.bias, d.pool) == \
               (kinds[o["kind"]], o["cin"], o["cout"], o["stride"], o["pad"][0], o["pad"][1], acts[o["act"]], int(o["bias"]),
                int(o["pool"]))
        assert (d.res_src >= 0) == o["res"]
        # state-dict key scheme documented in include/howl_hip.h
        if d.feat < 0:
            key = "downsample.0"
        elif d.sub < 0:
            key = f"model.features.{d.feat}.0"
        elif d.wrapped:
            key = f"model.features.{d.feat}.conv.{d.sub}.0"
        else:
            key = f"model.features.{d.feat}.conv.{d.sub}"
        assert key == o["key"]
        assert d.w_off == off
        off += int(np.prod(om.conv_shape(o))) + (o["cout"] if o["bias"] else 0) + 2 * o["cout"]
    assert lib.cdll.howl_mobilenet_buffer_floats() == sum(2 * o["cout"] for o in otab)
    # known answer from the literature: torchvision's mobilenet_v2 (width 1.0) has 3,504,872 parameters with its 1000-way
    # classifier, 2,223,872 of them in `features` -- the layer table (+ the 36-parameter downsample stem in front) must add up to
    # exactly that.  (torchvision itself is not available here: this pins the architecture, not the arithmetic.)
    downsample = 3 * 1 * 9 + 3 + 3 + 3
    assert lib.cdll.howl_mobilenet_param_floats(1000) - downsample == 3504872
    assert lib.cdll.howl_mobilenet_param_floats(1000) - downsample - (1000 * 1280 + 1000) == 2223872


@pytest.mark.parametrize("B,T,dropout", [(6, 41, False), (5, 30, True)])
def test_forward_backward_vs_oracle(lib, B, T, dropout):
    C, M = 5, 40
    torch.manual_seed(B * 100 + T)
    x = torch.randn(B, 3, M, T) * 1.5                       # the kernels read channel 0 through strides
    labels = torch.arange(B) % C
    keep = (torch.rand(B, om.LAST_CHANNEL) >= 0.2).float() if dropout else None
    sd = om.mobilenet_init(C)
    flat, names = flat_params(lib, sd, C)
    bufs = flat_buffers(sd)
    xn = np.ascontiguousarray(x.numpy())
    sb, sm, st = 3 * M * T, T, 1
    ws = np.zeros(lib.cdll.howl_mobilenet_workspace_bytes(B, M, T, C), np.uint8)
    logits = np.zeros((B, C), np.float32)
    mask = None if keep is None else np.ascontiguousarray(keep.numpy())
    scale = 1.0 / (1.0 - om.DROPOUT_P) if dropout else 1.0
    lib.call("howl_mobilenet_fwd", ptr(flat), ptr(bufs), C, ptr(xn), sb, sm, st, B, M, T, 1, ptr(mask), scale, ptr(logits),
             ptr(ws), ws.size, None)

    ref, grads, osd = oracle_step(sd, x, labels, keep)
    np.testing.assert_allclose(logits, ref.numpy(), rtol=0, atol=5e-4)   # within the 1e-3 of BASELINE's north star
    assert (logits.argmax(1) == ref.numpy().argmax(1)).all()
    np.testing.assert_allclose(bufs, flat_buffers({k: v.detach() for k, v in osd.items()}), rtol=1e-4, atol=1e-5)

    p = torch.softmax(ref, 1)
    p[torch.arange(B), labels] -= 1
    dlogits = np.ascontiguousarray((p / B).numpy().astype(np.float32))
    g = np.full(flat.size, np.nan, np.float32)
    lib.call("howl_mobilenet_bwd", ptr(flat), C, ptr(xn), sb, sm, st, B, M, T, ptr(mask), scale, ptr(dlogits), ptr(g), ptr(ws),
             ws.size, None)
    assert np.isfinite(g).all()
    views, off = [], 0
    for gr in grads:
        views.append(g[off:off + gr.numel()].reshape(gr.shape))
        off += gr.numel()
    assert off == g.size
    check_grads(views, sd, x, labels, keep, grads)

    # eval mode: running statistics, no dropout -- well conditioned, compared directly
    elog = np.zeros((B, C), np.float32)
    lib.call("howl_mobilenet_fwd", ptr(flat), ptr(bufs), C, ptr(xn), sb, sm, st, B, M, T, 0, None, 1.0, ptr(elog), ptr(ws),
             ws.size, None)
    esd = {k: v.clone() for k, v in sd.items()}
    off = 0
    for l in om.layer_table():
        for name in (".running_mean", ".running_var"):
            n = esd[l["bn"] + name].numel()
            esd[l["bn"] + name] = torch.from_numpy(bufs[off:off + n].copy())
            off += n
    eref = om.mobilenet_forward(esd, x, False)
    np.testing.assert_allclose(elog, eref.numpy(), rtol=0, atol=5e-5)

    # what the launch plan refuses, both directions refuse, with the same reason and before anything is launched
    Bx, Mx, Tx = 512, 80, 20000
    with pytest.raises(HowlHipError, match=r"howl_mobilenet_fwd: batch too large for the stem kernels"):
        lib.call("howl_mobilenet_fwd", ptr(flat), ptr(bufs), C, ptr(xn), sb, sm, st, Bx, Mx, Tx, 1, ptr(mask), scale, ptr(logits),
                 ptr(ws), ws.size, None)
    with pytest.raises(HowlHipError, match=r"howl_mobilenet_bwd: batch too large for the stem kernels"):
        lib.call("howl_mobilenet_bwd", ptr(flat), C, ptr(xn), sb, sm, st, Bx, Mx, Tx, ptr(mask), scale, ptr(dlogits), ptr(g), ptr(ws),
                 ws.size, None)
    with pytest.raises(HowlHipError, match=r"howl_mobilenet_bwd: bad shape"):
        lib.call("howl_mobilenet_bwd", ptr(flat), C, ptr(xn), sb, sm, st, B, M, 0, ptr(mask), scale, ptr(dlogits), ptr(g), ptr(ws),
                 ws.size, None)


# ---- layer-local float64 checks (tests/mb_layerwise.py) --------------------------------------------------------------------
# (B, M, T, labels, dropout, layout of x, also eval mode).  (5, 40, 30): the shape of the oracle comparison above, with dropout;
# (3, 33, 27): odd mel count, nothing divides; (2, 80, 21): 80 mel bins; x as (B, T, M) frames -- st = M, sm = 1, slack between
# utterances -- with 3 labels (13 x 40 x 9: 65 row chunks in the first depthwise data gradient, so the two-level fold runs) and with 35.
LAYERWISE = [(5, 40, 30, 5, True, "bmt", True), (3, 33, 27, 5, False, "bmt", False), (2, 80, 21, 5, False, "bmt", False),
             (13, 40, 9, 3, True, "btm", False), (2, 40, 37, 35, False, "btm", False)]
BIG_DEVICE = (5, 40, 30, 5, True, "bmt")      # once more on an emulated 256-CU device: 32-row forward and 32 x 64 data-gradient tiles


def _child(mode, case, cus):
    import json
    import os
    import subprocess
    import sys
    here = Path(__file__).resolve().parent
    python = [sys.executable] + [flag for flag, on in (("-s", sys.flags.no_user_site), ("-E", sys.flags.ignore_environment)) if on]
    env = dict(os.environ, HIPEMU_CUS=str(cus), PYTHONPATH=os.pathsep.join([str(here.parent), str(here)]))
    r = subprocess.run(python + [str(here / "mb_layerwise.py"), mode] + [str(int(v)) for v in case[:5]] + [case[5]], env=env,
                       capture_output=True, text=True, timeout=2400, cwd=here.parent)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    return json.loads(r.stdout.split("RESULT", 1)[1])


@pytest.mark.parametrize("B,M,T,C,dropout,layout,eval_too", LAYERWISE)
def test_every_layer_vs_float64(lib, B, M, T, C, dropout, layout, eval_too):
    """Every layer's forward and backward, each from the kernels' own neighbouring tensors, against float64 (see mb_layerwise)."""
    ml.run_case(lib, ml.HostMem(), B, M, T, C, dropout, layout, eval_too=eval_too)


def test_every_layer_vs_float64_on_256_cus():
    out = _child("check", BIG_DEVICE, 256)
    assert "training" in out["reports"]


def test_layerwise_cases_cover_the_kernel_instances(lib):
    """The cases above must keep exercising every instance the launchers can pick (read from the published plan): a case set that
    stops doing so fails here.  More than MB_R2 row blocks (two-level fold) is also required of the device cases."""
    tab = ml.layer_table(lib)
    seen = set(_child("plan", BIG_DEVICE, 256)["coverage"])
    assert "pw_fwd tile 32 materialised producer" in seen and "pw_dgrad tile 32 without ss_in" in seen, seen
    for B, M, T, C, *_ in LAYERWISE:
        seen |= ml.coverage(tab, ml.workspace_map(lib, B, M, T, C))
    assert (ml.REQUIRED | {"two-level arrival"}) <= seen, sorted((ml.REQUIRED | {"two-level arrival"}) - seen)


def test_workspace_map_refuses_what_the_plan_refuses(lib):
    d = ml.HowlMbWsLayer()
    with pytest.raises(HowlHipError, match=r"howl_mobilenet_workspace_layer: batch too large for the stem kernels"):
        lib.call("howl_mobilenet_workspace_layer", 512, 80, 20000, 5, 0, ctypes.byref(d))
    with pytest.raises(HowlHipError, match=r"howl_mobilenet_workspace_layer: bad shape"):
        lib.call("howl_mobilenet_workspace_layer", 4, 40, 0, 5, 0, ctypes.byref(d))
    with pytest.raises(HowlHipError, match=r"howl_mobilenet_workspace_layer: index out of range"):
        lib.call("howl_mobilenet_workspace_layer", 4, 40, 41, 5, 54, ctypes.byref(d))
    wsl = ml.workspace_map(lib, 4, 40, 41, 5)
    assert 4 * wsl[-1].total_floats + 256 == lib.cdll.howl_mobilenet_workspace_bytes(4, 40, 41, 5)
    offs = sorted(o for w in wsl[:-1] for o in (w.z, w.g, w.y, w.ss, w.bc) if o >= 0)
    assert len(set(offs)) == len(offs) and offs[-1] < wsl[-1].dz1 < wsl[-1].pooled < wsl[-1].pooled_d < wsl[-1].total_floats


def test_layerwise_comparison_rules():
    """The comparison itself: a decided element must match its own reference; an undecided one may match the other side, within
    the same bound and no further; NaN never passes."""
    def run(got, ref, bound, alt=None, und=None):
        c = object.__new__(ml.Check)
        c.ratios, c.fails = {}, []
        t = lambda v: torch.tensor(v, dtype=torch.float64)
        c.cmp("x", "here", t(got), t(ref), t(bound), alt=None if alt is None else t(alt),
              und=None if und is None else torch.tensor(und), layout="c")
        return c.fails, c.ratios["x"]
    assert run([1.0, 2.0], [1.0, 2.0 + 1e-7], [0.0, 2e-7]) == ([], pytest.approx(0.5))
    assert len(run([1.0, 2.0], [1.0 + 1e-9, 2.0], [0.0, 1e-7])[0]) == 1            # a zero bound means exactly equal
    assert len(run([float("nan")], [0.0], [1.0])[0]) == 1
    # masked reference 0, unmasked 3: the kernel's 3 passes only where the element is undecided
    assert run([3.0], [0.0], [1e-6], alt=[3.0], und=[True])[0] == []
    assert len(run([3.0], [0.0], [1e-6], alt=[3.0], und=[False])[0]) == 1
    assert len(run([2.9], [0.0], [1e-6], alt=[3.0], und=[True])[0]) == 1
