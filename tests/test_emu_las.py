"""The las model (include/howl_hip_las.h, howl_amd/csrc/las.hip) on the hipemu emulator: header / exports / ctypes tables; forward
(eval, train) and every gradient against the float64 restatement of tests/las_util.py and against the reference's own numbers
(golden G17, tests/golden/g17_las*.npz); running statistics; the three identically zero gradients; the same eval-mode bits whatever
an utterance's neighbours; refusals; registry, config and the strict load of the reference's 35 keys; guard-page bounds of every
buffer in child processes (as tests/test_emu_gru.py runs its cases)."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for _p in (str(ROOT), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import las_util as u  # noqa: E402

PLACEMENTS = ("tail", "head")
# "window" (B = 9, T = 81) is too slow for the emulator: tests/test_gpu_las.py runs it.  Both feature layouts on A and on the
# case with a one-column second tile; the bounds cases below run both layouts on A, B, C and one.
PARITY = [("A", False), ("A", True), ("B", False), ("C", False), ("one", False), ("one", True), ("tile16", False), ("tile17", False),
          ("tile17", True)]
TIMEOUT = 900


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


@pytest.fixture(scope="module")
def golden():
    return u.load_golden()


def golden_case_a(g):
    return (torch.from_numpy(g["a/x"]), g["a/lengths"].tolist(), torch.from_numpy(g["a/labels"]), torch.from_numpy(g["a/keep_mask"]))


def check_golden_grads(grads, g):
    """{name: gradient} against G17: in full where it is recorded in full, else row sums, column sums and the strided sample; the
    bound of tests/test_emu_gru.py's golden check, 2e-5 max(1, |recorded|max)."""
    for k in u.PARAMS:
        gr = torch.as_tensor(grads[k]).double()
        if "a/grad/" + k in g:
            views = {"grad": gr}
        else:
            views = {"gradrow": gr.sum(1), "gradcol": gr.sum(0), "gradsample": gr.reshape(-1)[::97]}
        for tag, v in views.items():
            want = g[f"a/{tag}/{k}"]
            assert tuple(v.shape) == want.shape, (k, tag)
            assert u.maxerr(v, want) < 2e-5 * max(1.0, float(np.abs(want).max())), (k, tag, u.maxerr(v, want))


# ---- header, exports, tables -------------------------------------------------------------------------------------------------------

def test_library_exports_the_las_header(built, emu):
    from howl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip_las.h").read_text(), flags=re.S)
    hdr = set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))
    assert hdr == {"howl_las_supported", "howl_las_workspace_bytes", "howl_las_fwd", "howl_las_bwd"}, hdr
    table = set(lib.LAS_SIGNATURES) | set(lib.LAS_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    others = [lib.SIGNATURES, lib.SIZE_FUNCS, lib.STREAM_SIGNATURES, lib.STREAM_SIZE_FUNCS, lib.LSTM_STREAM_SIGNATURES,
              lib.LSTM_STREAM_SIZE_FUNCS, lib.DECIDE_SIGNATURES, lib.DECIDE_SIZE_FUNCS, lib.CTC_LONG_SIGNATURES, lib.CTC_LONG_SIZE_FUNCS,
              lib.GRU_SIGNATURES, lib.GRU_SIZE_FUNCS]
    assert not table & set().union(*others)
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert {n for n in exported if n.startswith("howl_las_")} == hdr, path
    # the argument counts of the header and of the tables agree, and the structs hold what the header declares
    for name, argtypes in {**lib.LAS_SIGNATURES, **lib.LAS_SIZE_FUNCS}.items():
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == len(argtypes), name
    assert len(lib.HowlLasParams._fields_) == len(lib.HowlLasGrads._fields_) == len(u.PARAMS) == 25
    assert len(lib.HowlLasBuffers._fields_) == len(u.BUFFERS) == 6
    assert [f for f, _ in lib.HowlLasParams._fields_] == re.findall(r"const float\* (\w+);", text)
    assert [f for f, _ in lib.HowlLasGrads._fields_] == [f for f, _ in lib.HowlLasParams._fields_]
    assert re.search(r"#define HOWL_LAS_MAX_FRAMES (\d+)", text).group(1) == "8192"


# ---- the yardstick itself -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", tuple(u.CASES))
def test_fp32_cpu_model_is_inside_the_bounds(name):
    """The same model in fp32 on torch CPU stays inside the logits / loss bounds, and no ReLU or max-pool decision flipped for the
    committed seeds: its gradient error (the ``noise`` of the gradient bound) is rounding, below the bound's fixed part."""
    r = u.case_reference(name)
    u.check_logits(name, r["eval32"]["logits"], r["eval64"], "fp32 eval")
    u.check_logits(name, r["train32"]["logits"], r["train64"], "fp32 train")
    u.check_loss(name, r["train32"]["logits"], r["labels"], r["train64"])
    for k in u.PARAMS:
        g64 = r["train64"]["grads"][k]
        assert u.maxerr(r["train32"]["grads"][k], g64) < 2e-5 * max(1.0, float(g64.abs().max())), (name, k)


def test_restated_model_is_the_reference(golden):
    """las_util's float64 model (which keeps the -100 steps) on G17's state and inputs gives the reference's own numbers (fp32
    there): logits, loss, every recorded gradient view, the running statistics; and the state has the reference's 35 keys."""
    g, state = golden
    xa, la, labels, keep = golden_case_a(g)
    r = u.reference(state, xa, la, labels, keep, train=True)
    assert u.maxerr(r["logits"], g["a/train_logits"]) < 5e-5 and abs(float(r["loss"]) - float(g["a/loss"])) < 1e-4
    check_golden_grads(r["grads"], g)
    u.check_buffers("G17 A", r["buffers"], {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})
    assert u.maxerr(u.reference(state, xa, la)["logits"], g["a/eval_logits"]) < 5e-5
    assert u.maxerr(u.reference(state, torch.from_numpy(g["b/x"]), None)["logits"], g["b/eval_logits"]) < 5e-5
    assert len(state) == 35 and list(state) == list(u.RefLas(4).state_dict())
    assert sum(state[k].numel() for k in u.PARAMS) == 471180


# ---- parity --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,time_major", PARITY)
def test_las_vs_fp64(emu, name, time_major):
    r = u.case_reference(name)
    ev = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], False, x_time_major=time_major)
    u.check_logits(name, ev["logits"], r["eval64"], "eval")
    for k in u.BUFFERS:                                                  # eval mode touches no buffer
        assert torch.equal(ev["buffers"][k], r["state"][k]), k
    tr = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], True, r["mask"], r["dlogits"], x_time_major=time_major)
    u.check_logits(name, tr["logits"], r["train64"], "train")
    u.check_loss(name, tr["logits"], r["labels"], r["train64"])
    u.check_grads(name, tr["grads"], r["train64"], r["train32"])         # (the three zero gradients are == 0 exactly)
    u.check_buffers(name, tr["buffers"], r["train64"])
    for k in u.PARAMS:                                                   # no parameter is written
        assert torch.equal(tr["params"][k], r["state"][k]), k
    if r["lengths"] is not None:                                         # the lengths are not written
        assert tr["lengths"].tolist() == list(r["lengths"])
    if not time_major:
        again = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], True, r["mask"], r["dlogits"])
        assert torch.equal(again["logits"], tr["logits"]) and all(torch.equal(a, b) for a, b in zip(again["grads"], tr["grads"]))


def test_las_without_dropout_mask(emu):
    """Training mode with a null mask (p = 0): the float64 model with every unit kept and scale 1."""
    r = u.case_reference("A")
    r64 = u.reference(r["state"], r["x"], r["lengths"], r["labels"], None, train=True)
    r32 = u.reference(r["state"], r["x"], r["lengths"], r["labels"], None, train=True, dtype=torch.float32)
    z = r64["logits"].clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(z, r["labels"]).backward()
    tr = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], True, None, z.grad.float())
    u.check_logits("A", tr["logits"], r64, "train, no mask")
    u.check_grads("A no mask", tr["grads"], r64, r32)


def test_las_vs_golden(emu, golden):
    g, state = golden
    xa, la, labels, keep = golden_case_a(g)
    u.check_logits("G17 A", u.run_library(emu, u.Plain(), state, xa, la, False)["logits"], {"logits": torch.from_numpy(g["a/eval_logits"])}, "eval")
    u.check_logits("G17 B", u.run_library(emu, u.Plain(), state, torch.from_numpy(g["b/x"]), None, False)["logits"],
                   {"logits": torch.from_numpy(g["b/eval_logits"])}, "eval")
    r64 = u.reference(state, xa, la, labels, keep, train=True)
    r32 = u.reference(state, xa, la, labels, keep, train=True, dtype=torch.float32)
    z = r64["logits"].clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(z, labels).backward()
    tr = u.run_library(emu, u.Plain(), state, xa, la, True, keep, z.grad.float())
    gold = {"logits": torch.from_numpy(g["a/train_logits"]), "loss": torch.from_numpy(g["a/loss"])}
    u.check_logits("G17 A", tr["logits"], gold, "train")
    u.check_loss("G17 A", tr["logits"], labels, gold)
    u.check_grads("G17 A", tr["grads"], r64, r32)
    check_golden_grads(dict(zip(u.PARAMS, tr["grads"])), g)
    u.check_buffers("G17 A", tr["buffers"], {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})


# ---- the same bits whatever the neighbours ---------------------------------------------------------------------------------------------

def test_eval_logits_do_not_depend_on_the_batch(emu):
    """Utterance 2 of case A (9 frames of 21: 3 steps of 6) alone, and at every position among a workgroup's four with other,
    LONGER neighbours (whose steps 3..5 the reference would give this utterance a weight of e^-100 for)."""
    r = u.case_reference("A")
    whole = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], False)["logits"]
    alone = u.run_library(emu, u.Plain(), r["state"], r["x"][2:3], [9], False)["logits"]
    assert torch.equal(alone[0], whole[2])
    g = torch.Generator().manual_seed(77)
    for pos in range(4):
        x = torch.randn(6, 3, 40, 21, generator=g)
        x[pos] = r["x"][2]
        lengths = [21] * 6
        lengths[pos] = 9
        got = u.run_library(emu, u.Plain(), r["state"], x, lengths, False)["logits"]
        assert torch.equal(got[pos], whole[2]), pos


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_las_refusals(emu):
    from guard_mem import Arena
    u.check_refusals(emu, Arena("tail", log=open(os.devnull, "w")))


def test_model_registry_and_config(golden):
    from howl_amd.model import (FixedAttentionModuleConfig, LASClassifier, LASClassifierConfig, LASEncoderConfig, RegisteredModel)
    assert "las" in RegisteredModel.registered_names() and RegisteredModel.find_registered_class("las") is LASClassifier
    cfg = LASClassifierConfig()
    assert (cfg.dnn_size, cfg.dropout, cfg.fixed_attn_config.num_heads, cfg.fixed_attn_config.hidden_size) == (256, 0.1, 4, 96)
    assert (cfg.las_config.num_spec_channels, cfg.las_config.num_layers) == (3, 1)
    m = LASClassifier(4)
    assert LASClassifier.FEATURE_CHANNELS == 3 and LASClassifier.NEEDS_LENGTHS and not m.is_sequential
    ref = u.RefLas(4).state_dict()
    assert list(m.state_dict()) == list(ref) and len(ref) == 35
    sd = m.state_dict()
    for alias, k in u.ALIASES.items():                                   # one tensor under two names, as the reference registers it
        assert sd[alias].data_ptr() == sd[k].data_ptr()
    hot = m.hot_parameters()
    assert [tuple(p.shape) for p in hot] == [tuple(ref[k].shape) for k in u.PARAMS] and len({id(p) for p in hot}) == 25
    assert [k for k, _ in m.named_parameters()] == u.PARAMS and sum(p.numel() for p in hot) == 471180
    _, state = golden
    m.load_state_dict(state, strict=True)                                # the reference's 35 keys
    assert all(torch.equal(p, state[k]) for k, p in zip(u.PARAMS, m.hot_parameters()))
    enc, att = LASEncoderConfig, FixedAttentionModuleConfig
    for kw, name in ((dict(las_config=enc(hidden_size=128)), "hidden_size"), (dict(las_config=enc(num_mels=80)), "num_mels"),
                     (dict(las_config=enc(num_latent_channels=4)), "num_latent_channels"), (dict(las_config=enc(use_maxpool=False)), "use_maxpool"),
                     (dict(las_config=enc(num_layers=2)), "num_layers"), (dict(las_config=enc(num_spec_channels=1)), "num_spec_channels"),
                     (dict(fixed_attn_config=att(num_heads=2)), "num_heads"), (dict(dnn_size=128), "dnn_size")):
        with pytest.raises(NotImplementedError, match=name):
            LASClassifier(4, LASClassifierConfig(**kw))


def test_model_through_the_emulated_package(emu, golden):
    """``LASClassifier`` end to end on the emulator: strict load of G17's state, golden logits, autograd gradients, lengths
    untouched, unsorted lengths, a one-channel input and an eval-mode backward refused."""
    import emu_util
    g, state = golden
    xa, _, labels, keep = golden_case_a(g)
    with emu_util.emulated_package():
        from howl_amd.model import LASClassifier
        m = LASClassifier(4)
        m.load_state_dict(state, strict=True)
        m.eval()
        la = torch.from_numpy(g["a/lengths"]).clone()
        with torch.no_grad():
            assert u.maxerr(m(xa, la), g["a/eval_logits"]) < 5e-5
            assert u.maxerr(m(torch.from_numpy(g["b/x"]), None), g["b/eval_logits"]) < 5e-5
        assert la.tolist() == g["a/lengths"].tolist()
        with pytest.raises(RuntimeError, match="sorted in decreasing order"):
            m(xa, torch.tensor([3, 21, 17, 9, 1]))
        with pytest.raises(RuntimeError, match="three feature channels"):
            m(xa[:, :1], la)
        with pytest.raises(NotImplementedError, match="training-mode forward"):
            torch.nn.functional.cross_entropy(m(xa, la), labels).backward()
        m.train()
        m.forced_keep_mask = keep
        logits = m(xa, la)
        torch.nn.functional.cross_entropy(logits, labels).backward()
        assert u.maxerr(logits.detach(), g["a/train_logits"]) < 5e-5
        r64 = u.reference(state, xa, la.tolist(), labels, keep, train=True)
        r32 = u.reference(state, xa, la.tolist(), labels, keep, train=True, dtype=torch.float32)
        u.check_grads("LASClassifier", [p.grad for p in m.hot_parameters()], r64, r32)
        u.check_buffers("LASClassifier", m.state_dict(), {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})


# ---- bounds: every operand in a guarded mapping, each placement in a child process ----------------------------------------------------

# "-gemm": the weight gradients and the row GEMMs on the kernels howl_gemm.hip.h picks at training sizes (from 2048 rows on), made
# to take these few rows
BOUNDS_CASES = ("A", "B", "C", "one", "A-gemm")


def run_bounds(case, placement):
    """Child-process body: every operand ends at (tail) or starts behind (head) a PROT_NONE page, the workspace is exactly
    howl_las_workspace_bytes long; both feature layouts, eval and train + backward."""
    import emu_util
    from guard_mem import Arena
    if case.endswith("-gemm"):
        os.environ.update(HOWL_WGRAD_BIG_MIN_ROWS="1", HOWL_ROWGEMM_MIN_ROWS="1")
        case = case[:-5]
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    r = u.case_reference(case)
    for time_major in (False, True):
        al = Arena(placement)
        real_call = lib.call

        def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
            print(f"guard_mem: --- {name} ({case}, {placement})", file=sys.stderr)
            al.describe()
            return real_call(name, *args)
        lib.call = call
        try:
            u.run_library(lib, al, r["state"], r["x"], r["lengths"], False, x_time_major=time_major)
            tr = u.run_library(lib, al, r["state"], r["x"], r["lengths"], True, r["mask"], r["dlogits"], x_time_major=time_major)
            u.check_grads(case, tr["grads"], r["train64"], r["train32"])
        finally:
            lib.call = real_call
        al.check()


@pytest.fixture(scope="module")
def bounds_results(emu):
    from concurrent.futures import ThreadPoolExecutor
    env = dict(os.environ, OMP_NUM_THREADS="1")
    python = [sys.executable] + [flag for flag, on in (("-s", sys.flags.no_user_site), ("-E", sys.flags.ignore_environment)) if on]

    def one(job):
        try:
            p = subprocess.run(python + [__file__, *job], capture_output=True, text=True, timeout=TIMEOUT, env=env, cwd=ROOT)
            return job, p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:
            return job, "timeout", e.stdout or "", e.stderr or ""
    jobs = [(s, pl) for s in BOUNDS_CASES for pl in PLACEMENTS]
    with ThreadPoolExecutor(max_workers=6) as ex:
        return {job: r for job, *r in ex.map(one, jobs)}


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("case", BOUNDS_CASES)
def test_las_bounds(bounds_results, case, placement):
    from test_emu_bounds import name_fault
    rc, out, err = bounds_results[(case, placement)]
    if rc != 0:
        tail = "\n".join([l for l in err.splitlines() if not l.startswith("guard_mem:")][-40:])
        maps = [l for l in err.splitlines() if l.startswith("guard_mem:")]
        pytest.fail(f"{case} [{placement}] exited {rc}\n{name_fault(err)}\n{tail}\n--- last buffer map ---\n" + "\n".join(maps[-40:]),
                    pytrace=False)


if __name__ == "__main__":
    run_bounds(sys.argv[1], sys.argv[2])
    print(json.dumps({"case": sys.argv[1], "placement": sys.argv[2], "ok": True}))
