"""The small-cnn and seq-cnn models (include/howl_hip_cnn.h, howl_amd/csrc/cnn.hip) on the hipemu emulator: header / exports / ctypes
tables; forward (eval, train) and every gradient against the float64 restatement of tests/cnn_util.py and against the reference's
own numbers (tests/golden/g19_small_cnn.npz, g20_seq_cnn.npz); running statistics; the same eval-mode bits whatever an utterance's
neighbours; refusals; the registry; guard-page bounds of every buffer in child processes (as tests/test_emu_gru.py runs its cases)."""
import json
import logging
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

import cnn_util as u  # noqa: E402

PLACEMENTS = ("tail", "head")
EMU_CASES = ("s26", "s40", "s41", "q5", "q22", "q81")      # "q150" and "s26b" take the emulator minutes: tests/test_gpu_cnn.py runs them
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


def load_golden(kind):
    g = np.load(u.GOLDEN[kind])
    return g, {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}


def golden_targets(kind, g):
    if kind == u.SMALL:
        return torch.from_numpy(g["a/labels"])
    return dict(targets=torch.from_numpy(g["a/targets"]), target_lengths=torch.from_numpy(g["a/target_lengths"]),
                input_lengths=torch.from_numpy(g["a/input_lengths"]))


# ---- header, exports, tables -------------------------------------------------------------------------------------------------------

def test_library_exports_the_cnn_header(built, emu):
    from howl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip_cnn.h").read_text(), flags=re.S)
    hdr = set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))
    assert hdr == {"howl_cnn_supported", "howl_cnn_workspace_bytes", "howl_cnn_out_rows", "howl_cnn_fwd", "howl_cnn_bwd"}, hdr
    table = set(lib.CNN_SIGNATURES) | set(lib.CNN_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    others = [lib.SIGNATURES, lib.SIZE_FUNCS, lib.STREAM_SIGNATURES, lib.STREAM_SIZE_FUNCS, lib.LSTM_STREAM_SIGNATURES,
              lib.LSTM_STREAM_SIZE_FUNCS, lib.DECIDE_SIGNATURES, lib.DECIDE_SIZE_FUNCS, lib.CTC_LONG_SIGNATURES, lib.CTC_LONG_SIZE_FUNCS,
              lib.GRU_SIGNATURES, lib.GRU_SIZE_FUNCS, lib.LAS_SIGNATURES, lib.LAS_SIZE_FUNCS, lib.TIMESTRETCH_SIGNATURES, lib.TIMESTRETCH_SIZE_FUNCS]
    assert not table & set().union(*others)
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert {n for n in exported if n.startswith("howl_cnn_")} == hdr, path
    # the argument counts of the header and of the tables agree, and the structs hold what the header declares
    for name, argtypes in {**lib.CNN_SIGNATURES, **lib.CNN_SIZE_FUNCS}.items():
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == len(argtypes), name
    assert len(lib.HowlCnnParams._fields_) == len(lib.HowlCnnGrads._fields_) == len(u.PARAMS) == 12
    assert len(lib.HowlCnnBuffers._fields_) == len(u.BUFFERS) == 6
    assert [f for f, _ in lib.HowlCnnParams._fields_] == re.findall(r"const float\* (\w+);", text)
    assert [f for f, _ in lib.HowlCnnBuffers._fields_] == re.findall(r"^\s*(?:float|long long)\* (bn\d_\w+);", text, flags=re.M)
    assert re.search(r"#define HOWL_CNN_MAX_FRAMES (\d+)", text).group(1) == "8192"
    assert re.search(r"#define HOWL_CNN_MAX_LABELS (\d+)", text).group(1) == "64"
    assert (int(re.search(r"#define HOWL_CNN_SMALL (\d+)", text).group(1)), int(re.search(r"#define HOWL_CNN_SEQ (\d+)", text).group(1))) == \
        (lib.CNN_SMALL, lib.CNN_SEQ) == (u.SMALL, u.SEQ)


# ---- the yardstick itself -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(u.CASES))
def test_fp32_cpu_model_is_inside_the_bounds(name):
    """The same model in fp32 on torch CPU stays inside the scores' bound, and no ReLU or max-pool decision flipped for the committed
    seeds: every decision of the float64 forward is at least ``MARGIN`` from its tie -- an fp32 convolution of 1200 terms of
    magnitude 0.03 is a few 1e-7 off -- and the fp32 model's gradient error (the ``noise`` of the gradient bound) is rounding,
    below the bound's fixed part."""
    r = u.case_reference(name)
    margin = u.decision_margin(r["kind"], r["state"], r["x"], r["mask"])
    print(f"cnn {name}: decision margin {margin:.3e}")
    assert margin > u.MARGIN, (name, margin)
    u.check_logits(name, r["eval32"]["logits"], r["eval64"], "fp32 eval")
    u.check_logits(name, r["train32"]["logits"], r["train64"], "fp32 train")
    assert torch.isfinite(r["train64"]["loss"])
    for k in u.PARAMS:
        g64 = r["train64"]["grads"][k]
        assert u.maxerr(r["train32"]["grads"][k], g64) < 2e-5 * max(1.0, float(g64.abs().max())), (name, k)


@pytest.mark.parametrize("kind", (u.SMALL, u.SEQ))
def test_restated_model_is_the_reference(kind):
    """cnn_util's float64 model on the golden state and inputs gives the reference's own numbers (fp32 there)."""
    g, state = load_golden(kind)
    xa, keep = torch.from_numpy(g["a/x"]), torch.from_numpy(g["a/keep_mask"]).float()
    r = u.reference(kind, state, xa, golden_targets(kind, g), keep, train=True)
    assert u.maxerr(r["logits"], g["a/train_logits"]) < 5e-5 and abs(float(r["loss"]) - float(g["a/loss"])) < 1e-4
    for k in u.PARAMS:
        assert u.maxerr(r["grads"][k], g["a/grad/" + k]) < 2e-5 * max(1.0, float(np.abs(g["a/grad/" + k]).max())), k
    u.check_buffers("golden", r["buffers"], {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})
    assert u.maxerr(u.reference(kind, state, xa)["logits"], g["a/eval_logits"]) < 5e-5
    assert u.maxerr(u.reference(kind, state, torch.from_numpy(g["b/x"]))["logits"], g["b/eval_logits"]) < 5e-5
    assert sorted(state) == sorted(u.RefCnn(kind, 4).state_dict())
    assert sum(v.numel() for k, v in u.RefCnn(kind, 2).state_dict().items() if k in u.PARAMS) == (132818 if kind == u.SMALL else 117458)
    if kind == u.SEQ:
        assert g["a/input_lengths"].tolist() == [u.compute_length(int(n)) for n in g["a/lengths"]] and g["a/input_lengths"].min() >= 5


# ---- parity --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", EMU_CASES)
def test_cnn_vs_fp64(emu, name):
    """Eval and train + backward against float64; the features in place (mel-major) for eval and the first training call, time-major
    for the second, which must give the same bits: repeated calls and both stride orders are bit-identical."""
    r = u.case_reference(name)
    kind = r["kind"]
    ev = u.run_library(emu, u.Plain(), kind, r["state"], r["x"], False)
    u.check_logits(name, ev["logits"], r["eval64"], "eval")
    for k in u.BUFFERS:                                                  # eval mode touches no buffer
        assert torch.equal(ev["buffers"][k], r["state"][k]), k
    tr = u.run_library(emu, u.Plain(), kind, r["state"], r["x"], True, r["mask"], r["dlogits"])
    u.check_logits(name, tr["logits"], r["train64"], "train")
    u.check_loss(name, kind, tr["logits"], r["targets"], r["train64"])
    u.check_grads(name, tr["grads"], r["train64"], r["train32"])
    u.check_buffers(name, tr["buffers"], r["train64"])
    for k in u.PARAMS:                                                   # no parameter is written
        assert torch.equal(tr["params"][k], r["state"][k]), k
    again = u.run_library(emu, u.Plain(), kind, r["state"], r["x"], True, r["mask"], r["dlogits"], x_time_major=True)
    assert torch.equal(again["logits"], tr["logits"]) and all(torch.equal(a, b) for a, b in zip(again["grads"], tr["grads"]))


@pytest.mark.parametrize("name", ("s26", "q22"))
def test_cnn_without_dropout_mask(emu, name):
    """Training mode with a null mask (p = 0): the float64 model with every unit kept and scale 1."""
    r = u.case_reference(name)
    kind = r["kind"]
    r64 = u.reference(kind, r["state"], r["x"], r["targets"], None, train=True)
    r32 = u.reference(kind, r["state"], r["x"], r["targets"], None, train=True, dtype=torch.float32)
    z = r64["logits"].clone().requires_grad_(True)
    u.loss_of(kind, z, r["targets"]).backward()
    tr = u.run_library(emu, u.Plain(), kind, r["state"], r["x"], True, None, z.grad.float())
    u.check_logits(name, tr["logits"], r64, "train, no mask")
    u.check_grads(name + " no mask", tr["grads"], r64, r32)


@pytest.mark.parametrize("kind", (u.SMALL, u.SEQ))
def test_cnn_vs_golden(emu, kind):
    g, state = load_golden(kind)
    xa, keep, targets = torch.from_numpy(g["a/x"]), torch.from_numpy(g["a/keep_mask"]).float(), golden_targets(kind, g)
    u.check_logits("golden A", u.run_library(emu, u.Plain(), kind, state, xa.expand(-1, 3, -1, -1).contiguous(), False)["logits"],
                   {"logits": torch.from_numpy(g["a/eval_logits"])}, "eval")
    u.check_logits("golden B", u.run_library(emu, u.Plain(), kind, state, torch.from_numpy(g["b/x"]).expand(-1, 3, -1, -1).contiguous(), False)["logits"],
                   {"logits": torch.from_numpy(g["b/eval_logits"])}, "eval")
    r64 = u.reference(kind, state, xa, targets, keep, train=True)
    r32 = u.reference(kind, state, xa, targets, keep, train=True, dtype=torch.float32)
    z = r64["logits"].clone().requires_grad_(True)
    u.loss_of(kind, z, targets).backward()
    tr = u.run_library(emu, u.Plain(), kind, state, xa.expand(-1, 3, -1, -1).contiguous(), True, keep, z.grad.float())
    gold = {"logits": torch.from_numpy(g["a/train_logits"]), "loss": torch.from_numpy(g["a/loss"])}
    u.check_logits("golden A", tr["logits"], gold, "train")
    u.check_loss("golden A", kind, tr["logits"], targets, gold)
    u.check_grads("golden A", tr["grads"], r64, r32)
    for k, got in zip(u.PARAMS, tr["grads"]):      # and the reference's own gradients (fp32 there, 16 mantissa bits recorded)
        ref = g["a/grad/" + k]
        assert u.maxerr(got.reshape(ref.shape), ref) < 4e-5 * max(1.0, float(np.abs(ref).max())), k
    u.check_buffers("golden A", tr["buffers"], {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})


# ---- the same bits whatever the neighbours ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("s26", "q22"))
def test_eval_logits_do_not_depend_on_the_batch(emu, name):
    r = u.case_reference(name)
    kind = r["kind"]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 3, 40, r["x"].shape[-1], generator=g)
    alone = u.run_library(emu, u.Plain(), kind, r["state"], r["x"][:1], False)["logits"]
    for pos in range(3):
        xx = x.clone()
        xx[pos] = r["x"][0]
        got = u.run_library(emu, u.Plain(), kind, r["state"], xx, False)["logits"]
        assert torch.equal(got[pos] if kind == u.SMALL else got[:, pos], alone[0] if kind == u.SMALL else alone[:, 0]), pos


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", (u.SMALL, u.SEQ))
def test_cnn_refusals(emu, kind):
    from guard_mem import Arena
    u.check_refusals(emu, Arena("tail", log=open(os.devnull, "w")), kind)


# ---- registry and model -----------------------------------------------------------------------------------------------------------------

def test_model_registry_and_config(emu, caplog, monkeypatch):
    from howl_amd.model import CnnSettings, RegisteredModel, SequentialCnn, SmallCnn
    monkeypatch.delenv("NUM_LABELS", raising=False)
    assert RegisteredModel.find_registered_class("small-cnn") is SmallCnn and RegisteredModel.find_registered_class("seq-cnn") is SequentialCnn
    # every name the reference's registry has
    assert {"converted", "mobilenet", "small-cnn", "seq-cnn", "res8", "seq-lstm", "lstm", "gru", "las"} <= set(RegisteredModel.registered_names())
    cfg = CnnSettings()
    assert (cfg.num_labels, cfg.num_maps1, cfg.num_maps2, cfg.num_hidden_input, cfg.hidden_size) == (2, 48, 64, 384, 128)
    monkeypatch.setenv("NUM_LABELS", "7")
    assert CnnSettings().num_labels == 7
    monkeypatch.delenv("NUM_LABELS")
    for cls, kind, count in ((SmallCnn, u.SMALL, 132818), (SequentialCnn, u.SEQ, 117458)):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            m = cls(2)
        assert not caplog.records                                        # the constructor argument and NUM_LABELS agree
        assert list(m.state_dict()) == list(u.RefCnn(kind, 2).state_dict())
        assert sum(p.numel() for p in m.parameters()) == count
        assert [tuple(p.shape) for p in m.hot_parameters()] == [tuple(u.RefCnn(kind, 2).state_dict()[k].shape) for k in u.PARAMS]
        with caplog.at_level(logging.WARNING):
            m = cls(4)                                                   # the reference's quirk: the head keeps config.num_labels
        assert any("NUM_LABELS" in rec.getMessage() for rec in caplog.records)
        assert m.output[3].out_features == 2 and m.num_labels == 2
        from howl_amd.model.cnn import require_supported_labels
        with pytest.raises(ValueError, match="NUM_LABELS"):
            require_supported_labels(m)
        m = cls(4, CnnSettings(num_labels=4))
        require_supported_labels(m)
        _, state = load_golden(kind)
        m.load_state_dict(state, strict=True)
        with pytest.raises(NotImplementedError, match="num_maps1"):
            cls(2, CnnSettings(num_maps1=32))
    import emu_util
    with emu_util.emulated_package():
        m = SequentialCnn(2)
        for T in range(5, 301):
            assert m.compute_length(T) == SequentialCnn.out_rows(T) == u.compute_length(T), T
        assert m.compute_length(81) == 10 and m.compute_length(5) == 1
        lengths = torch.arange(5, 301)
        assert SequentialCnn.output_lengths(lengths).tolist() == [m.compute_length(int(T)) for T in lengths]
        assert [T for T in range(1, 60) if SmallCnn.out_rows(T)] == list(range(26, 42)) and SmallCnn.out_rows(40) == 2


@pytest.mark.parametrize("kind", (u.SMALL, u.SEQ))
def test_model_through_the_emulated_package(emu, kind):
    """Both classes end to end on the emulator: strict load of the golden state, golden scores, autograd gradients, the
    ``_fwd_version`` guard, inputs outside the range and an eval-mode backward refused."""
    import emu_util
    g, state = load_golden(kind)
    xa, keep, targets = torch.from_numpy(g["a/x"]), torch.from_numpy(g["a/keep_mask"]).float(), golden_targets(kind, g)
    with emu_util.emulated_package():
        from howl_amd.model import CnnSettings, SequentialCnn, SmallCnn
        m = (SmallCnn if kind == u.SMALL else SequentialCnn)(4, CnnSettings(num_labels=4))
        m.load_state_dict(state, strict=True)
        m.eval()
        with torch.no_grad():
            assert u.maxerr(m(xa, None), g["a/eval_logits"]) < 5e-5
            assert u.maxerr(m(torch.from_numpy(g["b/x"]), None), g["b/eval_logits"]) < 5e-5
        for T, text in ((25, "26..41"), (42, "26..41")) if kind == u.SMALL else ((4, "5..8192"),):
            with pytest.raises(ValueError, match=text):
                m(torch.zeros(1, 1, 40, T), None)
        with pytest.raises(ValueError, match="NUM_MELS=40"):
            m(torch.zeros(1, 1, 80, 40), None)
        with pytest.raises(NotImplementedError, match="training-mode forward"):
            u.loss_of(kind, m(xa, None), targets).backward()
        m.train()
        m.forced_keep_mask = keep
        stale = m(xa, None)
        logits = m(xa, None)
        with pytest.raises(RuntimeError, match="newer forward"):
            u.loss_of(kind, stale, targets).backward()
        logits = m(xa, None)
        u.loss_of(kind, logits, targets).backward()
        assert u.maxerr(logits.detach(), g["a/train_logits"]) < 5e-5
        r64 = u.reference(kind, state, xa, targets, keep, train=True)
        r32 = u.reference(kind, state, xa, targets, keep, train=True, dtype=torch.float32)
        u.check_grads(m.NAME, [p.grad for p in m.hot_parameters()], r64, r32)
        assert int(m.encoder1[3].num_batches_tracked) == 3 + 3


# ---- bounds: every operand in a guarded mapping, each placement in a child process ----------------------------------------------------

# "-gemm": the head's weight gradients on the kernels howl_gemm.hip.h picks at training sizes (from 2048 rows on), made to take
# these few rows
BOUNDS_CASES = ("s26", "s41", "q5", "q22", "q81", "q22-gemm")


def run_bounds(case, placement):
    """Child-process body: every operand ends at (tail) or starts behind (head) a PROT_NONE page, the workspace is exactly
    howl_cnn_workspace_bytes long; both feature layouts, eval and train + backward."""
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
            if not time_major:
                u.run_library(lib, al, r["kind"], r["state"], r["x"], False)
            tr = u.run_library(lib, al, r["kind"], r["state"], r["x"], True, r["mask"], r["dlogits"], x_time_major=time_major)
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
def test_cnn_bounds(bounds_results, case, placement):
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
