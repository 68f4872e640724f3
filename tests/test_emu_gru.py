"""The gru model (include/howl_hip_gru.h, howl_amd/csrc/gru.hip) on the hipemu emulator: header / exports / ctypes tables; forward
(eval, train) and every gradient against the float64 restatement of tests/gru_util.py and against the reference's own numbers
(tests/golden/g16_gru.npz); running statistics; the same eval-mode bits whatever an utterance's neighbours; refusals; guard-page
bounds of every buffer in child processes (as tests/test_emu_ctc_long.py runs its cases)."""
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

import gru_util as u  # noqa: E402

PLACEMENTS = ("tail", "head")
EMU_CASES = ("A", "B", "one")      # "window" (B = 9, T = 101) takes the emulator ~20 s: tests/test_gpu_gru.py runs it
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
    g = np.load(u.GOLDEN)
    return g, {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}


# ---- header, exports, tables -------------------------------------------------------------------------------------------------------

def test_library_exports_the_gru_header(built, emu):
    from howl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip_gru.h").read_text(), flags=re.S)
    hdr = set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))
    assert hdr == {"howl_gru_supported", "howl_gru_workspace_bytes", "howl_gru_fwd", "howl_gru_bwd"}, hdr
    table = set(lib.GRU_SIGNATURES) | set(lib.GRU_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    others = [lib.SIGNATURES, lib.SIZE_FUNCS, lib.STREAM_SIGNATURES, lib.STREAM_SIZE_FUNCS, lib.LSTM_STREAM_SIGNATURES,
              lib.LSTM_STREAM_SIZE_FUNCS, lib.DECIDE_SIGNATURES, lib.DECIDE_SIZE_FUNCS, lib.CTC_LONG_SIGNATURES, lib.CTC_LONG_SIZE_FUNCS]
    assert not table & set().union(*others)
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert {n for n in exported if n.startswith("howl_gru_")} == hdr, path
    # the argument counts of the header and of the tables agree, and the structs hold what the header declares
    for name, argtypes in {**lib.GRU_SIGNATURES, **lib.GRU_SIZE_FUNCS}.items():
        args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == len(argtypes), name
    assert len(lib.HowlGruParams._fields_) == len(lib.HowlGruGrads._fields_) == len(u.PARAMS) == 16
    assert len(lib.HowlGruBuffers._fields_) == len(u.BUFFERS) == 6
    assert [f for f, _ in lib.HowlGruParams._fields_] == re.findall(r"const float\* (\w+);", text)
    assert re.search(r"#define HOWL_GRU_MAX_FRAMES (\d+)", text).group(1) == "8192"


# ---- the yardstick itself -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("A", "B", "one", "window"))
def test_fp32_cpu_model_is_inside_the_bounds(name):
    """The same model in fp32 on torch CPU stays inside the logits / loss bounds, and no ReLU or max-pool decision flipped for the
    committed seeds: its gradient error (the ``noise`` of the gradient bound) is rounding, below the bound's fixed part."""
    r = u.case_reference(name)
    u.check_logits(name, r["eval32"]["logits"], r["eval64"], "fp32 eval")
    u.check_logits(name, r["train32"]["logits"], r["train64"], "fp32 train")
    for k in u.PARAMS:
        g64 = r["train64"]["grads"][k]
        assert u.maxerr(r["train32"]["grads"][k], g64) < 2e-5 * max(1.0, float(g64.abs().max())), (name, k)


def test_restated_model_is_the_reference(golden):
    """gru_util's float64 model on G16's state and inputs gives the reference's own numbers (fp32 there)."""
    g, state = golden
    xa, la, labels, keep = torch.from_numpy(g["a/x"]), g["a/lengths"].tolist(), torch.from_numpy(g["a/labels"]), torch.from_numpy(g["a/keep_mask"])
    r = u.reference(state, xa, la, labels, keep, train=True)
    assert u.maxerr(r["logits"], g["a/train_logits"]) < 5e-5 and abs(float(r["loss"]) - float(g["a/loss"])) < 1e-4
    for k in u.PARAMS:
        assert u.maxerr(r["grads"][k], g["a/grad/" + k]) < 2e-5 * max(1.0, float(np.abs(g["a/grad/" + k]).max())), k
    assert u.maxerr(u.reference(state, torch.from_numpy(g["b/x"]), None)["logits"], g["b/eval_logits"]) < 5e-5
    assert sorted(state) == sorted(u.RefGru(4).state_dict())


# ---- parity --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("time_major", (False, True))
@pytest.mark.parametrize("name", EMU_CASES)
def test_gru_vs_fp64(emu, name, time_major):
    r = u.case_reference(name)
    ev = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], False, x_time_major=time_major)
    u.check_logits(name, ev["logits"], r["eval64"], "eval")
    for k in u.BUFFERS:                                                  # eval mode touches no buffer
        assert torch.equal(ev["buffers"][k], r["state"][k]), k
    tr = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], True, r["mask"], r["dlogits"], x_time_major=time_major)
    u.check_logits(name, tr["logits"], r["train64"], "train")
    u.check_loss(name, tr["logits"], r["labels"], r["train64"])
    u.check_grads(name, tr["grads"], r["train64"], r["train32"])
    u.check_buffers(name, tr["buffers"], r["train64"])
    for k in u.PARAMS:                                                   # no parameter is written
        assert torch.equal(tr["params"][k], r["state"][k]), k
    again = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], True, r["mask"], r["dlogits"], x_time_major=time_major)
    assert torch.equal(again["logits"], tr["logits"]) and all(torch.equal(a, b) for a, b in zip(again["grads"], tr["grads"]))


def test_gru_without_dropout_mask(emu):
    """Training mode with a null mask (p = 0): the float64 model with every unit kept and scale 1."""
    r = u.case_reference("A")
    r64 = u.reference(r["state"], r["x"], r["lengths"], r["labels"], None, train=True)
    r32 = u.reference(r["state"], r["x"], r["lengths"], r["labels"], None, train=True, dtype=torch.float32)
    z = r64["logits"].clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(z, r["labels"]).backward()
    tr = u.run_library(emu, u.Plain(), r["state"], r["x"], r["lengths"], True, None, z.grad.float())
    u.check_logits("A", tr["logits"], r64, "train, no mask")
    u.check_grads("A no mask", tr["grads"], r64, r32)


def test_gru_vs_golden(emu, golden):
    g, state = golden
    xa, la, labels = torch.from_numpy(g["a/x"]), g["a/lengths"].tolist(), torch.from_numpy(g["a/labels"])
    keep = torch.from_numpy(g["a/keep_mask"])
    u.check_logits("G16 A", u.run_library(emu, u.Plain(), state, xa, la, False)["logits"], {"logits": torch.from_numpy(g["a/eval_logits"])}, "eval")
    u.check_logits("G16 B", u.run_library(emu, u.Plain(), state, torch.from_numpy(g["b/x"]), None, False)["logits"],
                   {"logits": torch.from_numpy(g["b/eval_logits"])}, "eval")
    r64 = u.reference(state, xa, la, labels, keep, train=True)
    r32 = u.reference(state, xa, la, labels, keep, train=True, dtype=torch.float32)
    z = r64["logits"].clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(z, labels).backward()
    tr = u.run_library(emu, u.Plain(), state, xa, la, True, keep, z.grad.float())
    gold = {"logits": torch.from_numpy(g["a/train_logits"]), "loss": torch.from_numpy(g["a/loss"])}
    u.check_logits("G16 A", tr["logits"], gold, "train")
    u.check_loss("G16 A", tr["logits"], labels, gold)
    u.check_grads("G16 A", tr["grads"], r64, r32)
    u.check_buffers("G16 A", tr["buffers"], {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})


# ---- the same bits whatever the neighbours ---------------------------------------------------------------------------------------------

def test_eval_logits_do_not_depend_on_the_batch(emu):
    """Utterance 2 of case A (9 frames of 21) alone, and at every position among a workgroup's four with other neighbours."""
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

def test_gru_refusals(emu):
    from guard_mem import Arena
    u.check_refusals(emu, Arena("tail", log=open(os.devnull, "w")))


def test_model_registry_and_config():
    from howl_amd.model import LASEncoderConfig, RegisteredModel, SimpleGru
    assert "gru" in RegisteredModel.registered_names() and RegisteredModel.find_registered_class("gru") is SimpleGru
    cfg = LASEncoderConfig()
    assert (cfg.num_mels, cfg.num_spec_channels, cfg.num_latent_channels, cfg.hidden_size, cfg.num_layers, cfg.use_maxpool) == (40, 3, 8, 96, 1, True)
    m = SimpleGru(4)
    assert list(m.state_dict()) == list(u.RefGru(4).state_dict())
    assert [tuple(p.shape) for p in m.hot_parameters()] == [tuple(u.RefGru(4).state_dict()[k].shape) for k in u.PARAMS]
    for kw, name in ((dict(hidden_size=128), "hidden_size"), (dict(num_mels=80), "num_mels"), (dict(num_latent_channels=4), "num_latent_channels"),
                     (dict(use_maxpool=False), "use_maxpool")):
        with pytest.raises(NotImplementedError, match=name):
            SimpleGru(4, LASEncoderConfig(**kw))


def test_model_through_the_emulated_package(emu, golden):
    """``SimpleGru`` end to end on the emulator: strict load of G16's state, golden logits, autograd gradients, lengths untouched,
    unsorted lengths and an eval-mode backward refused."""
    import emu_util
    g, state = golden
    xa, labels, keep = torch.from_numpy(g["a/x"]), torch.from_numpy(g["a/labels"]), torch.from_numpy(g["a/keep_mask"])
    with emu_util.emulated_package():
        from howl_amd.model import SimpleGru
        m = SimpleGru(4)
        m.load_state_dict(state, strict=True)
        m.eval()
        la = torch.from_numpy(g["a/lengths"]).clone()
        with torch.no_grad():
            assert u.maxerr(m(xa, la), g["a/eval_logits"]) < 5e-5
            assert u.maxerr(m(torch.from_numpy(g["b/x"]), None), g["b/eval_logits"]) < 5e-5
        assert la.tolist() == g["a/lengths"].tolist()
        with pytest.raises(RuntimeError, match="sorted in decreasing order"):
            m(xa, torch.tensor([3, 21, 17, 9, 1]))
        with pytest.raises(NotImplementedError, match="training-mode forward"):
            torch.nn.functional.cross_entropy(m(xa, la), labels).backward()
        m.train()
        m.forced_keep_mask = keep
        logits = m(xa, la)
        torch.nn.functional.cross_entropy(logits, labels).backward()
        assert u.maxerr(logits.detach(), g["a/train_logits"]) < 5e-5
        r64 = u.reference(state, xa, la.tolist(), labels, keep, train=True)
        r32 = u.reference(state, xa, la.tolist(), labels, keep, train=True, dtype=torch.float32)
        u.check_grads("SimpleGru", [p.grad for p in m.hot_parameters()], r64, r32)
        u.check_buffers("SimpleGru", m.state_dict(), {"buffers": {k: torch.from_numpy(g["a/after/" + k]) for k in u.BUFFERS}})


# ---- bounds: every operand in a guarded mapping, each placement in a child process ----------------------------------------------------

# "-gemm": the weight gradients and dX^ on the kernels howl_gemm.hip.h picks at training sizes (from 2048 rows on), made to
# take these few rows
BOUNDS_CASES = ("A", "B", "one", "A-gemm")


def run_bounds(case, placement):
    """Child-process body: every operand ends at (tail) or starts behind (head) a PROT_NONE page, the workspace is exactly
    howl_gru_workspace_bytes long; both feature layouts, eval and train + backward."""
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
def test_gru_bounds(bounds_results, case, placement):
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
