"""Streaming res8 (include/howl_hip_stream.h, howl_amd/csrc/res8_stream.hip) on the hipemu emulator: one launch from the windows'
PCM to their probabilities, against the float64 oracle with the eager chain's own error as the yardstick; independence of the
windows; the G8 labels through the engine's fused ingest_frame; header / exports / ctypes table; guard-page bounds in child
processes (as tests/test_emu_bounds.py runs its cases); staleness of the session's prepared state."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for _p in (str(ROOT), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PLACEMENTS = ("tail", "head")
TIMEOUT = 900


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena():
    from guard_mem import Arena
    return Arena("tail", log=open(os.devnull, "w"))


# ---- 1. against the fp64 oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("L", [8000, 16000])
def test_logits_against_the_fp64_oracle(emu, L, C):
    """e_fused <= 2 e_eager + 1e-6 on the logits, probs == softmax(logits) and rows summing to 1 within 1e-6 (N = 3 windows)."""
    import stream_util
    stream_util.check_against_oracle(_arena(), emu, L, C)


# ---- 2. independence -------------------------------------------------------------------------------------------------------------

def test_windows_are_independent_and_launches_repeat(emu):
    import stream_util
    stream_util.check_independence(_arena(), emu)


# ---- 3. G8 labels through the engine ---------------------------------------------------------------------------------------------

def test_fused_ingest_frame_gives_the_g8_labels(golden):
    import emu_util
    import stream_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        stream_util.check_g8_labels(golden, torch.device("cpu"), lib.get())


def test_engine_switch_defaults_off_and_follows_the_environment(golden, monkeypatch):
    import emu_util
    import stream_util
    import torch
    with emu_util.emulated_package():
        monkeypatch.delenv("HOWL_STREAM_FUSED", raising=False)
        from howl_amd.model.inference import FrameInferenceEngine
        e = stream_util.g8_engine(golden, torch.device("cpu"), fused=None)
        assert FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context).fused_windows is False
        monkeypatch.setenv("HOWL_STREAM_FUSED", "1")
        assert FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context).fused_windows is True
        # a window outside the kernel's range (2 s) keeps the launch chain
        on = FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context)
        assert on._fused_session(torch.zeros(8000)) is not None and on._fused_session(torch.zeros(32000)) is None


# ---- 4. header, exports, table ---------------------------------------------------------------------------------------------------

def header_functions():
    text = (ROOT / "include" / "howl_hip_stream.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_stream_header(built, emu):
    from howl_amd import lib
    hdr = header_functions()
    assert len(hdr) == 4, hdr
    table = set(lib.STREAM_SIGNATURES) | set(lib.STREAM_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    assert not table & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS))
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert hdr <= exported, (path, hdr - exported)
    lb = lib.Library(built)      # resolves every symbol and sets argtypes
    assert lb.cdll.howl_res8_stream_state_bytes(4) > 6 * 45 * 45 * 9 * 4 and lb.cdll.howl_res8_stream_state_bytes(65) == 0
    for L, M, C, ok in [(8000, 40, 4, 1), (16000, 40, 64, 1), (16599, 40, 4, 1), (400, 40, 1, 1), (399, 40, 4, 0), (16600, 40, 4, 0),
                        (8000, 80, 4, 0), (8000, 40, 65, 0), (8000, 40, 0, 0)]:
        assert lb.cdll.howl_res8_stream_supported(L, M, C) == ok, (L, M, C)


def test_argument_errors_name_the_entry_point(built):
    import ctypes
    from howl_amd import lib
    lb = lib.Library(built)
    with pytest.raises(lib.HowlHipError, match=r"howl_res8_stream_windows: null pointer"):
        lb.call("howl_res8_stream_windows", None, None, 8000, 1, 8000, None, 40, 1e-7, None, 4, None, None, None)
    with pytest.raises(lib.HowlHipError, match=r"howl_res8_stream_prepare: null pointer"):
        lb.call("howl_res8_stream_prepare", None, 4, None, 0, None)
    one = ctypes.c_void_p(16)      # never dereferenced: the shape is refused first
    with pytest.raises(lib.HowlHipError, match=r"howl_res8_stream_windows: L=32000 samples.*unsupported"):
        lb.call("howl_res8_stream_windows", one, one, 32000, 1, 32000, one, 40, 1e-7, None, 4, one, None, None)
    with pytest.raises(lib.HowlHipError, match=r"howl_res8_stream_windows: N=8193 windows unsupported"):
        lb.call("howl_res8_stream_windows", one, one, 0, 8193, 8000, one, 40, 1e-7, None, 4, one, None, None)
    prm = lib.HowlRes8Params()
    with pytest.raises(lib.HowlHipError, match=r"howl_res8_stream_prepare: state of 16 bytes"):
        lb.call("howl_res8_stream_prepare", ctypes.byref(prm), 4, one, 16, None)


# ---- 5. bounds: every operand in a guarded mapping, each placement in a child process ----------------------------------------------

BOUNDS_SHAPES = {"N1_L8000": (1, 8000), "N3_L8000": (3, 8000), "N3_L16000": (3, 16000), "N1_L400": (1, 400)}


def run_bounds(shape, placement):
    """Child-process body: prepare + windows with every operand ending at (tail) or starting behind (head) a PROT_NONE page; the PCM
    rows end at the guard page (ld == L), probs / logits are sentinel buffers whose promised region is exactly [N, C]."""
    import emu_util
    import stream_util
    from guard_mem import Arena
    N, L = BOUNDS_SHAPES[shape]
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    al = Arena(placement)
    real_call = lib.call

    def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
        print(f"guard_mem: --- {name} ({shape}, {placement})", file=sys.stderr)
        al.describe()
        return real_call(name, *args)
    lib.call = call
    stream_util.check_against_oracle(al, lib, L, 4, N=N, seed=N)
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
    jobs = [(s, pl) for s in BOUNDS_SHAPES for pl in PLACEMENTS]
    with ThreadPoolExecutor(max_workers=8) as ex:
        return {job: r for job, *r in ex.map(one, jobs)}


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("shape", list(BOUNDS_SHAPES))
def test_stream_bounds(bounds_results, shape, placement):
    from test_emu_bounds import name_fault
    rc, out, err = bounds_results[(shape, placement)]
    if rc != 0:
        tail = "\n".join([l for l in err.splitlines() if not l.startswith("guard_mem:")][-40:])
        maps = [l for l in err.splitlines() if l.startswith("guard_mem:")]
        pytest.fail(f"{shape} [{placement}] exited {rc}\n{name_fault(err)}\n{tail}\n--- last buffer map ---\n" + "\n".join(maps[-40:]),
                    pytrace=False)


# ---- 6. staleness ----------------------------------------------------------------------------------------------------------------

def test_session_prepares_again_after_load_state_dict():
    import emu_util
    import stream_util
    import torch
    with emu_util.emulated_package():
        stream_util.check_staleness(torch.device("cpu"))


if __name__ == "__main__":
    run_bounds(sys.argv[1], sys.argv[2])
    print(json.dumps({"shape": sys.argv[1], "placement": sys.argv[2], "ok": True}))
