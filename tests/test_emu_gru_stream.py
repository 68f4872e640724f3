"""Streaming gru (include/howl_hip_gru_stream.h, howl_amd/csrc/gru_stream.hip) on the hipemu emulator: one launch from the windows'
PCM to their probabilities, against the float64 oracle with the eager chain's own error as the yardstick, every operand in a
guarded mapping (tests/guard_mem.py Arena); independence of the windows; refusals; the G8 clip through the engine's fused
ingest_frame; the session reads the model in place; header / exports / ctypes tables.  The launch of 257 windows (more workgroups
than compute units) is the device's business: tests/test_gpu_gru_stream.py."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for _p in (str(ROOT), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gru_stream_util  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena(placement="tail"):
    from guard_mem import Arena
    return Arena(placement, log=open(os.devnull, "w"))


# ---- 1 / 3. against the fp64 oracle, every operand in a guarded mapping -------------------------------------------------------------

@pytest.mark.parametrize("N,L,C,variant", gru_stream_util.CASES, ids=gru_stream_util.CASE_IDS)
def test_logits_against_the_fp64_oracle(emu, N, L, C, variant):
    """e_fused <= 2 e_eager + 1e-6 on the logits, probs == softmax(logits) and rows summing to 1 within 1e-6; every operand ends at
    a PROT_NONE page, exactly [N, C] written, canaries intact."""
    gru_stream_util.check_against_oracle(_arena(), emu, N, L, C, variant)


@pytest.mark.parametrize("N,L,C", [(1, 512, 4), (3, 16599, 64)])
def test_no_operand_is_read_below_its_start(emu, N, L, C):
    """The smallest and the largest case again with every operand starting right behind a PROT_NONE page."""
    gru_stream_util.check_against_oracle(_arena("head"), emu, N, L, C)


# ---- 2. independence -------------------------------------------------------------------------------------------------------------

def test_windows_are_independent_and_launches_repeat(emu):
    gru_stream_util.check_independence(_arena(), emu, many=0)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_point_and_write_nothing(emu):
    gru_stream_util.check_refusals(_arena(), emu)


# ---- 5. through the engine -------------------------------------------------------------------------------------------------------

def test_fused_and_eager_ingest_frame_agree_over_the_g8_clip(golden):
    """The oracle's conditions over all 37 windows; the engine itself over the first five (the device test runs all 37)."""
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        gru_stream_util.check_engine(golden, torch.device("cpu"), lib.get(), first=5)


def test_engine_switch_is_opt_in(golden, monkeypatch):
    import emu_util
    import torch
    with emu_util.emulated_package():
        monkeypatch.delenv("HOWL_STREAM_FUSED", raising=False)
        from howl_amd.model.inference import FrameInferenceEngine
        from howl_amd.model.rnn import GruStreamSession
        e = gru_stream_util.gru_engine(golden, torch.device("cpu"), fused=None)
        assert FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context).fused_windows is False
        monkeypatch.setenv("HOWL_STREAM_FUSED", "1")
        on = FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context)
        assert on.fused_windows is True
        on.std = on.std.to(torch.device("cpu"))
        # a window outside the kernel's range (2 s) keeps the launch chain
        assert isinstance(on._fused_session(torch.zeros(8000)), GruStreamSession) and on._fused_session(torch.zeros(32000)) is None


# ---- 6. the session sees every write ---------------------------------------------------------------------------------------------

def test_session_answers_for_the_weights_as_they_are():
    import emu_util
    import torch
    with emu_util.emulated_package():
        gru_stream_util.check_session(torch.device("cpu"))


# ---- 7. header, exports, tables --------------------------------------------------------------------------------------------------

def header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip_gru_stream.h").read_text(), flags=re.S)


def header_functions():
    return set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", header_text()))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_gru_stream_header(built, emu):
    from howl_amd import lib
    hdr = header_functions()
    assert hdr == {"howl_gru_stream_supported", "howl_gru_stream_workspace_bytes", "howl_gru_stream_windows"}, hdr
    table = set(lib.GRU_STREAM_SIGNATURES) | set(lib.GRU_STREAM_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    others = [getattr(lib, n) for n in dir(lib) if (n.endswith("SIGNATURES") or n.endswith("SIZE_FUNCS")) and not n.startswith("GRU_STREAM_")]
    assert len(others) >= 20 and all(isinstance(t, dict) for t in others)
    assert not any(table & set(t) for t in others)
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" [TW] (howl_gru_stream_[a-z0-9_]+)\n", out))      # (weak definitions: gru_stream.hip says why)
        assert exported == hdr, (path, hdr ^ exported)
    # the argument counts of the header and of the tables agree
    text = header_text()
    for name, argtypes in {**lib.GRU_STREAM_SIGNATURES, **lib.GRU_STREAM_SIZE_FUNCS}.items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(argtypes), (name, args)
    lb = lib.Library(built)      # resolves every symbol and sets argtypes
    assert lb.cdll.howl_gru_stream_supported(8000, 40, 12) == 1 and lb.cdll.howl_gru_stream_supported(8000, 80, 12) == 0
    assert lb.cdll.howl_gru_stream_workspace_bytes(2, 8000) == 2 * lb.cdll.howl_gru_stream_workspace_bytes(1, 8000) > 0
