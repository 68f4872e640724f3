"""Streaming small-cnn / seq-cnn (include/howl_hip_cnn_stream.h, howl_amd/csrc/cnn_stream.hip) on the hipemu emulator: one launch
from the PCM to the probabilities, against the float64 oracle with the eager chain's own error as the yardstick, every operand in a
guarded mapping (tests/guard_mem.py Arena); seq-cnn clips on the seams of the kernel's row tile; independence; refusals and range
tables; both engines with the switch on and off; the sessions read the model in place; header / exports / ctypes tables.  The
clip of 1,638,399 samples and the launch of 257 windows are the device's business: tests/test_gpu_cnn_stream.py."""
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

import cnn_stream_util as u  # noqa: E402
from cnn_util import SEQ, SMALL  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena(placement="tail"):
    from guard_mem import Arena
    return Arena(placement, log=open(os.devnull, "w"))


# ---- against the fp64 oracle, every operand in a guarded mapping ----------------------------------------------------------------

@pytest.mark.parametrize("case", u.SMALL_CASES, ids=u.small_id)
def test_small_cnn_logits_against_the_fp64_oracle(emu, case):
    """e_fused <= 2 e_eager + 1e-6 on the logits, probs == softmax(logits) and rows summing to 1 within 1e-6; every operand ends at
    a PROT_NONE page, exactly [N, C] written, canaries intact."""
    N, L, C, variant = case
    u.check_small(_arena(), emu, N, L, C, variant)


@pytest.mark.parametrize("case", u.SEQ_CASES, ids=u.seq_id)
def test_seq_cnn_logits_against_the_fp64_oracle(emu, case):
    """The same bound over every row of every clip, tile seams included; rows behind a clip's own are zeros; exactly
    (N, rows(L_max), C) written."""
    sizes, C, variant = case
    u.check_seq(_arena(), emu, sizes, C, variant)


def test_no_operand_is_read_below_its_start(emu):
    """The smallest and the largest small-cnn case and the shortest and the three-tile seq-cnn clip again with every operand starting
    right behind a PROT_NONE page."""
    u.check_small(_arena("head"), emu, *u.SMALL_CASES[0])
    u.check_small(_arena("head"), emu, *u.SMALL_CASES[3])
    u.check_seq(_arena("head"), emu, *u.SEQ_CASES[0])
    u.check_seq(_arena("head"), emu, *u.SEQ_CASES[13])
    assert u.rows_of(u.SEQ_CASES[0][0][0]) == 1 and u.rows_of(u.SEQ_CASES[13][0][0]) == 2 * u.R + 1


# ---- independence ---------------------------------------------------------------------------------------------------------------

def test_windows_are_independent_and_launches_repeat(emu):
    u.check_small_independence(_arena(), emu, many=0)


def test_clips_are_independent_of_their_launch(emu):
    u.check_seq_independence(_arena(), emu)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [SMALL, SEQ], ids=["small", "seq"])
def test_refusals_name_the_entry_point_and_write_nothing(emu, kind):
    u.check_refusals(_arena(), emu, kind)


def test_range_tables_have_zeros_at_every_edge(emu):
    u.check_tables(emu)


# ---- through the engines --------------------------------------------------------------------------------------------------------

def test_fused_and_eager_ingest_frame_agree_over_the_g8_clip(golden):
    """The oracle's conditions over all 37 windows; the engine itself over the first five (the device test runs all 37)."""
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_small_engine(golden, torch.device("cpu"), lib.get(), first=5)


def test_frame_engine_switch_is_opt_in(golden, monkeypatch):
    import emu_util
    import torch
    with emu_util.emulated_package():
        u.check_small_switch(golden, torch.device("cpu"), monkeypatch)


def test_fused_and_eager_infer_agree_on_two_chunks(golden):
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_seq_infer(golden, torch.device("cpu"), lib.get())


def test_infer_many_matches_the_per_clip_loop(golden):
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_seq_infer_many(golden, torch.device("cpu"), lib.get())


def test_lstm_session_counts_one_row_per_frame():
    from howl_amd.model.rnn import LstmStreamSession
    assert [LstmStreamSession.rows_of(n) for n in (400, 799, 800, 16000)] == [3, 4, 5, 81]


# ---- the sessions see every write -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [SMALL, SEQ], ids=["small", "seq"])
def test_session_answers_for_the_weights_as_they_are(kind):
    import emu_util
    import torch
    with emu_util.emulated_package():
        u.check_session(kind, torch.device("cpu"))


# ---- header, exports, tables ----------------------------------------------------------------------------------------------------

def header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip_cnn_stream.h").read_text(), flags=re.S)


def header_functions():
    return set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", header_text()))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_cnn_stream_header(built, emu):
    from howl_amd import lib
    hdr = header_functions()
    assert hdr == {"howl_cnn_stream_supported", "howl_cnn_stream_workspace_bytes", "howl_cnn_stream_rows", "howl_cnn_stream_windows",
                   "howl_cnn_stream_clips"}, hdr
    table = set(lib.CNN_STREAM_SIGNATURES) | set(lib.CNN_STREAM_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    others = [getattr(lib, n) for n in dir(lib) if (n.endswith("SIGNATURES") or n.endswith("SIZE_FUNCS")) and not n.startswith("CNN_STREAM_")]
    assert len(others) >= 22 and all(isinstance(t, dict) for t in others)
    assert not any(table & set(t) for t in others)
    assert lib.CNN_STREAM_TILE_ROWS == u.R
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" [TW] (howl_cnn_stream_[a-z0-9_]+)\n", out))      # (weak definitions: cnn_stream.hip says why)
        assert exported == hdr, (path, hdr ^ exported)
    # the argument counts of the header and of the tables agree
    text = header_text()
    for name, argtypes in {**lib.CNN_STREAM_SIGNATURES, **lib.CNN_STREAM_SIZE_FUNCS}.items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(argtypes), (name, args)
    lb = lib.Library(built)      # resolves every symbol and sets argtypes
    assert lb.cdll.howl_cnn_stream_supported(SMALL, 8000, 40, 12) == 1 and lb.cdll.howl_cnn_stream_supported(SMALL, 8000, 80, 12) == 0
    assert lb.cdll.howl_cnn_stream_rows(SEQ, 16000) == 10 and lb.cdll.howl_cnn_stream_workspace_bytes(SEQ, 2, 16000) == 16
