"""Streaming seq-lstm / lstm (include/howl_hip_lstm_stream.h, howl_amd/csrc/lstm_stream.hip) on the hipemu emulator: one launch
from N ragged PCM chunks to their frame probabilities and carried state, against the float64 oracle with the eager chain's own
error as the yardstick; state carry; independence of the streams; the engines (G8 history, infer_many, the frame engine with
`lstm`); header / exports / ctypes tables; guard-page bounds in child processes (as tests/test_emu_bounds.py runs its cases)."""
import json
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

PLACEMENTS = ("tail", "head")
TIMEOUT = 1800
W = 16      # the kernel's window: frame counts of exactly W, W + 1 and 2 W + 3 are 3000..3199, 3200..3399 and 6800..6999 samples


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena():
    from guard_mem import Arena
    return Arena("tail", log=open(os.devnull, "w"))


# ---- 1. against the fp64 oracle ------------------------------------------------------------------------------------------------

ORACLE_CASES = {
    # name: (n_samples per stream, C, start state, ZMUV, last_only)
    "N1_C3": ([8000], 3, False, True, False),
    "N3_C5_state": ([400, 4321, 3200], 5, True, True, False),                    # 3 frames; W + 1 frames
    "N4_C12": ([16000, 1000, 3000, 6800], 12, False, True, False),                # W and 2 W + 3 frames
    "N5_C5_no_zmuv": ([8000, 3199, 3399, 6999, 1000], 5, True, False, False),
    "N9_C3": ([4321, 400, 8000, 3000, 1000, 3200, 6800, 16000, 2345], 3, False, True, False),
    "N1_C5_last_only": ([8000], 5, False, True, True),
    "N5_C12_last_only_state": ([8000, 3000, 3400, 7000, 1000], 12, True, True, True),
    "N3_C3_last_only_no_zmuv": ([1000, 16000, 4321], 3, False, False, True),      # (compute_lengths needs >= 712 samples)
}


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_logits_and_state_against_the_fp64_oracle(emu, case):
    """e_fused <= 2 e_eager + 1e-6 on the logits and on (h, c); probs == softmax(logits) and rows summing to 1 within 1e-6; rows
    past a stream's frame count exactly zero."""
    import lstm_stream_util as u
    lengths, C, state, zmuv, last_only = ORACLE_CASES[case]
    assert [u.num_frames(n) for n in (3000, 3200, 6800)] == [W, W + 1, 2 * W + 3]
    u.check_case(_arena(), emu, lengths, C, state=state, zmuv=zmuv, last_only=last_only, what=case + ".")


# ---- 2. state carry ----------------------------------------------------------------------------------------------------------------

def test_state_carried_over_two_chunks_of_the_g15_clips(emu, golden):
    import lstm_stream_util as u
    u.check_state_carry(_arena(), emu, golden)


# ---- 3. independence and repeatability -----------------------------------------------------------------------------------------------

def test_streams_are_independent_and_launches_repeat(emu):
    import lstm_stream_util as u
    u.check_independence(_arena(), emu)


# ---- 4. / 5. the engines -------------------------------------------------------------------------------------------------------------

def test_fused_infer_gives_the_g8_history_in_one_launch(golden):
    import emu_util
    import lstm_stream_util as u
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_g8_history(golden, torch.device("cpu"), lib.get())


def test_infer_many_equals_the_clip_by_clip_loop(golden):
    import emu_util
    import lstm_stream_util as u
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_infer_many(golden, torch.device("cpu"), lib.get())


def test_switch_defaults_off_and_the_call_log_is_todays(golden, monkeypatch):
    import emu_util
    import lstm_stream_util as u
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_switch_default(golden, torch.device("cpu"), lib.get(), monkeypatch)


def test_frame_engine_with_lstm_one_launch_per_window(golden):
    import emu_util
    import lstm_stream_util as u
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_frame_engine_lstm(golden, torch.device("cpu"), lib.get())


def test_fused_and_eager_calls_alternate_on_one_streaming_model(golden):
    import emu_util
    import lstm_stream_util as u
    import torch
    with emu_util.emulated_package():
        u.check_streaming_alternation(golden, torch.device("cpu"))


def test_session_contract(golden):
    import emu_util
    import lstm_stream_util as u
    import torch
    with emu_util.emulated_package():
        u.check_session(golden, torch.device("cpu"))


# ---- 6. header, exports, tables ------------------------------------------------------------------------------------------------------

def header_functions():
    text = (ROOT / "include" / "howl_hip_lstm_stream.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_lstm_stream_header(built, emu):
    from howl_amd import lib
    hdr = header_functions()
    assert hdr == {"howl_lstm_stream_supported", "howl_lstm_stream_chunks"}, hdr
    table = set(lib.LSTM_STREAM_SIGNATURES) | set(lib.LSTM_STREAM_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    assert not table & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS) | set(lib.STREAM_SIGNATURES) | set(lib.STREAM_SIZE_FUNCS))
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert hdr <= exported, (path, hdr - exported)
    lb = lib.Library(built)      # resolves every symbol and sets argtypes
    # every edge of the range, on both sides
    for L, M, C, ok in [(8000, 40, 5, 1), (400, 40, 1, 1), (399, 40, 5, 0), (1638399, 40, 64, 1), (1638400, 40, 5, 0),
                        (8000, 80, 5, 0), (8000, 39, 5, 0), (8000, 40, 64, 1), (8000, 40, 65, 0), (8000, 40, 1, 1), (8000, 40, 0, 0)]:
        assert lb.cdll.howl_lstm_stream_supported(L, M, C) == ok, (L, M, C)
        assert emu.cdll.howl_lstm_stream_supported(L, M, C) == ok, (L, M, C)


def test_argument_errors_name_the_entry_point(built):
    import ctypes
    from howl_amd import lib
    lb = lib.Library(built)
    one = ctypes.c_void_p(16)      # never dereferenced: every call below is refused first
    lp = lib.HowlLstmParams(one, one, one, one)
    hp = lib.HowlHeadParams(one, one, one, one)

    def call(lstm=lp, head=hp, pcm=one, ld=8000, N=1, L=8000, M=40, h=None, c=None, C=5, last_only=0, probs=one, out_ld=41 * 5):
        lb.call("howl_lstm_stream_chunks", ctypes.byref(lstm) if lstm is not None else None, ctypes.byref(head), pcm, ld, N, L, None, None, one, M,
                1e-7, None, h, c, C, last_only, probs, None, out_ld, None)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: null pointer"):
        call(pcm=None)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: null pointer"):
        call(lstm=None)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: null pointer in HowlLstmParams"):
        call(lstm=lib.HowlLstmParams(one, None, one, one))
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: null pointer in HowlHeadParams"):
        call(head=lib.HowlHeadParams(one, one, None, one))
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: N=0 streams unsupported"):
        call(N=0)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: N=8193 streams unsupported"):
        call(N=8193)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: L_max=399 samples.*unsupported"):
        call(L=399)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: L_max=8000 samples, M=80.*unsupported"):
        call(M=80)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: L_max=8000 samples, M=40, C=65 unsupported"):
        call(C=65, out_ld=41 * 65)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: out_ld=204 floats per stream, this call writes 205"):
        call(out_ld=204)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: out_ld=4 floats per stream, this call writes 5"):
        call(last_only=1, out_ld=4)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: h and c come as a pair"):
        call(h=one)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: negative stream stride"):
        call(ld=-1)
    with pytest.raises(lib.HowlHipError, match=r"howl_lstm_stream_chunks: .*16-byte aligned"):
        call(lstm=lib.HowlLstmParams(ctypes.c_void_p(20), one, one, one))


# ---- 7. bounds: every operand in a guarded mapping, each placement in a child process --------------------------------------------------

BOUNDS_CASES = {
    # the smallest and the largest n_samples, N not a multiple of 4
    "N3_small_large": dict(lengths=[400, 16000, 4321], C=5, state=True),
    "N5_last_only": dict(lengths=[16000, 712, 3000, 3200, 6800], C=3, state=False, last_only=True),
    "N1_400": dict(lengths=[400], C=12, state=False),
    "out_of_contract": None,
}


def run_bounds(case, placement):
    """Child-process body: every operand ends at (tail) or starts behind (head) a PROT_NONE page; the PCM rows end at the guard
    page, probs / logits / h / c are buffers whose promised region is exactly what the header says is written."""
    import emu_util
    import lstm_stream_util as u
    from guard_mem import Arena
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    al = Arena(placement)
    real_call = lib.call

    def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
        print(f"guard_mem: --- {name} ({case}, {placement})", file=sys.stderr)
        al.describe()
        return real_call(name, *args)
    lib.call = call
    if BOUNDS_CASES[case] is None:
        u.check_out_of_contract(al, lib)
    else:
        u.check_case(al, lib, what=case + ".", **BOUNDS_CASES[case])
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
    with ThreadPoolExecutor(max_workers=8) as ex:
        return {job: r for job, *r in ex.map(one, jobs)}


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("case", list(BOUNDS_CASES))
def test_lstm_stream_bounds(bounds_results, case, placement):
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
