"""Streaming las (include/howl_hip_las_stream.h, howl_amd/csrc/las_stream.hip) on the hipemu emulator: one launch from the windows'
PCM to their probabilities, against the float64 oracle with the eager chain's own error as the yardstick; independence of the
windows; refusals; the G8 clip through the engine's fused ingest_frame; staleness of the session's prepared state; header /
exports / ctypes tables; guard-page bounds in child processes (as tests/test_emu_res8_stream.py runs its cases).  The launch of
257 windows (more workgroups than compute units) is the device's business: tests/test_gpu_las_stream.py."""
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

import las_stream_util  # noqa: E402

PLACEMENTS = ("tail", "head")
TIMEOUT = 900


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena():
    from guard_mem import Arena
    return Arena("tail", log=open(os.devnull, "w"))


# ---- 1 / 3. against the fp64 oracle, every operand in a guarded mapping -------------------------------------------------------------

@pytest.mark.parametrize("N,L,C", las_stream_util.CASES)
def test_logits_against_the_fp64_oracle(emu, N, L, C):
    """e_fused <= 2 e_eager + 1e-6 on the logits, probs == softmax(logits) and rows summing to 1 within 1e-6; guards intact."""
    las_stream_util.check_against_oracle(_arena(), emu, N, L, C)


# ---- 2. independence -------------------------------------------------------------------------------------------------------------

def test_windows_are_independent_and_launches_repeat(emu):
    las_stream_util.check_independence(_arena(), emu, many=0)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_point_and_write_nothing(emu):
    las_stream_util.check_refusals(_arena(), emu)


# ---- 5. through the engine -------------------------------------------------------------------------------------------------------

def test_fused_and_eager_ingest_frame_agree_over_the_g8_clip(golden):
    """The oracle's conditions over all 37 windows; the engine itself over the first five (the device test runs all 37)."""
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        las_stream_util.check_engine(golden, torch.device("cpu"), lib.get(), first=5)


def test_engine_switch_is_opt_in(golden, monkeypatch):
    import emu_util
    import torch
    with emu_util.emulated_package():
        monkeypatch.delenv("HOWL_STREAM_FUSED", raising=False)
        from howl_amd.model.inference import FrameInferenceEngine
        from howl_amd.model.rnn import LasStreamSession
        e = las_stream_util.las_engine(golden, torch.device("cpu"), fused=None)
        assert FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context).fused_windows is False
        monkeypatch.setenv("HOWL_STREAM_FUSED", "1")
        on = FrameInferenceEngine(500, 63, e.model, e.zmuv, e.context)
        assert on.fused_windows is True
        on.std = on.std.to(torch.device("cpu"))
        # a window outside the kernel's range (2 s) keeps the launch chain
        assert isinstance(on._fused_session(torch.zeros(8000)), LasStreamSession) and on._fused_session(torch.zeros(32000)) is None


# ---- 6. staleness ----------------------------------------------------------------------------------------------------------------

def test_session_prepares_again_after_load_state_dict_and_refresh():
    import emu_util
    import torch
    with emu_util.emulated_package():
        las_stream_util.check_staleness(torch.device("cpu"))


# ---- 7. header, exports, tables --------------------------------------------------------------------------------------------------

def header_functions():
    text = (ROOT / "include" / "howl_hip_las_stream.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_las_stream_header(built, emu):
    from howl_amd import lib
    hdr = header_functions()
    assert len(hdr) == 5 and all(n.startswith("howl_las_stream_") for n in hdr), hdr
    table = set(lib.LAS_STREAM_SIGNATURES) | set(lib.LAS_STREAM_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    assert not table & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS) | set(lib.LAS_SIGNATURES) | set(lib.LAS_SIZE_FUNCS))
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" [TW] (howl_las_stream_[a-z0-9_]+)\n", out))      # (weak definitions: las_stream.hip says why)
        assert exported == hdr, (path, hdr ^ exported)
    lb = lib.Library(built)      # resolves every symbol and sets argtypes
    assert lb.cdll.howl_las_stream_state_bytes(4) > 4 * 2 * 384 * 352 and lb.cdll.howl_las_stream_state_bytes(65) == 0
    assert lb.cdll.howl_las_stream_workspace_bytes(2, 8000) == 2 * lb.cdll.howl_las_stream_workspace_bytes(1, 8000) > 0


# ---- 3. bounds: the smallest and the largest case, each placement in a child process ------------------------------------------------

BOUNDS_SHAPES = {"N1_L512_C4": (1, 512, 4), "N3_L16599_C64": (3, 16599, 64)}


def run_bounds(shape, placement):
    """Child-process body: prepare + windows with every operand ending at (tail) or starting behind (head) a PROT_NONE page; the PCM
    rows end at the guard page (ld == L), probs / logits are sentinel buffers whose promised region is exactly [N, C]."""
    import emu_util
    from guard_mem import Arena
    N, L, C = BOUNDS_SHAPES[shape]
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    al = Arena(placement)
    real_call = lib.call

    def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
        print(f"guard_mem: --- {name} ({shape}, {placement})", file=sys.stderr)
        al.describe()
        return real_call(name, *args)
    lib.call = call
    las_stream_util.check_against_oracle(al, lib, N, L, C)
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
    with ThreadPoolExecutor(max_workers=4) as ex:
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


if __name__ == "__main__":
    run_bounds(sys.argv[1], sys.argv[2])
    print(json.dumps({"shape": sys.argv[1], "placement": sys.argv[2], "ok": True}))
