"""The engines' decision logic on the device (include/howl_hip_decide.h, howl_amd/csrc/decide.hip) on the hipemu emulator: every
decision against the host loops as they stand, bit for bit -- random cases in both modes, the normalisation, the threshold edge,
degenerate shapes, independence of the clips, refusals and fallbacks, both engines with the switch on and off; header / exports /
ctypes tables; guard-page bounds in child processes (as tests/test_emu_bounds.py runs its cases)."""
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
TIMEOUT = 900


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena():
    from guard_mem import Arena
    return Arena("tail", log=open(os.devnull, "w"))


# ---- 1. random cases against the host replay ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    import decide_util as u
    cs = u.random_cases()
    return cs, u.host_results(cs)


def test_random_cases_equal_the_host_replay_in_both_modes(emu, cases):
    import decide_util as u
    u.check_random_cases(_arena(), emu, *cases)


# ---- 2. - 5. ---------------------------------------------------------------------------------------------------------------------------------

def test_normalisation_bit_for_bit(emu):
    import decide_util as u
    u.check_normalisation(_arena(), emu)


def test_threshold_edge_and_colour_map_without_the_label(emu):
    import decide_util as u
    u.check_threshold_edge(_arena(), emu)


def test_degenerate_shapes(emu):
    import decide_util as u
    u.check_degenerate(_arena(), emu)


def test_clips_are_independent_and_launches_repeat(emu):
    import decide_util as u
    u.check_independence(_arena(), emu)


def test_matcher_window_longer_than_the_lds_tail_reads_the_history_back(emu):
    import decide_util as u
    u.check_long_window(_arena(), emu)


# ---- 6. refusals, tables, fallback --------------------------------------------------------------------------------------------------------------

def header_functions():
    text = (ROOT / "include" / "howl_hip_decide.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_decide_header(built, emu):
    import decide_util as u
    from howl_amd import lib
    hdr = header_functions()
    assert hdr == {"howl_decide_supported", "howl_decide_clips"}, hdr
    table = set(lib.DECIDE_SIGNATURES) | set(lib.DECIDE_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    assert not table & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS) | set(lib.STREAM_SIGNATURES) | set(lib.STREAM_SIZE_FUNCS) |
                        set(lib.LSTM_STREAM_SIGNATURES) | set(lib.LSTM_STREAM_SIZE_FUNCS))
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert hdr <= exported, (path, hdr - exported)
    # the ctypes record is the header's struct: the constants and the field order
    text = (ROOT / "include" / "howl_hip_decide.h").read_text()
    consts = dict(re.findall(r"#define (HOWL_DECIDE_[A-Z_]+) (\d+)", text))
    assert consts == {"HOWL_DECIDE_MAX_CLASSES": "64", "HOWL_DECIDE_MAX_SEQUENCE": "16", "HOWL_DECIDE_MAX_CLIPS": "8192",
                      "HOWL_DECIDE_MAX_FRAMES": "8192", "HOWL_DECIDE_RING_FRAMES": str(u.RING)}, consts
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct {"):text.index("} HowlDecideConfig;")], flags=re.S)
    fields = re.findall(r"(\w+)(?:\[\w+\])?;", body)
    assert fields == [n for n, _ in lib.HowlDecideConfig._fields_], fields
    u.check_supported_table(lib.Library(built), emu)


def test_argument_errors_name_the_entry_point(built):
    import decide_util as u
    from howl_amd import lib
    u.check_argument_errors(lib.Library(built))


def test_decider_supported_and_the_switch_default(monkeypatch):
    import decide_util as u
    import emu_util
    with emu_util.emulated_package():
        u.check_decider_supported()
    u.check_switch_default(monkeypatch)


def test_ring_overflow_sets_status_and_is_replayed_on_the_host():
    import decide_util as u
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_ring_overflow(torch.from_numpy, lib.get())


# ---- 7. the engines -------------------------------------------------------------------------------------------------------------------------------

def test_sequence_engine_with_the_switch_on_equals_off(golden):
    import decide_util as u
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_sequence_engine(golden, torch.device("cpu"), lib.get(), sizes=(8000, 6000, 4321, 3000, 1000, 400), later=slice(3, None))


def test_frame_engine_with_the_switch_on_equals_off(golden):
    import decide_util as u
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_frame_engine(golden, torch.device("cpu"), lib.get(), extra_windows=(1, 0, 2, 0), later=slice(2, None))


def test_sequence_engine_gives_the_g8_history_with_the_switch_on(golden):
    import decide_util as u
    import emu_util
    import torch
    with emu_util.emulated_package():
        from howl_amd import lib
        u.check_g8_sequence(golden, torch.device("cpu"), lib.get())


# ---- bounds: every operand in a guarded mapping, each placement in a child process -----------------------------------------------------------------

BOUNDS_CASES = ("clamped", "degenerate", "threshold_edge")


def run_bounds(case, placement):
    """Child-process body: every operand ends at (tail) or starts behind (head) a PROT_NONE page."""
    import decide_util as u
    import emu_util
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
    {"clamped": u.check_clamped, "degenerate": u.check_degenerate, "threshold_edge": u.check_threshold_edge}[case](al, lib)
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
def test_decide_bounds(bounds_results, case, placement):
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
