"""CTC for targets beyond 31 labels (include/howl_hip_ctc_long.h, howl_amd/csrc/ctc_long.hip) on the hipemu emulator: header /
exports / ctypes tables; parity with torch's CPU log_softmax + ctc_loss + autograd at the whole-clip tests' bounds on both sides
of every switch between the kernel bodies; the same bits whichever body runs an utterance; the per-utterance contract; refusals;
window edges; guard-page bounds in child processes (as tests/test_emu_decide.py runs its cases)."""
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

import ctc_long_util as u  # noqa: E402

PLACEMENTS = ("tail", "head")
TIMEOUT = 900


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


# ---- header, exports, tables -------------------------------------------------------------------------------------------------------

def header_functions():
    text = (ROOT / "include" / "howl_hip_ctc_long.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_ctc_long_header(built, emu):
    from howl_amd import lib
    hdr = header_functions()
    assert hdr == {"howl_ctc_long_supported", "howl_ctc_long_window_rows", "howl_ctc_long_workspace_floats", "howl_ctc_loss_long"}, hdr
    table = set(lib.CTC_LONG_SIGNATURES) | set(lib.CTC_LONG_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    assert not table & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS) | set(lib.STREAM_SIGNATURES) | set(lib.STREAM_SIZE_FUNCS) |
                        set(lib.LSTM_STREAM_SIGNATURES) | set(lib.LSTM_STREAM_SIZE_FUNCS) | set(lib.DECIDE_SIGNATURES) |
                        set(lib.DECIDE_SIZE_FUNCS))
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert hdr <= exported, (path, hdr - exported)
    # howl_ctc_loss_long takes howl_ctc_loss's argument list, in the header and in the table
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip_ctc_long.h").read_text(), flags=re.S)
    short = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip.h").read_text(), flags=re.S)
    args = lambda t, name: re.sub(r"\s+", " ", re.search(rf"\b{name}\s*\((.*?)\)\s*;", t, flags=re.S).group(1))
    assert args(text, "howl_ctc_loss_long") == args(short, "howl_ctc_loss")
    assert lib.CTC_LONG_SIGNATURES["howl_ctc_loss_long"] == lib.SIGNATURES["howl_ctc_loss"]
    assert re.search(r"#define HOWL_CTC_LONG_MAX_LABELS (\d+)", text).group(1) == "255"
    for l in (lib.Library(built), emu):
        u.check_size_functions(l)


# ---- parity --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", u.EMU_CASES)
def test_ctc_long_vs_torch(emu, name):
    logits, targets, in_len, tgt_len, blank, loss64, grad64, noise = u.case(name)
    nll, loss, dz = u.emu_run(emu, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank)
    u.check_parity(name, loss, torch.from_numpy(dz), in_len, loss64, grad64, noise)
    again = u.emu_run(emu, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank)             # bit-identical repeats
    assert np.array_equal(again[0], nll) and again[1] == loss and np.array_equal(again[2], dz)
    nll2, loss2, none = u.emu_run(emu, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank, want_grad=False)
    assert none is None and loss2 == loss and np.array_equal(nll2, nll)                             # loss only: no workspace
    nll3, _, dz3 = u.emu_run(emu, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank, want_loss=False)   # deferred mean
    assert np.array_equal(nll3, nll) and np.array_equal(dz3, dz)


@pytest.mark.parametrize("M", [32, 64, 255])
def test_ctc_long_window_edges(emu, M):
    assert emu.cdll.howl_ctc_long_window_rows(M) == u.window_rows(M)

    def runner(logits, targets, in_len, tgt_len, blank):
        _, loss, dz = u.emu_run(emu, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank)
        return loss, torch.from_numpy(dz)
    u.check_window_edges(runner, M)


# ---- the same bits whichever body runs an utterance ---------------------------------------------------------------------------------

@pytest.mark.parametrize("T,B,C,Lmax,seed", u.short_cases())
def test_ctc_long_bits_do_not_depend_on_the_instantiation(emu, T, B, C, Lmax, seed):
    u.check_independence(u.Plain(), emu, T, B, C, Lmax, seed)


# ---- contract, refusals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["label", "length", "input"])
def test_ctc_long_contract(emu, kind):
    from guard_mem import Arena
    u.check_contract(Arena("tail", log=open(os.devnull, "w")), emu, kind)


def test_ctc_long_refusals(emu):
    u.check_cabi_refusals(emu)
    assert emu.cdll.howl_ctc_supported(40, 5, 32) == 0          # the short entry keeps its range


def test_ops_long_targets_keyword(emu):
    """ops.ctc_loss / ctc_loss_fwd_bwd with long_targets=True through the emulated package: the long entry runs, the default
    still refuses 32 labels and more with its own message, and beyond 255 labels the message names the batch's longest target."""
    import emu_util
    from howl_amd.lib import HowlHipError
    logits, targets, in_len, tgt_len, blank, loss64, grad64, noise = u.case("k2-32")
    with emu_util.emulated_package():
        from howl_amd import lib, ops
        seen = []
        real = lib.Library.call

        def spy(self, name, *args):
            seen.append((name, args[8]) if name.startswith("howl_ctc_loss") else (name, None))
            return real(self, name, *args)
        lib.Library.call = spy
        try:
            assert ops.ctc_long_supported(8192, 64, 255) and not ops.ctc_long_supported(100, 5, 256)
            z = logits.clone().requires_grad_(True)
            out = ops.ctc_loss(z.permute(1, 0, 2), targets, in_len, tgt_len, blank, long_targets=True)
            (3.0 * out).backward()
            loss, dz = ops.ctc_loss_fwd_bwd(logits.permute(1, 0, 2), targets, in_len, tgt_len, blank, long_targets=True)
            assert seen == [("howl_ctc_loss_long", 32), ("howl_ctc_loss_long", 32)]
            u.check_parity("ops k2-32", float(loss), dz.permute(1, 0, 2), in_len, loss64, grad64, noise)
            assert torch.equal(out.detach(), loss) and torch.equal(z.grad, 3.0 * dz.permute(1, 0, 2))
            with pytest.raises(HowlHipError, match=r"outside howl_ctc_loss's range \(T <= 8192, C <= 64, targets <= 31\)"):
                ops.ctc_loss(logits.permute(1, 0, 2), targets, in_len, tgt_len, blank)
            wide = torch.zeros(4, 300, dtype=torch.int64)
            for fn in (ops.ctc_loss, ops.ctc_loss_fwd_bwd):
                with pytest.raises(HowlHipError, match=r"longest target has 300 labels: outside howl_ctc_loss_long's range .*<= 255"):
                    fn(logits.permute(1, 0, 2), wide, in_len, torch.tensor([300, 3, 3, 3]), blank, long_targets=True)
            assert len(seen) == 2                                    # refused on the host: nothing reached the library
        finally:
            lib.Library.call = real


# ---- bounds: every operand in a guarded mapping, each placement in a child process ----------------------------------------------------

# one case per kernel body (K = 1, 2, 4, 8), each of several windows, plus one-window launches of the two ends
BOUNDS_CASES = {"k1": (140, 3, 5, 31), "k2": (150, 3, 6, 63), "k4": (90, 3, 5, 64), "k8": (600, 3, 64, 255), "k2-one-window": (64, 3, 5, 32),
                "k8-one-window": (32, 3, 3, 128)}


def run_bounds(case, placement):
    """Child-process body: every operand ends at (tail) or starts behind (head) a PROT_NONE page; the target matrix has row stride
    exactly max_target_length, the workspace exactly howl_ctc_long_workspace_floats floats."""
    import emu_util
    from ctc_util import make_case
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
    T, B, C, M = BOUNDS_CASES[case]
    if T >= 2 * M - 1:
        logits, targets, in_len, tgt_len, blank = u.structured_case(T, B, C, M, 31)
    else:                        # too few frames for M equal labels: the longest target is declared, not held
        logits, targets, in_len, tgt_len, blank = make_case(T, B, C, min(M, T // 2), 31)
    for grad in (True, False):
        u.call(al, lib, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank, max_target=M, want_grad=grad, tag=f".grad{int(grad)}")
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
@pytest.mark.parametrize("case", sorted(BOUNDS_CASES))
def test_ctc_long_bounds(bounds_results, case, placement):
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
