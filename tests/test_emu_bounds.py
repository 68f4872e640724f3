"""Bounds tests on the hipemu emulator: every launching entry point runs with each operand in its own guarded mapping
(tests/guard_mem.py: PROT_NONE pages on either side, canaries in the slack, sentinel-filled outputs), once with every buffer
ending at its upper guard page ("tail") and once starting at its lower one ("head"), and against the oracle.  Each (case,
placement) runs in a child process of its own, so an out-of-bounds access faults that case alone, with the emulator's report
(address, block, thread) and the buffer map in its message.  The cases are tests/bounds_cases.py, shared with the device's
sentinel-band tests (tests/test_gpu_bounds.py)."""
import ctypes
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for _p in (str(ROOT), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# entry points that launch nothing: version, errors, profiling, shutdown, size / range queries and the layer table
EXEMPT = {
    "howl_version": "returns the ABI version",
    "howl_profile_enable": "profiling switch",
    "howl_profile_read": "profiling counters (host)",
    "howl_profile_read_work": "profiling counters (host)",
    "howl_shutdown": "releases side queues and events",
    "howl_seq_head_ctc_supported": "range query",
    "howl_mobilenet_layer": "host layer table",
    "howl_mobilenet_workspace_layer": "host query of the launch plan (workspace map)",
}
PLACEMENTS = ("tail", "head")
TIMEOUT = 900


def _cases():
    import bounds_cases
    return bounds_cases.CASES


def emu_case_ids():
    return [name for name, c in _cases().items() if c.emu]


def run_case(case_id, placement):
    """Child-process body: one case on the emulator with guarded buffers."""
    import emu_util
    from guard_mem import Arena
    c = _cases()[case_id]
    for k, v in c.env.items():
        os.environ[k] = v
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    al = Arena(placement)
    real_call = lib.call

    def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
        print(f"guard_mem: --- {name} ({case_id}, {placement})", file=sys.stderr)
        al.describe()
        return real_call(name, *args)
    lib.call = call
    c.fn(al, lib, None, **c.params)
    al.check()


@pytest.fixture(scope="module")
def results(request):
    """Every selected (case, placement) in a child process, eight at a time; the library is built once up front."""
    import emu_util
    emu_util.emu_lib()
    jobs = sorted({(it.callspec.params["case_id"], it.callspec.params["placement"]) for it in request.session.items
                   if getattr(it, "originalname", None) == "test_bounds" and hasattr(it, "callspec")})
    env = dict(os.environ, OMP_NUM_THREADS="1")
    # the children start the way this interpreter did (user site-packages ignored or not)
    python = [sys.executable] + [flag for flag, on in (("-s", sys.flags.no_user_site), ("-E", sys.flags.ignore_environment)) if on]

    def one(job):
        cid, pl = job
        try:
            p = subprocess.run(python + [__file__, cid, pl], capture_output=True, text=True, timeout=TIMEOUT, env=env, cwd=ROOT)
            return job, p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:
            return job, "timeout", e.stdout or "", e.stderr or ""
    with ThreadPoolExecutor(max_workers=8) as ex:
        return {job: r for job, *r in ex.map(one, jobs)}


def name_fault(err):
    """The buffer a fault address lies next to: hipemu's report against the last buffer map the child printed."""
    m = re.search(r"hipemu: SIG\w+ at address (0x[0-9a-f]+|\(nil\))", err)
    if not m or m.group(1) == "(nil)":
        return ""
    addr = int(m.group(1), 16)
    block = err[:m.start()].rsplit("guard_mem: ---", 1)[-1]
    best = None
    for name, lo, hi in re.findall(r"guard_mem: (\S+)\s+\[0x([0-9a-f]+), 0x([0-9a-f]+)\)", block):
        lo, hi = int(lo, 16), int(hi, 16)
        if lo <= addr < hi:
            d, what = -1, f"fault address 0x{addr:x} inside buffer '{name}'"
        elif addr >= hi:
            d, what = addr - hi, f"fault address 0x{addr:x}: {addr - hi} bytes past the end of buffer '{name}'"
        else:
            d, what = lo - addr, f"fault address 0x{addr:x}: {lo - addr} bytes before the start of buffer '{name}'"
        if best is None or d < best[0]:
            best = (d, what)
    return best[1] if best else ""


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("case_id", emu_case_ids())
def test_bounds(results, case_id, placement):
    rc, out, err = results[(case_id, placement)]
    if rc != 0:
        tail = "\n".join([l for l in err.splitlines() if not l.startswith("guard_mem:")][-40:])
        maps = [l for l in err.splitlines() if l.startswith("guard_mem:")]
        pytest.fail(f"{case_id} [{placement}] exited {rc}\n{name_fault(err)}\n{tail}\n--- last buffer map ---\n" + "\n".join(maps[-40:]),
                    pytrace=False)


def test_every_launching_entry_point_has_a_case():
    from howl_amd import lib
    covered = set()
    for c in _cases().values():
        covered |= set(c.entry_points)
    launching = set(lib.SIGNATURES)
    assert covered <= launching, covered - launching
    assert not (set(EXEMPT) & covered), set(EXEMPT) & covered
    assert launching == covered | set(EXEMPT), sorted(launching ^ (covered | set(EXEMPT)))


def test_every_case_runs_somewhere():
    assert all(c.emu or c.gpu for c in _cases().values())


# ---- the guard itself (nothing here touches a guard page) -------------------------------------------------------------------

def _maps():
    out = []
    for line in Path("/proc/self/maps").read_text().splitlines():
        a, perms = line.split()[:2]
        lo, hi = (int(x, 16) for x in a.split("-"))
        out.append((lo, hi, perms))
    return out


def _perms(addr, maps):
    for lo, hi, perms in maps:
        if lo <= addr < hi:
            return perms
    return None


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_guard_pages_surround_every_buffer(placement):
    from guard_mem import PAGE, Arena
    al = Arena(placement, log=open(os.devnull, "w"))
    arrs = [al.buf("a", 1, np.float32), al.buf("b", (3, 5), np.float32), al.buf("c", 4097, np.int64), al.buf("d", 0, np.float32),
            al.buf("e", 7, np.uint8)]
    maps = _maps()
    for a, b in zip(arrs, al.bufs):
        assert b.lo % 16 == 0 and b.hi - b.lo == a.nbytes
        end = b.lo + ((a.nbytes + 15) & ~15)
        upper = b.lo + max(1, -(-(end - b.lo) // PAGE)) * PAGE if placement == "head" else end
        if placement == "tail":
            assert upper % PAGE == 0 and upper - b.hi < 16          # ends at the guard (<= 15 bytes of aligned slack)
            assert _perms(upper, maps) == "---p" and _perms(upper - 1, maps) == "rw-p"
        else:
            assert b.lo % PAGE == 0 and _perms(b.lo - 1, maps) == "---p"
            assert _perms(upper, maps) == "---p"
    al.check()


def test_canary_and_promise_violations_are_reported():
    from guard_mem import Arena, sentinel_mask
    al = Arena("tail", log=open(os.devnull, "w"))
    a = al.buf("slack", 3, np.float32)                       # 12 bytes: 4 bytes of canary before the guard
    o = al.buf("out", (2, 4), np.float32, "sentinel", promised=lambda x: np.arange(4)[None, :] < 3)
    assert sentinel_mask(o).all() and np.isnan(o).all()
    o[:, :3] = 1.0
    al.check()                                               # column 3 is not promised
    ctypes.memset(a.ctypes.data + 12, 0, 1)                  # the first slack byte, inside the data page
    bad = al.problems()
    assert len(bad) == 1 and bad[0].startswith("slack: canary above")
    h = Arena("head", log=open(os.devnull, "w"))
    p = h.buf("promised", 5, np.float32, "sentinel", promised="all")
    p[:4] = 0.0
    assert h.problems() == ["promised: 1 promised element(s) never written (first at [4])"]


if __name__ == "__main__":
    run_case(sys.argv[1], sys.argv[2])
    print(json.dumps({"case": sys.argv[1], "placement": sys.argv[2], "ok": True}))
