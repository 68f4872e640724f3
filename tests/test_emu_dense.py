"""The dense kernels of howl_amd/csrc/howl_gemm.hip.h through include/howl_hip_dense.h on the hipemu emulator: header / exports /
ctypes tables, then the case table of tests/dense_util.py on guard_mem.Arena in both placements -- every operand ends at (tail) or
starts behind (head) a PROT_NONE page, so the kernels' unconditional clamped loads (M - 4, kend - 1, rows - 1) fault when a clamp
is off.  One child process per group of cases and placement (a fault ends the child, not the suite); the children report every
case's verdict, the kernel instances the dispatcher chose and the worst error / bound per instance.

HOWL_DENSE_REPORT=<file> appends the error / bound figures to that file (profiles/dense_bounds.txt is made this way)."""
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

import dense_util as u  # noqa: E402

PLACEMENTS = ("tail", "head")
TIMEOUT = 900


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "howl_hip_dense.h").read_text(), flags=re.S)


def test_library_exports_the_dense_header(emu):
    import __graft_entry__ as ge
    from howl_amd import lib
    ge.build()
    hdr = set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", header_text()))
    table = set(lib.DENSE_SIGNATURES) | set(lib.DENSE_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    assert not table & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS))
    for path in (ge.LIB, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (howl_[a-z0-9_]+)\n", out))
        assert hdr <= exported, (path, hdr - exported)
    # the family numbers of the header are the ones the Python table names
    fams = {int(n): name for name, n in re.findall(r"#define HOWL_DENSE_([A-Z0-9_]+) (\d+)\s", header_text())
            if name not in ("MAX_CHOICES", "MAX_SLAB_JOBS", "MAX_WGRAD_JOBS")}
    assert sorted(fams) == sorted(lib.DENSE_FAMILIES) == list(range(1, 13))
    assert re.search(r"#define HOWL_DENSE_LIN \(1 << 30\)", header_text()) and lib.DENSE_LIN == 1 << 30
    # the header states the own-copy limitation
    assert "not the same\n * code object" in (ROOT / "include" / "howl_hip_dense.h").read_text()


def test_written_out_instance_list():
    assert len(u.REACHABLE) == len(set(u.REACHABLE)) == 2 + 7 + 14 + 8 + 4 + 5 + 6
    assert not set(u.UNREACHABLE) & set(u.REACHABLE)


@pytest.fixture(scope="module")
def children(emu):
    from concurrent.futures import ThreadPoolExecutor
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("HOWL_ROWGEMM_MIN_ROWS", "HOWL_WGRAD_BIG_MIN_ROWS", "HOWL_GEMM_NO_ROWGEMM", "HOWL_WGRAD_NO_DUAL"):
        env.pop(k, None)
    python = [sys.executable] + [flag for flag, on in (("-s", sys.flags.no_user_site), ("-E", sys.flags.ignore_environment)) if on]

    def one(job):
        try:
            p = subprocess.run(python + [str(HERE / "dense_util.py"), *job], capture_output=True, text=True, timeout=TIMEOUT, env=env, cwd=ROOT)
            return job, p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:
            return job, "timeout", e.stdout or "", e.stderr or ""
    jobs = [(g, pl) for g in u.GROUPS for pl in PLACEMENTS]
    with ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as ex:
        out = {}
        for job, rc, stdout, stderr in ex.map(one, jobs):
            report = None
            if rc == 0:
                report = json.loads(stdout.strip().splitlines()[-1])
            out[job] = (rc, report, stderr)
    path = os.environ.get("HOWL_DENSE_REPORT")
    if path:
        ratios = {}
        for rc, report, _ in out.values():
            for k, v in (report or {}).get("ratios", {}).items():
                ratios[k] = max(ratios.get(k, 0.0), v)
        with open(path, "a") as f:
            f.write("\n".join(u.report_lines("emu", ratios)) + "\n")
    return out


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", u.names("emu"))
def test_dense(children, name, placement):
    rc, report, err = children[(u.CASES[name].group, placement)]
    if rc != 0:
        from test_emu_bounds import name_fault
        last = [l for l in err.splitlines() if l.startswith("dense: ---")][-1:]
        tail = "\n".join(err.splitlines()[-30:])
        pytest.fail(f"the child of group {u.CASES[name].group} [{placement}] exited {rc}; it was running {last}\n{name_fault(err)}\n{tail}",
                    pytrace=False)
    r = report["results"][name]
    assert r["ok"], r.get("msg")


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_every_instance_is_reached(children, placement):
    seen = set()
    for g in u.GROUPS:
        rc, report, _ = children[(g, placement)]
        assert rc == 0, f"group {g} [{placement}] exited {rc}"
        seen |= set(report["seen"])
    assert sorted(seen) == u.REACHABLE, (sorted(set(u.REACHABLE) - seen), sorted(seen - set(u.REACHABLE)))
    assert not seen & set(u.UNREACHABLE)
