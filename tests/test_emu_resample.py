"""The resampler (include/howl_hip_resample.h, howl_amd/csrc/resample.hip) on the hipemu emulator: the coefficient bank against
the float64 formula, the kernel against the float64 restatement of its contract within the derived bound (six rate pairs x four
sample formats, a ragged batch of 7 each), the definition itself against ``scipy.signal.resample_poly``, what the filter does to
a tone below and a tone above the new Nyquist, the properties without tolerance, the refusals, header / exports / ctypes table,
guard pages around every operand (in child processes), and the banks' ``from_files`` under ``emulated_package``."""
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
# non-zero taps per output, from a float64 prototype of the definition
NONZERO_TAPS = {48000: 383, 44100: 353, 8000: 128, 22050: 177, 11025: 128, 32000: 255}


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena():
    from guard_mem import Arena
    return Arena("tail", log=open(os.devnull, "w"))


# ---- 1. the bank against the formula -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr_in", [48000, 44100, 32000, 22050, 11025, 8000])
def test_bank_is_the_formula(emu, sr_in):
    import resample_util as u
    assert u.check_bank(None, emu, sr_in) == NONZERO_TAPS[sr_in]


# ---- 2. the kernel against float64 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["f32x1", "i16x1", "i16x2", "f32x3"])
@pytest.mark.parametrize("sr_in", [48000, 44100, 32000, 22050, 11025, 8000])
def test_ragged_batch_against_the_float64_restatement(emu, sr_in, fmt):
    """Measured on the emulator: the worst error is 0.6 % (48 kHz) to 3.2 % (8 kHz) of the bound (printed with -s)."""
    import resample_util as u
    al = _arena()
    u.check_kernel(al, emu, sr_in, fmt)
    al.check()


# ---- 3. the definition against an independent implementation -----------------------------------------------------------------------------

@pytest.mark.parametrize("sr_in", [48000, 44100])
def test_definition_is_resample_poly_with_the_prototype(sr_in):
    """Pins the contract, not the code under test: the float64 restatement over the FORMULA's bank equals
    scipy.signal.resample_poly(x, U, D, window=prototype) / U (scipy multiplies an array window by `up`)."""
    import resample_util as u
    from scipy.signal import resample_poly
    U, D = u.ratio(sr_in)
    W = u.Z * max(U, D)
    j_lo, j_hi = -((W - 1) // U), (W + U - 2) // U
    bank = u.formula_bank(U, D, j_lo, j_hi - j_lo + 1)
    for length in (1, 777, 4410):
        x = u.mono64(u.signal(length, 1, u.F32, sr_in, 21), 1)
        mine = u.restate(x, bank, U, D, j_lo)
        theirs = resample_poly(x, U, D, window=u.prototype(U, D)) / U
        assert len(mine) == len(theirs) == u.full_len(length, U, D)
        assert np.max(np.abs(mine - theirs)) <= 1e-12, float(np.max(np.abs(mine - theirs)))


# ---- 4. what the filter does -------------------------------------------------------------------------------------------------------------

def test_tones_below_and_above_the_new_nyquist(emu):
    """Restatement figures (float64, printed with -s): 1 kHz tone error 1e-8 .. 3e-8, 9.6 kHz tone RMS 4e-10 .. 7e-9."""
    import resample_util as u
    al = _arena()
    u.check_tones(al, emu)
    al.check()


# ---- 5. properties without tolerance -----------------------------------------------------------------------------------------------------

def test_identity_mean_and_placement_give_the_same_bits(emu):
    import resample_util as u
    al = _arena()
    u.check_exact(al, emu)
    al.check()


# ---- 6. refusals; header, exports, table -------------------------------------------------------------------------------------------------

def test_refusals_have_messages(emu):
    import resample_util as u
    from howl_amd import lib
    u.check_refusals(emu, lib.HowlHipError)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_resample_header(built, emu):
    import ctypes
    import resample_util as u
    from howl_amd import lib
    text = (ROOT / "include" / "howl_hip_resample.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    hdr = set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", code))
    assert hdr == {"howl_resample_plan", "howl_resample_bank_floats", "howl_resample_bank", "howl_resample_out_len", "howl_resample_clips"}, hdr
    assert set(lib.RESAMPLE_SIGNATURES) | set(lib.RESAMPLE_SIZE_FUNCS) == hdr
    assert set(lib.RESAMPLE_SIZE_FUNCS) == set(re.findall(r"size_t (howl_[a-z0-9_]+)\(", code))
    assert not hdr & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS) | set(lib.TIMESTRETCH_SIGNATURES))
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        assert hdr <= set(re.findall(r" T (howl_[a-z0-9_]+)\n", out)), path
    # the records are the header's structs (field order, size), the constants the header's
    body = code[code.index("typedef struct {", code.index("HowlResamplePlan;")):code.index("} HowlResampleClip;")]
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [n for n, _ in lib.RESAMPLE_CLIP_FIELDS] == list(u.CLIP_DTYPE.names), fields
    assert np.dtype(lib.RESAMPLE_CLIP_FIELDS) == u.CLIP_DTYPE and u.CLIP_DTYPE.itemsize == 24
    body = code[code.index("typedef struct {"):code.index("} HowlResamplePlan;")]
    assert re.findall(r"(\w+)\s*[;,]", body) == [n for n, _ in lib.HowlResamplePlan._fields_]
    assert ctypes.sizeof(lib.HowlResamplePlan) == 40
    consts = dict(re.findall(r"#define (HOWL_RESAMPLE_[A-Z0-9_]+) ([0-9]+)", text))
    assert consts == {"HOWL_RESAMPLE_MAX_CLIPS": str(lib.RESAMPLE_MAX_CLIPS), "HOWL_RESAMPLE_MAX_FRAMES": str(lib.RESAMPLE_MAX_FRAMES),
                      "HOWL_RESAMPLE_MAX_CHANNELS": "8", "HOWL_RESAMPLE_MIN_RATE": "4000", "HOWL_RESAMPLE_MAX_RATE": "192000",
                      "HOWL_RESAMPLE_MAX_UP": "640", "HOWL_RESAMPLE_MAX_DECIMATION": "16", "HOWL_RESAMPLE_ZEROS": str(u.Z),
                      "HOWL_RESAMPLE_F32": str(lib.RESAMPLE_F32), "HOWL_RESAMPLE_I16": str(lib.RESAMPLE_I16)}, consts
    assert (u.F32, u.I16) == (lib.RESAMPLE_F32, lib.RESAMPLE_I16)
    # the built library refuses like the emulator's and makes the same bank (host code: no device needed)
    gpu_lib = lib.Library(built)
    u.check_refusals(gpu_lib, lib.HowlHipError)
    for sr in (44100, 8000, 16000):
        assert np.array_equal(u.plan_and_bank(gpu_lib, sr)[1], u.plan_and_bank(emu, sr)[1])


def test_every_supported_rate_of_the_header_plans(emu):
    import ctypes
    import resample_util as u
    from howl_amd.lib import HowlResamplePlan
    for sr in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000, 4000):
        plan = HowlResamplePlan()
        emu.call("howl_resample_plan", sr, 16000, ctypes.byref(plan))
        assert (plan.up, plan.down) == u.ratio(sr) and plan.up <= 640


# ---- 8. the banks ------------------------------------------------------------------------------------------------------------------------

def test_from_files_fills_both_banks(emu, tmp_path):
    import emu_util
    import resample_util as u
    with emu_util.emulated_package():
        u.check_banks(tmp_path, "cpu", emu)


def test_read_wav_widths_and_errors(tmp_path):
    import wave
    from howl_amd.training.data import read_wav, wav_header
    vals = np.asarray([0, 1, -1, 8388607, -8388608, 4660], np.int64)
    for width, scale in ((1, 128.0), (3, 8388608.0), (4, 2147483648.0)):
        p = tmp_path / f"w{width}.wav"
        if width == 1:
            ints = np.asarray([128, 129, 127, 255, 0, 200], np.int64)
            raw, want = ints.astype(np.uint8).tobytes(), (ints - 128) / scale
        elif width == 3:
            raw, want = b"".join(int(v).to_bytes(3, "little", signed=True) for v in vals), vals / scale
        else:
            raw, want = (vals << 8).astype("<i4").tobytes(), (vals << 8) / scale
        with wave.open(str(p), "wb") as w:
            w.setnchannels(2)
            w.setsampwidth(width)
            w.setframerate(22050)
            w.writeframes(raw)
        got, sr, ch = read_wav(p)
        assert (sr, ch, got.dtype) == (22050, 2, np.float32) and wav_header(p) == (22050, 2, width, 3)
        assert np.array_equal(got, want.astype(np.float32))
    bad = tmp_path / "not_a_wav.wav"
    bad.write_bytes(b"ID3\x03" + bytes(64))
    for fn in (read_wav, wav_header):
        with pytest.raises(ValueError, match="not_a_wav.wav"):
            fn(bad)
        with pytest.raises(ValueError, match="missing.wav"):
            fn(tmp_path / "missing.wav")


# ---- 7. bounds: every operand in a guarded mapping, each placement in a child process ------------------------------------------------------

BOUNDS_CASES = ("batch_44100_i16x2", "batch_48000_f32x3", "exact")


def run_bounds(case, placement):
    """Child-process body: samples, bank, records and output each end at (tail) or start behind (head) a PROT_NONE page."""
    import emu_util
    import resample_util as u
    from guard_mem import Arena
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    al = Arena(placement)
    real_call = lib.call

    def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
        if name == "howl_resample_clips":
            print(f"guard_mem: --- {name} ({case}, {placement})", file=sys.stderr)
            al.describe()
        return real_call(name, *args)
    lib.call = call
    quiet = lambda *a: None
    if case == "exact":
        u.check_exact(al, lib)
    else:
        _, sr, fmt = case.split("_")
        u.check_kernel(al, lib, int(sr), fmt, quiet)
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
def test_resample_bounds(bounds_results, case, placement):
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
