"""Time-stretch test helpers: the phase-vocoder contract of ``howl_timestretch_clips`` restated in numpy (float64 with the
literal phase accumulator and ``np.fft``; float32 with the unit-phasor form), the input builders of the kernel tests, and the
checks the emulator and the device tests share (every operand a buffer of the test's allocator, as in tests/decide_util.py).

The arithmetic is what ``librosa.effects.time_stretch(y, rate)`` computes in librosa 0.8.x (``stft`` pads with ``reflect``):
N = 2048, hop 512, periodic Hann."""
import ctypes
import math

import numpy as np

N_FFT, HOP = 2048, 512
MIN_LEN = N_FFT
F32_TINY = float(np.finfo(np.float32).tiny)

# HowlStretchClip of include/howl_hip_timestretch.h
CLIP_DTYPE = np.dtype([("rate", np.float64), ("src_row", np.int64), ("dst_off", np.int64), ("len", np.int32), ("out_len", np.int32),
                       ("n_out", np.int32), ("bg_idx", np.int32), ("bg_off", np.int32), ("alpha", np.float32)])
FLAG_NO_COPY = 1


def hann(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


def geometry(length: int, rate: float):
    """(n_in, n_out, out_len, n_used) of a clip: input frames, time steps, output samples, frames the inverse uses."""
    n_in = 1 + length // HOP
    n_out = len(np.arange(0, n_in, rate, dtype=np.float64))
    out_len = int(round(length / rate))
    return n_in, n_out, out_len, min(n_out, int(math.ceil((out_len + N_FFT) / HOP)))


def _stft(y, dtype):
    w = hann(dtype)
    yp = np.pad(np.asarray(y, dtype), N_FFT // 2, mode="reflect")
    n_in = 1 + len(y) // HOP
    frames = np.stack([yp[HOP * f: HOP * f + N_FFT] * w for f in range(n_in)], axis=1)
    D = np.fft.rfft(frames, axis=0)
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    return np.concatenate([D.astype(ctype), np.zeros((D.shape[0], 2), ctype)], axis=1), n_in


def _istft(cols, out_len, dtype):
    """cols: (1025, n_out) -> ``out_len`` samples (overlap-add at hop 512, w^2 envelope, drop 1024, crop / zero pad)."""
    w = hann(dtype)
    n_used = min(cols.shape[1], int(math.ceil((out_len + N_FFT) / HOP)))
    y = np.zeros(N_FFT + HOP * (n_used - 1), dtype)
    wss = np.zeros_like(y)
    for t in range(n_used):
        y[HOP * t: HOP * t + N_FFT] += np.fft.irfft(cols[:, t], N_FFT).astype(dtype) * w
        wss[HOP * t: HOP * t + N_FFT] += w * w
    nz = wss > F32_TINY
    y[nz] /= wss[nz]
    y = y[N_FFT // 2:]
    out = np.zeros(out_len, dtype)
    out[:min(out_len, len(y))] = y[:out_len]
    return out


def stretch_f64(y, rate: float):
    """The contract, literally: float64, ``np.fft``, the phase accumulator with ``angle`` and the wrap to [-pi, pi]."""
    y = np.asarray(y, np.float64)
    D, n_in = _stft(y, np.float64)
    steps = np.arange(0, n_in, rate, dtype=np.float64)
    phi = np.linspace(0, np.pi * HOP, D.shape[0])
    acc = np.angle(D[:, 0])
    cols = np.zeros((D.shape[0], len(steps)), np.complex128)
    for t, step in enumerate(steps):
        i, a = int(step), np.mod(step, 1.0)
        c0, c1 = D[:, i], D[:, i + 1]
        cols[:, t] = ((1.0 - a) * np.abs(c0) + a * np.abs(c1)) * np.exp(1j * acc)
        d = np.angle(c1) - np.angle(c0) - phi
        d = d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))
        acc = acc + phi + d
    return _istft(cols, int(round(len(y) / rate)), np.float64)


def _unit(z, ftype):
    m = np.abs(z).astype(ftype)
    safe = np.where(m > 0, m, ftype(1))
    return np.where(m > 0, z / safe, np.ones_like(z)), m


def stretch_f32_phasor(y, rate: float):
    """The same contract in float32 with a unit phasor per bin in place of the phase accumulator: phi[k] = k pi / 2, so
    exp(j acc[t+1]) = exp(j acc[t]) u(D[:, i+1]) conj(u(D[:, i])), u(z) = z / |z|, u(0) = 1; renormalised each step.  The step
    index stays float64."""
    f32, c64 = np.float32, np.complex64
    y = np.asarray(y, f32)
    D, n_in = _stft(y, f32)
    steps = np.arange(0, n_in, rate, dtype=np.float64)
    p, _ = _unit(D[:, 0], f32)
    p = p.astype(c64)
    cols = np.zeros((D.shape[0], len(steps)), c64)
    for t, step in enumerate(steps):
        i, a = int(step), f32(np.mod(step, 1.0))
        u0, m0 = _unit(D[:, i], f32)
        u1, m1 = _unit(D[:, i + 1], f32)
        cols[:, t] = (((f32(1) - a) * m0 + a * m1).astype(f32) * p).astype(c64)
        p = (p * u1.astype(c64) * np.conj(u0.astype(c64))).astype(c64)
        p = (p / np.abs(p).astype(f32)).astype(c64)
    return _istft(cols, int(round(len(y) / rate)), f32)


# ---- inputs --------------------------------------------------------------------------------------------------------------
CASE_LENGTHS = (2048, 5000, 16000)
CASE_RATES = (0.3, 0.77, 1.31, 1.7)
# the ragged batch of 7: (clip, rate); every length and every rate appears
BATCH7 = ((0, 0.3), (1, 0.77), (2, 1.31), (0, 1.7), (1, 0.3), (2, 0.77), (2, 1.7))


def make_clips():
    """0.25 sin(2 pi 311 n / 16000) + 0.05 U(-1, 1) from default_rng(1234); the 16000-sample clip has samples 3000:6000 set to
    exactly zero (the segment on which every precision agrees that u(0) = 1)."""
    rng = np.random.default_rng(1234)
    clips = []
    for L in CASE_LENGTHS:
        n = np.arange(L)
        y = (0.25 * np.sin(2.0 * np.pi * 311.0 * n / 16000.0) + 0.05 * rng.uniform(-1.0, 1.0, L)).astype(np.float32)
        if L == 16000:
            y[3000:6000] = 0.0
        clips.append(y)
    return clips


_REF = {}


def references():
    """{(clip, rate): (float64 restatement, gap)} for every case of BATCH7 (and rate 1.0 of every clip), computed once;
    gap = max |float32 unit-phasor restatement - float64 restatement|, the yardstick of the kernel's tolerance."""
    if not _REF:
        clips = make_clips()
        for c, r in set(BATCH7) | {(c, 1.0) for c in range(len(clips))}:
            ref = stretch_f64(clips[c], r)
            gap = float(np.max(np.abs(stretch_f32_phasor(clips[c], r).astype(np.float64) - ref)))
            _REF[(c, r)] = (ref, gap)
    return _REF


def dense_bank(clips):
    bank = np.zeros((len(clips), max(len(c) for c in clips)), np.float32)
    for i, c in enumerate(clips):
        bank[i, :len(c)] = c
    return bank


def ragged_bank(clips):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    return np.concatenate(clips).astype(np.float32), offs


def descriptors(lengths, rates, src_rows, mix=None):
    """HowlStretchClip records for clips of ``lengths`` at ``rates`` read from bank rows ``src_rows``, outputs back to back;
    returns (records, total output floats).  ``mix`` = (bg_idx, bg_off, alpha) per clip."""
    rec = np.zeros(len(lengths), CLIP_DTYPE)
    off = 0
    for k, (L, r) in enumerate(zip(lengths, rates)):
        _, n_out, out_len, _ = geometry(L, r)
        rec[k] = (r, src_rows[k], off, L, out_len, n_out, 0, 0, 0.0)
        if mix is not None:
            rec[k]["bg_idx"], rec[k]["bg_off"], rec[k]["alpha"] = mix[0][k], mix[1][k], mix[2][k]
        off += out_len
    return rec, off


# ---- checks shared by the emulator (guard_mem.Arena) and the device (guard_mem.Banded) tests ----------------------------------------
TOLERANCE_FACTOR = 8.0      # the kernel may be this many times the float32-restatement gap away from the float64 restatement


def run(al, lib, bank, bank_ld, rec, total, bg=None, bg_ld=0, flags=0):
    """One ``howl_timestretch_clips`` call with every operand a buffer of allocator ``al`` (the records twice: the host copy the
    entry point validates, and the allocator's copy the kernel reads); every output sample is promised.  Returns the output."""
    words = np.ascontiguousarray(rec).view(np.int64)
    b = al.buf("bank", bank.shape, np.float32, bank)
    r = al.buf("clips", words.shape, np.int64, words)
    g = None if bg is None else al.buf("bg", bg.shape, np.float32, bg)
    o = al.buf("out", total, np.float32, "sentinel", promised="all")
    host = np.ascontiguousarray(rec)
    lib.call("howl_timestretch_clips", al.ptr(b), bank_ld, int(bank.size), al.ptr(g), bg_ld, 0 if bg is None else int(bg.size),
             ctypes.c_void_p(host.ctypes.data), al.ptr(r), len(host), al.ptr(o), total, flags, None)
    al.sync()
    return np.array(al.get(o))


def split(out, rec):
    return [out[int(r["dst_off"]): int(r["dst_off"]) + int(r["out_len"])] for r in rec]


def batch7_records(ragged=True):
    clips = make_clips()
    if ragged:
        bank, offs = ragged_bank(clips)
        rows, ld = [int(offs[c]) for c, _ in BATCH7], 1
    else:
        bank, rows, ld = dense_bank(clips), [c for c, _ in BATCH7], max(len(c) for c in clips)
    rec, total = descriptors([len(clips[c]) for c, _ in BATCH7], [r for _, r in BATCH7], rows)
    return bank, ld, rec, total


def check_batch7(al, lib, report=print):
    """The ragged batch of 7 against the float64 restatement: exact lengths (every promised sample written, nothing else), an
    exact zero tail, max-abs error within TOLERANCE_FACTOR x the case's measured gap.  Returns [(clip, rate, error, gap)]."""
    refs = references()
    bank, ld, rec, total = batch7_records()
    assert total == sum(len(refs[k][0]) for k in BATCH7)
    got = split(run(al, lib, bank, ld, rec, total), rec)
    rows = []
    for (c, r), g in zip(BATCH7, got):
        ref, gap = refs[(c, r)]
        _, _, out_len, n_used = geometry(len(make_clips()[c]), r)
        assert len(g) == out_len == len(ref) and np.isfinite(g).all()
        tail = min(out_len, HOP * (n_used - 1) + N_FFT // 2)        # fix_length's zero padding starts here
        assert not g[tail:].any() and not ref[tail:].any()
        err = float(np.max(np.abs(g.astype(np.float64) - ref)))
        report(f"timestretch clip {c} ({len(ref)} out) rate {r}: kernel error {err:.3e}, f32-f64 gap {gap:.3e}, ratio {err / gap:.2f}")
        rows.append((c, r, err, gap))
    for c, r, err, gap in rows:
        assert err <= TOLERANCE_FACTOR * gap, (c, r, err, gap)
    return rows


def check_identity(al, lib, report=print):
    """Rate 1.0 THROUGH the transform (copy shortcut off) reproduces the input to the same bound; with the shortcut, exactly."""
    clips, refs = make_clips(), references()
    bank, offs = ragged_bank(clips)
    rec, total = descriptors([len(c) for c in clips], [1.0] * len(clips), [int(o) for o in offs[:-1]])
    through = split(run(al, lib, bank, 1, rec, total, flags=FLAG_NO_COPY), rec)
    copied = split(run(al, lib, bank, 1, rec, total), rec)
    for c, (y, t, k) in enumerate(zip(clips, through, copied)):
        gap = refs[(c, 1.0)][1]
        err = float(np.max(np.abs(t.astype(np.float64) - y)))
        report(f"timestretch clip {c} rate 1.0 through the transform: error {err:.3e}, f32-f64 gap {gap:.3e}, ratio {err / gap:.2f}")
        assert err <= TOLERANCE_FACTOR * gap, (c, err, gap)
        assert np.array_equal(k, y)


def check_mix(al, lib):
    """DatasetMixer's operands, applied while reading, give what stretching (or copying) the pre-mixed clips gives."""
    clips = make_clips()[:2]
    rng = np.random.default_rng(77)
    bg = (0.2 * rng.uniform(-1.0, 1.0, (3, 7000))).astype(np.float32)
    bg_idx, bg_off, alpha = [2, 0, 1], [123, 2000, 7000 - 2048], np.asarray([0.15, 0.4, 0.0], np.float32)
    which, rates = [0, 1, 0], [0.77, 1.0, 1.31]
    mixed = []
    for c, j, o, a in zip(which, bg_idx, bg_off, alpha):
        y = clips[c]
        mixed.append(y if a == 0 else (y * (np.float32(1) - a) + bg[j, o:o + len(y)] * a).astype(np.float32))
    bank, offs = ragged_bank(clips)
    rec, total = descriptors([len(clips[c]) for c in which], rates, [int(offs[c]) for c in which], mix=(bg_idx, bg_off, alpha))
    got = run(al, lib, bank, 1, rec, total, bg=bg, bg_ld=bg.shape[1])
    mbank, moffs = ragged_bank(mixed)
    mrec, mtotal = descriptors([len(m) for m in mixed], rates, [int(o) for o in moffs[:-1]])
    want = run(al, lib, mbank, 1, mrec, mtotal)
    assert total == mtotal and np.array_equal(got, want)
    assert np.array_equal(split(got, rec)[1], mixed[1])             # the rate-1.0 clip: the mix itself


def check_layouts(al, lib):
    """A dense (N, Lmax) bank and a ragged bank give the same bits."""
    bank, ld, rec, total = batch7_records(ragged=True)
    dbank, dld, drec, dtotal = batch7_records(ragged=False)
    assert total == dtotal
    assert np.array_equal(run(al, lib, bank, ld, rec, total), run(al, lib, dbank, dld, drec, dtotal))


def check_refusals(lib, error):
    """Every refusal with its message; nothing is launched (the pointers are host arrays)."""
    import pytest
    y = make_clips()[0]
    out = np.zeros(20000, np.float32)

    def attempt(rec, B=None, bank=y):
        host = np.ascontiguousarray(rec)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        lib.call("howl_timestretch_clips", p(bank), 1, int(bank.size), None, 0, 0, p(host), p(host), len(host) if B is None else B, p(out),
                 int(out.size), 0, None)

    one = lambda L, r: descriptors([L], [r], [0])[0]
    ok = one(2048, 0.77)
    for B in (0, 8193):
        with pytest.raises(error, match=rf"howl_timestretch_clips: B={B} clips unsupported"):
            attempt(np.repeat(ok, max(B, 1)), B=B)
    for rate in (0.29, 1.71):
        with pytest.raises(error, match=rf"howl_timestretch_clips: clip 0: rate={rate} unsupported"):
            attempt(one(2048, rate))
    with pytest.raises(error, match=r"howl_timestretch_clips: clip 0: len=2047 samples with rate=0.77 unsupported"):
        attempt(one(2047, 0.77))
    short = one(2047, 1.0)                                          # a short clip at rate 1.0 is accepted (and copied)
    bad = ok.copy()
    bad["out_len"] += 1
    with pytest.raises(error, match=r"howl_timestretch_clips: clip 0: out_len=2661, n_out=7; len=2048 at rate=0.77\S* gives 2660 and 7"):
        attempt(bad)
    far = ok.copy()
    far["dst_off"] = out.size - 100
    with pytest.raises(error, match=r"outside the destination"):
        attempt(far)
    far = ok.copy()
    far["src_row"] = 1
    with pytest.raises(error, match=r"outside the bank"):
        attempt(far)
    far = ok.copy()
    far["alpha"] = 0.5
    with pytest.raises(error, match=r"alpha=0.5 without a background bank"):
        attempt(far)
    return short
