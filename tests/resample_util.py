"""Resampler test helpers: the contract of ``include/howl_hip_resample.h`` restated in numpy float64 (the prototype filter from
the formula with ``scipy.special.i0``, the polyphase sum over a bank, the channel mean), the input builders of the kernel tests,
and the checks the emulator and the device tests share (every operand a buffer of the test's allocator, as in
tests/timestretch_util.py).

    h(t)    = rolloff sinc(rolloff t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta)  for |t| < Z, else 0
    c[p][j] = s h(s (p/U - j)),  s = min(1, U/D),  p = (n D) mod U,  j = k - floor(n D / U)
    out[n]  = sum_k c[p][j] x[k],  x = channel mean, 0 outside the clip,  n < ceil(len U / D)
"""
import ctypes
import math
from fractions import Fraction

import numpy as np

Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
TILE = 256                      # outputs per workgroup of resample.hip
TARGET = 16000
RATES = (48000, 44100, 32000, 22050, 11025, 8000)
F32, I16 = 0, 1
FORMATS = {"f32x1": (F32, 1), "i16x1": (I16, 1), "i16x2": (I16, 2), "f32x3": (F32, 3)}
EPS = 2.0 ** -24

# HowlResampleClip of include/howl_hip_resample.h
CLIP_DTYPE = np.dtype([("src_off", np.int64), ("dst_off", np.int64), ("len", np.int32), ("out_len", np.int32)])


# ---- the contract in float64 -------------------------------------------------------------------------------------------------
def ratio(sr_in, sr_out=TARGET):
    f = Fraction(sr_out, sr_in)
    return f.numerator, f.denominator


def full_len(length, U, D):
    return -((-length * U) // D)


def h(t):
    """The prototype at float64 times ``t``; |t| >= Z gives 0."""
    from scipy.special import i0
    t = np.asarray(t, np.float64)
    inside = np.abs(t) < Z
    u = np.where(inside, t / Z, 0.0)
    return np.where(inside, ROLLOFF * np.sinc(ROLLOFF * t) * i0(BETA * np.sqrt(1.0 - u * u)) / i0(BETA), 0.0)


def formula_bank(U, D, j_lo, taps):
    """c[p][j_lo + i] in float64 for p < U, i < taps.  The time is the contract's s (p/U - j) in float64; whether |t| < Z is decided
    on the exact integers |p - j U| < Z max(U, D) (at 44.1 kHz phase 64, j = -176 has |t| = Z exactly, which float64 may miss)."""
    s = min(1.0, U / D)
    p = np.arange(U, dtype=np.int64)[:, None]
    j = (j_lo + np.arange(taps, dtype=np.int64))[None, :]
    t = s * (p.astype(np.float64) / U - j.astype(np.float64))
    inside = np.abs(p - j * U) < Z * max(U, D)
    return np.where(inside, s * h(np.where(inside, t, 0.0)), 0.0)


def prototype(U, D):
    """The same filter as ONE FIR at rate U * sr_in for ``scipy.signal.resample_poly(x, U, D, window=prototype)``: taps
    s h(s m / U) for |m| <= L, odd length, centred."""
    s = min(1.0, U / D)
    L = int(math.ceil(Z * U / s))
    m = np.arange(-L, L + 1, dtype=np.float64)
    return s * h(s * m / U)


def mono64(v, channels):
    """Float64 channel mean of interleaved samples (int16 as v / 32768)."""
    v = np.asarray(v)
    x = v.astype(np.float64) / 32768.0 if v.dtype == np.int16 else v.astype(np.float64)
    return x.reshape(-1, channels).mean(axis=1)


def mono32(v, channels):
    """The contract's float32 channel mean: sum in channel order, then one division."""
    v = np.asarray(v)
    x = (v.astype(np.float32) / np.float32(32768.0) if v.dtype == np.int16 else v.astype(np.float32)).reshape(-1, channels)
    acc = x[:, 0].copy()
    for ch in range(1, channels):
        acc = (acc + x[:, ch]).astype(np.float32)
    return acc if channels == 1 else (acc / np.float32(channels)).astype(np.float32)


def restate(x, bank, U, D, j_lo, out_len=None, absx=None):
    """out[n] = sum_i bank[p][i] x[floor(n D / U) + j_lo + i] in float64 for n < out_len (default: the full length); with ``absx``
    also sum_i |bank[p][i]| absx[...], the magnitude the error bound scales with."""
    x = np.asarray(x, np.float64)
    bank = np.asarray(bank, np.float64)
    taps = bank.shape[1]
    n_out = full_len(len(x), U, D) if out_len is None else out_len
    n = np.arange(n_out, dtype=np.int64)
    base, p = (n * D) // U, (n * D) % U
    pad = taps + abs(j_lo) + 8
    k = base[:, None] + j_lo + np.arange(taps)[None, :] + pad
    need = int(k.max()) + 1 if n_out else 0
    xp = np.zeros(max(need, len(x) + 2 * pad))
    xp[pad:pad + len(x)] = x
    out = np.einsum("nt,nt->n", bank[p], xp[k])
    if absx is None:
        return out
    ap = np.zeros_like(xp)
    ap[pad:pad + len(x)] = absx
    return out, np.einsum("nt,nt->n", np.abs(bank[p]), ap[k])


def bound(taps, channels, mag):
    """|out - ref| <= (taps + channels + 2) 2^-24 sum_k |c_k| mean_ch |x_k,ch| -- any summation order, with or without FMA: each
    product and each partial sum rounds once (taps roundings along the longest chain), the mean costs ``channels`` more, the
    coefficient's own rounding is in the bank, two spare."""
    return (taps + channels + 2) * EPS * mag


# ---- the library's plan and bank --------------------------------------------------------------------------------------------
_PLANS = {}


def plan_and_bank(lib, sr_in, sr_out=TARGET):
    """(HowlResamplePlan, its bank as a (up, taps) float32 array) from the library under test."""
    from howl_amd.lib import HowlResamplePlan
    key = (str(lib.path), sr_in, sr_out)
    if key not in _PLANS:
        plan = HowlResamplePlan()
        lib.call("howl_resample_plan", sr_in, sr_out, ctypes.byref(plan))
        n = lib.cdll.howl_resample_bank_floats(ctypes.byref(plan))
        assert n == plan.up * plan.taps
        bank = np.full(n + 8, np.float32(7.0))                        # eight floats behind the bank stay as they are
        lib.call("howl_resample_bank", ctypes.byref(plan), ctypes.c_void_p(bank.ctypes.data))
        assert (bank[n:] == 7.0).all()
        _PLANS[key] = (plan, bank[:n].reshape(plan.up, plan.taps).copy())
    return _PLANS[key]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def signal(n_frames, channels, fmt, sr, seed):
    """0.2 sin(2 pi f n / sr + phase) + 0.1 U(-1, 1) per channel (peak 0.3), interleaved; int16 is round(32768 x)."""
    rng = np.random.default_rng(seed)
    n = np.arange(n_frames)[:, None]
    f = 440.0 + 170.0 * np.arange(channels)[None, :]
    x = 0.2 * np.sin(2.0 * np.pi * f * n / sr + 0.7 * np.arange(channels)[None, :]) + 0.1 * rng.uniform(-1.0, 1.0, (n_frames, channels))
    if fmt == I16:
        return np.round(32768.0 * x).astype(np.int16).reshape(-1)
    return x.astype(np.float32).reshape(-1)


def batch_lengths(U, D, taps):
    """(len, out_len) of the ragged batch of 7: one frame; taps/2 - 1 frames (all edge); one output tile minus 1, exactly one, one
    plus 1; about three tiles; one clip capped below its full length."""
    def for_outputs(n_out):
        length = -((-n_out * D) // U)
        assert full_len(length, U, D) >= n_out
        return length, n_out
    out = [(1, full_len(1, U, D)), (taps // 2 - 1, full_len(taps // 2 - 1, U, D))]
    out += [for_outputs(TILE - 1), for_outputs(TILE), for_outputs(TILE + 1), for_outputs(3 * TILE - 59)]
    length, _ = for_outputs(TILE + 150)
    out.append((length, full_len(length, U, D) - 97))
    return out


def layout(pairs, src_gap=(37, 5, 11, 3, 29, 1, 17, 9), dst_gap=(13, 7, 1, 19, 3, 31, 5, 2)):
    """Records with sources and destinations at odd offsets and gaps between them; -> (records, source frames, output floats)."""
    rec = np.zeros(len(pairs), CLIP_DTYPE)
    s = d = 0
    for b, (length, out_len) in enumerate(pairs):
        s += src_gap[b % len(src_gap)]
        d += dst_gap[b % len(dst_gap)]
        rec[b] = (s, d, length, out_len)
        s += length
        d += out_len
    return rec, s + src_gap[-1], d + dst_gap[-1]


def written_mask(rec, total):
    m = np.zeros(total, bool)
    for r in rec:
        m[int(r["dst_off"]):int(r["dst_off"]) + int(r["out_len"])] = True
    return m


# ---- the call ---------------------------------------------------------------------------------------------------------------
def run(al, lib, plan, bank, src, fmt, channels, rec, total):
    """One ``howl_resample_clips`` call with every operand a buffer of allocator ``al`` (the records twice: the host copy the entry
    point validates and the allocator's copy the kernel reads); the output is sentinel-filled, exactly the records' ranges are
    promised.  Returns the whole output buffer."""
    from guard_mem import sentinel_mask
    words = np.ascontiguousarray(rec).view(np.int64)
    s = al.buf("src", src.shape, src.dtype, src)
    k = al.buf("bank", bank.size, np.float32, np.ascontiguousarray(bank).reshape(-1))
    r = al.buf("clips", words.shape, np.int64, words)
    mask = written_mask(rec, total)
    o = al.buf("out", total, np.float32, "sentinel", promised=mask)
    host = np.ascontiguousarray(rec)
    lib.call("howl_resample_clips", al.ptr(s), int(src.size), fmt, channels, al.ptr(k), int(bank.size), ctypes.byref(plan),
             ctypes.c_void_p(host.ctypes.data), al.ptr(r), len(host), al.ptr(o), total, None)
    al.sync()
    out = np.array(al.get(o))
    assert sentinel_mask(out)[~mask].all(), "an output outside [dst_off, dst_off + out_len) was written"
    assert not sentinel_mask(out)[mask].any(), "a promised output was not written"
    return out


def split(out, rec):
    return [out[int(r["dst_off"]): int(r["dst_off"]) + int(r["out_len"])] for r in rec]


def make_source(rec, n_frames, channels, fmt, sr, seed=0):
    """A source buffer of ``n_frames`` frames: junk between the clips (never read into a result), each clip its own signal."""
    src = signal(n_frames, channels, fmt, sr, seed + 1000)
    clips = []
    for b, r in enumerate(rec):
        c = signal(int(r["len"]), channels, fmt, sr, seed + b)
        o = int(r["src_off"]) * channels
        src[o:o + c.size] = c
        clips.append(c)
    return src, clips


# ---- checks shared by the emulator (guard_mem.Arena) and the device (guard_mem.Banded) tests ---------------------------------------
def check_bank(al, lib, sr_in, report=print):
    """The library's plan and bank against Fraction / integer ceil and the float64 formula: every entry within one float32
    rounding of the formula (2^-24 |value|, plus 1e-12 for the two float64 evaluations), exact zeros at |t| >= Z and in the
    padding, the non-zero taps per output of the issue's table."""
    plan, bank = plan_and_bank(lib, sr_in)
    U, D = ratio(sr_in)
    assert (plan.up, plan.down, plan.sr_in, plan.sr_out) == (U, D, sr_in, TARGET)
    assert plan.s == min(1.0, U / D) and plan.taps % 4 == 0 and plan.taps - 4 < plan.j_hi - plan.j_lo + 1 <= plan.taps
    for length in (1, 2, 3, 159, 160, 441, 442, 16000, 44100, 48001, (1 << 24) - 1):
        assert lib.cdll.howl_resample_out_len(ctypes.byref(plan), length) == full_len(length, U, D) == math.ceil(Fraction(length * U, D))
    want = formula_bank(U, D, plan.j_lo, plan.taps)
    err = np.abs(bank.astype(np.float64) - want)
    assert (err <= EPS * np.abs(want) + 1e-12).all(), float(err.max())
    assert (bank[want == 0.0] == 0.0).all()
    p = np.arange(U)[:, None]
    j = (plan.j_lo + np.arange(plan.taps))[None, :]
    outside = np.abs(p - j * U) >= Z * max(U, D)
    assert (bank[outside] == 0.0).all() and not outside[:, :plan.j_hi - plan.j_lo + 1].all(axis=0).any()     # no column is spare
    nonzero = int((~outside).sum(axis=1).max())
    # one step beyond the range every phase is silent
    assert (np.abs(p - (plan.j_lo - 1) * U) >= Z * max(U, D)).all() and (np.abs(p - (plan.j_hi + 1) * U) >= Z * max(U, D)).all()
    report(f"resample {sr_in} -> {TARGET}: U/D = {U}/{D}, taps {plan.taps} (j {plan.j_lo}..{plan.j_hi}), non-zero per output <= {nonzero}, "
           f"bank error {float(err.max()):.2e}")
    return nonzero


def check_kernel(al, lib, sr_in, fmt_name, report=print):
    """The ragged batch of 7 of one rate pair in one sample format against the float64 restatement (the bank as read back from the
    library, means and sums in float64), within the derived bound; everything outside the clips' ranges keeps the sentinel."""
    fmt, channels = FORMATS[fmt_name]
    plan, bank = plan_and_bank(lib, sr_in)
    U, D = plan.up, plan.down
    rec, n_frames, total = layout(batch_lengths(U, D, plan.taps))
    src, clips = make_source(rec, n_frames, channels, fmt, sr_in, seed=sr_in % 977)
    got = split(run(al, lib, plan, bank, src, fmt, channels, rec, total), rec)
    worst = 0.0
    for b, (r, c, g) in enumerate(zip(rec, clips, got)):
        absx = np.abs(c.astype(np.float64) / (32768.0 if fmt == I16 else 1.0)).reshape(-1, channels).mean(axis=1)
        ref, mag = restate(mono64(c, channels), bank, U, D, plan.j_lo, int(r["out_len"]), absx)
        lim = bound(plan.taps, channels, mag)
        err = np.abs(g.astype(np.float64) - ref)
        assert np.isfinite(g).all() and len(g) == int(r["out_len"])
        share = float(np.max(err / np.maximum(lim, 1e-300)))
        worst = max(worst, share)
        assert (err <= lim).all(), (sr_in, fmt_name, b, float(err.max()), float(lim[np.argmax(err)]))
    report(f"resample {sr_in} {fmt_name}: worst error {100 * worst:.1f} % of the bound")
    return worst


def check_tones(al, lib, report=print):
    """What the filter does, at 44.1 kHz float32 mono: a 1 kHz tone of amplitude 0.3 against the analytic tone at 16 kHz over the
    outputs at least ``taps`` from either end (the device may miss it by the restatement's own error plus the bound of
    check_kernel), and a 9.6 kHz tone -- above the new Nyquist -- whose output RMS is within that bound of the restatement's."""
    sr = 44100
    plan, bank = plan_and_bank(lib, sr)
    U, D = plan.up, plan.down
    n_in = 6615                                                        # 0.15 s -> 2400 outputs
    n = np.arange(n_in)
    figures = {}
    for name, f in (("1 kHz", 1000.0), ("9.6 kHz", 9600.0)):
        x = (0.3 * np.sin(2.0 * np.pi * f * n / sr)).astype(np.float32)
        rec, n_frames, total = layout([(n_in, full_len(n_in, U, D))])
        src = np.zeros(n_frames, np.float32)
        src[int(rec[0]["src_off"]):int(rec[0]["src_off"]) + n_in] = x
        got = split(run(al, lib, plan, bank, src, F32, 1, rec, total), rec)[0].astype(np.float64)
        ref, mag = restate(x, bank, U, D, plan.j_lo, None, np.abs(x.astype(np.float64)))
        lim = bound(plan.taps, 1, mag)
        keep = slice(plan.taps, len(ref) - plan.taps)
        assert len(got) == len(ref) == 2400
        if f < TARGET / 2:
            tone = 0.3 * np.sin(2.0 * np.pi * f * np.arange(len(ref)) / TARGET)
            e_ref, e_dev = float(np.max(np.abs(ref - tone)[keep])), float(np.max(np.abs(got - tone)[keep]))
            figures[name] = e_ref
            report(f"resample {name} tone at {sr}: restatement error {e_ref:.3e}, device error {e_dev:.3e}, bound {float(lim[keep].max()):.3e}")
            assert e_ref < 1e-6                                        # the filter passes the tone (recorded: 1.1e-8 .. 2.3e-8)
            assert e_dev <= e_ref + float(lim[keep].max())
        else:
            r_ref, r_dev = float(np.sqrt(np.mean(ref[keep] ** 2))), float(np.sqrt(np.mean(got[keep] ** 2)))
            figures[name] = r_ref
            report(f"resample {name} tone at {sr}: restatement RMS {r_ref:.3e}, device RMS {r_dev:.3e}, bound {float(lim[keep].max()):.3e}")
            assert r_ref < 1e-6                                        # the filter stops the tone (recorded: 4e-10 .. 7e-9)
            assert abs(r_dev - r_ref) <= float(lim[keep].max())
        assert (np.abs(got - ref) <= lim).all()
    return figures


def check_exact(al, lib):
    """The properties without tolerance: identity at 16 kHz mono int16, the float32 channel mean at 16 kHz stereo, and the same
    bits for a clip alone, in a batch, at another dst_off, at another src_off, in a dense row and in the ragged flat bank."""
    # U = D = 1
    plan, bank = plan_and_bank(lib, TARGET)
    assert (plan.up, plan.down, plan.taps, plan.j_lo, plan.j_hi) == (1, 1, 4, 0, 0) and bank.tolist() == [[1.0, 0.0, 0.0, 0.0]]
    for channels in (1, 2):
        rec, n_frames, total = layout([(700, 700), (1, 1), (257, 200)])
        src, clips = make_source(rec, n_frames, channels, I16, TARGET, seed=3)
        got = split(run(al, lib, plan, bank, src, I16, channels, rec, total), rec)
        for r, c, g in zip(rec, clips, got):
            want = mono32(c, channels)[:int(r["out_len"])]
            if channels == 1:
                assert np.array_equal(want, c.astype(np.float32)[:len(want)] / 32768.0)
            assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
    # neighbours, dst_off, src_off, destination layout: 44.1 kHz stereo int16 and 48 kHz mono float32 (both row sources)
    for sr, fmt, channels in ((44100, I16, 2), (48000, F32, 1)):
        plan, bank = plan_and_bank(lib, sr)
        U, D = plan.up, plan.down
        pairs = batch_lengths(U, D, plan.taps)
        rec, n_frames, total = layout(pairs)
        src, clips = make_source(rec, n_frames, channels, fmt, sr, seed=9)
        batch = split(run(al, lib, plan, bank, src, fmt, channels, rec, total), rec)
        which = 5                                                      # the clip of about three tiles
        length, out_len = pairs[which]
        for src_gap, dst_gap in (((0,), (0,)), ((TILE,), (TILE,)), ((101,), (3,)), ((2,), (1021,))):
            one, frames, tot = layout([pairs[which]], src_gap, dst_gap)
            s1 = signal(frames, channels, fmt, sr, 77)
            o = int(one[0]["src_off"]) * channels
            s1[o:o + clips[which].size] = clips[which]
            alone = split(run(al, lib, plan, bank, s1, fmt, channels, one, tot), one)[0]
            assert np.array_equal(alone.view(np.uint32), batch[which].view(np.uint32)), (sr, src_gap, dst_gap)
        # dense rows (dst_off = i * max_len, out_len capped: truncate_length) against the ragged flat bank (4-aligned starts)
        max_len = TILE + 40
        dense, ragged = rec.copy(), rec.copy()
        at = 0
        for b in range(len(rec)):
            cap = min(full_len(int(rec[b]["len"]), U, D), max_len)
            dense[b]["out_len"] = ragged[b]["out_len"] = cap
            dense[b]["dst_off"], ragged[b]["dst_off"] = b * max_len, at
            at += (cap + 3) & ~3
        d = split(run(al, lib, plan, bank, src, fmt, channels, dense, len(rec) * max_len), dense)
        g = split(run(al, lib, plan, bank, src, fmt, channels, ragged, at), ragged)
        for b, (x, y) in enumerate(zip(d, g)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
            full = batch[b][:len(x)]
            assert np.array_equal(x[:len(full)].view(np.uint32), full.view(np.uint32))      # a capped clip is a prefix of the whole


def write_wav(path, samples_i16, sr, channels):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(samples_i16, dtype="<i2").tobytes())


BANK_KINDS = ((16000, 1), (44100, 2), (48000, 1), (8000, 1))


def check_banks(tmp_path, device, lib, report=print):
    """Twelve int16 clips of 0.2 .. 0.6 s at 16000/1ch, 44100/2ch, 48000/1ch and 8000/1ch through both ``from_files``: every clip
    against the float64 restatement within check_kernel's bound, lengths, 4-aligned offsets, zero padding, truncation at
    ``max_len``; and an all-16 kHz-mono set through ``from_files`` and through the constructors with ``read_wav16k``: equal bits.
    ``lib`` is the library the package runs on (for the bank the restatement reads)."""
    import torch
    from types import SimpleNamespace
    from howl_amd.training.data import ClipBank, WakeWordClipBank, read_wav, read_wav16k
    rng = np.random.default_rng(8)
    paths, raws, kinds = [], [], []
    for i in range(12):
        sr, channels = BANK_KINDS[i % 4]
        frames = int(sr * rng.uniform(0.2, 0.6))
        raw = signal(frames, channels, I16, sr, 50 + i)
        paths.append(tmp_path / f"clip{i:02d}.wav")
        write_wav(paths[-1], raw, sr, channels)
        got, r, c = read_wav(paths[-1])
        assert (r, c) == (sr, channels) and got.dtype == np.int16 and np.array_equal(got, raw)
        raws.append(raw)
        kinds.append((sr, channels))
    meta = [SimpleNamespace(path=p, transcription="", end_timestamps=None) for p in paths]
    refs = []
    for raw, (sr, channels) in zip(raws, kinds):
        plan, bank = plan_and_bank(lib, sr)
        absx = np.abs(raw.astype(np.float64) / 32768.0).reshape(-1, channels).mean(axis=1)
        ref, mag = restate(mono64(raw, channels), bank, plan.up, plan.down, plan.j_lo, None, absx)
        refs.append((ref, bound(plan.taps, channels, mag)))
        assert len(ref) == full_len(len(raw) // channels, *ratio(sr))
    lengths = [len(r) for r, _ in refs]

    ww = WakeWordClipBank.from_files(paths, meta, None, device)
    flat = ww.flat.cpu().numpy()
    at, seen = 0, np.zeros(flat.size, bool)
    for i, (ref, lim) in enumerate(refs):
        assert ww.offsets[i] == at and at % 4 == 0 and ww.examples[i].num_samples == lengths[i] and int(ww.lengths[i]) == lengths[i]
        got = ww.clip(i).cpu().numpy()
        assert (np.abs(got.astype(np.float64) - ref) <= lim).all(), i
        seen[at:at + lengths[i]] = True
        at += (lengths[i] + 3) & ~3
    assert flat.size == at and ww.max_len == max(lengths) and len(ww) == 12 and not flat[~seen].any()
    assert ww.rows.shape == (at, 1)

    max_len = 5000
    assert min(lengths) < max_len < max(lengths)
    cb = ClipBank.from_files(paths, list(range(12)), max_len, device)
    audio = cb.audio.cpu().numpy()
    assert audio.shape == (12, max_len) and cb.labels.cpu().tolist() == list(range(12)) and cb.max_len == max_len
    assert cb.lengths_host.tolist() == [min(n, max_len) for n in lengths] == cb.lengths.cpu().tolist()
    for i, (ref, lim) in enumerate(refs):
        n = min(lengths[i], max_len)
        assert (np.abs(audio[i, :n].astype(np.float64) - ref[:n]) <= lim[:n]).all(), i
        assert not audio[i, n:].any()
        assert np.array_equal(audio[i, :n], ww.clip(i).cpu().numpy()[:n])              # dense rows and the flat bank: the same bits

    # 16 kHz mono int16 files: from_files is the constructor's bank, bit for bit
    plain = [p for p, k in zip(paths, kinds) if k == (16000, 1)]
    more = tmp_path / "one_sample.wav"
    write_wav(more, np.asarray([-32768], np.int16), 16000, 1)
    plain.append(more)
    pmeta = [SimpleNamespace(path=p, transcription="", end_timestamps=None) for p in plain]
    a, b = WakeWordClipBank.from_files(plain, pmeta, None, device), WakeWordClipBank([read_wav16k(p) for p in plain], pmeta, None, device)
    assert torch.equal(a.flat, b.flat) and a.offsets == b.offsets and torch.equal(a.lengths, b.lengths) and a.max_len == b.max_len
    assert [(e.clip_id, e.num_samples) for e in a.examples] == [(e.clip_id, e.num_samples) for e in b.examples]
    a = ClipBank.from_files(plain, [0] * len(plain), 4000, device)
    b = ClipBank([read_wav16k(p) for p in plain], [0] * len(plain), 4000, device)
    assert torch.equal(a.audio, b.audio) and torch.equal(a.lengths, b.lengths) and torch.equal(a.lengths_host, b.lengths_host)
    assert torch.equal(a.labels, b.labels)
    report(f"resample banks: {len(paths)} clips, lengths {min(lengths)}..{max(lengths)}")


def check_refusals(lib, error):
    """Every refusal of the header with its status (-1) and message; the output keeps its bytes (host arrays: nothing launches)."""
    import pytest
    from guard_mem import fill_sentinel, sentinel_mask
    from howl_amd.lib import HowlResamplePlan
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for sr_in, sr_out in ((44101, 16000), (3999, 16000), (192001, 16000), (16000, 3999), (11025, 16001), (192000, 4000)):
        plan = HowlResamplePlan()
        with pytest.raises(error, match=rf"howl_resample_plan failed \(-1\): howl_resample_plan: {sr_in} Hz -> {sr_out} Hz unsupported"):
            lib.call("howl_resample_plan", sr_in, sr_out, ctypes.byref(plan))
    plan, bank = plan_and_bank(lib, 44100)
    bank = np.ascontiguousarray(bank).reshape(-1)
    src = signal(3000, 2, I16, 44100, 1)
    out = np.zeros(2000, np.float32)
    fill_sentinel(out)
    ok = np.zeros(1, CLIP_DTYPE)
    ok[0] = (10, 5, 2000, full_len(2000, 160, 441))

    def attempt(rec, B=None, plan=plan, bank_floats=bank.size, fmt=I16, channels=2, src_elems=src.size, out_floats=out.size):
        host = np.ascontiguousarray(rec)
        lib.call("howl_resample_clips", p(src), src_elems, fmt, channels, p(bank), bank_floats, ctypes.byref(plan), p(host), p(host),
                 len(host) if B is None else B, p(out), out_floats, None)

    def refused(pattern, rec=ok, **kw):
        with pytest.raises(error, match=r"howl_resample_clips failed \(-1\): howl_resample_clips: " + pattern):
            attempt(rec, **kw)
        assert sentinel_mask(out).all()

    for B in (0, 8193):
        refused(rf"B={B} clips unsupported", np.repeat(ok, max(B, 1)), B=B)
    long = ok.copy()
    long["len"] = (1 << 24) + 1
    refused(r"clip 0: len=16777217 frames unsupported", long, src_elems=1 << 26)
    empty = ok.copy()
    empty["len"] = 0
    refused(r"clip 0: len=0 frames unsupported", empty)
    over = ok.copy()
    over["out_len"] += 1
    refused(r"clip 0: out_len=727; len=2000 at 160/441 gives at most 726", over)
    neg = ok.copy()
    neg["out_len"] = -1
    refused(r"clip 0: out_len=-1", neg)
    far = ok.copy()
    far["src_off"] = 1001
    refused(r"clip 0: source frames \[1001, \+2000\) outside the buffer of 3000 frames", far)
    far["src_off"] = -1
    refused(r"clip 0: source frames \[-1, \+2000\) outside", far)
    far = ok.copy()
    far["dst_off"] = out.size - 725
    refused(r"clip 0: output \[1275, \+726\) outside the destination of 2000 floats", far)
    far["dst_off"] = -1
    refused(r"clip 0: output \[-1, \+726\) outside", far)
    second = np.repeat(ok, 2)
    second[1]["dst_off"] = 1500
    refused(r"clip 1: output \[1500, \+726\) outside", second)
    refused(rf"bank of {bank.size - 4} floats; the plan for 44100 Hz -> 16000 Hz has 160 x {plan.taps}", bank_floats=bank.size - 4)
    for field, value in (("taps", plan.taps + 4), ("j_lo", plan.j_lo - 1), ("up", 1), ("s", 1.0), ("sr_in", 44101)):
        bad = HowlResamplePlan.from_buffer_copy(plan)
        setattr(bad, field, value)
        refused(r"the plan is not howl_resample_plan's for \d+ Hz -> 16000 Hz", plan=bad)
        assert lib.cdll.howl_resample_bank_floats(ctypes.byref(bad)) == 0 and lib.cdll.howl_resample_out_len(ctypes.byref(bad), 100) == 0
        scratch = np.zeros(4, np.float32)
        with pytest.raises(error, match=r"howl_resample_bank: the plan is not"):
            lib.call("howl_resample_bank", ctypes.byref(bad), p(scratch))
        assert not scratch.any()
    refused(r"format=2 unsupported", fmt=2)
    for channels in (0, 9):
        refused(rf"channels={channels} unsupported \(1\.\.8\)", channels=channels)
    # what is not refused: out_len 0 (nothing to write, nothing launched)
    none = ok.copy()
    none["out_len"] = 0
    attempt(none)
    assert sentinel_mask(out).all()
