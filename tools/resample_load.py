"""The resample launch and the banks' ``from_files`` on 512 clips of 1 s, in one run, for two sources: 48 kHz mono int16 and
44.1 kHz stereo int16 (both -> 16 kHz).

Protocol (one process, one card):

* ``cpu``: for scale and before the device is opened, ``scipy.signal.resample_poly`` with the same prototype (rebuilt from the
  library's bank) on the channel mean of the same clips, dealt to ``--workers`` processes (default 16); wall time of the whole set,
  best of 2.  Skipped, and said so, if scipy does not import.
* ``launch``: ``howl_resample_clips`` alone -- samples, bank and records already on the device, the destination a ragged flat
  bank -- 5 launches of warm-up, then ``--repeats`` repeats of ``--steps`` launches each between two HIP events, one synchronise
  per repeat, the two sources alternating repeat by repeat; the MEDIAN repeat is the time.  Next to it the algorithm's FLOP,
  2 x (non-zero taps per output) x outputs, and that rate as a share of the vector fp32 peak (157.3 TFLOP/s).
* ``from_files``: ``WakeWordClipBank.from_files`` and ``ClipBank.from_files`` on the same 512 wav files (written to a temporary
  directory), end to end: headers, reading, upload, launch, one synchronise; host clock, median of ``--repeats`` after one warm-up.

Prints one JSON line and writes it, under the command that produced it, to ``--out`` (default profiles/resample.txt)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
os.environ.setdefault("NUM_MELS", "40")

PEAK_VECTOR_FP32 = 157.3e12
SOURCES = (("48000x1", 48000, 1), ("44100x2", 44100, 2))
_CPU = {}


def make_clips(sr, channels, n_clips, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    n = np.arange(sr)[:, None]
    out = []
    for k in range(n_clips):
        f = 200.0 + 11.0 * (k % 97) + 60.0 * np.arange(channels)[None, :]
        x = 0.2 * np.sin(2.0 * np.pi * f * n / sr) + 0.1 * rng.uniform(-1.0, 1.0, (sr, channels))
        out.append(np.round(32767.0 * x).astype(np.int16).reshape(-1))
    return out


def prototype_from_bank(bank, up, j_lo):
    """The polyphase bank laid out as ONE FIR at rate up x sr_in (tap m = p - j up), for ``resample_poly(..., window=)``."""
    import numpy as np
    taps = bank.shape[1]
    p = np.arange(up)[:, None]
    m = p - (j_lo + np.arange(taps)[None, :]) * up
    L = int(np.abs(m).max())
    proto = np.zeros(2 * L + 1)
    proto[m + L] = bank
    return proto


def _cpu_init(proto, up, down, channels):
    _CPU.update(proto=proto, up=up, down=down, channels=channels)


def _cpu_one(raw):
    import numpy as np
    from scipy.signal import resample_poly
    x = (raw.astype(np.float32) / 32768.0).reshape(-1, _CPU["channels"]).mean(axis=1)
    return len(resample_poly(x, _CPU["up"], _CPU["down"], window=_CPU["proto"]) / _CPU["up"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "resample.txt"))
    args = ap.parse_args()
    import numpy as np
    from howl_amd import ops
    N = args.clips
    clips = {name: make_clips(sr, ch, N, seed=sr) for name, sr, ch in SOURCES}
    plans = {name: ops.resample_plan(sr, 16000) for name, sr, ch in SOURCES}            # host only: the device is still closed

    # ---- cpu: scipy, before this process opens the device (the workers never do) ----
    cpu_ms, cpu_note = {}, None
    try:
        import scipy
        from multiprocessing import get_context
        for name, sr, ch in SOURCES:
            plan, bank = plans[name]
            proto = prototype_from_bank(bank.astype(np.float64), plan.up, plan.j_lo)
            with get_context("spawn").Pool(args.workers, initializer=_cpu_init, initargs=(proto, plan.up, plan.down, ch)) as pool:
                best = None
                for _ in range(2):
                    t0 = time.perf_counter()
                    lens = pool.map(_cpu_one, clips[name], chunksize=max(1, N // (4 * args.workers)))
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                assert all(n == 16000 for n in lens)
            cpu_ms[name] = round(best * 1e3, 1)
        cpu_note = f"scipy {scipy.__version__} resample_poly, {args.workers} processes, channel mean included, best of 2"
    except ImportError as e:
        cpu_note = f"scipy does not import here ({e}): device numbers alone"

    import torch
    from howl_amd.training.data import ClipBank, WakeWordClipBank
    from types import SimpleNamespace
    dev = torch.device("cuda:0")
    launches, flop = {}, {}
    for name, sr, ch in SOURCES:
        plan, bank = plans[name]
        src = torch.from_numpy(np.concatenate(clips[name])).to(dev)
        bank_dev = torch.from_numpy(bank).reshape(-1).to(dev)
        rec = ops.resample_records([sr * k for k in range(N)], [sr] * N, [16000 * k for k in range(N)], [16000] * N)
        rec_dev = torch.from_numpy(rec.view(np.int64).copy()).to(dev)
        out = torch.zeros(16000 * N, device=dev)
        launches[name] = (lambda a=(src, ch, plan, bank_dev, rec, rec_dev, out): ops.resample_clips(*a))
        nonzero = int((bank != 0).sum(axis=1).max())
        flop[name] = dict(nonzero_taps=nonzero, row_taps=plan.taps, outputs=16000 * N, flop=2 * nonzero * 16000 * N)
    for fn in launches.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in launches}
    for _ in range(args.repeats):
        for name, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    med = {name: statistics.median(v) for name, v in us.items()}

    files_ms = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, sr, ch in SOURCES:
            paths = []
            for k, raw in enumerate(clips[name]):
                paths.append(Path(tmp) / f"{name}_{k:04d}.wav")
                with wave.open(str(paths[-1]), "wb") as w:
                    w.setnchannels(ch)
                    w.setsampwidth(2)
                    w.setframerate(sr)
                    w.writeframes(raw.tobytes())
            meta = [SimpleNamespace(path=p, transcription="", end_timestamps=None) for p in paths]
            for kind, make in (("WakeWordClipBank", lambda: WakeWordClipBank.from_files(paths, meta, None, dev)),
                               ("ClipBank", lambda: ClipBank.from_files(paths, [0] * N, 16000, dev))):
                times = []
                for r in range(args.repeats + 1):
                    t0 = time.perf_counter()
                    bank_obj = make()
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                    del bank_obj
                files_ms[f"{kind}.{name}"] = round(statistics.median(times[1:]), 1)

    result = {
        "metric": f"{N} clips x 1 s -> 16 kHz; launch: us between HIP events ({args.repeats} repeats of {args.steps} launches, alternating; "
                  f"medians); from_files: ms end to end, host clock, median of {args.repeats}",
        "launch_us": {name: [round(v, 1) for v in vals] for name, vals in us.items()},
        "launch_us_median": {name: round(v, 1) for name, v in med.items()},
        "work": flop,
        "launch_tflops": {name: round(flop[name]["flop"] / med[name] / 1e6, 2) for name in med},
        "launch_share_of_vector_fp32_peak": {name: round(flop[name]["flop"] / (med[name] * 1e-6) / PEAK_VECTOR_FP32, 4) for name in med},
        "from_files_ms": files_ms,
        "cpu_ms": cpu_ms, "cpu": cpu_note,
    }
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("python tools/resample_load.py " + " ".join(sys.argv[1:]) + "   # on " + torch.cuda.get_device_name(0) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
