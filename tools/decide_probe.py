"""`howl_decide_clips` alone between two HIP events, away from the engines: N = 4 / 64 / 4096 clips of 241 frames in both modes, each
launch timed after idle and right behind a burst of three 8192^3 matmuls (are low clocks on a 16-workgroup launch part of its time?).
Seeded synthetic probabilities (the generator of tests/decide_util.py: a piecewise-constant label track with 30 % blank frames, the
same 64 clips for both modes); a window of 2000 ms; smoothing 0 ms (a ring of one frame) and 50 ms (five frames in sequence
mode, one in frame mode).  What it is for: the launch's time as a function of its inputs, apart from the engines' models.  Prints one line per
case: median of 30 launches after 10."""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def random_probs(rng, mode, C, T):
    import numpy as np
    track = np.empty(T, np.int64)
    t = 0
    while t < T:
        dwell = int(rng.integers(1, 13 if mode == 0 else 5))
        track[t:t + dwell] = rng.integers(0, min(C, 3)) if rng.random() < 0.35 else rng.integers(0, C)
        t += dwell
    if mode == 0:
        track[rng.random(T) < 0.3] = C - 1
    z = rng.standard_normal((T, C))
    z[np.arange(T), track] += 6.0 * rng.random(T)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def main():
    import numpy as np
    import torch
    from howl_amd import ops
    from howl_amd.model.decision import DeviceDecider
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    T, C = 241, 5
    base = np.stack([random_probs(rng, 0, C, T) for _ in range(64)])
    big = torch.randn(8192, 8192, device=dev)
    cases = [(0, 0.0, 4), (0, 0.0, 64), (0, 0.0, 4096), (0, 50.0, 64), (1, 50.0, 4), (1, 50.0, 64), (1, 50.0, 4096), (1, 0.0, 64)]
    for mode, smoothing, N in cases:
        delta = 12.5 if mode == 0 else 63.0
        dd = DeviceDecider(mode, C, 4, 3, 0.0, smoothing, 2000.0, 500.0, [0, 1, 2] * 3)
        cfg, keep = dd._config(dev)
        if True:
            probs = torch.from_numpy(np.tile(base, (max(1, N // 64), 1, 1))[:N]).to(dev)
            nf = torch.full((N,), T, dtype=torch.int32, device=dev)
            dl = torch.full((N,), delta, dtype=torch.float64, device=dev)
            for burst in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                us = []
                for _ in range(40):
                    if burst:
                        for _ in range(3):
                            big @ big
                    e0.record()
                    ops.decide_clips(cfg, probs, nf, dl, T)
                    e1.record()
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3)
                med = statistics.median(us[10:])
                print(f"mode {mode} smoothing_ms={smoothing:4.0f} N={N:5d} frames={T} behind_matmul_burst={burst}: launch {med:9.1f} us = {med / T:6.2f} us per frame", flush=True)


if __name__ == "__main__":
    main()
