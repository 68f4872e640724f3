"""`howl_ctc_loss_long` alone between two HIP events: loss + gradient at T = 1000 frames, B = 64, C = 5 with every target of 31,
63, 127 and 255 labels (the kernel bodies with 1, 2, 4 and 8 states per lane), and in the same process, alternating with it,
`howl_ctc_loss` at 31 labels (the same kernel body: the two times must agree within the run-to-run spread) and torch's device
`F.ctc_loss` + backward on log_softmax of the same logits (the reference's path, for orientation).  Seeded logits; targets without
a label twice in a row, so L frames align them.  Prints one line per case: median and 10th / 90th percentile of 50 timed calls after
10 warm-up calls, and for the library's kernels the time per dependent time step (2 T - window steps per utterance).
`--out FILE` also appends the lines to FILE."""
import ctypes
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

T, B, C, BLANK = 1000, 64, 5, 4
WARMUP, TIMED = 10, 50


def main():
    import numpy as np
    import torch
    from howl_amd import lib
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None
    dev = torch.device("cuda:0")
    L = lib.get()
    rng = np.random.default_rng(0)
    logits = torch.from_numpy(rng.normal(0, 2.0, (B, T, C)).astype(np.float32)).to(dev)      # (B, T, C), addressed as (T, B, C)
    in_len = torch.full((B,), T, dtype=torch.int64, device=dev)
    nll = torch.empty(B, device=dev)
    loss = torch.empty((), device=dev)
    dz = torch.empty_like(logits)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def say(line):
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()

    def timed(fn):
        us = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(WARMUP + TIMED):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us = sorted(us[WARMUP:])
        return statistics.median(us), us[len(us) // 10], us[-1 - len(us) // 10]

    def library_call(entry, labels):
        targets = ((torch.arange(labels)[None, :] + torch.arange(B)[:, None]) % (C - 1)).to(dev)
        tl = torch.full((B,), labels, dtype=torch.int64, device=dev)
        if entry == "howl_ctc_loss":
            nws, window = int(L.cdll.howl_ctc_workspace_floats(T, B)), 128
        else:
            nws, window = int(L.cdll.howl_ctc_long_workspace_floats(T, B, labels)), int(L.cdll.howl_ctc_long_window_rows(labels))
        ws = torch.empty(nws, device=dev)
        fn = lambda: L.call(entry, vp(logits), C, T * C, T, B, C, vp(targets), labels, labels, vp(in_len), vp(tl), BLANK, vp(nll), vp(loss),
                            vp(dz), C, T * C, vp(ws), nws, stream)
        return fn, window, (targets, tl, ws)

    def vendor_call(labels):
        targets = ((torch.arange(labels)[None, :] + torch.arange(B)[:, None]) % (C - 1)).to(dev)
        tl = torch.full((B,), labels, dtype=torch.int64, device=dev)
        z = logits.clone().requires_grad_(True)

        def fn():
            z.grad = None
            lp = torch.log_softmax(z.permute(1, 0, 2), -1)
            torch.nn.functional.ctc_loss(lp, targets, in_len, tl, BLANK).backward()
        return fn

    def report(name, labels, med, lo, hi, window=None):
        per_step = "" if window is None else f" = {med * 1e3 / (2 * T - min(window, T)):7.1f} ns per dependent time step"
        say(f"{name:<34} T={T} B={B} C={C} labels={labels:3d}: {med:9.1f} us (p10 {lo:9.1f}, p90 {hi:9.1f}){per_step}")

    # 31 labels: the short entry and the long entry run the same kernel body -- alternate them, three rounds each
    short_fn, w, keep_a = library_call("howl_ctc_loss", 31)
    long_fn, _, keep_b = library_call("howl_ctc_loss_long", 31)
    for rnd in range(3):
        report(f"howl_ctc_loss (round {rnd})", 31, *timed(short_fn), window=w)
        report(f"howl_ctc_loss_long (round {rnd})", 31, *timed(long_fn), window=w)
    for labels in (63, 127, 255):
        fn, w, keep = library_call("howl_ctc_loss_long", labels)
        report("howl_ctc_loss_long", labels, *timed(fn), window=w)
    for labels in (31, 63, 127, 255):
        report("torch log_softmax + F.ctc_loss + bwd", labels, *timed(vendor_call(labels)))
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
