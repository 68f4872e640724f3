"""Latency of the live client's window, eager launch chain against the one-launch streaming kernel (Res8StreamSession).

Protocol: wall time per window of ``FrameInferenceEngine.ingest_frame``, from the call to the label, host copy included; 500 ms
windows at a 63 ms stride over the 10 s synthetic clips that ``bench.py --config eval`` uses; 200 windows of warm-up per path, then
five repeats of 1000 windows each, the MEDIAN of each repeat; eager (``fused_windows = False``) and fused alternate repeat by repeat,
in one process, on one card.  In addition, for N = 64 and N = 256 windows per launch: ``Res8StreamSession.probabilities`` alone
between two HIP events beside ``engine.window_probabilities`` on the same windows (wall time, host copy included: what that call
is).  Prints one JSON line.  ``--windows`` / ``--repeats`` shorten a run (a profiler pass); the protocol is the default.

``--model las``: the same protocol for the las model (LasStreamSession), with the launch alone at N = 1 as well.

``--model gru``: the protocol of ``--model las`` for the gru model (GruStreamSession), and the recurrence's time per dependent step:
for the fused kernel the slope of the launch alone at N = 1 between ``frames = 1`` (2 steps) and ``frames = T`` (22 steps), for
``gru_fwd4_kernel`` its launch (the library's HIP-event brackets around it, ``howl_profile_read``) over the 22 steps it walks.

``--model seq-lstm``: the same protocol for ``InferenceEngine.infer`` (LstmStreamSession): (a) 8000-sample chunks (what the live
client feeds), (b) 16000-sample chunks, both with the state carried from call to call; (c) ``infer_many`` on 64 clips of 1 - 3 s
against the clip-by-clip ``[reset(); infer(clip)]`` loop (per CALL of 64 clips; ``--windows`` / 20 calls per repeat); and the
kernel alone between two HIP events for each of the three shapes.

``--model decide``: case (c)'s 64 clips through ``infer_many`` with the decision logic on the host and on the device
(``device_decisions`` off / on, DeviceDecider), alternating repeat by repeat, in one process: (d) ``InferenceEngine`` (seq-lstm,
``HOWL_STREAM_FUSED=1``) with the settings of (c), (e) the same with the blank weighted down so that most frames reach the smoother
and the matcher, (f) ``FrameInferenceEngine`` (res8) on the same clips; and ``howl_decide_clips`` alone between two HIP events on
the probabilities of each.  Each pair is checked for equal results first.

``--model small-cnn``: the protocol of ``--model las`` for the small-cnn model (SmallCnnStreamSession).

``--model seq-cnn``: the protocol of ``--model seq-lstm`` for the seq-cnn model (SeqCnnStreamSession; the model carries no state), and
in addition case (c) with the decision logic on the device (``device_decisions`` on: fused + DeviceDecider against fused alone,
alternating).  The eager leg of every pair is the launch chain the engines run with the switch off."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
os.environ.setdefault("NUM_MELS", "40")


def setup(model_name, use_blank):
    """-> (context, model, std, zmuv, clips) on cuda:0: the three-word context, the eval-mode model (res8 with its closed-form state,
    the others from seed 2024), the frontend, and the ZMUV statistics of the first second of the 8 synthetic clips of 10 s."""
    import torch
    from howl_amd.context import InferenceContext
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.utils.synth import res8_closed_form_state, synthetic_pcm
    dev = torch.device("cuda:0")
    ctx = InferenceContext(["hey", "fire", "fox"], token_type="word", use_blank=use_blank)
    if model_name != "res8":
        torch.manual_seed(2024)
    if model_name in ("small-cnn", "seq-cnn"):      # (the head's width is the settings', as in the reference)
        from howl_amd.model import CnnSettings
        model = RegisteredModel.find_registered_class(model_name)(ctx.num_labels, CnnSettings(num_labels=ctx.num_labels)).to(dev)
    else:
        model = RegisteredModel.find_registered_class(model_name)(ctx.num_labels).to(dev)
    if model_name == "res8":
        model.load_state_dict(res8_closed_form_state(ctx.num_labels), strict=False)
    model.eval()
    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    clips = synthetic_pcm(8, 160000, seed=77).to(dev)
    zmuv.update(std(clips[:1, :16000]))
    return ctx, model, std, zmuv, clips


def launch_us(fn):
    """``fn()`` 60 times, each between two HIP events: the median of the last 50, us."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(60):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us[10:])


def alternate(paths, run, warm, calls, repeats):
    """``run(path, n, first)`` -> the wall times of ``n`` calls on ``path``, starting at item ``first`` of whatever it walks.  ``warm``
    calls of warm-up per path, then ``repeats`` repeats of ``calls`` calls, the paths alternating repeat by repeat
    -> {path: [the median of each repeat, us]} for the paths True and False (one that is not in ``paths``: [])."""
    for path in paths:
        run(path, warm, 0)
    medians = {True: [], False: []}
    for r in range(repeats):
        for path in paths:
            medians[path].append(statistics.median(run(path, calls, r * calls)) * 1e6)
    return medians


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--fused-only", action="store_true", help="skip the eager path (a kernel-trace pass over the one launch)")
    ap.add_argument("--eager-only", action="store_true", help="seq-lstm: skip the fused path (a kernel-trace pass over the launch chain)")
    ap.add_argument("--model", choices=["res8", "las", "gru", "seq-lstm", "decide", "small-cnn", "seq-cnn"], default="res8")
    args = ap.parse_args()
    if args.model in ("seq-lstm", "seq-cnn"):
        return main_seq_lstm(args, args.model)
    if args.model == "decide":
        return main_decide(args)
    import torch
    from howl_amd.model.inference import FrameInferenceEngine
    from howl_amd.utils import audio_utils
    ctx, model, std, zmuv, clips = setup(args.model, use_blank=False)
    engine = FrameInferenceEngine(500, 63, model, zmuv, ctx)
    starts, chunk = audio_utils.stride_starts(160000, 500, 63, 16000)
    frames = [clip[s:s + chunk] for clip in clips for s in starts]     # views: 8 x 151 windows, walked round-robin

    def run(fused, n, first):
        engine.fused_windows = fused
        engine.reset()
        times = []
        for i in range(n):
            frame = frames[(first + i) % len(frames)]
            t0 = time.perf_counter()
            engine.ingest_frame(frame, curr_time=63.0 * i)
            times.append(time.perf_counter() - t0)
        return times

    medians = alternate([True] if args.fused_only else [False, True], run, args.warmup, args.windows, args.repeats)

    many = []
    session = model.stream_session(std, zmuv)
    for n in ((1, 64, 256) if args.model in ("las", "gru", "small-cnn") else (64, 256)):
        stride = (160000 - chunk) // n // 2 * 2
        clip = clips[0, :chunk + (n - 1) * stride].contiguous()
        windows = clip.as_strided((n, chunk), (stride, 1))
        row = {"windows_per_launch": n, "fused_launch_us_median": round(launch_us(lambda: session.probabilities(windows)), 2)}
        if not args.fused_only and n > 1:
            eng = FrameInferenceEngine(500, 1000.0 * stride / 16000 + 1e-6, model, zmuv, ctx)
            assert audio_utils.stride_starts(clip.numel(), 500, eng.eval_stride_size_ms, 16000)[0] == [stride * k for k in range(n)]
            eager_us = []
            for i in range(60):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.window_probabilities(clip)
                eager_us.append((time.perf_counter() - t0) * 1e6)
            t_f = []
            for i in range(60):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                session.probabilities(windows).cpu()
                t_f.append((time.perf_counter() - t0) * 1e6)
            row["fused_call_and_host_copy_us_median"] = round(statistics.median(t_f[10:]), 2)
            row["eager_window_probabilities_us_median"] = round(statistics.median(eager_us[10:]), 2)
        many.append(row)
    per_step = gru_per_step(model, std, zmuv, session, clips[:1, :chunk]) if args.model == "gru" else None
    torch.cuda.synchronize()
    fused_m, eager_m = medians[True], medians[False]
    print(json.dumps({
        "model": args.model,
        "metric": "ingest_frame wall time per window, us (500 ms windows, 63 ms stride, 10 s synthetic clips; median of each repeat)",
        "windows_per_repeat": args.windows, "warmup_windows": args.warmup,
        "fused_us_medians": [round(v, 2) for v in fused_m], "eager_us_medians": [round(v, 2) for v in eager_m],
        "requirement_max_fused_below_min_eager": (max(fused_m) < min(eager_m)) if eager_m else None,
        "many_windows": many, **({"recurrence_us_per_dependent_step": per_step} if per_step else {})}), flush=True)


def gru_per_step(model, std, zmuv, session, window):
    """One 8000-sample window (T = 41, T1 = 22): the fused launch between two HIP events at 2 and at 22 recurrence steps -> the slope
    per dependent step; gru_fwd4_kernel between the library's own HIP events over its 22 steps."""
    import ctypes
    import torch
    from howl_amd import lib
    T = 1 + window.size(1) // 200
    t1 = (T + 4) // 2
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launch, queued = {}, {}
    for frames in (1, T):
        launch[min((frames + 4) // 2, t1)] = launch_us(lambda: session.probabilities(window, frames=frames))
        # 200 launches between one pair of events: per launch, the larger of the kernel's time and the host's time to issue it
        torch.cuda.synchronize()
        e0.record()
        for i in range(200):
            session.probabilities(window, frames=frames)
        e1.record()
        e1.synchronize()
        queued[min((frames + 4) // 2, t1)] = e0.elapsed_time(e1) * 1e3 / 200
    (s_lo, t_lo), (s_hi, t_hi) = sorted(launch.items())
    feat = std.log_mel_for_model(window, zmuv)
    lengths = std.compute_lengths(torch.tensor([window.size(1)]))
    lb = lib.get()
    for i in range(10):
        model(feat, lengths)
    torch.cuda.synchronize()
    lb.call("howl_profile_enable", 1)
    for i in range(50):
        model(feat, lengths)
    torch.cuda.synchronize()
    lb.call("howl_profile_enable", 0)
    eager = {}
    tags = ("gru_enc_fwd", "gru_fwd", "gru_head")
    for i, tag in enumerate(tags):
        tot, cnt = ctypes.c_double(), ctypes.c_int()
        lb.call("howl_profile_read", tag.encode(), ctypes.byref(tot), ctypes.byref(cnt), int(i == len(tags) - 1))
        eager[tag] = round(tot.value * 1e3 / max(cnt.value, 1), 2)
    return {"fused_launch_us": {f"{k}_steps": round(v, 2) for k, v in launch.items()},
            "fused_us_per_step": round((t_hi - t_lo) / (s_hi - s_lo), 3),
            "fused_us_per_launch_200_queued": {f"{k}_steps": round(v, 2) for k, v in queued.items()},
            "eager_launches_us": eager, "gru_fwd4_steps": t1, "gru_fwd4_us_per_step": round(eager["gru_fwd"] / t1, 3)}


def main_seq_lstm(args, model_name="seq-lstm"):
    import numpy as np
    import torch
    from howl_amd.model.inference import InferenceEngine
    ctx, model, std, zmuv, clips = setup(model_name, use_blank=True)
    model.streaming()
    engine = InferenceEngine(model, zmuv, ctx)
    engine.sequence = [0, 1, 2, 0, 1, 2, 0, 1, 2]                      # never present: every call walks all of its frames
    paths = [True] if args.fused_only else ([False] if args.eager_only else [False, True])

    def chunks_of(size):
        return [clip[s:s + size] for clip in clips for s in range(0, 160000 - size + 1, size)]

    def run_chunks(fused, chunks, n, first):
        engine.fused_chunks = fused
        engine.reset()
        times = []
        for i in range(n):
            chunk = chunks[(first + i) % len(chunks)]
            t0 = time.perf_counter()
            engine.infer(chunk)
            times.append(time.perf_counter() - t0)
        return times

    rng = np.random.default_rng(7)
    sizes = [int(v) for v in rng.integers(16000, 48001, 64)]
    many = [clips[i % 8, :n].contiguous() for i, n in enumerate(sizes)]

    def run_many(fused, n, first):
        engine.fused_chunks = fused
        times = []
        for i in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if fused:
                engine.infer_many(many)
            else:
                for clip in many:
                    engine.reset()
                    engine.infer(clip)
            times.append(time.perf_counter() - t0)
        return times

    out = {"model": model_name,
           "metric": f"InferenceEngine.infer / infer_many wall time per call, us ({model_name}, host copy included; median of each repeat)",
           "calls_per_repeat": args.windows, "warmup_calls": args.warmup}
    for name, size in (("a_8000_sample_chunks", 8000), ("b_16000_sample_chunks", 16000)):
        chunks = chunks_of(size)
        med = alternate(paths, lambda fused, n, first: run_chunks(fused, chunks, n, first), args.warmup, args.windows, args.repeats)
        out[name] = {"fused_us_medians": [round(v, 2) for v in med[True]], "eager_us_medians": [round(v, 2) for v in med[False]]}
    n_many = max(2, args.windows // 20)
    med = alternate(paths, run_many, max(1, args.warmup // 20), n_many, args.repeats)
    session = model.stream_session(std, zmuv)
    out["c_infer_many_64_clips_1_to_3_s"] = {"calls_per_repeat": n_many, "frames_per_call": sum(session.rows_of(n) for n in sizes),
                                            "fused_us_medians": [round(v, 2) for v in med[True]],
                                            "eager_loop_us_medians": [round(v, 2) for v in med[False]]}
    if model_name == "seq-cnn" and not args.eager_only:
        # (c) again, both legs fused: the decision logic on the host (False) against DeviceDecider (True)
        def run_decide(on, n, first):
            engine.device_decisions = on
            return run_many(True, n, first)
        engine.fused_chunks, engine.device_decisions = True, False
        want = (engine.infer_many(many), [list(h) for h in engine.clip_histories])
        engine.device_decisions = True
        assert (engine.infer_many(many), engine.clip_histories) == want, "the device decisions differ from the host replay"
        med = alternate([False, True], run_decide, max(1, args.warmup // 20), n_many, args.repeats)
        engine.device_decisions = False
        out["d_infer_many_64_clips_fused_decisions_host_vs_device"] = {
            "calls_per_repeat": n_many, "fused_host_decisions_us_medians": [round(v, 2) for v in med[False]],
            "fused_device_decisions_us_medians": [round(v, 2) for v in med[True]]}
    if args.eager_only:
        print(json.dumps(out), flush=True)
        return
    # the kernel alone, between two HIP events
    pad = torch.nn.utils.rnn.pad_sequence(many, batch_first=True)
    ns = torch.tensor(sizes, dtype=torch.int64, device=clips.device)
    kernel = {}
    for name, pcm, n_samples in (("a_N1_8000", clips[:1, :8000], None), ("b_N1_16000", clips[:1, :16000], None), ("c_N64_1_to_3_s", pad, ns)):
        kernel[name] = round(launch_us(lambda: session.probabilities(pcm, n_samples=n_samples, return_state=False)), 2)
    out["launch_us_median_between_hip_events"] = kernel
    torch.cuda.synchronize()
    print(json.dumps(out), flush=True)


def main_decide(args):
    import numpy as np
    import torch
    from howl_amd.model.decision import DeviceDecider
    from howl_amd.model.inference import FrameInferenceEngine, InferenceEngine
    ctx, lstm, std, zmuv, clips = setup("seq-lstm", use_blank=True)
    fctx, res8, _, _, _ = setup("res8", use_blank=False)      # (both engines behind the one ZMUV)
    dev = clips.device
    rng = np.random.default_rng(7)
    sizes = [int(v) for v in rng.integers(16000, 48001, 64)]           # case (c)'s clips
    many = [clips[i % 8, :n].contiguous() for i, n in enumerate(sizes)]

    seq = InferenceEngine(lstm.streaming(), zmuv, ctx)
    seq.fused_chunks = True
    seq.sequence = [0, 1, 2, 0, 1, 2, 0, 1, 2]                         # never present: every call walks all of its frames
    frame = FrameInferenceEngine(500, 63, res8, zmuv, fctx)
    frame.sequence = [0, 1, 2, 0, 1, 2, 0, 1, 2]

    def both(engine, calls, warm):
        def run(on, n, first):
            engine.device_decisions = on
            times = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                engine.infer_many(many)
                times.append(time.perf_counter() - t0)
            return times

        engine.device_decisions = False
        want = (engine.infer_many(many), [list(h) for h in engine.clip_histories])
        engine.device_decisions = True
        assert (engine.infer_many(many), engine.clip_histories) == want, "the device decisions differ from the host replay"
        med = alternate([False, True], run, warm, calls, args.repeats)
        return {"calls_per_repeat": calls, "history_entries_per_call": sum(len(h) for h in want[1]),
                "host_decisions_us_medians": [round(v, 2) for v in med[False]], "device_decisions_us_medians": [round(v, 2) for v in med[True]]}

    calls, warm = max(2, args.windows // 20), max(1, args.warmup // 20)
    out = {"metric": "infer_many wall time per call of 64 clips of 1 - 3 s, us (host copy included; median of each repeat), decision logic "
                     "on the host against DeviceDecider", "frames_per_call_sequence_engine": sum(1 + n // 200 for n in sizes)}
    out["d_sequence_engine_as_case_c"] = both(seq, calls, warm)
    seq.inference_weights = np.array([1.0, 1.0, 1.0, 1.0, 0.01])
    out["e_sequence_engine_blank_weighted_down"] = both(seq, calls, warm)
    out["f_frame_engine_res8"] = both(frame, calls, warm)
    out["f_frame_engine_res8"]["windows_per_call"] = sum(len(p) for p in frame.window_probabilities_many(many))

    # the decision launch alone, between two HIP events, on the probabilities of each case
    def launch_alone(decider, probs, n_frames, deltas):
        from howl_amd import ops
        cfg, keep = decider._config(dev)
        nf = torch.tensor(n_frames, dtype=torch.int32, device=dev)
        dl = torch.tensor(deltas, dtype=torch.float64, device=dev)
        return round(launch_us(lambda: ops.decide_clips(cfg, probs, nf, dl, max(n_frames))), 2)

    session = lstm.stream_session(std, zmuv)
    pad = torch.nn.utils.rnn.pad_sequence(many, batch_first=True)
    probs, _ = session.probabilities(pad, n_samples=torch.tensor(sizes, dtype=torch.int64, device=dev), return_state=False)
    frames = [1 + n // 200 for n in sizes]
    deltas = [int(n / 16000 * 1000) / f for n, f in zip(sizes, frames)]
    alone = {"e_N64_sequence_mode_blank_weighted_down": launch_alone(DeviceDecider.from_engine(seq, 0), probs, frames, deltas)}
    seq.inference_weights = 1
    alone["d_N64_sequence_mode"] = launch_alone(DeviceDecider.from_engine(seq, 0), probs, frames, deltas)
    (members, wprobs), = frame._window_probabilities_device(many)
    counts = [n for _, n, _ in members]
    padded = torch.nn.utils.rnn.pad_sequence(list(wprobs.split(counts)), batch_first=True)
    alone["f_N64_frame_mode"] = launch_alone(DeviceDecider.from_engine(frame, 1), padded, counts, [63.0] * len(counts))
    out["decide_launch_us_median_between_hip_events"] = alone
    torch.cuda.synchronize()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
