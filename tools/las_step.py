"""The las model's fused training step at 512 x 1 s, 12 labels, beside the lstm model's frame step in the same run.

Protocol: ``FusedTrainer.step`` on a (512, 16000) synthetic PCM batch (81 frames: 21 las steps per direction, both directions in one
launch; 81 LSTM steps), every utterance full length; 10 steps of warm-up per model, then five repeats of 30 steps each between two
HIP events (one synchronise per repeat), las and lstm alternating repeat by repeat, in one process, on one card; the MEDIAN repeat
is the step time.  Then, in a pass of its own (the library's HIP-event brackets slow the host down), the per-launch times of 30
steps of each model: ``howl_profile_read`` per tag, and for the four-sequence recurrences the time per dependent step -- the
yardstick: the las step issues 6 x 96 k-steps of v_mfma_f32_4x4x1 per workgroup step against the LSTM's 8 x 168.  Prints one JSON
line.  ``--steps`` / ``--repeats`` shorten a run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
os.environ.setdefault("NUM_MELS", "40")

LAS_TAGS = ("logmel", "las_enc_fwd", "las_lstm_fwd", "las_attn", "las_head", "las_lstm_bwd", "gemm", "las_enc_bwd")
LSTM_TAGS = ("logmel", "lstm_fwd", "lstm_bwd", "gemm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    from howl_amd import lib as hlib
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.training.fused import FusedTrainer
    from howl_amd.utils.synth import synthetic_pcm
    dev = torch.device("cuda:0")
    lb = hlib.get()
    B, L, C = args.batch, 16000, 12
    pcm = synthetic_pcm(B, L).to(dev)
    labels = (torch.arange(B) % C).to(dev)
    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    zmuv.update(std(pcm[:8]))
    frames = 1 + L // 200
    lengths = torch.full((B,), frames, dtype=torch.int64, device=dev)
    torch.manual_seed(2025)
    trainers = {}
    for name in ("las", "lstm"):
        model = RegisteredModel.find_registered_class(name)(C).to(dev).train()
        trainers[name] = FusedTrainer(model, std, zmuv, lr=1e-4, weight_decay=1e-5)

    def run(name, n):
        for _ in range(n):
            trainers[name].step(pcm, labels, lengths, frames)

    for name in trainers:
        run(name, args.warmup)
    torch.cuda.synchronize()
    us = {name: [] for name in trainers}
    for _ in range(args.repeats):
        for name in trainers:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, args.steps)
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)

    launches = {}
    for name, tags in (("las", LAS_TAGS), ("lstm", LSTM_TAGS)):
        lb.call("howl_profile_enable", 1)
        run(name, args.steps)
        torch.cuda.synchronize()
        lb.call("howl_profile_enable", 0)
        row = {}
        for i, tag in enumerate(tags):                                  # a read with reset clears every tag
            tot, cnt = ctypes.c_double(0), ctypes.c_int(0)
            lb.call("howl_profile_read", tag.encode(), ctypes.byref(tot), ctypes.byref(cnt), int(i == len(tags) - 1))
            row[tag] = {"us_per_step": round(tot.value * 1e3 / args.steps, 2), "brackets_per_step": round(cnt.value / args.steps, 2)}
        launches[name] = row
    las_steps, lstm_steps = (((frames + 2) // 2) + 2) // 2, frames
    step_us = statistics.median(us["las"])
    per_step = {"las_fwd4": launches["las"]["las_lstm_fwd"]["us_per_step"] / las_steps, "las_bwd4": launches["las"]["las_lstm_bwd"]["us_per_step"] / las_steps,
                "lstm_fwd4": launches["lstm"]["lstm_fwd"]["us_per_step"] / lstm_steps, "lstm_bwd4": launches["lstm"]["lstm_bwd"]["us_per_step"] / lstm_steps}
    print(json.dumps({
        "metric": f"FusedTrainer.step, us per step between HIP events ({B} x 1 s, {frames} frames, {C} labels; {args.repeats} repeats of "
                  f"{args.steps} steps, las and lstm alternating)",
        "las_step_us": [round(v, 1) for v in us["las"]], "las_step_us_median": round(step_us, 1),
        "lstm_step_us": [round(v, 1) for v in us["lstm"]], "lstm_step_us_median": round(statistics.median(us["lstm"]), 1),
        "launch_brackets_us_per_training_step": launches,
        "las_gemm_path_share_of_bracketed_time": round(launches["las"]["gemm"]["us_per_step"] / max(sum(v["us_per_step"] for v in launches["las"].values()), 1e-9), 3),
        "recurrence_steps": {"las (per direction, both in one launch)": las_steps, "lstm": lstm_steps},
        "recurrence_us_per_dependent_step": {k: round(v, 3) for k, v in per_step.items()},
        "las_fwd_step_over_lstm_fwd_step": round(per_step["las_fwd4"] / per_step["lstm_fwd4"], 3),
        "las_bwd_step_over_lstm_bwd_step": round(per_step["las_bwd4"] / per_step["lstm_bwd4"], 3)}), flush=True)


if __name__ == "__main__":
    main()
