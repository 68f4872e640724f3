"""The small-cnn and seq-cnn fused training steps: small-cnn's frame step at 512 x 0.5 s and seq-cnn's CTC step at 512 x 1 s.

Protocol: ``FusedTrainer.step`` (small-cnn, 30 labels) on a (512, 8000) synthetic PCM batch and ``FusedTrainer.step_sequence``
(seq-cnn, 5 labels, targets of three labels) on a (512, 16000) one, every utterance full length; 10 steps of warm-up per model, then
five repeats of 30 steps each between two HIP events (one synchronise per repeat), the two models alternating repeat by repeat, in
one process, on one card; the MEDIAN repeat is the step time.  Then, in a pass of its own (the library's HIP-event brackets slow the
host down), the per-launch times of 30 steps of each model: ``howl_profile_read_work`` per tag.  The two convolutions' forward
brackets (``cnn_conv0``: conv0 + its BatchNorm fold; ``cnn_conv1``: conv1 + its fold) are set against the fp32 MFMA peak with the
FLOPs of the dense convolution over the POOLED region (what the kernels compute: the column and the odd row the pool drops are
never formed).  Prints one JSON line.  ``--steps`` / ``--repeats`` shorten a run."""
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

TAGS = ("logmel", "cnn_conv0", "cnn_conv1", "cnn_head", "gemm", "cnn_conv1_bwd", "cnn_conv0_bwd")
FP32_MFMA_PEAK = 157.3e12      # v_mfma_f32_16x16x4_f32 / 32x32x2_f32, FLOP/s


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
    from howl_amd.model import CnnSettings, RegisteredModel
    from howl_amd.training.fused import FusedTrainer
    from howl_amd.utils.synth import synthetic_pcm
    dev = torch.device("cuda:0")
    lb = hlib.get()
    B = args.batch
    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    torch.manual_seed(2025)
    runs, frames = {}, {}
    for name, L, C in (("small-cnn", 8000, 30), ("seq-cnn", 16000, 5)):
        pcm = synthetic_pcm(B, L).to(dev)
        if name == "small-cnn":
            zmuv.update(std(pcm[:8]))
        model = RegisteredModel.find_registered_class(name)(C, CnnSettings(num_labels=C)).to(dev).train()
        trainer = FusedTrainer(model, std, zmuv, lr=1e-4, weight_decay=1e-5)
        T = 1 + L // 200
        frames[name] = T
        if name == "small-cnn":
            labels = (torch.arange(B) % C).to(dev)
            runs[name] = (lambda trainer=trainer, pcm=pcm, labels=labels: trainer.step(pcm, labels))
        else:
            lengths = torch.full((B,), T, dtype=torch.int64, device=dev)
            targets = torch.tensor([[1 + (b + j) % (C - 1) for j in range(3)] for b in range(B)], device=dev)
            tl = torch.full((B,), 3, dtype=torch.int64, device=dev)
            runs[name] = (lambda trainer=trainer, pcm=pcm, lengths=lengths, targets=targets, tl=tl, T=T:
                          trainer.step_sequence(pcm, lengths, targets, tl, 0, max_target=3, max_frames=T))

    def run(name, n):
        for _ in range(n):
            runs[name]()

    for name in runs:
        run(name, args.warmup)
    torch.cuda.synchronize()
    us = {name: [] for name in runs}
    for _ in range(args.repeats):
        for name in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, args.steps)
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)

    launches, share = {}, {}
    for name in runs:
        lb.call("howl_profile_enable", 1)
        run(name, args.steps)
        torch.cuda.synchronize()
        lb.call("howl_profile_enable", 0)
        row = {}
        for i, tag in enumerate(TAGS):                                  # a read with reset clears every tag
            tot, cnt, work = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_double(0)
            lb.call("howl_profile_read_work", tag.encode(), ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work), int(i == len(TAGS) - 1))
            row[tag] = {"us_per_step": round(tot.value * 1e3 / args.steps, 2), "brackets_per_step": round(cnt.value / args.steps, 2),
                        "gflop_per_step": round(work.value / args.steps / 1e9, 3)}
        launches[name] = row
        for tag in ("cnn_conv0", "cnn_conv1"):      # forward brackets only: the backward's convolutions run on the vector ALUs
            t = row[tag]["us_per_step"] * 1e-6
            share[f"{name} {tag}"] = round(row[tag]["gflop_per_step"] * 1e9 / t / FP32_MFMA_PEAK, 4) if t > 0 else None
    print(json.dumps({
        "metric": f"FusedTrainer.step (small-cnn, {B} x 0.5 s, {frames['small-cnn']} frames, 30 labels) and step_sequence (seq-cnn, {B} x 1 s, "
                  f"{frames['seq-cnn']} frames, 5 labels), us per step between HIP events; {args.repeats} repeats of {args.steps} steps, alternating",
        "small_cnn_step_us": [round(v, 1) for v in us["small-cnn"]], "small_cnn_step_us_median": round(statistics.median(us["small-cnn"]), 1),
        "seq_cnn_step_us": [round(v, 1) for v in us["seq-cnn"]], "seq_cnn_step_us_median": round(statistics.median(us["seq-cnn"]), 1),
        "launch_brackets_us_per_training_step": launches,
        "forward_conv_bracket_share_of_fp32_mfma_peak": share}), flush=True)


if __name__ == "__main__":
    main()
