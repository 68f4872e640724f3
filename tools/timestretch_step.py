"""Time-stretch augmentation beside the step it feeds, in one run: 512 clips of 1 s, the rates of one seeded batch.

Protocol (one process, one card; 5 steps of warm-up, then ``--repeats`` repeats of ``--steps`` calls each between two HIP events,
one synchronise per repeat, the four measurements alternating repeat by repeat; the MEDIAN repeat is the time):

* ``stretch``: the ``howl_timestretch_clips`` launch alone (records already on the device) -- 512 ragged clips at the rates
  ``clip(RandomState(0).normal(1, 0.2, 512), 0.3, 1.7)``;
* ``collate_plain`` / ``collate_stretch``: ``DeviceCollate.frame_batch`` (host draws, uploads, launches) without and with
  ``timestretch=True``, the Timestretch gate held open so that every batch stretches;
* ``res8_step``: ``FusedTrainer.step`` on the (512, 8000) batch a frame collate hands over (500-ms windows, 12 labels).

The yardstick is ``collate_plain + res8_step`` of the same run: what a training step cost before the stretch existed.  Prints one
JSON line and writes it, with the per-repeat times, to ``--out`` (default profiles/timestretch.txt)."""
import argparse
import json
import os
import random
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
os.environ.setdefault("NUM_MELS", "40")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "timestretch.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from howl_amd import ops
    from howl_amd.data.collate import DeviceCollate
    from howl_amd.data.transform.batchifier import DeviceClip, WakeWordFrameBatchifier
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.data.transform.transform import StandardAudioTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.training.fused import FusedTrainer
    from howl_amd.utils.synth import synthetic_pcm
    dev = torch.device("cuda:0")
    B, L, C, window_ms = args.batch, 16000, 12, 500
    pcm = synthetic_pcm(B, L).to(dev)
    flat = pcm.reshape(-1, 1)
    offs = [L * k for k in range(B)]
    rates = np.clip(np.random.RandomState(0).normal(1.0, 0.2, B), 0.3, 1.7)
    rec, total = ops.stretch_records(offs, [L] * B, rates)
    rec_dev = torch.from_numpy(rec.view(np.int64).copy()).to(dev)

    examples = [DeviceClip(k, L, {300.0 + 5 * (k % 60): 1 + k % (C - 1), 700.0: 2}, "a b") for k in range(B)]
    collates = {flag: DeviceCollate(flat, torch.full((B,), L), None, max_len=L, row_offsets=offs, seed=7, timestretch=flag) for flag in (False, True)}
    collates[True]._stretch.augment_params[0].prob = 1.0                 # every batch stretches (the draw is still made)
    batchifiers = {flag: WakeWordFrameBatchifier(0, window_size_ms=window_ms, rand=random.Random(5)) for flag in (False, True)}

    std = StandardAudioTransform().to(dev).eval()
    zmuv = ZmuvTransform().to(dev)
    zmuv.update(std(pcm[:8]))
    torch.manual_seed(2025)
    model = RegisteredModel.find_registered_class("res8")(C).to(dev).train()
    trainer = FusedTrainer(model, std, zmuv, lr=1e-4, weight_decay=1e-5)
    batch = collates[False].frame_batch(examples, batchifiers[False])
    labels = batch.labels

    work = {
        "stretch": lambda: ops.time_stretch(flat, rec, rec_dev, total),
        "collate_plain": lambda: collates[False].frame_batch(examples, batchifiers[False]),
        "collate_stretch": lambda: collates[True].frame_batch(examples, batchifiers[True]),
        "res8_step": lambda: trainer.step(batch.audio_data, labels),
    }
    for fn in work.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in work}
    for _ in range(args.repeats):
        for name, fn in work.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    med = {name: statistics.median(v) for name, v in us.items()}
    before = med["collate_plain"] + med["res8_step"]
    out_frames = int(sum(min(int(n), -(-(int(o) + 2048) // 512)) for n, o in zip(rec["n_out"], rec["out_len"])))
    result = {
        "metric": f"us per call between HIP events ({B} clips x 1 s; {args.repeats} repeats of {args.steps} calls, alternating; medians)",
        "rates": {"min": round(float(rates.min()), 3), "median": round(float(np.median(rates)), 3), "max": round(float(rates.max()), 3)},
        "stretch_out_samples": total, "stretch_out_frames": out_frames, "stretch_in_frames": B * (1 + L // 512),
        "us": {name: [round(v, 1) for v in vals] for name, vals in us.items()},
        "us_median": {name: round(v, 1) for name, v in med.items()},
        "stretch_us_per_out_frame_per_workgroup": round(med["stretch"] / (out_frames / B), 3),
        "collate_plain_plus_res8_step_us": round(before, 1),
        "collate_stretch_plus_res8_step_us": round(med["collate_stretch"] + med["res8_step"], 1),
        "ratio_with_over_without": round((med["collate_stretch"] + med["res8_step"]) / before, 3),
        "stretch_launch_over_collate_plus_step": round(med["stretch"] / before, 3),
    }
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("tools/timestretch_step.py on " + torch.cuda.get_device_name(0) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
