"""Shared by tests/test_emu_decide.py (hipemu, guarded host buffers) and tests/test_gpu_decide.py (device, sentinel bands): the
decision-logic entry points of include/howl_hip_decide.h called through an allocator of tests/guard_mem.py, and the yardstick: the
host path as it stands -- the engines' own loops (InferenceEngine._run_frames, FrameInferenceEngine._run_fsm) over _weighted,
ProbabilitySmoother and SequenceMatcher, run on real engine objects around a model-less context, instrumented from outside.

Equality is exact everywhere: flags, label values, fp64 stamps bit for bit, end_time, first_kept, n_labels.  No tolerance."""
import ctypes
import types
from collections import Counter

import numpy as np
import torch

from howl_amd.lib import HowlDecideConfig

RING = 32                   # HOWL_DECIDE_RING_FRAMES
SEQUENCES = ([0, 1, 2], [1], [2, 0], [0, 0, 1])
EVENTS = ("blank_skip", "multi_frame_ring", "dropped", "reset_after_partial", "below_threshold", "sustained")


# ---- the yardstick: the host loops, instrumented ---------------------------------------------------------------------------------------

def host_engine(mode, C, blank=None, negative=0, threshold=0.0, smoothing_ms=50.0, window_ms=2000.0, tolerance_ms=500.0, sequence=(0, 1, 2),
                weights=None, color_map=None, stride_ms=63):
    """A real InferenceEngine (mode 0) / FrameInferenceEngine (mode 1) without a model, with the given settings assigned the way
    callers retune an engine after construction."""
    from howl_amd.model.inference import FrameInferenceEngine, InferenceEngine
    ctx = types.SimpleNamespace(num_labels=C, blank_label=C - 1 if blank is None else blank, negative_label=negative, coloring=None)
    model = types.SimpleNamespace(streaming_state=None)
    engine = InferenceEngine(model, None, ctx) if mode == 0 else FrameInferenceEngine(500, stride_ms, model, None, ctx)
    engine.threshold, engine.smoothing_window_ms, engine.inference_window_ms = threshold, smoothing_ms, window_ms
    engine.tolerance_window_ms, engine.sequence = tolerance_ms, list(sequence)
    engine.inference_weights = 1 if weights is None else np.asarray(weights, np.float64)
    engine._smoother.negative_label, engine._smoother.color_map = negative, color_map
    engine.negative_label = negative
    engine.device_decisions = False
    return engine


def _scan_events(matcher, history, events):
    """SequenceMatcher.present's scan over the history it has just been given, counting the branches it takes -> its verdict."""
    if not matcher.sequence:
        return False
    matched, anchor, holding = 0, 0.0, None
    for stamp, label in history:
        if label == matcher.sequence[matched]:
            matched += 1
            if matched == len(matcher.sequence):
                return True
            holding, anchor = label, stamp
        elif label == holding:
            anchor = stamp
            events["sustained"] += 1
        elif anchor + matcher.tolerance_ms < stamp:
            if matched:
                events["reset_after_partial"] += 1
            matched, anchor, holding = 0, 0.0, None
    return False


def host_run(engine, mode, probs, delta_ms):
    """One clip through the engine's own loop -> dict(present, history: every entry appended, first_kept, n_labels, end_time,
    events).  The instrumentation wraps the engine's methods; the decisions are the unwrapped code's."""
    events = Counter()
    full, looked = [], [0]
    real_append, real_weighted, real_present = engine._append_probability_frame, engine._weighted, engine.sequence_present

    def append(prediction, curr_time=None):
        label = real_append(prediction, curr_time=curr_time)
        full.append(engine.label_history[-1])
        frames = engine._smoother.frames
        if len(frames) > 1:
            events["multi_frame_ring"] += 1
        if not np.max(np.vstack([p for _, p in frames]), axis=0).max() >= engine.threshold:
            events["below_threshold"] += 1
        events["ring_max"] = max(events["ring_max"], len(frames))
        return label

    def weighted(prediction):
        looked[0] += 1
        return real_weighted(prediction)

    def present(curr_time=None):
        before = len(engine.label_history)
        verdict = real_present(curr_time)
        if len(engine.label_history) < before:
            events["dropped"] += 1
        assert _scan_events(engine._matcher, engine.label_history, events) == verdict
        return verdict

    engine._append_probability_frame, engine._weighted, engine.sequence_present = append, weighted, present
    try:
        engine.reset()
        probs = np.ascontiguousarray(probs, np.float32)
        if len(probs) == 0:
            found = False
        elif mode == 0:
            found = engine._run_frames(probs, delta_ms * len(probs))      # (the loop divides by the frame count again: exact for these)
            assert (delta_ms * len(probs)) / len(probs) == delta_ms
        else:
            assert engine.eval_stride_size_ms == delta_ms
            found = engine._run_fsm(probs)
        events["blank_skip"] += looked[0] - len(full)
        out = dict(present=bool(found), history=list(full), n_labels=len(full), first_kept=len(full) - len(engine.label_history),
                   end_time=float(engine.curr_time), events=events)
        assert full[out["first_kept"]:] == engine.label_history
    finally:
        del engine._append_probability_frame, engine._weighted, engine.sequence_present
        engine.reset()
    return out


# ---- the device side -----------------------------------------------------------------------------------------------------------------

def engine_config(al, engine, mode, tag=""):
    """HowlDecideConfig of an engine's settings, the weights and the colour table in buffers of their own."""
    C = engine.context.num_labels
    cfg = HowlDecideConfig(mode=mode, C=C, blank=int(engine.blank_idx) if mode == 0 else -1, negative=int(engine._smoother.negative_label),
                           threshold=float(engine.threshold), smoothing_ms=float(engine.smoothing_window_ms),
                           window_ms=float(engine.inference_window_ms), tolerance_ms=float(engine.tolerance_window_ms), seq_len=len(engine.sequence))
    for i, v in enumerate(engine.sequence):
        cfg.sequence[i] = int(v)
    keep = []
    if not np.isscalar(engine.inference_weights):
        keep.append(al.buf(tag + "weights", C, np.float64, np.asarray(engine.inference_weights, np.float64)))
        cfg.weights = al.ptr(keep[-1])
    cmap = engine._smoother.color_map
    if cmap is not None:
        table = np.full(C, -1, np.int32)
        for k, v in cmap.items():
            table[k] = v
        keep.append(al.buf(tag + "color", C, np.int32, table))
        cfg.color = al.ptr(keep[-1])
    return cfg, keep


def device_run(al, lib, cfg, clips, deltas, n_frames=None, T_max=None, weighted=False, tag="", hist_ld=None):
    """ONE howl_decide_clips launch on N ragged clips ((T_n, C) arrays).  The probabilities are a (N, T_max, C) buffer whose rows
    behind a clip's frames hold the NaN sentinel; outputs are exactly as large as the header says, every promised element checked.
    -> dict of numpy arrays."""
    from guard_mem import sentinel_mask
    N, C = len(clips), cfg.C
    T_max = max(len(c) for c in clips) if T_max is None else T_max
    rows = np.zeros((N, max(T_max, 1), C), np.float32)
    rows.view(np.uint32)[...] = 0x7FA5A5A5
    for i, c in enumerate(clips):
        rows[i, :len(c)] = c
    pb = al.buf(tag + "probs", rows.shape, np.float32, rows)
    nf = np.array([len(c) for c in clips] if n_frames is None else n_frames, np.int32)
    nfb = al.buf(tag + "n_frames", N, np.int32, nf)
    dlb = al.buf(tag + "delta_ms", N, np.float64, np.asarray(deltas, np.float64))
    small = {k: al.buf(tag + k, N, np.int32, "sentinel", promised="all") for k in ("present", "status", "n_labels", "first_kept")}
    end = al.buf(tag + "end_time", N, np.float64, "sentinel", promised="all")
    ld = T_max if hist_ld is None else hist_ld
    counts = {}

    def appended(a):      # evaluated at check() time: exactly the first n_labels entries of a row are written
        return np.arange(a.shape[1])[None, :] < counts["n_labels"][:, None]
    ht = al.buf(tag + "hist_time", (N, max(ld, 1)), np.float64, "sentinel", promised=appended)
    hl = al.buf(tag + "hist_label", (N, max(ld, 1)), np.int32, "sentinel", promised=appended)
    wb = al.buf(tag + "weighted", (N, max(T_max, 1), C), np.float32, "sentinel") if weighted else None
    lib.call("howl_decide_clips", ctypes.byref(cfg), al.ptr(pb), rows.shape[1] * C, C, N, T_max, al.ptr(nfb), al.ptr(dlb), al.ptr(small["present"]),
             al.ptr(small["status"]), al.ptr(small["n_labels"]), al.ptr(small["first_kept"]), al.ptr(end), al.ptr(ht), al.ptr(hl), ld,
             al.ptr(wb), None)
    al.sync()
    out = {k: al.get(v).copy() for k, v in small.items()}
    counts["n_labels"] = out["n_labels"]
    out.update(end_time=al.get(end).copy(), hist_time=al.get(ht).copy(), hist_label=al.get(hl).copy())
    if weighted:
        out["weighted"] = al.get(wb).copy()
    for i in range(N):
        k = int(out["n_labels"][i])
        assert 0 <= out["first_kept"][i] <= k <= T_max, (i, out["first_kept"][i], k)
        assert sentinel_mask(out["hist_time"][i, k:]).all() and sentinel_mask(out["hist_label"][i, k:]).all(), f"clip {i}: written behind n_labels"
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_equals_host(dev, i, host, what=""):
    """Clip i of a launch against its host run: flag, counts, end time, every history entry (dropped ones included)."""
    assert dev["status"][i] == 0, f"{what}: status {dev['status'][i]}"
    assert bool(dev["present"][i]) == host["present"], f"{what}: present {dev['present'][i]} != {host['present']}"
    assert dev["n_labels"][i] == host["n_labels"] and dev["first_kept"][i] == host["first_kept"], \
        f"{what}: n_labels / first_kept {dev['n_labels'][i]} / {dev['first_kept'][i]} != {host['n_labels']} / {host['first_kept']}"
    k = host["n_labels"]
    stamps = np.array([s for s, _ in host["history"]], np.float64)
    labels = np.array([l for _, l in host["history"]], np.int32)
    assert np.array_equal(dev["hist_label"][i, :k], labels), f"{what}: labels differ"
    assert same_bits(dev["hist_time"][i, :k], stamps), f"{what}: stamps differ"
    assert same_bits(dev["end_time"][i:i + 1], np.array([host["end_time"]], np.float64)), f"{what}: end_time {dev['end_time'][i]!r} != {host['end_time']!r}"


# ---- test 1: random cases --------------------------------------------------------------------------------------------------------------

def softmax32(z):
    z = z.astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def random_probs(rng, mode, C, T):
    """softmax(N(0,1) + 6 U(0,1) on a piecewise-constant label track); dwell 1..12 frames (sequence mode) or 1..4 (frame mode); the
    track prefers the labels the sequences are made of; in sequence mode the blank C-1 is drawn on 30 % of the frames."""
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
    return softmax32(z)


def group_settings(g):
    """The settings of group g (16 groups of 4 ragged clips: one launch each)."""
    mode = g % 2
    C = (3, 5, 8, 12)[(g // 2) % 4]
    return dict(mode=mode, C=C, blank=C - 1, negative=C - 2 if mode == 0 else C - 1, threshold=(0.0, 0.5, 0.8)[g % 3],
                smoothing_ms=(30.0, 50.0)[(g // 2) % 2], window_ms=2000.0, tolerance_ms=100.0 if g % 7 == 6 else 500.0,
                sequence=SEQUENCES[(g + g // 4) % 4], weights=[0.5, 2.0] + [1.0] * (C - 2) if g % 3 == 2 else None,
                color_map={0: 0, 1: 1, 2: 1} if g % 5 == 4 else None)


def random_cases(groups=range(16), clips_per_group=4):
    """[(settings, [probs], delta)] with default_rng(0): 64 clips, 1..399 frames at 12.5 ms (sequence mode) or 1..119 at 63 ms."""
    rng = np.random.default_rng(0)
    out = []
    for g in range(16):
        s = group_settings(g)
        clips = [random_probs(rng, s["mode"], s["C"], int(rng.integers(1, 400 if s["mode"] == 0 else 120))) for _ in range(clips_per_group)]
        if g in groups:
            out.append((s, clips, 12.5 if s["mode"] == 0 else 63))
    return out


def host_results(cases):
    """The host replay of every clip (computed once, shared) and the coverage condition on the inputs: each event of the logic
    occurs, at least a quarter of the clips end in a detection and at least a quarter do not."""
    res, events, found, total = [], Counter(), 0, 0
    for s, clips, delta in cases:
        engine = host_engine(**{**s, "stride_ms": delta})
        runs = [host_run(engine, s["mode"], p, delta) for p in clips]
        res.append(runs)
        for r in runs:
            events.update({k: v for k, v in r["events"].items() if k != "ring_max"})
            events["ring_max"] = max(events["ring_max"], r["events"]["ring_max"])
            found += r["present"]
            total += 1
    print(f"decide cases: {total} clips, {found} detections, events {dict(events)}")
    for k in EVENTS:
        assert events[k] >= 1, f"the case set never produces the event {k!r}: {dict(events)}"
    assert 4 * found >= total and 4 * (total - found) >= total, (found, total)
    assert events["ring_max"] <= RING
    return res


def check_random_cases(al, lib, cases, host):
    for g, ((s, clips, delta), runs) in enumerate(zip(cases, host)):
        engine = host_engine(**{**s, "stride_ms": delta})
        cfg, keep = engine_config(al, engine, s["mode"], f"g{g}.")
        dev = device_run(al, lib, cfg, clips, [delta] * len(clips), tag=f"g{g}.")
        for i, r in enumerate(runs):
            assert_equals_host(dev, i, r, f"group {g} ({s['mode']=}, C={s['C']}) clip {i} of {len(clips[i])} frames")
    al.check()


# ---- test 2: normalisation ---------------------------------------------------------------------------------------------------------------

NORM_CLASSES = (1, 3, 7, 8, 9, 15, 16, 17, 33, 64)


def numpy_order_sum(a):
    """np.sum of up to 128 fp32 elements as the kernel computes it: left to right below eight; from eight on eight strided
    accumulators over the whole blocks of eight, folded pairwise, then the rest one by one."""
    a = np.asarray(a, np.float32)
    n = len(a)
    if n < 8:
        s = np.float32(0.0)
        for v in a:
            s = np.float32(s + v)
        return s
    r = a[:8].copy()
    for i in range(8, n - n % 8, 8):
        r = (r + a[i:i + 8]).astype(np.float32)
    s = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3])) + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
    for v in a[n - n % 8:]:
        s = np.float32(s + v)
    return s


def check_normalisation(al, lib, rows=100):
    rng = np.random.default_rng(2)
    for C in NORM_CLASSES:
        for with_weights in (False, True):
            weights = (0.25 + 2.0 * rng.random(C)) if with_weights else None
            engine = host_engine(1, C, sequence=(), weights=weights, negative=0, stride_ms=63)
            p = softmax32(3.0 * rng.standard_normal((rows, C)))
            want = np.stack([engine._weighted(r) for r in p])
            assert want.dtype == np.float32
            # host only: the stated reduction order IS this NumPy's (otherwise the kernel is not the one to blame)
            for r in p:
                w = (r * engine.inference_weights).astype(np.float32)
                assert numpy_order_sum(w).tobytes() == w.sum().tobytes(), \
                    f"np.sum of {C} fp32 elements does not follow the pairwise order the kernel implements (numpy {np.__version__})"
            cfg, keep = engine_config(al, engine, 1, f"C{C}w{int(with_weights)}.")
            dev = device_run(al, lib, cfg, [p], [63.0], weighted=True, tag=f"C{C}w{int(with_weights)}.")
            assert same_bits(dev["weighted"][0], want), f"C={C} weights={with_weights}: {np.argwhere(dev['weighted'][0] != want)[:3].tolist()}"
            assert dev["n_labels"][0] == rows and dev["present"][0] == 0 and dev["first_kept"][0] == 0
    al.check()


# ---- test 3: threshold edge ----------------------------------------------------------------------------------------------------------------

def check_threshold_edge(al, lib):
    row = np.array([[0.5, 0.25, 0.25]] * 3, np.float32)
    assert row[0].sum() == np.float32(1.0) and same_bits(row[0] / row[0].sum(), row[0])
    above = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    for mode in (0, 1):
        for cmap in (None, {1: 1, 2: 2}, {0: 1, 1: 1, 2: 2}):
            for thr, label in ((0.5, 0), (above, 2)):
                engine = host_engine(mode, 3, blank=2, negative=2, threshold=thr, sequence=(1, 1, 1, 1), color_map=cmap, stride_ms=63)
                host = host_run(engine, mode, row, 63)
                want = label if cmap is None or label == 2 else cmap.get(label, 2)
                assert [l for _, l in host["history"]] == [want] * 3, (mode, cmap, thr, host["history"])
                tag = f"m{mode}c{0 if cmap is None else len(cmap)}t{int(thr > 0.5)}."
                cfg, keep = engine_config(al, engine, mode, tag)
                dev = device_run(al, lib, cfg, [row], [63.0], tag=tag)
                assert_equals_host(dev, 0, host, tag)
    al.check()


# ---- test 4: degenerate shapes ---------------------------------------------------------------------------------------------------------------

def check_degenerate(al, lib):
    rng = np.random.default_rng(4)
    C = 5
    p = random_probs(rng, 1, C, 40)
    first = np.zeros((6, C), np.float32)
    first[:, 1] = 1.0
    blank = np.zeros((30, C), np.float32)
    blank[:, C - 1] = 0.9
    blank[:, 0] = 0.1
    for mode, delta in ((0, 12.5), (1, 63)):
        for name, seq, clips in (("empty_and_one", [0, 1, 2], [p[:0], p[:1], p]),
                                 ("no_sequence", [], [p, p[:7]]),
                                 ("first_frame", [1], [first, p[:3]]),
                                 ("all_blank", [0, 1], [blank, p[:9]])):
            engine = host_engine(mode, C, negative=C - 2, threshold=0.3, smoothing_ms=50.0, window_ms=300.0, sequence=seq, stride_ms=delta)
            tag = f"m{mode}.{name}."
            cfg, keep = engine_config(al, engine, mode, tag)
            dev = device_run(al, lib, cfg, clips, [delta] * len(clips), tag=tag)
            hosts = [host_run(engine, mode, c, delta) for c in clips]
            for i, h in enumerate(hosts):
                assert_equals_host(dev, i, h, f"{tag}{i}")
            if name == "empty_and_one":
                assert dev["n_labels"][0] == 0 and dev["end_time"][0] == 0.0 and dev["present"][0] == 0
            if name == "no_sequence":
                assert not dev["present"].any() and not dev["first_kept"].any() and dev["n_labels"][0] == (len(p) if mode else hosts[0]["n_labels"])
            if name == "first_frame":
                assert dev["present"][0] == 1 and dev["n_labels"][0] == 1
            if name == "all_blank" and mode == 0:
                assert dev["n_labels"][0] == 0 and dev["end_time"][0] == hosts[0]["end_time"] > 0
    al.check()


def check_clamped(al, lib, big=False):
    """n_frames outside [0, T_max] are clamped inside the kernel: the smallest operands (C = 1, T_max = 1, N = 1 .. 5) and the
    largest (C = 64, T_max = 8192 with ``big``).  The emulator's guard-page run takes C = 64 with T_max = 40 for its speed: T_max =
    8192 runs on the device only, between sentinel bands."""
    rng = np.random.default_rng(5)
    for C, T_max in ((1, 1), (3, 7)) + (((64, 8192),) if big else ((64, 40),)):
        mode, delta = (0, 12.5) if C == 3 else (1, 63)
        N = 5
        p = [random_probs(rng, mode, C, T_max) for _ in range(N)]
        bad = np.array([T_max + 5, -3, 10 ** 6, -2 ** 31, T_max], np.int64)
        want = np.clip(bad, 0, T_max)
        engine = host_engine(mode, C, negative=0, threshold=0.2, smoothing_ms=50.0, window_ms=500.0, sequence=[0] * 16, stride_ms=delta)
        tag = f"clamp.C{C}.T{T_max}."
        cfg, keep = engine_config(al, engine, mode, tag)
        dev = device_run(al, lib, cfg, p, [delta] * N, n_frames=bad.astype(np.int32), T_max=T_max, tag=tag, weighted=not big)
        for i in range(N):
            assert_equals_host(dev, i, host_run(engine, mode, p[i][:want[i]], delta), f"{tag}{i}")
    al.check()


# ---- test 5: independence ----------------------------------------------------------------------------------------------------------------------

def check_independence(al, lib, sizes=(), long_frames=0):
    """A clip gives the same bytes alone, as any wave of a workgroup, at index 8 of 9 and on a repeated launch; with ``sizes`` also
    in full grids of that many clips, with ``long_frames`` next to one clip of that many frames."""
    rng = np.random.default_rng(6)
    mode, C, delta = 0, 5, 12.5
    engine = host_engine(mode, C, negative=3, threshold=0.4, smoothing_ms=50.0, window_ms=600.0, tolerance_ms=100.0, sequence=[0, 1, 2, 0, 1, 2, 0, 1])
    clips = [random_probs(rng, mode, C, T) for T in (150, 1, 33, 64, 65, 7, 90, 2, 120)]
    cfg, keep = engine_config(al, engine, mode, "ind.")
    keys = ("present", "status", "n_labels", "first_kept", "end_time")

    def run(cs, tag):
        return device_run(al, lib, cfg, cs, [delta] * len(cs), tag=tag)

    def same(dev, k, ref, j, what):
        n = int(ref["n_labels"][j])
        assert all(same_bits(dev[key][k:k + 1], ref[key][j:j + 1]) for key in keys), what
        assert same_bits(dev["hist_time"][k, :n], ref["hist_time"][j, :n]) and same_bits(dev["hist_label"][k, :n], ref["hist_label"][j, :n]), what
    ref = run(clips, "all.")
    assert_equals_host(ref, 0, host_run(engine, mode, clips[0], delta), "independence clip 0")
    assert ref["n_labels"][0] > 50 and ref["first_kept"][0] > 0
    again = run(clips, "again.")
    for j in range(len(clips)):
        same(again, j, ref, j, f"repeated launch, clip {j}")
    same(run(clips[:1], "solo."), 0, ref, 0, "alone")
    for wave in range(1, 4):
        same(run(clips[1:1 + wave] + clips[:1], f"wave{wave}."), wave, ref, 0, f"wave {wave} of a workgroup")
    same(run(clips[1:] + clips[:1], "moved."), 8, ref, 0, "index 8 of 9")
    for N in sizes:
        dev = run([clips[i % 9] for i in range(N)], f"N{N}.")
        for i in range(N):
            same(dev, i, ref, i % 9, f"N={N} clip {i}")
    if long_frames:
        long = random_probs(rng, mode, C, long_frames)
        dev = run([clips[0], long, clips[3]], "long.")
        same(dev, 0, ref, 0, "next to a long clip")
        same(dev, 2, ref, 3, "next to a long clip")
        assert_equals_host(dev, 1, host_run(engine, mode, long, delta), f"{long_frames} frames")
    al.check()


def check_long_window(al, lib, frames=(900, 700, 300, 257)):
    """A matcher window that keeps more entries than the kernel mirrors in LDS (DC_TAIL = 256): the drop test and the rescans read
    the older entries back from the caller's history arrays.  Sequence mode, a sequence that never completes (16 labels with a 100 ms tolerance), windows of 6000 ms (480 frames: drops and rescans over more than 256 kept
    entries) and of infinity (nothing dropped: the drop test reads entry 0 back on every frame)."""
    rng = np.random.default_rng(9)
    mode, C, delta = 0, 5, 12.5
    clips = [random_probs(rng, mode, C, T) for T in frames]
    for window in (6000.0, float("inf")):
        engine = host_engine(mode, C, negative=3, threshold=0.3, smoothing_ms=30.0, window_ms=window, tolerance_ms=100.0, sequence=[0, 1, 2, 1] * 4)
        tag = f"long.{window}."
        cfg, keep = engine_config(al, engine, mode, tag)
        dev = device_run(al, lib, cfg, clips, [delta] * len(clips), tag=tag)
        hosts = [host_run(engine, mode, c, delta) for c in clips]
        kept = [h["n_labels"] - h["first_kept"] for h in hosts]
        print(f"long window {window}: entries {[h['n_labels'] for h in hosts]}, kept at the end {kept}, first_kept {[h['first_kept'] for h in hosts]}")
        assert not any(h["present"] for h in hosts) and max(kept) > 256 + 32, kept      # the inputs do reach the read-back
        if window == 6000.0:
            assert hosts[0]["first_kept"] > 50 and hosts[0]["events"]["dropped"] > 50      # ... through drops, each followed by a rescan
        for i, h in enumerate(hosts):
            assert_equals_host(dev, i, h, f"{tag}{i}")
    al.check()


# ---- test 6: refusals -----------------------------------------------------------------------------------------------------------------------------

def supported_table():
    """[(config fields, T_max, supported)]"""
    base = dict(mode=0, C=5, blank=4, negative=3, threshold=0.5, smoothing_ms=50.0, window_ms=2000.0, tolerance_ms=500.0, seq_len=3)
    rows = [({}, 100, 1), (dict(mode=1), 100, 1), (dict(mode=2), 100, 0), (dict(mode=-1), 100, 0), (dict(C=1), 100, 1), (dict(C=64), 100, 1),
            (dict(C=65), 100, 0), (dict(C=0), 100, 0), (dict(seq_len=0), 100, 1), (dict(seq_len=16), 100, 1), (dict(seq_len=17), 100, 0),
            (dict(seq_len=-1), 100, 0), ({}, 8192, 1), ({}, 8193, 0), ({}, 0, 1), ({}, -1, 0), (dict(smoothing_ms=0.0), 100, 1),
            (dict(smoothing_ms=-1.0), 100, 0), (dict(smoothing_ms=float("inf")), 100, 0), (dict(smoothing_ms=float("nan")), 100, 0),
            (dict(threshold=float("nan")), 100, 0), (dict(window_ms=float("nan")), 100, 0), (dict(tolerance_ms=float("nan")), 100, 0),
            (dict(window_ms=float("inf")), 100, 1)]
    return [({**base, **d}, t, ok) for d, t, ok in rows]


def check_supported_table(*libs):
    for fields, t_max, ok in supported_table():
        cfg = HowlDecideConfig(**fields)
        for lb in libs:
            assert lb.cdll.howl_decide_supported(ctypes.byref(cfg), t_max) == ok, (fields, t_max)
    for lb in libs:
        assert lb.cdll.howl_decide_supported(None, 100) == 0


def check_decider_supported():
    """DeviceDecider.supported: the C range plus the ring's bound floor(smoothing_ms / min delta) + 1 <= 32."""
    from howl_amd.model.decision import DeviceDecider
    def d(**k):
        a = dict(mode=0, num_labels=5, blank=4, negative=3, threshold=0.5, smoothing_ms=50.0, window_ms=2000.0, tolerance_ms=500.0, sequence=[0, 1, 2])
        a.update(k)
        return DeviceDecider(**a)
    assert d().supported(400, 12.5) and d(smoothing_ms=387.5).supported(400, 12.5)              # 31 + 1 frames
    assert not d(smoothing_ms=400.0).supported(400, 12.5)                                         # 32 + 1
    assert d(smoothing_ms=400.0).supported(32, 12.5) and d(smoothing_ms=1e9).supported(32, 0.0)   # (a clip cannot hold more than it has)
    assert not d(smoothing_ms=1e9).supported(33, 0.0)
    assert not d(num_labels=65).supported(10, 12.5) and not d(sequence=[0] * 17).supported(10, 12.5) and not d().supported(8193, 12.5)
    assert not d(color_map={0: -1}).supported(10, 12.5) and not d(weights=np.ones(4)).supported(10, 12.5)
    assert d(weights=np.ones(5), color_map={}).supported(10, 12.5) and d(weights=1).weights is None
    assert d().supported(10, 12.5, 8192) and not d().supported(10, 12.5, 8193) and not d().supported(10, 12.5, 0)
    # a threshold that is not a Python number is compared in its own type on the host (np.float64: in fp64), not in fp32
    assert not d(threshold=np.float64(0.5)).supported(10, 12.5) and not d(threshold=np.float32(0.5)).supported(10, 12.5)
    assert d(threshold=0).supported(10, 12.5)


def check_ring_overflow(dev_of, lib):
    """A frame period the caller did not declare overflows the ring: status 1 from the kernel, the clip replayed on the host by
    DeviceDecider.run with the host loops' result (``dev_of``: numpy -> tensor on the side under test).  Both modes, with weights
    and a colour map, so that every branch of the replay is held to the engines' own loops."""
    from howl_amd.model.decision import DeviceDecider
    rng = np.random.default_rng(7)
    C = 5
    weights, cmap, seq = np.array([0.5, 2.0, 1.0, 1.5, 0.6]), {0: 0, 1: 1, 2: 1, 3: 3}, [0, 1] * 8
    for mode, slow in ((1, 63.0), (0, 12.5)):
        frames = [120, 20, 90]
        clips = [random_probs(rng, mode, C, T) for T in frames]
        deltas = [1.0, slow, 1.0]
        dd = DeviceDecider(mode, C, 4, 3, 0.4, 80.0, 2000.0, 500.0, seq, weights=weights, color_map=cmap)
        assert not dd.supported(120, 1.0) and dd.supported(120, slow)
        probs = np.zeros((3, 120, C), np.float32)
        for i, c in enumerate(clips):
            probs[i, :len(c)] = c
        seen = []
        real = dd.replay
        dd.replay = lambda p, delta: (seen.append(len(p)), real(p, delta))[1]
        present, hists, ends = dd.run(dev_of(probs), frames, deltas)
        assert seen == [120, 90], (mode, seen)                     # clips 0 and 2 overflowed (81 frames inside 80 ms), clip 1 did not
        for i, c in enumerate(clips):
            engine = host_engine(mode, C, negative=3, threshold=0.4, smoothing_ms=80.0, sequence=seq, weights=weights, color_map=cmap,
                                 stride_ms=deltas[i])
            h = host_run(engine, mode, c, deltas[i])
            assert h["n_labels"] > (32 if i != 1 else 0)
            assert present[i] == h["present"] and hists[i] == h["history"][h["first_kept"]:] and ends[i] == h["end_time"], (mode, i)


ARG_ERRORS = [
    (dict(probs=None), r"howl_decide_clips: null pointer"),
    (dict(cfg=None), r"howl_decide_clips: null pointer"),
    (dict(hist_label=None), r"howl_decide_clips: null pointer"),
    (dict(N=0), r"howl_decide_clips: N=0 clips unsupported"),
    (dict(N=8193), r"howl_decide_clips: N=8193 clips unsupported"),
    (dict(C=65), r"howl_decide_clips: C=65 classes unsupported"),
    (dict(seq_len=17), r"howl_decide_clips: seq_len=17 unsupported"),
    (dict(T_max=8193), r"howl_decide_clips: T_max=8193 frames unsupported"),
    (dict(mode=3), r"howl_decide_clips: mode=3 unsupported"),
    (dict(smoothing_ms=-1.0), r"howl_decide_clips: smoothing_ms=-1.*unsupported"),
    (dict(hist_ld=9), r"howl_decide_clips: hist_ld=9 entries per clip, a clip may append 10"),
    (dict(s_frame=-1), r"howl_decide_clips: negative stride"),
]


def check_argument_errors(lb):
    import pytest
    from howl_amd import lib
    one = ctypes.c_void_p(16)      # never dereferenced: every call below is refused first

    def call(cfg=True, probs=one, s_frame=5, N=1, T_max=10, hist_label=one, hist_ld=10, **fields):
        c = HowlDecideConfig(**{**dict(mode=0, C=5, blank=4, negative=3, threshold=0.5, smoothing_ms=50.0, window_ms=2000.0, tolerance_ms=500.0,
                                       seq_len=3), **fields})
        lb.call("howl_decide_clips", ctypes.byref(c) if cfg is not None else None, probs, 50, s_frame, N, T_max, one, one, one, one, one, one, one,
                one, hist_label, hist_ld, None, None)
    for kwargs, text in ARG_ERRORS:
        with pytest.raises(lib.HowlHipError, match=text):
            call(**kwargs)


# ---- test 7: the engines (the same code on the device and, inside emu_util.emulated_package(), on the emulator) ---------------------------

def _both_ways(engine, clips, library, launches):
    """infer_many with the switch off, then on -> (results, histories); equal entry for entry, the engine left reset, the entry point
    called ``launches`` times with the switch on and never with it off."""
    from stream_util import CallLog
    engine.device_decisions = False
    with CallLog(library) as log:
        want = engine.infer_many(clips)
    hists = [list(h) for h in engine.clip_histories]
    assert "howl_decide_clips" not in log.names, log.names
    engine.device_decisions = True
    with CallLog(library) as log:
        got = engine.infer_many(clips)
    assert log.names.count("howl_decide_clips") == launches, log.names
    assert got == want, (got, want)
    assert len(engine.clip_histories) == len(hists) == len(clips)
    for i, (a, b) in enumerate(zip(engine.clip_histories, hists)):
        assert a == b, f"clip {i}: label history differs"
        assert all(type(s) in (int, float) and type(l) is int for s, l in a)
    assert engine.label_history == [] and engine.curr_time == 0 and engine.pred_history == [] and engine.model.streaming_state is None
    engine.device_decisions = False
    return want, hists


def check_sequence_engine(golden, dev, library, sizes=(16000, 12000, 8000, 6000, 4321, 1000, 400), later=slice(None)):
    """InferenceEngine (seq-lstm, fused_chunks on): the inputs of tests/lstm_stream_util.py, whose fp64 top-2 margin is asserted
    first; settings retuned after construction are honoured; a smoothing window beyond the ring falls back to the host replay.
    ``later``: the clips of the legs behind the first (the emulator takes the short ones)."""
    import lstm_stream_util as u
    from howl_amd.utils.synth import synthetic_pcm
    sd, _ = u.infer_many_inputs()
    pcm = synthetic_pcm(len(sizes), 16000, seed=77)
    clips = [pcm[i, :n].clone() for i, n in enumerate(sizes)]
    # the model answers "blank" on most of these frames: the two settings below weight the blank down, and the margin that makes exact
    # equality a fair demand is the one behind the weighting
    weightings = (np.array([1.0, 1.0, 1.0, 1.0, 0.01]), np.array([3.0, 1.0, 4.0, 1.0, 0.001]))
    p64 = np.concatenate([u.softmax64(u.oracle64(sd, c.numpy(), u.g4_pair())[0]) for c in clips])
    for w in weightings:
        q = np.sort(p64 * w / (p64 * w).sum(-1, keepdims=True), -1)
        worst = float((q[:, -1] - q[:, -2]).min())
        print(f"sequence engine inputs: {len(p64)} frames, fp64 top-2 margin behind the weights {w.tolist()}: {worst:.3e}")
        assert worst >= 1e-4, worst
    engine = u.seq_engine(golden, dev, sd, fused=True)
    dclips = [c.to(dev) for c in clips]
    engine.sequence, engine.smoothing_window_ms, engine.threshold, engine.inference_weights = [0, 2, 0, 3], 0, 0.0, weightings[0]
    first = _both_ways(engine, dclips, library, 1)
    seen = {l for h in first[1] for _, l in h}
    print(f"sequence engine: {sum(len(h) for h in first[1])} history entries, labels {sorted(seen)}, detections {first[0]}")
    assert sum(len(h) for h in first[1]) > 50 and len(seen) >= 3
    everything, dclips = dclips, dclips[later]
    first = (first[0][later], first[1][later])
    engine.sequence, engine.smoothing_window_ms, engine.threshold, engine.inference_window_ms = [2, 0], 50, 0.6, 700
    engine.tolerance_window_ms = 200
    engine.inference_weights = weightings[1]
    second = _both_ways(engine, dclips, library, 1)
    print(f"sequence engine, retuned: detections {second[0]}")
    assert second[1] != first[1], "the retuned settings change nothing on the host path: the inputs do not test them"
    assert any(second[0]) and not all(second[0])
    engine.smoothing_window_ms = 12.5 * 40                                    # 41 frames at a time: beyond the ring (for a clip that long)
    assert max(sizes) // 200 >= 40
    _both_ways(engine, everything, library, 0)
    engine.smoothing_window_ms, engine.fused_chunks = 50, False              # without the streaming launch: the plain loop of infer
    _both_ways(engine, dclips[-2:], library, 0)


def check_frame_engine(golden, dev, library, extra_windows=(9, 0, 5, 12, 2, 7, 3), later=slice(None)):
    """FrameInferenceEngine (res8): random weights, short synthetic clips, the fp64 top-2 margin of every window asserted first."""
    import stream_util as su
    from howl_amd.context import InferenceContext
    from howl_amd.data.transform.operator import ZmuvTransform
    from howl_amd.model import RegisteredModel
    from howl_amd.model.inference import FrameInferenceEngine
    from howl_amd.utils.synth import synthetic_pcm
    C = 4
    sd = su.random_state(C, 42)
    sizes = [8000 + 1008 * k + 37 * i for i, k in enumerate(extra_windows)] + [5000, 700]
    pcm = synthetic_pcm(len(sizes), max(sizes), seed=13)
    clips = [pcm[i, :n].clone() for i, n in enumerate(sizes)]
    rows = np.concatenate([np.stack([c.numpy()[s:s + 8000] for s in range(0, len(c) - 8000 + 1, 1008)]) for c in clips[:-2]])
    # random res8 weights answer with their output bias whatever the window holds: the output layer centred on these windows and
    # scaled to logits of spread 2, so that the labels vary from window to window
    z = su.oracle_logits64(sd, rows)
    k = 2.0 / z.std(0).mean()
    sd["output.bias"] = ((sd["output.bias"].double() - torch.from_numpy(z.mean(0))) * k).float()
    sd["output.weight"] = (sd["output.weight"].double() * k).float()
    p = su.softmax64(su.oracle_logits64(sd, rows))
    top = np.sort(p, -1)
    worst, labels = float((top[:, -1] - top[:, -2]).min()), set(p.argmax(-1).tolist())
    print(f"frame engine inputs: fp64 top-2 margin {worst:.3e}, labels {sorted(labels)}")
    assert worst >= 1e-2 and len(labels) >= 3, (worst, labels)      # (the fp32 paths' error on these logits is below 1e-3)
    ctx = InferenceContext(["hey", "fire", "fox"], token_type="word")
    assert ctx.num_labels == C
    model = RegisteredModel.find_registered_class("res8")(C)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model = model.to(dev).eval().streaming()
    zmuv = ZmuvTransform().to(dev)
    zmuv.mean.fill_(float(su.ZMUV_PAIR[0]))
    zmuv.mean2.fill_(float(su.ZMUV_PAIR[1]) ** 2 + float(su.ZMUV_PAIR[0]) ** 2)
    zmuv.total.fill_(1)
    engine = FrameInferenceEngine(500, 63, model, zmuv, ctx)
    dclips = [c.to(dev) for c in clips]
    engine.sequence, engine.threshold = sorted(labels)[:2], 0.0
    first = _both_ways(engine, dclips, library, 1)                    # (the two clips shorter than a window have none: no frame, no history)
    assert first[1][-1] == [] and first[1][-2] == [] and sum(len(h) for h in first[1]) >= len(extra_windows)
    many = engine.window_probabilities_many(dclips[-4:])
    assert [len(m) for m in many] == [0 if n < 8000 else (n - 8000) // 1008 + 1 for n in sizes[-4:]] and all(isinstance(m, np.ndarray) for m in many)
    assert all(m.dtype == np.float32 and m.shape[1] == C for m in many)
    engine.sequence, engine.threshold, engine.smoothing_window_ms, engine.inference_window_ms = [sorted(labels)[-1]] * 2, 0.55, 130, 300
    engine.MAX_WINDOWS_PER_LAUNCH = 7                                  # (and the probabilities in pieces)
    second = _both_ways(engine, dclips[later], library, 1)
    print(f"frame engine: detections {first[0]}, retuned {second[0]}")
    assert second[1] != first[1][later], "the retuned settings change nothing on the host path: the inputs do not test them"
    assert any(first[0] + second[0]) and not all(first[0] + second[0])
    # a smoothing window of 33 strides is beyond the ring only for clips that long: these keep the launch; a sequence of 20 labels
    # is outside the kernel's range: the host replay, no launch
    engine.smoothing_window_ms = 63 * 32
    engine.device_decisions = True
    assert engine._device_decider(1, 33, 63, 1) is None and engine._device_decider(1, 32, 63, 1) is not None
    engine.sequence = list(range(4)) * 5
    _both_ways(engine, dclips[-4:], library, 0)


def check_switch_default(monkeypatch):
    monkeypatch.delenv("HOWL_DECIDE_DEVICE", raising=False)
    from howl_amd.model.inference import FrameInferenceEngine, InferenceEngine
    ctx = types.SimpleNamespace(num_labels=5, blank_label=4, negative_label=3, coloring=None)
    assert InferenceEngine(types.SimpleNamespace(streaming_state=None), None, ctx).device_decisions is False
    for value, on in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv("HOWL_DECIDE_DEVICE", value)
        assert InferenceEngine(types.SimpleNamespace(streaming_state=None), None, ctx).device_decisions is on
        assert FrameInferenceEngine(500, 63, types.SimpleNamespace(streaming_state=None), None, ctx).device_decisions is on


# ---- test 8: the golden histories with the switch on --------------------------------------------------------------------------------------------

def check_g8_sequence(golden, dev, library):
    """tests/test_gpu_engine.py's G8 check of the sequence engine restated with the switch on: clip_histories[0] of infer_many is
    the reference engine's label history, bit for bit, and the verdict is its verdict -- as one stream launch and one decision
    launch."""
    import lstm_stream_util as u
    from oracle import models as om
    from stream_util import CallLog
    from howl_amd.settings import SETTINGS
    g = golden("g8_seq_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    SETTINGS.inference_engine.smoothing_window_ms = 0
    try:
        engine = u.seq_engine(golden, dev, om.lstm_init(int(g["num_labels"])), fused=True)
        engine.device_decisions = True
        with CallLog(library) as log:
            present = engine.infer_many([torch.from_numpy(np.asarray(g["clip"], np.float32)).to(dev)])
        assert log.names.count("howl_decide_clips") == 1 and log.names.count("howl_lstm_stream_chunks") == 1, log.names
        assert present == [bool(g["present"])]
        hist = np.array(engine.clip_histories[0], dtype=np.float64)
        assert hist.shape == g["label_history"].shape
        assert same_bits(hist, np.asarray(g["label_history"], np.float64)), np.abs(hist - g["label_history"]).max(0)
    finally:
        SETTINGS.reset()


def check_g8_frame(golden, dev, library):
    """The same for the frame engine (res8 with the closed-form weights, 500 ms windows at a 63 ms stride)."""
    import stream_util as su
    from stream_util import CallLog
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        engine = su.g8_engine(golden, dev, fused=False)
        engine.device_decisions = True
        with CallLog(library) as log:
            present = engine.infer_many([torch.from_numpy(np.asarray(g["clip"])).to(dev)])
        assert log.names.count("howl_decide_clips") == 1, log.names
        assert present == [bool(g["present"])]
        hist = np.array(engine.clip_histories[0], dtype=np.float64)
        assert hist.shape == g["label_history"].shape
        assert same_bits(hist, np.asarray(g["label_history"], np.float64)), np.abs(hist - g["label_history"]).max(0)
    finally:
        SETTINGS.reset()
