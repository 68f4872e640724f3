"""-m gpu: streaming res8 (include/howl_hip_stream.h) on the device -- the checks of tests/test_emu_res8_stream.py with every
operand between sentinel bands (tests/guard_mem.py Banded), the fused ingest_frame against the eager one over a whole clip, 256
windows in one launch against the batched engine, and the session from a worker thread on a stream of its own."""
import sys
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for _p in (str(HERE.parent), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stream_util  # noqa: E402
from gpu_util import DEV  # noqa: E402

pytestmark = pytest.mark.gpu


def _banded():
    from guard_mem import Banded
    return Banded("cuda")


def _no_band_changed(al):
    torch.cuda.synchronize()
    bad = al.problems()
    if bad:
        al.describe()
    assert not bad, "; ".join(bad)


# ---- 7 / 9: items 1 and 2 with canary bands around probs, logits, state and every input -----------------------------------------

@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("L", [8000, 16000])
def test_logits_against_the_fp64_oracle(L, C):
    from howl_amd import lib
    al = _banded()
    stream_util.check_against_oracle(al, lib.get(), L, C)
    _no_band_changed(al)


@pytest.mark.parametrize("N,L", [(1, 400), (1, 8000), (3, 8600), (257, 8000), (3, 16599)])
def test_sentinel_bands_around_every_operand(N, L):
    """The smallest and the largest window, a full grid and a frame count (44) that takes the four-wave instance: bands unchanged,
    [N, C] written and nothing else, results as item 1."""
    from howl_amd import lib
    al = _banded()
    stream_util.check_against_oracle(al, lib.get(), L, 5, N=N, seed=N)
    _no_band_changed(al)


def test_windows_are_independent_and_launches_repeat():
    from howl_amd import lib
    al = _banded()
    stream_util.check_independence(al, lib.get())
    _no_band_changed(al)


def test_fused_ingest_frame_gives_the_g8_labels(golden):
    from howl_amd import lib
    stream_util.check_g8_labels(golden, DEV, lib.get())


def test_session_prepares_again_after_load_state_dict():
    stream_util.check_staleness(DEV)


def _windows_of(clip, engine):
    from howl_amd.utils import audio_utils
    starts, chunk = audio_utils.stride_starts(clip.size(-1), engine.max_window_size_ms, engine.eval_stride_size_ms, engine.sample_rate)
    return clip.as_strided((len(starts), chunk), (starts[1] - starts[0], 1)), starts, chunk


def _oracle_probs(engine, windows):
    sd = {k: v.detach().cpu() for k, v in engine.model.state_dict().items()}
    pair = engine.zmuv.pair().cpu().numpy()
    return stream_util.softmax64(stream_util.oracle_logits64(sd, windows.cpu().numpy(), pair))


def test_fused_and_eager_ingest_frame_agree_over_the_g8_clip(golden):
    """Every window of the G8 clip through ingest_frame, fused and eager: the same label history; the probabilities within item 1's
    bound (the fp64 oracle as the reference, the eager path's error as the yardstick)."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        clip = torch.from_numpy(np.asarray(g["clip"])).to(DEV)
        hist, raw = {}, {}      # label histories / window probabilities, by path
        for fused in (False, True):
            engine = stream_util.g8_engine(golden, DEV, fused)
            windows, starts, chunk = _windows_of(clip, engine)
            for i, s in enumerate(starts):
                engine.ingest_frame(clip[s:s + chunk], curr_time=float(engine.eval_stride_size_ms * i))
            hist[fused] = np.array(engine.label_history, dtype=np.float64)
        assert hist[True].shape[0] == int(g["n_windows"]) and np.array_equal(hist[True], hist[False])
        ref = _oracle_probs(engine, windows)
        raw[True] = engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
        engine.fused_windows = False
        raw[False] = engine.window_probabilities(clip)
        e_fused, e_eager = np.abs(raw[True] - ref).max(), np.abs(raw[False] - ref).max()
        print(f"G8 clip, {len(starts)} windows: e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
        assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
    finally:
        SETTINGS.reset()


def test_256_windows_of_a_10s_clip_in_one_launch(golden):
    """Item 8: 256 windows (500 ms at a 37 ms stride) of a 10 s synthetic clip in ONE launch against engine.window_probabilities on
    the same windows: item 1's bound on the probabilities, argmax identical."""
    from howl_amd import lib
    from howl_amd.utils.synth import synthetic_pcm
    engine = stream_util.g8_engine(golden, DEV, fused=True)
    engine.eval_stride_size_ms = 37
    clip = synthetic_pcm(1, 160000, seed=77)[0, :8000 + 255 * 592].contiguous().to(DEV)
    windows, starts, chunk = _windows_of(clip, engine)
    assert windows.shape == (256, 8000)
    with stream_util.CallLog(lib.get()) as log:
        fused = engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
    assert log.names.count("howl_res8_stream_windows") == 1
    eager = engine.window_probabilities(clip)
    ref = _oracle_probs(engine, windows)
    e_fused, e_eager = np.abs(fused - ref).max(), np.abs(eager - ref).max()
    print(f"256 windows: e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
    assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
    assert np.array_equal(fused.argmax(1), eager.argmax(1))


# ---- 10: a worker thread, a stream of its own ------------------------------------------------------------------------------------

def test_session_from_a_worker_thread_on_its_own_stream(golden):
    """What the client's callback thread does: the fused ingest_frame loop and a many-window launch on a non-default stream from a
    worker thread give the bits of the main thread's default-stream run, while the main thread keeps its own session busy."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        clip = torch.from_numpy(np.asarray(g["clip"])).to(DEV)
        main_engine = stream_util.g8_engine(golden, DEV, fused=True)
        windows, starts, chunk = _windows_of(clip, main_engine)
        solo = main_engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
        out, start = {}, threading.Event()

        def worker():
            try:
                engine = stream_util.g8_engine(golden, DEV, fused=True)
                stream = torch.cuda.Stream(device=DEV)
                with torch.cuda.stream(stream):
                    start.wait()
                    labels = [engine.ingest_frame(clip[i * 1008: i * 1008 + 8000], curr_time=63.0 * i) for i in range(5)]
                    probs = engine._fused_session(clip[:chunk]).probabilities(windows)
                    stream.synchronize()
                out["labels"], out["probs"] = labels, probs.cpu().numpy()
            except BaseException as e:      # surfaces in the test thread
                out["exc"] = e

        th = threading.Thread(target=worker)
        th.start()
        start.set()
        mine = [main_engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy() for _ in range(20)]
        th.join(timeout=300)
        assert not th.is_alive() and "exc" not in out, out.get("exc")
        assert out["labels"] == [int(x) for x in g["label_history"][:5, 1]]
        assert np.array_equal(out["probs"], solo) and all(np.array_equal(m, solo) for m in mine)
    finally:
        SETTINGS.reset()
