"""-m gpu: the engines' decision logic on the device (include/howl_hip_decide.h) -- the checks of tests/test_emu_decide.py with
every operand between sentinel bands (tests/guard_mem.py Banded), all 64 random cases, full grids (N = 257, 1024), a clip of 8192
frames, the largest operands of the clamping case, the golden G8 histories with the switch on, a worker thread on a stream of its
own, and `train.main` with and without HOWL_DECIDE_DEVICE=1."""
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

import decide_util as u  # noqa: E402
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


def _lib():
    from howl_amd import lib
    return lib.get()


# ---- 1. - 5.: against the host replay, sentinel bands around every operand -----------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    cs = u.random_cases()
    return cs, u.host_results(cs)


def test_random_cases_equal_the_host_replay_in_both_modes(cases):
    al = _banded()
    u.check_random_cases(al, _lib(), *cases)
    _no_band_changed(al)


def test_normalisation_bit_for_bit():
    al = _banded()
    u.check_normalisation(al, _lib())
    _no_band_changed(al)


def test_threshold_edge_and_colour_map_without_the_label():
    al = _banded()
    u.check_threshold_edge(al, _lib())
    _no_band_changed(al)


def test_degenerate_shapes():
    al = _banded()
    u.check_degenerate(al, _lib())
    _no_band_changed(al)


def test_out_of_contract_frame_counts_are_clamped_smallest_and_largest_operands():
    al = _banded()
    u.check_clamped(al, _lib(), big=True)
    _no_band_changed(al)


def test_clips_are_independent_full_grids_and_a_clip_of_8192_frames():
    al = _banded()
    u.check_independence(al, _lib(), sizes=(257, 1024), long_frames=8192)
    _no_band_changed(al)


def test_matcher_window_longer_than_the_lds_tail_reads_the_history_back():
    al = _banded()
    u.check_long_window(al, _lib(), frames=(900, 700, 300, 257, 2000))
    _no_band_changed(al)


# ---- 6. refusals and fallback ------------------------------------------------------------------------------------------------------------------

def test_supported_table_and_argument_errors():
    u.check_supported_table(_lib())
    u.check_argument_errors(_lib())
    u.check_decider_supported()


def test_ring_overflow_sets_status_and_is_replayed_on_the_host():
    u.check_ring_overflow(lambda a: torch.from_numpy(a).to(DEV), _lib())


# ---- 7. the engines ---------------------------------------------------------------------------------------------------------------------------------

def test_sequence_engine_with_the_switch_on_equals_off(golden):
    u.check_sequence_engine(golden, DEV, _lib())


def test_frame_engine_with_the_switch_on_equals_off(golden):
    u.check_frame_engine(golden, DEV, _lib())


def test_switch_defaults_off(monkeypatch):
    u.check_switch_default(monkeypatch)


# ---- 8. device only -----------------------------------------------------------------------------------------------------------------------------------

def test_sequence_engine_gives_the_g8_history_with_the_switch_on(golden):
    u.check_g8_sequence(golden, DEV, _lib())


def test_frame_engine_gives_the_g8_history_with_the_switch_on(golden):
    u.check_g8_frame(golden, DEV, _lib())


def test_decider_from_a_worker_thread_on_its_own_stream():
    """DeviceDecider.run on a non-default stream from a worker thread gives the results of the main thread's default-stream run,
    while the main thread keeps launching its own."""
    from howl_amd.model.decision import DeviceDecider
    rng = np.random.default_rng(8)
    C, frames = 5, [150, 1, 64, 33, 90, 200]
    probs = np.zeros((len(frames), max(frames), C), np.float32)
    for i, T in enumerate(frames):
        probs[i, :T] = u.random_probs(rng, 0, C, T)
    dprobs = torch.from_numpy(probs).to(DEV)
    deltas = [12.5] * len(frames)

    def decider():
        return DeviceDecider(0, C, 4, 3, 0.4, 50.0, 600.0, 100.0, [0, 1, 2, 0, 1], weights=np.array([1.0, 2.0, 0.5, 1.0, 0.3]), color_map={0: 0, 1: 1, 2: 1})
    solo = decider().run(dprobs, frames, deltas)
    engine = u.host_engine(0, C, negative=3, threshold=0.4, smoothing_ms=50.0, window_ms=600.0, tolerance_ms=100.0, sequence=[0, 1, 2, 0, 1],
                           weights=[1.0, 2.0, 0.5, 1.0, 0.3], color_map={0: 0, 1: 1, 2: 1})
    for i, T in enumerate(frames):
        h = u.host_run(engine, 0, probs[i, :T], 12.5)
        assert solo[0][i] == h["present"] and solo[1][i] == h["history"][h["first_kept"]:] and solo[2][i] == h["end_time"], i
    out, start = {}, threading.Event()

    def worker():
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                mine = dprobs.clone()
                start.wait()
                res = [decider().run(mine, frames, deltas) for _ in range(5)]
                stream.synchronize()
            out["res"] = res
        except BaseException as e:      # surfaces in the test thread
            out["exc"] = e

    th = threading.Thread(target=worker)
    th.start()
    start.set()
    mine = [decider().run(dprobs, frames, deltas) for _ in range(20)]
    th.join(timeout=300)
    assert not th.is_alive() and "exc" not in out, out.get("exc")
    for r in out["res"] + mine:
        assert r == solo


def test_train_entry_point_counts_the_same_with_the_switch_on(tmp_path, monkeypatch):
    """`train.main` on a small --synthetic seq-lstm / ctc run with HOWL_STREAM_FUSED=1: the confusion counts of its evaluation with
    HOWL_DECIDE_DEVICE=1 are those of a run without, and with the switch every evaluation group is one decision launch whose
    verdicts and histories are those of the host replay on the same weights (each pass is scored both ways)."""
    from howl_amd.model.inference import InferenceEngine
    from stream_util import CallLog
    env = dict(NUM_EPOCHS="1", BATCH_SIZE="16", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.002", LR_DECAY="0.955", WEIGHT_DECAY="0.00001",
               NUM_MELS="40", DEVICE="cuda:0", OBJECTIVE="ctc", TOKEN_TYPE="word", VOCAB='["hey","fire","fox"]', INFERENCE_SEQUENCE="[0,1,2]",
               INFERENCE_THRESHOLD="0", SMOOTHING_WINDOW_MS="0", HOWL_STREAM_FUSED="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from howl_amd.settings import SETTINGS
    calls = []
    real = InferenceEngine.infer_many

    def counted(self, clips):
        clips = list(clips)
        host = None
        if self.device_decisions:
            self.device_decisions = False
            host = (real(self, clips), [list(h) for h in self.clip_histories])
            self.device_decisions = True
        with CallLog(_lib()) as log:
            res = real(self, clips)
        if host is not None:
            assert (list(res), self.clip_histories) == host
        calls.append((self.device_decisions, len(clips), log.names.count("howl_decide_clips")))
        return res
    monkeypatch.setattr(InferenceEngine, "infer_many", counted)
    results = {}
    try:
        from howl_amd.training.run import train
        for switch in ("0", "1"):
            monkeypatch.setenv("HOWL_DECIDE_DEVICE", switch)
            SETTINGS.reset()
            results[switch] = train.main(["--model", "seq-lstm", "--workspace", str(tmp_path / f"ws{switch}"), "--synthetic", "96", "--eval-freq", "1"])
        assert results["0"] == results["1"], results
        pos, neg = results["1"]
        assert pos["tp"] + pos["fn"] == 32 and neg["fp"] + neg["tn"] == 32
        off, on = [c for c in calls if not c[0]], [c for c in calls if c[0]]
        assert off and len(off) == len(on) and all(c[2] == 0 for c in off) and all(c[2] == -(-c[1] // 8192) for c in on), calls
    finally:
        SETTINGS.reset()
