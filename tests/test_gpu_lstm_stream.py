"""-m gpu: streaming seq-lstm / lstm (include/howl_hip_lstm_stream.h) on the device -- the checks of tests/test_emu_lstm_stream.py
with every operand between sentinel bands (tests/guard_mem.py Banded), full grids (N = 257, 1024), long clips (G15's audio, 1000
frames), the session from a worker thread on a stream of its own, and `train.main` scoring its CTC evaluation passes 64 clips per
launch."""
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

import lstm_stream_util as u  # noqa: E402
from gpu_util import DEV  # noqa: E402
from test_emu_lstm_stream import ORACLE_CASES  # noqa: E402

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


# ---- 1 / 7: against the fp64 oracle, sentinel bands around every operand -----------------------------------------------------------

@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_logits_and_state_against_the_fp64_oracle(case):
    from howl_amd import lib
    lengths, C, state, zmuv, last_only = ORACLE_CASES[case]
    al = _banded()
    u.check_case(al, lib.get(), lengths, C, state=state, zmuv=zmuv, last_only=last_only, what=case + ".")
    _no_band_changed(al)


def test_long_clips_g15_audio_and_1000_frames(golden):
    """G15's whole clips (64000 samples; 318 frames as compute_lengths counts them, through `frames`) and a clip of 1000 frames."""
    from howl_amd import lib
    from howl_amd.utils.synth import synthetic_pcm
    al = _banded()
    m = u.Model(al, lib.get(), u.random_state(5, 1515))
    audio = np.asarray(golden("g15_whole_clips_seq_lstm")["audio"], np.float32)
    long = synthetic_pcm(1, 199800, seed=4).numpy().astype(np.float32)[0]
    assert u.compute_lengths(audio.shape[1]) == 318 and u.num_frames(len(long)) == 1000
    for tag, clips, frames in (("g15.", [a.copy() for a in audio[:3]], [318] * 3), ("f1000.", [long, long[:4321].copy()], None)):
        zero = (np.zeros((len(clips), 128), np.float32), np.zeros((len(clips), 128), np.float32))
        probs, logits, (h, c) = m.chunks(clips, frames=frames, state=zero, tag=tag)
        e_fused = e_eager = s_fused = s_eager = 0.0
        for i, clip in enumerate(clips):
            fr = frames[i] if frames else u.num_frames(len(clip))
            ey, eh, ec = m.eager(clip, frames[i] if frames else None, tag=f"{tag}eager{i}.")
            oy, oh, oc = m.oracle(clip, frames[i] if frames else None)
            e_fused, e_eager = max(e_fused, np.abs(logits[i, :fr] - oy).max()), max(e_eager, np.abs(ey - oy).max())
            s_fused = max(s_fused, np.abs(h[i] - oh).max(), np.abs(c[i] - oc).max())
            s_eager = max(s_eager, np.abs(eh - oh).max(), np.abs(ec - oc).max())
            assert not probs[i, fr:].any() and not logits[i, fr:].any()
            assert np.abs(probs[i, :fr] - u.softmax64(logits[i, :fr])).max() <= 1e-6
        print(f"lstm stream long clips {tag} logits e_fused={e_fused:.3e} e_eager={e_eager:.3e}; (h, c) e_fused={s_fused:.3e} e_eager={s_eager:.3e}")
        assert e_fused <= 2 * e_eager + 1e-6 and s_fused <= 2 * s_eager + 1e-6, (e_fused, e_eager, s_fused, s_eager)
    _no_band_changed(al)


@pytest.mark.parametrize("N", [257, 1024])
def test_full_grids(N):
    """N = 257 and N = 1024 streams in one launch: eight ragged clips repeated over the batch.  The first eight against the oracle
    as item 1; every other stream the same bits as the clip it repeats (item 3 at scale); bands unchanged."""
    from howl_amd import lib
    from howl_amd.utils.synth import synthetic_pcm
    al = _banded()
    C = 5
    m = u.Model(al, lib.get(), u.random_state(C, N))
    lengths = [8000, 400, 4321, 3000, 16000, 1000, 3200, 6800]
    pcm = synthetic_pcm(8, 16000, seed=N).numpy().astype(np.float32)
    base = [pcm[i, :n].copy() for i, n in enumerate(lengths)]
    clips = [base[i % 8] for i in range(N)]
    zero = (np.zeros((N, 128), np.float32), np.zeros((N, 128), np.float32))
    probs, logits, (h, c) = m.chunks(clips, state=zero, tag="grid.")
    for i in range(8, N):
        assert np.array_equal(probs[i], probs[i % 8]) and np.array_equal(logits[i], logits[i % 8]), i
        assert np.array_equal(h[i], h[i % 8]) and np.array_equal(c[i], c[i % 8]), i
    e_fused = e_eager = 0.0
    for i, clip in enumerate(base):
        fr = u.num_frames(len(clip))
        ey, _, _ = m.eager(clip, tag=f"eager{i}.")
        oy, _, _ = m.oracle(clip)
        e_fused, e_eager = max(e_fused, np.abs(logits[i, :fr] - oy).max()), max(e_eager, np.abs(ey - oy).max())
        assert not probs[i, fr:].any()
    print(f"lstm stream N={N}: e_fused={e_fused:.3e} e_eager={e_eager:.3e}")
    assert e_fused <= 2 * e_eager + 1e-6, (e_fused, e_eager)
    _no_band_changed(al)


def test_out_of_contract_lengths_are_clamped():
    from howl_amd import lib
    al = _banded()
    u.check_out_of_contract(al, lib.get())
    _no_band_changed(al)


# ---- 2 / 3 ---------------------------------------------------------------------------------------------------------------------------

def test_state_carried_over_two_chunks_of_the_g15_clips(golden):
    from howl_amd import lib
    al = _banded()
    u.check_state_carry(al, lib.get(), golden)
    _no_band_changed(al)


def test_streams_are_independent_and_launches_repeat():
    from howl_amd import lib
    al = _banded()
    u.check_independence(al, lib.get())
    _no_band_changed(al)


# ---- 4 / 5: the engines ----------------------------------------------------------------------------------------------------------------

def test_fused_infer_gives_the_g8_history_in_one_launch(golden):
    from howl_amd import lib
    u.check_g8_history(golden, DEV, lib.get())


def test_infer_many_equals_the_clip_by_clip_loop(golden):
    from howl_amd import lib
    u.check_infer_many(golden, DEV, lib.get())


def test_switch_defaults_off_and_the_call_log_is_todays(golden, monkeypatch):
    from howl_amd import lib
    u.check_switch_default(golden, DEV, lib.get(), monkeypatch)


def test_frame_engine_with_lstm_one_launch_per_window(golden):
    from howl_amd import lib
    u.check_frame_engine_lstm(golden, DEV, lib.get())


def test_fused_and_eager_calls_alternate_on_one_streaming_model(golden):
    u.check_streaming_alternation(golden, DEV, clips=4)


def test_session_contract(golden):
    u.check_session(golden, DEV)


# ---- 8: device only ----------------------------------------------------------------------------------------------------------------------

def test_session_from_a_worker_thread_on_its_own_stream(golden):
    """The session on a non-default stream from a worker thread gives the bits of the main thread's default-stream run, while the
    main thread keeps a session of its own busy."""
    from howl_amd.utils.synth import synthetic_pcm
    sd = u.random_state(5, 808)
    pcm = synthetic_pcm(6, 16000, seed=8).to(DEV)
    n_samples = torch.tensor([16000, 400, 4321, 8000, 3200, 12345], dtype=torch.int64, device=DEV)

    def run(engine, rounds):
        session = engine._lstm_session(type(engine.model), 16000)
        outs = []
        for _ in range(rounds):
            probs, state = session.probabilities(pcm, n_samples=n_samples)
            probs2, state2 = session.probabilities(pcm, n_samples=n_samples, state=state)
            outs.append((probs.cpu().numpy(), probs2.cpu().numpy(), state2[0].cpu().numpy(), state2[1].cpu().numpy()))
        return outs
    main_engine = u.seq_engine(golden, DEV, sd, fused=True)
    solo = run(main_engine, 1)[0]
    out, start = {}, threading.Event()

    def worker():
        try:
            engine = u.seq_engine(golden, DEV, sd, fused=True)
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                start.wait()
                res = run(engine, 5)
                stream.synchronize()
            out["res"] = res
        except BaseException as e:      # surfaces in the test thread
            out["exc"] = e

    th = threading.Thread(target=worker)
    th.start()
    start.set()
    mine = run(main_engine, 20)
    th.join(timeout=300)
    assert not th.is_alive() and "exc" not in out, out.get("exc")
    for r in out["res"] + mine:
        assert all(np.array_equal(a, b) for a, b in zip(r, solo))


def test_train_entry_point_scores_ctc_evaluation_64_clips_per_launch(tmp_path, monkeypatch):
    """`train.main` on a small --synthetic seq-lstm / ctc run with HOWL_STREAM_FUSED=1: every evaluation pass goes through
    InferenceEngine.infer_many in groups of 64, each group ONE stream launch and no launch chain; the confusion counts add up to the
    clip count."""
    from howl_amd import lib
    from howl_amd.model.inference import InferenceEngine
    from stream_util import CallLog
    env = dict(NUM_EPOCHS="2", BATCH_SIZE="16", MAX_WINDOW_SIZE_SECONDS="0.5", LEARNING_RATE="0.002", LR_DECAY="0.955", WEIGHT_DECAY="0.00001",
               NUM_MELS="40", DEVICE="cuda:0", OBJECTIVE="ctc", TOKEN_TYPE="word", VOCAB='["hey","fire","fox"]', INFERENCE_SEQUENCE="[0,1,2]",
               INFERENCE_THRESHOLD="0", SMOOTHING_WINDOW_MS="0", HOWL_STREAM_FUSED="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from howl_amd.settings import SETTINGS
    SETTINGS.reset()
    calls = []
    real = InferenceEngine.infer_many

    def counted(self, clips):
        clips = list(clips)
        with CallLog(lib.get()) as log:
            res = real(self, clips)
        calls.append((len(clips), log.names.count("howl_lstm_stream_chunks"), sum(log.names.count(n) for n in u.CHAIN)))
        return res
    monkeypatch.setattr(InferenceEngine, "infer_many", counted)
    try:
        from howl_amd.training.run import train
        pos, neg = train.main(["--model", "seq-lstm", "--workspace", str(tmp_path / "ws"), "--synthetic", "96", "--eval-freq", "1"])
        assert pos["tp"] + pos["fn"] == 32 and neg["fp"] + neg["tn"] == 32
        assert calls and all(n <= 64 and launches == -(-n // 64) and chain == 0 for n, launches, chain in calls), calls
        assert sum(n for n, _, _ in calls) % 32 == 0 and sum(n for n, _, _ in calls) >= 64, calls      # whole passes over 32 + 32 clips
    finally:
        SETTINGS.reset()
