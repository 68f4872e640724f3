"""-m gpu: streaming small-cnn / seq-cnn (include/howl_hip_cnn_stream.h) on the device -- the checks of
tests/test_emu_cnn_stream.py with every operand between sentinel bands (tests/guard_mem.py Banded), a launch of more workgroups
than compute units, one clip at the top of the range (1,638,399 samples: index arithmetic at 8192 frames), and the small-cnn
session from a worker thread on a stream of its own."""
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

import cnn_stream_util as u  # noqa: E402
from cnn_util import SEQ, SMALL  # noqa: E402
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


@pytest.mark.parametrize("case", u.SMALL_CASES, ids=u.small_id)
def test_small_cnn_logits_against_the_fp64_oracle(case):
    """e_fused <= 2 e_eager + 1e-6; bands around probs, logits, ws, pcm, fbp, the pair and every parameter unchanged, exactly [N, C]
    written."""
    from howl_amd import lib
    al = _banded()
    N, L, C, variant = case
    u.check_small(al, lib.get(), N, L, C, variant)
    _no_band_changed(al)


@pytest.mark.parametrize("case", u.SEQ_CASES, ids=u.seq_id)
def test_seq_cnn_logits_against_the_fp64_oracle(case):
    from howl_amd import lib
    al = _banded()
    sizes, C, variant = case
    u.check_seq(al, lib.get(), sizes, C, variant)
    _no_band_changed(al)


def test_seq_cnn_clip_at_the_top_of_the_range():
    """One clip of 1,638,399 samples (8192 frames, 1024 rows, 128 tiles), C = 2, against the eager chain and the oracle under the
    same bound."""
    from howl_amd import lib
    al = _banded()
    assert u.rows_of(1638399) == 1024
    u.check_seq(al, lib.get(), [1638399], 2)
    _no_band_changed(al)


def test_windows_are_independent_and_launches_repeat():
    """With the launch of 257 windows of 8000 samples: more workgroups than compute units; rows 0, 1 and 256 equal their N = 1
    bits."""
    from howl_amd import lib
    al = _banded()
    u.check_small_independence(al, lib.get(), many=257)
    _no_band_changed(al)


def test_clips_are_independent_of_their_launch():
    from howl_amd import lib
    al = _banded()
    u.check_seq_independence(al, lib.get())
    _no_band_changed(al)


@pytest.mark.parametrize("kind", [SMALL, SEQ], ids=["small", "seq"])
def test_refusals_name_the_entry_point_and_write_nothing(kind):
    from howl_amd import lib
    al = _banded()
    u.check_refusals(al, lib.get(), kind)
    _no_band_changed(al)


def test_range_tables_have_zeros_at_every_edge():
    from howl_amd import lib
    u.check_tables(lib.get())


def test_fused_and_eager_ingest_frame_agree_over_the_g8_clip(golden):
    from howl_amd import lib
    u.check_small_engine(golden, DEV, lib.get())


def test_frame_engine_switch_is_opt_in(golden, monkeypatch):
    u.check_small_switch(golden, DEV, monkeypatch)


def test_fused_and_eager_infer_agree_on_two_chunks(golden):
    from howl_amd import lib
    u.check_seq_infer(golden, DEV, lib.get())


def test_infer_many_matches_the_per_clip_loop(golden):
    from howl_amd import lib
    u.check_seq_infer_many(golden, DEV, lib.get())


@pytest.mark.parametrize("kind", [SMALL, SEQ], ids=["small", "seq"])
def test_session_answers_for_the_weights_as_they_are(kind):
    u.check_session(kind, DEV)


def test_session_from_a_worker_thread_on_its_own_stream(golden):
    """What the client's callback thread does: five fused ingest_frame calls and a 37-window launch on a non-default stream from a
    worker thread give the bits of the main thread's default-stream run, while the main thread keeps its own session busy."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        clip = torch.from_numpy(np.asarray(g["clip"])).to(DEV)
        main_engine = u.small_engine(golden, DEV, fused=True)
        windows, starts, chunk = u.windows_of(clip, main_engine)
        solo = main_engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
        main_labels = [main_engine.ingest_frame(clip[i * 1008: i * 1008 + 8000], curr_time=63.0 * i) for i in range(5)]
        out, start = {}, threading.Event()

        def worker():
            try:
                engine = u.small_engine(golden, DEV, fused=True)
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
        assert out["labels"] == main_labels
        assert np.array_equal(out["probs"], solo) and all(np.array_equal(m, solo) for m in mine)
    finally:
        SETTINGS.reset()
