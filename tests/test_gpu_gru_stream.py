"""-m gpu: streaming gru (include/howl_hip_gru_stream.h) on the device -- the checks of tests/test_emu_gru_stream.py with every
operand between sentinel bands (tests/guard_mem.py Banded), a launch of more workgroups than compute units, and the session from
a worker thread on a stream of its own."""
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

import gru_stream_util  # noqa: E402
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


@pytest.mark.parametrize("N,L,C,variant", gru_stream_util.CASES, ids=gru_stream_util.CASE_IDS)
def test_logits_against_the_fp64_oracle(N, L, C, variant):
    """Checks 1 and 3: e_fused <= 2 e_eager + 1e-6; bands around probs, logits, ws, pcm, fbp, the pair and every parameter unchanged,
    exactly [N, C] written."""
    from howl_amd import lib
    al = _banded()
    gru_stream_util.check_against_oracle(al, lib.get(), N, L, C, variant)
    _no_band_changed(al)


def test_windows_are_independent_and_launches_repeat():
    """Check 2, with the launch of 257 windows of 8000 samples: more workgroups than compute units."""
    from howl_amd import lib
    al = _banded()
    gru_stream_util.check_independence(al, lib.get(), many=257)
    _no_band_changed(al)


def test_refusals_name_the_entry_point_and_write_nothing():
    from howl_amd import lib
    al = _banded()
    gru_stream_util.check_refusals(al, lib.get())
    _no_band_changed(al)


def test_fused_and_eager_ingest_frame_agree_over_the_g8_clip(golden):
    from howl_amd import lib
    gru_stream_util.check_engine(golden, DEV, lib.get())


def test_session_answers_for_the_weights_as_they_are():
    gru_stream_util.check_session(DEV)


def test_session_from_a_worker_thread_on_its_own_stream(golden):
    """Check 8, what the client's callback thread does: five fused ingest_frame calls and a 37-window launch on a non-default stream
    from a worker thread give the bits of the main thread's default-stream run, while the main thread keeps its own session busy."""
    from howl_amd.settings import SETTINGS
    g = golden("g8_frame_engine")
    SETTINGS.inference_engine.inference_sequence = [0, 1, 2]
    try:
        clip = torch.from_numpy(np.asarray(g["clip"])).to(DEV)
        main_engine = gru_stream_util.gru_engine(golden, DEV, fused=True)
        windows, starts, chunk = gru_stream_util.windows_of(clip, main_engine)
        solo = main_engine._fused_session(clip[:chunk]).probabilities(windows).cpu().numpy()
        main_labels = [main_engine.ingest_frame(clip[i * 1008: i * 1008 + 8000], curr_time=63.0 * i) for i in range(5)]
        out, start = {}, threading.Event()

        def worker():
            try:
                engine = gru_stream_util.gru_engine(golden, DEV, fused=True)
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
