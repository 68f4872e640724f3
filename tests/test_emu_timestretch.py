"""Time-stretch augmentation (include/howl_hip_timestretch.h, howl_amd/csrc/timestretch.hip) on the hipemu emulator: the kernel
against the float64 restatement of its contract with the measured tolerance, the properties that need none (rate 1.0, the mix
operands, the two bank layouts), the refusals, header / exports / ctypes table, guard pages around every operand (in child
processes), and the host side under ``emulated_package``: DeviceCollate(timestretch=True) against the reference's recorded draws
(golden G18), timestretch=False against a collate built without the argument, and frame_batch's windows against the restated
stretch of their clips."""
import json
import os
import random
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for _p in (str(ROOT), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PLACEMENTS = ("tail", "head")
TIMEOUT = 900


@pytest.fixture(scope="module")
def emu():
    import emu_util
    return emu_util.emu_lib()


def _arena():
    from guard_mem import Arena
    return Arena("tail", log=open(os.devnull, "w"))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------

def test_ragged_batch_of_7_against_the_float64_restatement(emu):
    """Measured on the emulator (kernel error / float32-float64 gap): clip 0 (2048) rate 0.3: 8.2e-8 / 9.2e-8, rate 1.7: 6.6e-8 /
    5.6e-8; clip 1 (5000) rate 0.77: 6.2e-8 / 8.8e-8, rate 0.3: 6.8e-8 / 9.6e-8; clip 2 (16000) rate 1.31: 7.3e-8 / 1.0e-7, rate 0.77:
    1.2e-7 / 2.3e-7, rate 1.7: 1.2e-7 / 2.1e-7 -- the bound is 8 x the gap."""
    import timestretch_util as u
    al = _arena()
    u.check_batch7(al, emu)
    al.check()


def test_rate_one_through_the_transform_reproduces_the_input(emu):
    import timestretch_util as u
    al = _arena()
    u.check_identity(al, emu)
    al.check()


def test_mix_operands_equal_a_premixed_clip(emu):
    import timestretch_util as u
    al = _arena()
    u.check_mix(al, emu)
    al.check()


def test_dense_and_ragged_banks_give_the_same_bits(emu):
    import timestretch_util as u
    al = _arena()
    u.check_layouts(al, emu)
    al.check()


def test_refusals_have_messages(emu):
    import timestretch_util as u
    from howl_amd import lib
    short = u.check_refusals(emu, lib.HowlHipError)
    # what is not refused: a clip under 2048 samples at rate 1.0 is copied
    y = u.make_clips()[0]
    al = _arena()
    assert np.array_equal(u.run(al, emu, y, 1, short, 2047), y[:2047])
    al.check()


# ---- header, exports, table ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_the_timestretch_header(built, emu):
    import timestretch_util as u
    from howl_amd import lib
    text = (ROOT / "include" / "howl_hip_timestretch.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    hdr = set(re.findall(r"\b(howl_[a-z0-9_]+)\s*\(", code))
    assert hdr == {"howl_timestretch_clips"}, hdr
    table = set(lib.TIMESTRETCH_SIGNATURES) | set(lib.TIMESTRETCH_SIZE_FUNCS)
    assert table == hdr, table ^ hdr
    assert not table & (set(lib.SIGNATURES) | set(lib.SIZE_FUNCS))
    for path in (built, emu.path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
        assert hdr <= set(re.findall(r" T (howl_[a-z0-9_]+)\n", out)), path
    # the numpy record is the header's struct (field order, 48 bytes), the constants are the header's
    body = code[code.index("typedef struct {"):code.index("} HowlStretchClip;")]
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [n for n, _ in lib.STRETCH_CLIP_FIELDS] == list(u.CLIP_DTYPE.names), fields
    assert np.dtype(lib.STRETCH_CLIP_FIELDS) == u.CLIP_DTYPE and u.CLIP_DTYPE.itemsize == 48
    consts = dict(re.findall(r"#define (HOWL_TIMESTRETCH_[A-Z_]+) ([0-9.u]+)", text))
    assert consts == {"HOWL_TIMESTRETCH_MAX_CLIPS": "8192", "HOWL_TIMESTRETCH_MIN_SAMPLES": str(lib.TIMESTRETCH_MIN_SAMPLES),
                      "HOWL_TIMESTRETCH_MAX_SAMPLES": "1048576", "HOWL_TIMESTRETCH_MIN_RATE": "0.3", "HOWL_TIMESTRETCH_MAX_RATE": "1.7",
                      "HOWL_TIMESTRETCH_NO_COPY": f"{lib.TIMESTRETCH_NO_COPY}u"}, consts
    # the built library refuses like the emulator's (no launch happens: host pointers are enough)
    u.check_refusals(lib.Library(built), lib.HowlHipError)


# ---- the host side ------------------------------------------------------------------------------------------------------------------------

def _g18():
    return np.load(HERE / "golden" / "g18_timestretch.npz")


def _small_bank(lengths, seed=5):
    import torch
    rng = np.random.default_rng(seed)
    clips = [(0.2 * np.sin(2 * np.pi * (200.0 + 90.0 * k) * np.arange(L) / 16000.0) + 0.04 * rng.uniform(-1, 1, L)).astype(np.float32)
             for k, L in enumerate(lengths)]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    return clips, torch.from_numpy(np.concatenate(clips)).reshape(-1, 1), torch.tensor(lengths), [int(o) for o in offs[:-1]]


def test_collate_draws_are_the_references(emu):
    """DeviceCollate(timestretch=True) against G18: the reference's TimestretchTransform -> TimeshiftTransform -> NoiseTransform
    under set_random_seed(0) -- gates, rates, stretched lengths, the lengths behind Timeshift, the scaled label maps, and where
    `random` and `np.random` stand afterwards.  The 1500-sample clip keeps rate 1.0 here (it still consumes its draw)."""
    import emu_util
    from howl_amd.utils.random_utils import set_random_seed
    g = _g18()
    lengths = [int(v) for v in g["lengths"]]
    long_enough = np.asarray(lengths) >= 2048
    assert not long_enough.all() and long_enough.sum() == 4
    maps = [{float(k): int(v) for k, v in zip(ks, vs) if v >= 0} for ks, vs in zip(g["in_keys"], g["in_vals"])]
    with emu_util.emulated_package():
        from howl_amd.data.collate import DeviceCollate
        _, bank, blen, offs = _small_bank(lengths)
        set_random_seed(0)
        collate = DeviceCollate(bank, blen, None, max_len=max(lengths), row_offsets=offs, timestretch=True)
        for b in range(len(g["gate"])):
            lens, shift, head, sigma, sp = collate.draw(list(range(len(lengths))))
            assert (collate.last_rates is not None) == bool(g["gate"][b]), b
            rates = collate.last_rates if collate.last_rates is not None else [1.0] * len(lengths)
            assert np.array_equal(np.asarray(rates)[long_enough], g["rates"][b][long_enough]), (b, rates)
            assert all(r == 1.0 for r, ok in zip(rates, long_enough) if not ok)
            assert np.array_equal(np.asarray(lens)[long_enough], g["stretched"][b][long_enough])
            assert np.array_equal((np.asarray(lens) - np.asarray(shift))[long_enough], g["shifted"][b][long_enough])
            for k, m in enumerate(maps):
                if long_enough[k]:
                    scaled = collate._stretch.scale_labels(m, rates[k]) if g["gate"][b] else m
                    want = {float(t): int(v) for t, v in zip(g["map_keys"][b, k], g["map_vals"][b, k]) if v >= 0}
                    assert scaled == want, (b, k, scaled, want)
        assert random.random() == float(g["next_random"]) and np.random.random_sample() == float(g["next_np_random"])
    assert g["gate"].any() and not g["gate"].all()


def test_transform_defaults_and_private_streams():
    from howl_amd.data.transform.transform import TimestretchTransform
    p = TimestretchTransform().default_params[0]
    assert (list(p.domain), p.name, p.current_value_idx, p.prob) == ([0.1, 0.2, 0.3], "timestretch", 1, 0.8)
    assert TimestretchTransform.stretched_length(2500, 1.0) == 2500 and TimestretchTransform.stretched_length(5, 2.0) == 2     # half to even
    assert TimestretchTransform.num_steps(5000, 0.77) == len(np.arange(0, 10, 0.77))
    assert TimestretchTransform().eval().draw_rates([4000], rand=random.Random(1)) is None


def test_timestretch_false_draws_what_it_drew_before(emu):
    import emu_util
    with emu_util.emulated_package():
        from howl_amd.data.collate import DeviceCollate
        lengths = [4000, 2500, 3000]
        _, bank, blen, offs = _small_bank(lengths)
        a = DeviceCollate(bank, blen, None, max_len=4000, row_offsets=offs, seed=11)
        b = DeviceCollate(bank, blen, None, max_len=4000, row_offsets=offs, seed=11, timestretch=False)
        c = DeviceCollate(bank, blen, None, max_len=4000, row_offsets=offs, seed=11, timestretch=True)
        np_state = np.random.get_state()[1].copy()
        same = True
        for _ in range(8):
            da, db, dc = a.draw([0, 1, 2]), b.draw([0, 1, 2]), c.draw([0, 1, 2])
            assert da == db and b.last_rates is None
            same = same and da == dc
        assert a.rand.getstate() == b.rand.getstate() and not same
        assert np.array_equal(np.random.get_state()[1], np_state)        # a seeded collate leaves the global generators alone
        with pytest.raises(NotImplementedError, match="timestretch"):
            c([0, 1, 2])


def _probe_seed(make, ids, want_noise=False):
    """A seed whose first batch opens the Timestretch gate and (unless ``want_noise``) keeps both Noise gates shut, so that
    the batch's content is the stretched clip's, sample for sample."""
    for seed in range(400):
        c = make(seed)
        lens, shift, head, sigma, sp = c.draw(ids)
        if c.last_rates is not None and (want_noise or (not any(sigma) and not any(sp))):
            return seed, (lens, shift, head, list(c.last_rates))
    raise AssertionError("no seed found")


def test_frame_batch_windows_come_from_the_stretched_clip(emu):
    """frame_batch with timestretch=True: the batchifier sees the stretched lengths and the scaled word end times, and every
    window equals the float64 restatement of its clip's stretch at the planned offsets, to 8 x the float32-float64 gap."""
    import emu_util
    import timestretch_util as u
    with emu_util.emulated_package():
        from howl_amd.data.collate import DeviceCollate
        from howl_amd.data.transform.batchifier import DeviceClip, WakeWordFrameBatchifier
        lengths = [4000, 2500, 1200, 3000]
        clips, bank, blen, offs = _small_bank(lengths)
        ids = list(range(4))
        make = lambda s: DeviceCollate(bank, blen, None, max_len=4000, row_offsets=offs, seed=s, timestretch=True)
        seed, (lens, shift, head, rates) = _probe_seed(make, ids)
        assert rates[2] == 1.0 and all(0.3 <= r <= 1.7 and r != 1.0 for k, r in enumerate(rates) if k != 2)
        examples = [DeviceClip(0, 4000, {120.0: 1, 200.0: 2}, "a b"), DeviceClip(1, 2500, {90.0: 1}, "a"), DeviceClip(2, 1200, {}, ""),
                    DeviceClip(3, 3000, {150.0: 2}, "b")]
        batchifier = WakeWordFrameBatchifier(0, positive_sample_prob=1.0, window_size_ms=100, rand=random.Random(3))
        seen = {}
        real_plan = batchifier.plan

        def plan(cropped):
            seen["clips"], seen["plan"] = list(cropped), real_plan(cropped)
            return seen["plan"]
        batchifier.plan = plan
        collate = make(seed)
        batch = collate.frame_batch(examples, batchifier)
        pl = seen["plan"]
        assert [c.num_samples for c in seen["clips"]] == [l - w for l, w in zip(lens, shift)]
        assert lens == [int(round(L / r)) for L, r in zip(lengths, rates)]
        for ex, c, r in zip(examples, seen["clips"], rates):
            assert c.timestamp_label_map == {(1 / r) * k: v for k, v in ex.timestamp_label_map.items()}
        audio = batch.audio_data.numpy()
        assert audio.shape == (4, 1600) and batch.lengths.tolist() == pl.length and batch.labels.tolist() == pl.labels
        for row, (k, start, n, d0) in enumerate(zip(pl.source, pl.start, pl.length, pl.dst_off)):
            ref = u.stretch_f64(clips[k], rates[k]) if rates[k] != 1.0 else clips[k].astype(np.float64)
            gap = float(np.max(np.abs(u.stretch_f32_phasor(clips[k], rates[k]) - ref))) if rates[k] != 1.0 else 0.0
            first = (shift[k] if head[k] else 0) + start
            want = np.zeros(1600)
            want[d0:d0 + n] = ref[first:first + n]
            assert np.max(np.abs(audio[row] - want)) <= u.TOLERANCE_FACTOR * gap, (row, k, rates[k])
        assert sum(n >= 1000 for n in pl.length) >= 2 and any(rates[k] != 1.0 and n >= 1000 for k, n in zip(pl.source, pl.length))


def test_sequence_batch_carries_whole_stretched_clips(emu):
    import emu_util
    import timestretch_util as u
    with emu_util.emulated_package():
        from howl_amd.data.collate import DeviceCollate
        from howl_amd.data.transform.batchifier import DeviceClip
        lengths = [2600, 2048, 3000]
        clips, bank, blen, offs = _small_bank(lengths, seed=6)
        make = lambda s: DeviceCollate(bank, blen, None, max_len=3000, row_offsets=offs, seed=s, timestretch=True)
        seed, (lens, shift, head, rates) = _probe_seed(make, [0, 1, 2])

        class Batchifier:      # AudioSequenceBatchifier's interface: order by length, labels from the examples
            def order_and_labels(self, examples, out_len):
                import torch
                order = [int(k) for k in np.argsort(-np.asarray(out_len))]
                return order, torch.zeros(len(order), 1, dtype=torch.long), torch.ones(len(order), dtype=torch.long)
        batch = make(seed).sequence_batch([DeviceClip(k, L) for k, L in enumerate(lengths)], Batchifier())
        out_len = [l - w for l, w in zip(lens, shift)]
        order = [int(k) for k in np.argsort(-np.asarray(out_len))]
        assert batch.audio_lengths.tolist() == [out_len[k] for k in order] and batch.audio_data.shape == (3, max(out_len))
        for row, k in enumerate(order):
            ref = u.stretch_f64(clips[k], rates[k])
            gap = float(np.max(np.abs(u.stretch_f32_phasor(clips[k], rates[k]) - ref)))
            first = shift[k] if head[k] else 0
            got = batch.audio_data[row].numpy()
            assert np.max(np.abs(got[:out_len[k]] - ref[first:first + out_len[k]])) <= u.TOLERANCE_FACTOR * gap
            assert not got[out_len[k]:].any()


# ---- bounds: every operand in a guarded mapping, each placement in a child process ----------------------------------------------------------

BOUNDS_CASES = ("batch7", "identity", "mix")


def run_bounds(case, placement):
    """Child-process body: bank, records, background and output each end at (tail) or start behind (head) a PROT_NONE page;
    there is no workspace.  The output is sentinel-filled and every sample of it promised."""
    import emu_util
    import timestretch_util as u
    from guard_mem import Arena
    lib = emu_util.emu_lib()
    lib.cdll.hipemu_enable_fault_report()
    al = Arena(placement)
    real_call = lib.call

    def call(name, *args):       # the buffer map goes out before every launch: a fault address names its buffer
        print(f"guard_mem: --- {name} ({case}, {placement})", file=sys.stderr)
        al.describe()
        return real_call(name, *args)
    lib.call = call
    quiet = lambda *a: None
    {"batch7": lambda: u.check_batch7(al, lib, quiet), "identity": lambda: u.check_identity(al, lib, quiet),
     "mix": lambda: u.check_mix(al, lib)}[case]()
    al.check()


@pytest.fixture(scope="module")
def bounds_results(emu):
    from concurrent.futures import ThreadPoolExecutor
    env = dict(os.environ, OMP_NUM_THREADS="1")
    python = [sys.executable] + [flag for flag, on in (("-s", sys.flags.no_user_site), ("-E", sys.flags.ignore_environment)) if on]

    def one(job):
        try:
            p = subprocess.run(python + [__file__, *job], capture_output=True, text=True, timeout=TIMEOUT, env=env, cwd=ROOT)
            return job, p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:
            return job, "timeout", e.stdout or "", e.stderr or ""
    jobs = [(s, pl) for s in BOUNDS_CASES for pl in PLACEMENTS]
    with ThreadPoolExecutor(max_workers=6) as ex:
        return {job: r for job, *r in ex.map(one, jobs)}


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("case", BOUNDS_CASES)
def test_timestretch_bounds(bounds_results, case, placement):
    from test_emu_bounds import name_fault
    rc, out, err = bounds_results[(case, placement)]
    if rc != 0:
        tail = "\n".join([l for l in err.splitlines() if not l.startswith("guard_mem:")][-40:])
        maps = [l for l in err.splitlines() if l.startswith("guard_mem:")]
        pytest.fail(f"{case} [{placement}] exited {rc}\n{name_fault(err)}\n{tail}\n--- last buffer map ---\n" + "\n".join(maps[-40:]),
                    pytrace=False)


if __name__ == "__main__":
    run_bounds(sys.argv[1], sys.argv[2])
    print(json.dumps({"case": sys.argv[1], "placement": sys.argv[2], "ok": True}))
