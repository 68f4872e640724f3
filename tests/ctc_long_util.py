"""Shared cases and checks for the long-target CTC tests (tests/test_emu_ctc_long.py on the emulator, tests/test_gpu_ctc_long.py
on the device).  The reference is ctc_util.reference -- torch's CPU log_softmax + ctc_loss + autograd -- in fp32 and in fp64; the
bounds are those of the whole-clip tests: |loss - loss64| < 2e-5 max(1, |loss64|), max|grad - grad64| < 1.5 noise + 1e-5 with
noise = torch-fp32's own distance from its fp64 run on the same case."""
import ctypes
import functools

import numpy as np
import torch

from ctc_util import make_case, reference

LOSS_RTOL, GRAD_NOISE_FACTOR, GRAD_ATOL = 2e-5, 1.5, 1e-5

# (T, B, C, Lmax, seed, structured): the ten parity cases.  The first is make_case as it comes, at a seed whose longest target
# has the 32 labels and whose losses are finite; the last gets its input lengths from the window (see case())
CASES = {
    "first-beyond-31": (40, 3, 5, 32, 39, False),
    "k2-32": (96, 4, 6, 32, 1, True),
    "k2-63": (160, 4, 5, 63, 2, True),
    "k4-64": (200, 4, 5, 64, 3, True),
    "k4-127": (300, 4, 12, 127, 4, True),
    "k8-128": (300, 4, 12, 128, 5, True),
    "k8-255-c64": (600, 4, 64, 255, 6, True),
    "k8-255": (1100, 3, 5, 255, 7, True),
    "k8-255-c2": (520, 3, 2, 255, 8, True),
    "k8-255-edges": (1100, 3, 5, 255, 9, True),
}
EMU_CASES = ("first-beyond-31", "k2-32", "k2-63", "k4-64", "k8-128", "k8-255-c2")


def states_per_lane(max_target):
    return 1 if max_target <= 31 else 2 if max_target <= 63 else 4 if max_target <= 127 else 8


def window_rows(max_target):
    """``howl_ctc_long_window_rows`` as the header states it."""
    return {1: 128, 2: 64, 4: 32, 8: 32}[states_per_lane(max_target)]


def structured_case(T, B, C, Lmax, seed, structured=True):
    """ctc_util.make_case with row 0 = Lmax times one label over all T frames (no skip transition anywhere, across every lane
    boundary; needs T >= 2 Lmax - 1), row 1 = Lmax labels alternating between two (one label when C == 2) with an input long
    enough for its alignment (a skip transition everywhere), the last row an empty target; the rows in between stay random."""
    logits, targets, in_len, tgt_len, blank = make_case(T, B, C, Lmax, seed)
    if not structured:
        return logits, targets, in_len, tgt_len, blank
    labels = [c for c in range(C) if c != blank]
    assert T >= 2 * Lmax - 1 and B >= 3
    targets[0, :Lmax] = labels[0]
    tgt_len[0], in_len[0] = Lmax, T
    row = torch.tensor([labels[i % 2] if len(labels) > 1 else labels[0] for i in range(Lmax)])
    targets[1, :Lmax] = row
    tgt_len[1] = Lmax
    need = Lmax + int((row[1:] == row[:-1]).sum())
    in_len[1] = max(int(in_len[1]), need)
    tgt_len[B - 1] = 0
    return logits, targets, in_len, tgt_len, blank


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits, targets, in_len, tgt_len, blank, loss64, grad64, noise): built once, shared, never written to."""
    T, B, C, Lmax, seed, structured = CASES[name]
    logits, targets, in_len, tgt_len, blank = structured_case(T, B, C, Lmax, seed, structured)
    if name == "k8-255-edges":
        w = window_rows(Lmax)
        in_len[1], in_len[2] = 16 * w + 1, 16 * w          # row 0 keeps T: 1100 = 34 w + 12
    return (logits, targets, in_len, tgt_len, blank) + reference_pair(logits, targets, in_len, tgt_len, blank)


def reference_pair(logits, targets, in_len, tgt_len, blank):
    _, _, grad32 = reference(logits, targets, in_len, tgt_len, blank)
    per64, loss64, grad64 = reference(logits.double(), targets, in_len, tgt_len, blank)
    assert bool(torch.isfinite(per64).all())
    return float(loss64), grad64, float((grad32.double() - grad64).abs().max())


def check_parity(name, loss, grad_btc, in_len, loss64, grad64, noise, report=None):
    """The bounds of the module docstring; prints err / noise before it asserts."""
    err = float((grad_btc.double() - grad64).abs().max())
    dl = abs(float(loss) - loss64)
    line = (f"ctc_long parity {name}: |loss-loss64|={dl:.3e} (bound {LOSS_RTOL * max(1.0, abs(loss64)):.3e}) "
            f"grad err={err:.3e} noise={noise:.3e} err/noise={err / max(noise, 1e-30):.3f} (bound 1.5 + 1e-5/noise)")
    print(line, flush=True)
    if report is not None:
        report.append(line)
    assert dl < LOSS_RTOL * max(1.0, abs(loss64)), line
    assert err < GRAD_NOISE_FACTOR * noise + GRAD_ATOL, line
    for b in range(grad_btc.shape[0]):
        assert not bool(grad_btc[b, int(in_len[b]):].any()), f"{name}: rows past the input length of utterance {b} are not zero"


def short_cases():
    """test_fused_ctc-style cases inside howl_ctc_loss's range for the instantiation-independence check."""
    return [(640, 4, 64, 31, 21), (300, 16, 5, 3, 22), (100, 3, 7, 12, 23)]


class Plain:
    """The allocator interface of guard_mem.Arena / Banded on plain numpy arrays (no guards): for the tests that compare values."""

    def buf(self, name, shape, dtype=np.float32, fill=0.0, placement=None, promised=None):
        a = np.empty(shape, dtype)
        if isinstance(fill, str):
            a[...] = np.nan if a.dtype.kind == "f" else 0
        else:
            a[...] = np.asarray(fill).reshape(a.shape) if isinstance(fill, np.ndarray) else fill
        return a

    @staticmethod
    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    @staticmethod
    def get(a):
        return a

    def sync(self):
        pass

    def check(self):
        pass


def call(al, lib, entry, z, tg, il, tl, blank, max_target=None, tgt_stride=None, want_grad=True, want_loss=True, tag="",
         ws_floats=None):
    """One call of ``howl_ctc_loss`` / ``howl_ctc_loss_long`` on buffers of the allocator ``al`` (Plain, guard_mem.Arena on the
    emulator, guard_mem.Banded on the device).  z: (B, T, C) numpy logits, addressed as (T, B, C); the targets go into a (B,
    tgt_stride) matrix, tgt_stride = max_target_length unless given, so its last row ends the buffer; the workspace is exactly
    the size function's; outputs are sentinel-filled and promised in full.  Returns (nll, loss, dlogits (B, T, C))."""
    z, tg, il, tl = (np.asarray(a.numpy() if isinstance(a, torch.Tensor) else a) for a in (z, tg, il, tl))
    B, T, C = z.shape
    max_target = int(tl.max()) if max_target is None else max_target
    stride = max(max_target, 1) if tgt_stride is None else tgt_stride
    rows = np.zeros((B, stride), np.int64)
    n = min(stride, tg.shape[1])
    rows[:, :n] = tg[:, :n]
    zb = al.buf("logits" + tag, (B, T, C), np.float32, np.ascontiguousarray(z))
    tb = al.buf("targets" + tag, (B, stride), np.int64, rows)
    ilb = al.buf("in_len" + tag, B, np.int64, np.ascontiguousarray(il))
    tlb = al.buf("tgt_len" + tag, B, np.int64, np.ascontiguousarray(tl))
    nll = al.buf("nll" + tag, B, np.float32, "sentinel", promised="all")
    loss = al.buf("loss" + tag, 1, np.float32, "sentinel", promised="all") if want_loss else None
    dz = al.buf("dlogits" + tag, (B, T, C), np.float32, "sentinel", promised="all") if want_grad else None
    if ws_floats is None:
        if not want_grad:
            ws_floats = 0
        elif entry == "howl_ctc_loss":
            ws_floats = int(lib.cdll.howl_ctc_workspace_floats(T, B))
        else:
            ws_floats = int(lib.cdll.howl_ctc_long_workspace_floats(T, B, max_target))
    ws = al.buf("workspace" + tag, ws_floats, np.float32, "sentinel") if ws_floats else None
    lib.call(entry, al.ptr(zb), C, T * C, T, B, C, al.ptr(tb), stride, max_target, al.ptr(ilb), al.ptr(tlb), blank, al.ptr(nll),
             al.ptr(loss), al.ptr(dz), C, T * C, al.ptr(ws), ws_floats, stream_of(al))
    al.sync()
    return (al.get(nll).copy(), float(al.get(loss)[0]) if want_loss else None, None if dz is None else al.get(dz).copy())


def stream_of(al):
    """The device allocator launches on torch's current stream; host allocators (the emulator) pass a null stream."""
    if hasattr(al, "torch"):
        return ctypes.c_void_p(al.torch.cuda.current_stream().cuda_stream)
    return None


def emu_run(lib, entry, logits_btc, targets, in_len, tgt_len, blank, **kw):
    return call(Plain(), lib, entry, logits_btc, targets, in_len, tgt_len, blank, **kw)


# ---- checks shared by the emulator and the device tests ----------------------------------------------------------------------------

def check_independence(al, lib, T, B, C, Lmax, seed):
    """A batch inside howl_ctc_loss's range, its target matrix at row stride 255: howl_ctc_loss, howl_ctc_loss_long at the true
    maximum and declared at 40, 100 and 255 labels (K = 2, 4, 8) give the same nll, loss and dlogits bits."""
    logits, targets, in_len, tgt_len, blank = make_case(T, B, C, Lmax, seed)
    true_max = int(tgt_len.max())
    base = call(al, lib, "howl_ctc_loss", logits, targets, in_len, tgt_len, blank, max_target=true_max, tgt_stride=255, tag=".short")
    assert np.isfinite(base[2]).all()
    for declared in (true_max, 40, 100, 255):
        got = call(al, lib, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank, max_target=declared, tgt_stride=255,
                   tag=f".long{declared}")
        assert np.array_equal(got[0], base[0]), f"nll differs at declared max_target_length {declared}"
        assert got[1] == base[1], f"loss differs at declared max_target_length {declared}"
        assert np.array_equal(got[2], base[2]), f"dlogits differ at declared max_target_length {declared}"
    al.check()


def contract_case():
    T, B, C, Lmax, seed, _ = CASES["k8-255-c64"]
    return structured_case(T, B, C, Lmax, seed)


def check_contract(al, lib, kind):
    """(600, 4, 64, 255): one utterance outside the contract gets nll = +inf and all-zero gradient rows; the others keep the
    bits of the run with it valid.  label: label C at position 200 of utterance 0; length: target length 256 above
    max_target_length 255 (utterance 1); input: input length -1 (utterance 2)."""
    logits, targets, in_len, tgt_len, blank = contract_case()
    B, T, C = logits.shape
    tg, il, tl = targets.numpy().copy(), in_len.numpy().copy(), tgt_len.numpy().copy()
    nll0, _, dz0 = call(al, lib, "howl_ctc_loss_long", logits, tg, il, tl, blank, max_target=255, tag=".valid")
    assert np.isfinite(nll0).all()
    if kind == "label":
        b = 0
        tg[b, 200] = C
    elif kind == "length":
        b = 1
        tl[b] = 256
    else:
        b = 2
        il[b] = -1
    nll1, loss1, dz1 = call(al, lib, "howl_ctc_loss_long", logits, tg, il, tl, blank, max_target=255, tag=".spoilt")
    assert nll1[b] == np.inf and loss1 == np.inf
    assert not dz1[b].any()
    others = [i for i in range(B) if i != b]
    assert np.array_equal(nll1[others], nll0[others])
    assert np.array_equal(dz1[others], dz0[others])
    al.check()


def check_cabi_refusals(lib):
    """Out of range (256 labels, C = 70, T = 8193), overlapping target rows, null pointers, a bad shape and a workspace that is
    too small are refused with text that names the entry point; the next valid call succeeds."""
    from howl_amd.lib import HowlHipError
    import pytest
    logits, targets, in_len, tgt_len, blank = make_case(12, 2, 5, 3, 0)
    al = Plain()
    good = call(al, lib, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank)
    for T, C, M in ((12, 5, 256), (12, 70, 3), (8193, 5, 3)):
        assert lib.cdll.howl_ctc_long_supported(T, C, M) == 0
        z = np.zeros((2, 12, 5), np.float32)        # refused before anything is addressed
        with pytest.raises(HowlHipError, match=r"howl_ctc_loss_long: .*range \(T <= 8192, C <= 64, targets <= 255\)"):
            lib.call("howl_ctc_loss_long", Plain.ptr(z), C, T * C, T, 2, C, Plain.ptr(np.zeros((2, 256), np.int64)), 256, M,
                     Plain.ptr(in_len.numpy()), Plain.ptr(tgt_len.numpy()), 4, Plain.ptr(np.zeros(2, np.float32)), None, None, 0, 0,
                     None, 0, None)
    assert lib.cdll.howl_ctc_long_supported(8192, 64, 255) == 1 and lib.cdll.howl_ctc_long_supported(1, 1, 0) == 1
    with pytest.raises(HowlHipError, match="howl_ctc_loss_long: target rows of stride 3 overlap"):
        call(al, lib, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank, max_target=40, tgt_stride=3)
    with pytest.raises(HowlHipError, match="howl_ctc_loss_long: null pointer"):
        lib.call("howl_ctc_loss_long", None, 5, 60, 12, 2, 5, None, 3, 3, None, None, 4, None, None, None, 0, 0, None, 0, None)
    with pytest.raises(HowlHipError, match="howl_ctc_loss_long: bad shape"):
        call(al, lib, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, 5)
    lg, tg, il, tl, bl = make_case(70, 2, 5, 3, 0)       # 70 frames: one window up to 63 labels, three windows of 32 beyond
    need = int(lib.cdll.howl_ctc_long_workspace_floats(70, 2, 100))
    assert need == 2 * 70 * 64 * 4
    with pytest.raises(HowlHipError, match=rf"howl_ctc_loss_long: .*workspace of .* = {need} floats \(got {need - 1}\)"):
        call(al, lib, "howl_ctc_loss_long", lg, tg, il, tl, bl, max_target=100, tgt_stride=100, ws_floats=need - 1)
    again = call(al, lib, "howl_ctc_loss_long", logits, targets, in_len, tgt_len, blank)
    assert np.array_equal(again[0], good[0]) and again[1] == good[1] and np.array_equal(again[2], good[2])


def check_size_functions(lib):
    for M, k, w in ((0, 1, 128), (31, 1, 128), (32, 2, 64), (63, 2, 64), (64, 4, 32), (127, 4, 32), (128, 8, 32), (255, 8, 32)):
        assert states_per_lane(M) == k and window_rows(M) == w
        assert lib.cdll.howl_ctc_long_window_rows(M) == w
        assert lib.cdll.howl_ctc_long_workspace_floats(w, 3, M) == 0
        assert lib.cdll.howl_ctc_long_workspace_floats(w + 1, 3, M) == 3 * (w + 1) * 64 * k
    assert lib.cdll.howl_ctc_long_window_rows(256) == 0 and lib.cdll.howl_ctc_long_window_rows(-1) == 0
    assert lib.cdll.howl_ctc_long_workspace_floats(8192, 2, 31) == lib.cdll.howl_ctc_workspace_floats(8192, 2)


def window_edge_case(M, seed):
    """One batch around the window w of the body that serves M labels: utterances of 2w + 1, 2w, w + 1, w and fewer than w
    frames, two random ones, and in front the one that holds the M labels (alternating, so M frames align it).  B = 8: the
    batch's 1 / B is a power of two."""
    w = window_rows(M)
    C, blank = 6, 5
    T = max(2 * w + 1, M + 8)
    rng = np.random.default_rng(seed)
    lens = [T, 2 * w + 1, 2 * w, w + 1, w, max(2, w // 2 - 3), int(rng.integers(w, 2 * w)), int(rng.integers(2, w))]
    lens = [lens[0]] + sorted(lens[1:], reverse=True)
    B = len(lens)
    logits = torch.from_numpy(rng.normal(0, 2.0, (B, T, C)).astype(np.float32))
    tgt_len = [M] + [int(min(M, rng.integers(1, n // 2 + 1))) for n in lens[1:]]
    targets = np.zeros((B, M), np.int64)
    targets[0] = np.arange(M) % 2
    for b in range(1, B):
        targets[b, :tgt_len[b]] = rng.integers(0, C - 1, tgt_len[b])
    short = lens.index(max(2, w // 2 - 3))
    return logits, torch.from_numpy(targets), torch.tensor(lens), torch.tensor(tgt_len), blank, w, short


def check_window_edges(runner, M, report=None):
    """runner(logits (B, T, C), targets, in_len, tgt_len, blank) -> (loss, grad (B, T, C) cpu tensor)."""
    logits, targets, in_len, tgt_len, blank, w, short = window_edge_case(M, 100 + M)
    B = logits.shape[0]
    loss, grad = runner(logits, targets, in_len, tgt_len, blank)
    check_parity(f"window-edges-{M}", loss, grad, in_len, *reference_pair(logits, targets, in_len, tgt_len, blank), report=report)
    sl = slice(short, short + 1)
    _, alone = runner(logits[sl, :w].contiguous(), targets[sl], in_len[sl], tgt_len[sl], blank)
    assert torch.equal(alone[0] * (1.0 / B), grad[short, :w]), "the short utterance's gradient bits depend on the batch around it"
