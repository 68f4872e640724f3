"""Layer-local float64 reference of the MobileNetClassifier kernels (howl_amd/csrc/mobilenet.hip).

After a training-mode ``howl_mobilenet_fwd`` + ``howl_mobilenet_bwd`` the workspace still holds, for every layer k, the
convolution output z_k, ss_k = [scale | shift | mean | rstd], the stored y_k of the linear bottlenecks, the masked incoming
gradient g_k and bc_k = [scale | c1 | c0] (``howl_mobilenet_workspace_layer`` says where).  Every quantity a kernel produced is
recomputed here in float64 FROM THE KERNEL'S OWN INPUTS TO THAT STEP (teacher forcing), so errors do not compound, a flipped
ReLU6 decision does not propagate, and the allowed error is a few float32 roundings:

  F1 z_k            convolution of the rebuilt input              element-wise, a-priori dot-product bound
  F2 ss_k, buffers  batch statistics of the kernel's z_k          long reduction: yardstick from a float32 reference
  F3 stored y_k     bn(z_k) (+ residual source)                   closed form
  F4 head           pooled, pooled_d, logits                      short sums
  B1 g_last         from dlogits through classifier / dropout / average pool / ReLU6 mask
  B2 g_{k-1}        transposed convolution of dz_k (+ residual gradient), times the activation mask of layer k-1
  B3 bc_k, dgamma_k, dbeta_k   from g_k, z_k, ss_k                 long reduction
  B4 dW_k (+ conv bias, classifier)   correlation of dz_k with the rebuilt input of layer k
  B5 every float of the gradient buffer is covered by exactly one of B3 / B4

Tolerances (u = 2^-24); none of them comes from what the kernels give:
  * short sums of known length K (F1, B2, F4 logits, classifier gradients): the a-priori bound of a length-K float32 dot product
    in ANY order, (K + 2) u sum|a_i||b_i|, plus the rounding of the operand's on-load transform carried through sum|w| dx
    (one fmaf: u (|z scale| + |shift|); dz, two fmaf: u (|scale g| + 2 |c1 z| + 2 |c0|)), times 2;
  * long reductions over pixels (F2, B3, B4): the same quantity from the same inputs in float32 torch gives the yardstick e32
    (its error against float64, in units of u sum|terms|, worst channel of the layer); the kernel may be off by
    max(8 e32, 16 u sum|terms| / sqrt(n)) -- for the variance max(8 e32, 16 u E[z^2]); what is DERIVED from such a sum (rstd,
    scale, shift, c1, c0, running buffers) gets the sum's allowance propagated exactly (an interval for rstd) plus one float32
    rounding per stored value;
  * closed forms of a few operations (F3, pooled_d, dz of features[0], eval-mode ss): 8 u (sum of |terms|).
Activation masks: the kernel decides by ONE float32 fmaf(z, scale, shift), which float64 cannot reproduce when the value is
within d = 4 u (|z scale| + |shift|) of 0 or 6 ("undecided").  There the kernel's value must match EITHER the masked or the
unmasked reference within the bound; nothing is skipped, and more than 1e-4 undecided elements in a layer fail the case.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from howl_amd.lib import HowlMbLayer, HowlMbWsLayer
from oracle import mobilenet as om

U = 2.0 ** -24
TINY = 1e-300
DENSE, PW, DW = 0, 1, 2
ACT_NONE, ACT_RELU6, ACT_RELU = 0, 1, 2
KIND = {DENSE: "dense3x3", PW: "pointwise", DW: "depthwise"}
MAX_UNDECIDED = 1e-4
PLAN_FIELDS = ("f_tile", "f_cx", "f_ry", "d_tile", "d_ry", "d_chunks", "nslab")


# ---- memory: the same driver runs on host memory (emulator) and on device buffers ------------------------------------------
class HostMem:
    def put(self, a):
        return np.ascontiguousarray(a)

    def ptr(self, h):
        return None if h is None else ctypes.c_void_p(h.ctypes.data)

    def get(self, h):
        return h


class DevMem:
    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def ptr(self, h):
        return None if h is None else ctypes.c_void_p(h.data_ptr())

    def get(self, h):
        torch.cuda.synchronize()
        return h.cpu().numpy()


# ---- the plan, as the library publishes it ---------------------------------------------------------------------------------
def layer_table(lib):
    out = []
    for i in range(lib.cdll.howl_mobilenet_num_layers()):
        d = HowlMbLayer()
        lib.call("howl_mobilenet_layer", i, ctypes.byref(d))
        out.append(d)
    return out


def workspace_map(lib, B, M, T, C):
    """One HowlMbWsLayer per layer + the tail entry (index num_layers)."""
    out = []
    for i in range(lib.cdll.howl_mobilenet_num_layers() + 1):
        d = HowlMbWsLayer()
        lib.call("howl_mobilenet_workspace_layer", B, M, T, C, i, ctypes.byref(d))
        out.append(d)
    return out


def layer_key(d):
    if d.feat < 0:
        return "downsample.0"
    if d.sub < 0:
        return f"model.features.{d.feat}.0"
    return f"model.features.{d.feat}.conv.{d.sub}.0" if d.wrapped else f"model.features.{d.feat}.conv.{d.sub}"


def plan_text(w):
    return " ".join(f"{n}={getattr(w, n)}" for n in PLAN_FIELDS)


def coverage(tab, wsl):
    """The kernel instances one problem exercises, from the published plan fields alone."""
    seen = set()
    for k, (l, w) in enumerate(zip(tab, wsl)):
        kind = KIND[l.kind]
        if w.nslab > 1:
            seen.add(f"nslab>1 {kind}")
        if max(w.f_ry, w.d_ry, w.d_chunks) > w.group_rows:
            seen.add("two-level arrival")
        if l.kind == PW:
            seen.add(f"pw_fwd tile {w.f_tile} {'materialised' if w.f_yout >= 0 else 'on-load'} producer")
            seen.add(f"pw_dgrad tile {w.d_tile} {'with' if w.b_ss >= 0 else 'without'} ss_in")
        elif l.kind == DW:
            seen.add(f"dw stride {l.stride} wo%4 {'==' if w.wo % 4 == 0 else '!='} 0")
            if l.cout <= 32:
                seen.add("dw C<=32")
    return seen


REQUIRED = ({f"pw_fwd tile {t} {p} producer" for t in (32, 64) for p in ("materialised", "on-load")} |
            {f"pw_dgrad tile {t} {s} ss_in" for t in (32, 64) for s in ("with", "without")} |
            {f"dw stride {s} wo%4 {e} 0" for s in (1, 2) for e in ("==", "!=")} |
            {"dw C<=32"} | {f"nslab>1 {k}" for k in KIND.values()})


# ---- run the kernels ---------------------------------------------------------------------------------------------------------
def make_inputs(B, M, T, C, dropout, layout, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, M, T, generator=gen) * 1.5).numpy()
    keep = (torch.rand(B, om.LAST_CHANNEL, generator=gen) >= 0.2).float().numpy() if dropout else None
    if layout == "bmt":                       # channel 0 of (B, 3, M, T) features
        buf = np.full((B, 3, M, T), np.nan, np.float32)
        buf[:, 0] = x
        strides = (3 * M * T, T, 1)
    else:                                     # (B, T, M) frames-major, with slack between utterances
        assert layout == "btm"
        buf = np.full((B, T + 3, M), np.nan, np.float32)
        buf[:, :T] = x.transpose(0, 2, 1)
        strides = ((T + 3) * M, 1, M)
    return x, keep, buf, strides


def run_kernels(lib, mem, B, M, T, C, dropout=False, layout="bmt", seed=0, eval_too=False):
    """Training-mode forward + backward (dlogits = d mean cross-entropy / d logits at the kernel's own logits) through the C ABI;
    returns host copies of everything the checks read."""
    tab, wsl = layer_table(lib), workspace_map(lib, B, M, T, C)
    sd = om.mobilenet_init(C)
    params = np.concatenate([sd[n].numpy().reshape(-1) for n in om.mobilenet_param_names()]).astype(np.float32)
    assert params.size == lib.cdll.howl_mobilenet_param_floats(C)
    gen = torch.Generator().manual_seed(seed + 1)   # non-trivial running statistics: the momentum update is visible in both terms
    nbuf = lib.cdll.howl_mobilenet_buffer_floats()
    bufs0 = np.empty(nbuf, np.float32)
    for l in tab:
        bufs0[l.rmean_off:l.rmean_off + l.cout] = 0.3 * torch.randn(l.cout, generator=gen).numpy()
        bufs0[l.rvar_off:l.rvar_off + l.cout] = 0.5 + torch.rand(l.cout, generator=gen).numpy()
    x, keep, xbuf, (sb, sm, st) = make_inputs(B, M, T, C, dropout, layout, seed)
    scale = 1.0 / (1.0 - om.DROPOUT_P) if dropout else 1.0
    nbytes = lib.cdll.howl_mobilenet_workspace_bytes(B, M, T, C)
    assert nbytes >= 4 * wsl[-1].total_floats > 0
    d_params, d_bufs, d_x = mem.put(params), mem.put(bufs0.copy()), mem.put(xbuf)
    d_mask = None if keep is None else mem.put(keep)
    d_ws = mem.put(np.zeros(nbytes, np.uint8))
    d_logits = mem.put(np.full((B, C), np.nan, np.float32))
    p = mem.ptr
    lib.call("howl_mobilenet_fwd", p(d_params), p(d_bufs), C, p(d_x), sb, sm, st, B, M, T, 1, p(d_mask), scale, p(d_logits), p(d_ws),
             nbytes, None)
    logits = np.array(mem.get(d_logits))
    assert np.isfinite(logits).all()
    prob = torch.softmax(torch.from_numpy(logits).double(), 1)
    prob[torch.arange(B), torch.arange(B) % C] -= 1
    dlogits = (prob / B).float().numpy()
    d_dl = mem.put(dlogits)
    d_g = mem.put(np.full(params.size, np.nan, np.float32))
    lib.call("howl_mobilenet_bwd", p(d_params), C, p(d_x), sb, sm, st, B, M, T, p(d_mask), scale, p(d_dl), p(d_g), p(d_ws), nbytes,
             None)
    cap = dict(tab=tab, wsl=wsl, B=B, M=M, T=T, C=C, params=params, bufs0=bufs0, bufs1=np.array(mem.get(d_bufs)), x=x, keep=keep,
               scale=scale, logits=logits, dlogits=dlogits, grads=np.array(mem.get(d_g)),
               ws=np.array(mem.get(d_ws)).view(np.float32))
    if eval_too:      # eval mode on the updated running statistics: ss comes from bn_eval_ss_kernel, nothing else may move
        lib.call("howl_mobilenet_fwd", p(d_params), p(d_bufs), C, p(d_x), sb, sm, st, B, M, T, 0, None, 1.0, p(d_logits), p(d_ws),
                 nbytes, None)
        cap["eval"] = dict(cap, logits=np.array(mem.get(d_logits)), ws=np.array(mem.get(d_ws)).view(np.float32),
                           bufs_after=np.array(mem.get(d_bufs)), keep=None, scale=1.0)
    return cap


# ---- float64 (or float32) convolutions by taps: one code path for the value, its magnitude and the float32 yardstick ------------
def _taps(X, l, ho, wo):
    Xp = F.pad(X, (l.pad_w, l.pad_w, l.pad_h, l.pad_h))
    s = l.stride
    for kh in range(3):
        for kw in range(3):
            yield kh, kw, Xp[:, :, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s]


def conv_fwd(X, W, l, ho, wo):
    if l.kind == PW:
        return torch.einsum("bihw,oi->bohw", X, W[:, :, 0, 0])
    out = 0
    for kh, kw, Xs in _taps(X, l, ho, wo):
        out = out + (Xs * W[:, 0, kh, kw].view(1, -1, 1, 1) if l.kind == DW else torch.einsum("bihw,oi->bohw", Xs, W[:, :, kh, kw]))
    return out


def conv_dgrad(dz, W, l, hin, win):
    if l.kind == PW:
        return torch.einsum("bohw,oi->bihw", dz, W[:, :, 0, 0])
    B, _, ho, wo = dz.shape
    s = l.stride
    gp = torch.zeros(B, l.cin, hin + 2 * l.pad_h, win + 2 * l.pad_w, dtype=dz.dtype)
    for kh in range(3):
        for kw in range(3):
            view = gp[:, :, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s]
            view += dz * W[:, 0, kh, kw].view(1, -1, 1, 1) if l.kind == DW else torch.einsum("bohw,oi->bihw", dz, W[:, :, kh, kw])
    return gp[:, :, l.pad_h:l.pad_h + hin, l.pad_w:l.pad_w + win]


def conv_wgrad(dz, X, l):
    if l.kind == PW:
        return torch.einsum("bohw,bihw->oi", dz, X)[:, :, None, None]
    ho, wo = dz.shape[2:]
    out = torch.zeros(l.cout, 1 if l.kind == DW else l.cin, 3, 3, dtype=dz.dtype)
    for kh, kw, Xs in _taps(X, l, ho, wo):
        if l.kind == DW:
            out[:, 0, kh, kw] = (dz * Xs).sum((0, 2, 3))
        else:
            out[:, :, kh, kw] = torch.einsum("bohw,bihw->oi", dz, Xs)
    return out


def _act(v, act):
    return torch.clamp(v, 0.0, 6.0) if act == ACT_RELU6 else (torch.clamp(v, min=0.0) if act == ACT_RELU else v)


def _pool2(v):      # MaxPool2d((1, 2)): an odd last column is dropped
    wp = v.shape[3] // 2
    return v[..., :2 * wp].reshape(*v.shape[:3], wp, 2).amax(-1)


def _c(v):
    return v.view(1, -1, 1, 1)


class Failure(AssertionError):
    pass


class Check:
    """All comparisons of one capture.  ``ratios[class]`` is the worst |kernel - float64| / allowed seen, ``ref_units[class]`` the worst
    float32-reference error of the long reductions (units of u sum|terms|), ``undecided[k]`` the undecided mask elements of layer k."""

    def __init__(self, cap):
        self.__dict__.update(cap)
        self.nl = len(self.tab)
        self.ratios, self.ref_units, self.undecided, self.fails = {}, {}, {}, []
        self.cover = np.zeros(self.grads.size, np.int32)
        self.feature_params = self.params.size - self.C * om.LAST_CHANNEL - self.C

    # -- views ------------------------------------------------------------------------------------------------------------------
    def t32(self, off, B, H, W, C):
        return torch.from_numpy(self.ws[off:off + B * H * W * C].reshape(B, H, W, C)).permute(0, 3, 1, 2)

    def z32(self, k):
        l, w = self.tab[k], self.wsl[k]
        return self.t32(w.z, self.B, w.ho, w.wo, l.cout)

    def g32(self, k):
        l, w = self.tab[k], self.wsl[k]
        return self.t32(w.g, self.B, w.ho, w.wo, l.cout)

    def y32(self, k):
        l, w = self.tab[k], self.wsl[k]
        return self.t32(w.y, self.B, w.hy, w.wy, l.cout)

    def rows(self, off, n, C):
        return torch.from_numpy(self.ws[off:off + n * C].reshape(n, C).copy())

    def weight(self, k, src=None):
        l = self.tab[k]
        shape = (l.cout, l.cin, 3, 3) if l.kind == DENSE else ((l.cout, 1, 3, 3) if l.kind == DW else (l.cout, l.cin, 1, 1))
        src = self.params if src is None else src
        return torch.from_numpy(src[l.w_off:l.w_off + int(np.prod(shape))].reshape(shape))

    def vec(self, off, n, src=None):
        src = self.params if src is None else src
        return torch.from_numpy(src[off:off + n])

    def where(self, k):
        l, w = self.tab[k], self.wsl[k]
        return f"layer {k} {layer_key(l)} ({KIND[l.kind]} {l.cin}->{l.cout} stride {l.stride}; {plan_text(w)})"

    # -- comparison ---------------------------------------------------------------------------------------------------------------
    def cmp(self, cls, where, got, ref, bound, alt=None, und=None, layout="bchw"):
        got, ref, bound = got.double(), ref.double(), bound.double()
        err = (got - ref).abs()
        bad = ~(err <= bound)           # (NaN is bad)
        ratio = err / (bound + TINY)
        if und is not None:
            other = ~((got - alt.double()).abs() <= bound)
            take = und & bad & ~other   # undecided elements that match the other reference
            bad = bad & ~take
            ratio = torch.where(take, (got - alt.double()).abs() / (bound + TINY), ratio)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        worst = ratio.max().item() if ratio.numel() else 0.0
        self.ratios[cls] = max(self.ratios.get(cls, 0.0), worst)
        if bad.any():
            idx = tuple(int(i) for i in np.unravel_index(int(torch.where(bad, ratio, torch.full_like(ratio, -1.0)).argmax()),
                                                         tuple(got.shape)))
            at = f"[{layout}]={idx}"
            if layout == "bchw" and len(idx) == 4:
                at = f"(b,h,w,c)=({idx[0]},{idx[2]},{idx[3]},{idx[1]})"
            self.fails.append(f"{cls} {where}: {int(bad.sum())} of {bad.numel()} off; worst at {at}: kernel {got[idx].item():.9g} "
                              f"float64 {ref[idx].item():.9g} error {err[idx].item():.3g} allowed {bound[idx].item():.3g}")

    def long_tol(self, cls, v64, v32, mag, n, var_floor=False):
        """Allowance of a long reduction over n terms: v32 is the float32 reference of v64, mag = sum|terms| (per output)."""
        units = ((v32.double() - v64).abs() / (U * mag + TINY)).max().item()
        self.ref_units[cls] = max(self.ref_units.get(cls, 0.0), units)
        floor = 16.0 * U * mag * (1.0 if var_floor else 1.0 / math.sqrt(n))
        return torch.maximum(8.0 * units * U * mag, floor)

    # -- rebuilt operands -----------------------------------------------------------------------------------------------------------
    def ss(self, k):
        return self.rows(self.wsl[k].ss, 4, self.tab[k].cout).double()

    def preact(self, k):
        """Float64 pre-activation z_k scale + shift from the kernel's ss_k, and the rounding of the kernel's one fmaf."""
        ss, Z = self.ss(k), self.z32(k).double()
        pre = Z * _c(ss[0]) + _c(ss[1])
        return pre, U * ((Z * _c(ss[0])).abs() + _c(ss[1]).abs())

    def layer_input(self, k):
        """The input of layer k as its kernels rebuild it (float64) and the rounding that rebuild carries."""
        if k == 0:
            X = torch.from_numpy(self.x).double()[:, None]
            return X, torch.zeros_like(X)
        lp = self.tab[k - 1]
        if lp.act == ACT_NONE:      # a stored y: the exact operand
            X = self.y32(k - 1).double()
            return X, torch.zeros_like(X)
        pre, d = self.preact(k - 1)
        X = _act(pre, lp.act)
        return (_pool2(X), _pool2(d)) if lp.pool else (X, d)

    def layer_input32(self, k):
        if k == 0:
            return torch.from_numpy(self.x)[:, None]
        lp = self.tab[k - 1]
        if lp.act == ACT_NONE:
            return self.y32(k - 1)
        ss = self.rows(self.wsl[k - 1].ss, 4, lp.cout)
        X = _act(self.z32(k - 1) * _c(ss[0]) + _c(ss[1]), lp.act)
        return _pool2(X) if lp.pool else X

    def dz(self, k):
        """dz_k = scale g_k + c1 z_k + c0 in float64 from the kernel's bc_k, the rounding of the kernel's two fmaf, and the sum of the
        three terms' magnitudes (with a small batch they cancel almost completely: |dz| says nothing about the rounding level)."""
        l, w = self.tab[k], self.wsl[k]
        if k == 1:      # features[0]: materialised by dz_apply_kernel, checked in B.dz1
            t = self.t32(self.wsl[-1].dz1, self.B, w.ho, w.wo, l.cout).double()
            return t, torch.zeros_like(t), t.abs()
        bc = self.rows(w.bc, 3, l.cout).double()
        G, Z = self.g32(k).double(), self.z32(k).double()
        a, b, c = G * _c(bc[0]), Z * _c(bc[1]), _c(bc[2])
        return a + b + c, U * (a.abs() + 2 * b.abs() + 2 * c.abs()), a.abs() + b.abs() + c.abs()

    def dz32(self, k):
        l, w = self.tab[k], self.wsl[k]
        if k == 1:
            return self.t32(self.wsl[-1].dz1, self.B, w.ho, w.wo, l.cout)
        bc = self.rows(w.bc, 3, l.cout)
        return self.g32(k) * _c(bc[0]) + (self.z32(k) * _c(bc[1]) + _c(bc[2]))

    # -- forward ------------------------------------------------------------------------------------------------------------------
    def forward(self, training=True):
        B = self.B
        for k in range(self.nl):
            l, w, where = self.tab[k], self.wsl[k], self.where(k)
            X, dX = self.layer_input(k)
            assert tuple(X.shape) == (B, l.cin, w.hin, w.win), (k, X.shape)
            W = self.weight(k).double()
            K = (9 * l.cin if l.kind == DENSE else (9 if l.kind == DW else l.cin)) + (1 if l.bias else 0)
            ref, mag = conv_fwd(X, W, l, w.ho, w.wo), conv_fwd(X.abs(), W.abs(), l, w.ho, w.wo)
            if l.bias:
                b = self.vec(l.b_off, l.cout).double()
                ref, mag = ref + _c(b), mag + _c(b.abs())
            bound = 2.0 * ((K + 2) * U * mag + conv_fwd(dX, W.abs(), l, w.ho, w.wo))
            self.cmp("F1 z", where, self.z32(k), ref, bound)
            if training:
                self.stats(k)
            else:
                self.eval_ss(k)
            if l.act == ACT_NONE:      # stored y_k = bn(z_k) (+ the block input)
                ss, Z = self.ss(k), self.z32(k).double()
                a, c = Z * _c(ss[0]), _c(ss[1])
                ref, mag = a + c, a.abs() + c.abs()
                if l.res_src >= 0:
                    r = self.y32(l.res_src).double()
                    ref, mag = ref + r, mag + r.abs()
                self.cmp("F3 y", where, self.y32(k), ref, 8.0 * U * mag)
        self.head()

    def stats(self, k):
        l, w, where = self.tab[k], self.wsl[k], self.where(k)
        Z32 = self.z32(k)
        Z = Z32.double()
        n = Z.numel() // l.cout
        mean, ea, ez2 = Z.mean((0, 2, 3)), Z.abs().mean((0, 2, 3)), (Z * Z).mean((0, 2, 3))
        var = Z.var((0, 2, 3), unbiased=False)
        tol_m = self.long_tol("F2 mean", mean * n, Z32.sum((0, 2, 3)), ea * n, n) / n
        tol_v = self.long_tol("F2 var", var, Z32.var((0, 2, 3), unbiased=False), ez2, n, var_floor=True)
        gamma, beta = self.vec(l.gamma_off, l.cout).double(), self.vec(l.beta_off, l.cout).double()
        rstd = 1.0 / torch.sqrt(var + om.BN_EPS)
        d_rstd = torch.maximum(1.0 / torch.sqrt(torch.clamp(var - tol_v, min=0.0) + om.BN_EPS) - rstd,
                               rstd - 1.0 / torch.sqrt(var + tol_v + om.BN_EPS))
        scale = gamma * rstd
        shift = beta - mean * scale
        d_scale = gamma.abs() * d_rstd
        ss = self.ss(k)
        flat = dict(layout="c")
        self.cmp("F2 mean", where + " ss.mean", ss[2], mean, tol_m + U * mean.abs(), **flat)
        self.cmp("F2 var", where + " ss.rstd", ss[3], rstd, d_rstd + U * rstd, **flat)
        self.cmp("F2 var", where + " ss.scale", ss[0], scale, d_scale + U * scale.abs(), **flat)
        self.cmp("F2 mean", where + " ss.shift", ss[1], shift,
                 scale.abs() * tol_m + mean.abs() * d_scale + U * (beta.abs() + (mean * scale).abs()), **flat)
        mom = om.BN_MOMENTUM
        rm0, rv0 = self.vec(l.rmean_off, l.cout, self.bufs0).double(), self.vec(l.rvar_off, l.cout, self.bufs0).double()
        unb = n / (n - 1.0) if n > 1 else 1.0
        self.cmp("F2 running_mean", where, self.vec(l.rmean_off, l.cout, self.bufs1), (1 - mom) * rm0 + mom * mean,
                 mom * tol_m + 8.0 * U * (((1 - mom) * rm0).abs() + (mom * mean).abs()), **flat)
        self.cmp("F2 running_var", where, self.vec(l.rvar_off, l.cout, self.bufs1), (1 - mom) * rv0 + mom * var * unb,
                 mom * unb * tol_v + 8.0 * U * (((1 - mom) * rv0).abs() + (mom * var * unb).abs()), **flat)

    def eval_ss(self, k):
        l, where = self.tab[k], self.where(k)
        rm, rv = self.vec(l.rmean_off, l.cout, self.bufs1).double(), self.vec(l.rvar_off, l.cout, self.bufs1).double()
        gamma, beta = self.vec(l.gamma_off, l.cout).double(), self.vec(l.beta_off, l.cout).double()
        rstd = 1.0 / torch.sqrt(rv + om.BN_EPS)
        scale = gamma * rstd
        ss = self.ss(k)
        flat = dict(layout="c")
        self.cmp("E ss", where + " ss.mean", ss[2], rm, 0.0 * rm, **flat)
        self.cmp("E ss", where + " ss.rstd", ss[3], rstd, 8.0 * U * rstd, **flat)
        self.cmp("E ss", where + " ss.scale", ss[0], scale, 8.0 * U * scale.abs(), **flat)
        self.cmp("E ss", where + " ss.shift", ss[1], beta - rm * scale, 8.0 * U * (beta.abs() + (rm * scale).abs()), **flat)

    def head(self):
        k = self.nl - 1
        l, w, tail = self.tab[k], self.wsl[k], self.wsl[-1]
        B, C, HW = self.B, l.cout, w.hy * w.wy
        pre, d = self.preact(k)
        a = _act(pre, l.act)
        where = self.where(k)
        pooled = torch.from_numpy(self.ws[tail.pooled:tail.pooled + B * C].reshape(B, C))
        pooled_d = torch.from_numpy(self.ws[tail.pooled_d:tail.pooled_d + B * C].reshape(B, C))
        self.cmp("F4 pooled", where, pooled, a.mean((2, 3)),
                 2.0 * ((HW + 2) * U * a.abs().sum((2, 3)) + d.sum((2, 3))) / HW, layout="bc")
        ref = pooled.double()
        if self.keep is not None:
            ref = ref * torch.from_numpy(self.keep).double() * self.scale
        self.cmp("F4 pooled_d", where, pooled_d, ref, 8.0 * U * ref.abs(), layout="bc")
        wc = self.vec(self.feature_params, self.C * C).reshape(self.C, C).double()
        bias = self.vec(self.feature_params + self.C * C, self.C).double()
        pd = pooled_d.double()
        self.cmp("F4 logits", "classifier", torch.from_numpy(self.logits), pd @ wc.T + bias,
                 2.0 * (C + 3) * U * (pd.abs() @ wc.abs().T + bias.abs()), layout="bl")

    # -- backward -----------------------------------------------------------------------------------------------------------------
    def mask(self, k):
        """(passes, undecided) of layer k's activation derivative at float64, from the kernel's z_k and ss_k."""
        l = self.tab[k]
        pre, d = self.preact(k)
        d = 4.0 * d
        if l.act == ACT_NONE:
            return torch.ones_like(pre, dtype=torch.bool), torch.zeros_like(pre, dtype=torch.bool)
        if l.act == ACT_RELU:
            return pre > 0, pre.abs() < d
        return (pre > 0) & (pre < 6), (pre.abs() < d) | ((pre - 6.0).abs() < d)

    def count_undecided(self, k, und):
        self.undecided[k] = int(und.sum())
        if und.sum().item() > MAX_UNDECIDED * und.numel():
            self.fails.append(f"masks {self.where(k)}: {int(und.sum())} of {und.numel()} activation decisions are within rounding of 0 or 6")

    def backward(self):
        B, nl = self.B, self.nl
        tail = self.wsl[-1]
        # B1: the last layer's g from dlogits
        k = nl - 1
        l, w = self.tab[k], self.wsl[k]
        C, HW = l.cout, w.hy * w.wy
        wc = self.vec(self.feature_params, self.C * C).reshape(self.C, C).double()
        dl = torch.from_numpy(self.dlogits).double()
        ms = torch.from_numpy(self.keep).double() * self.scale if self.keep is not None else torch.ones(B, C, dtype=torch.float64)
        d = (dl @ wc) * ms / HW
        bound = 2.0 * (self.C + 5) * U * (dl.abs() @ wc.abs()) * ms / HW
        passes, und = self.mask(k)
        self.count_undecided(k, und)
        full = d[:, :, None, None].expand(B, C, w.ho, w.wo)
        bound = bound[:, :, None, None].expand_as(full)
        self.cmp("B1 g_last", self.where(k), self.g32(k), full * passes, torch.where(und, bound, bound * passes),
                 alt=full * ~passes, und=und)
        # classifier gradients: sums over the batch
        pd = torch.from_numpy(self.ws[tail.pooled_d:tail.pooled_d + B * C].reshape(B, C)).double()
        off = self.feature_params
        self.cmp("B4 classifier", "model.classifier.1.weight", self.vec(off, self.C * C, self.grads).reshape(self.C, C), dl.T @ pd,
                 2.0 * (B + 2) * U * (dl.abs().T @ pd.abs()), layout="lc")
        self.cmp("B4 classifier", "model.classifier.1.bias", self.vec(off + self.C * C, self.C, self.grads), dl.sum(0),
                 2.0 * (B + 2) * U * dl.abs().sum(0), layout="l")
        self.cover[off:off + self.C * C + self.C] += 1

        addend = {self.tab[j].res_src: j for j in range(nl) if self.tab[j].res_src >= 0}
        for k in range(nl - 1, -1, -1):
            l, w, where = self.tab[k], self.wsl[k], self.where(k)
            self.bn_backward(k)
            if k == 1:
                self.dz1()
            dz, ddz, dza = self.dz(k)
            self.wgrad(k, dz, dza)
            if k == 0:
                break
            # B2: g_{k-1}
            j = k - 1
            lj, wj = self.tab[j], self.wsl[j]
            W = self.weight(k).double()
            K = l.cout if l.kind == PW else (9 if l.kind == DW else 4 * l.cout)
            dy = conv_dgrad(dz, W, l, w.hin, w.win)
            bound = (K + 2) * U * conv_dgrad(dz.abs(), W.abs(), l, w.hin, w.win) + conv_dgrad(ddz, W.abs(), l, w.hin, w.win)
            if j in addend:      # y_j also feeds the residual sum of layer addend[j], whose dy is its g (no activation)
                ga = self.g32(addend[j]).double()
                bound = bound + U * (dy.abs() + ga.abs())
                dy = dy + ga
            bound = 2.0 * bound
            wherej = f"{self.where(j)} <- data gradient of {where}"
            if j == 0:
                self.stem_unpool(dy, bound, wherej)
                continue
            passes, und = self.mask(j)
            self.count_undecided(j, und)
            self.cmp("B2 g", wherej, self.g32(j), dy * passes, torch.where(und, bound, bound * passes), alt=dy * ~passes, und=und)

    def stem_unpool(self, dy, bound, where):
        """g_0 from the gradient of the pooled downsample output: through MaxPool2d((1,2)) (the first maximum wins) and the ReLU."""
        w0 = self.wsl[0]
        Wp = w0.wy
        pre, d = self.preact(0)
        d = 4.0 * d
        pa, pb = pre[..., 0:2 * Wp:2], pre[..., 1:2 * Wp:2]
        da, db = d[..., 0:2 * Wp:2], d[..., 1:2 * Wp:2]
        ra, rb = pa.clamp(min=0), pb.clamp(min=0)
        first = ra >= rb
        und = (pa.abs() < da) | (pb.abs() < db) | ((torch.maximum(pa, pb) > 0) & ((ra - rb).abs() < da + db))
        ref, bnd, alt, undf = (torch.zeros_like(pre) for _ in range(4))
        sa, sb = first & (pa > 0), ~first & (pb > 0)
        ref[..., 0:2 * Wp:2], ref[..., 1:2 * Wp:2] = dy * sa, dy * sb
        alt[..., 0:2 * Wp:2], alt[..., 1:2 * Wp:2] = dy * ~sa, dy * ~sb
        bnd[..., 0:2 * Wp:2], bnd[..., 1:2 * Wp:2] = bound, bound
        undf[..., 0:2 * Wp:2], undf[..., 1:2 * Wp:2] = und.double(), und.double()
        undf = undf > 0
        self.count_undecided(0, undf)
        G = self.g32(0).double()
        # decided elements: exact zero where the gradient does not pass; undecided: the masked or the unmasked value
        passes = torch.zeros_like(pre)
        passes[..., 0:2 * Wp:2], passes[..., 1:2 * Wp:2] = sa.double(), sb.double()
        self.cmp("B2 g", where, G, ref, torch.where(undf, bnd, bnd * passes), alt=alt, und=undf)

    def bn_backward(self, k):
        """B3: dbeta = sum g, dgamma = sum g xhat, bc = [scale | c1 | c0]."""
        l, w, where = self.tab[k], self.wsl[k], self.where(k)
        ss32 = self.rows(w.ss, 4, l.cout)
        ss = ss32.double()
        G32, Z32 = self.g32(k), self.z32(k)
        G, Z = G32.double(), Z32.double()
        n = G.numel() // l.cout
        t2 = G * ((Z - _c(ss[2])) * _c(ss[3]))
        S1, S2 = G.sum((0, 2, 3)), t2.sum((0, 2, 3))
        tol1 = self.long_tol("B3 dbeta", S1, G32.sum((0, 2, 3)), G.abs().sum((0, 2, 3)), n)
        tol2 = self.long_tol("B3 dgamma", S2, (G32 * ((Z32 - _c(ss32[2])) * _c(ss32[3]))).sum((0, 2, 3)), t2.abs().sum((0, 2, 3)), n)
        flat = dict(layout="c")
        self.cmp("B3 dbeta", where, self.vec(l.beta_off, l.cout, self.grads), S1, tol1 + U * S1.abs(), **flat)
        self.cmp("B3 dgamma", where, self.vec(l.gamma_off, l.cout, self.grads), S2, tol2 + U * S2.abs(), **flat)
        self.cover[l.beta_off:l.beta_off + l.cout] += 1
        self.cover[l.gamma_off:l.gamma_off + l.cout] += 1
        bc = self.rows(w.bc, 3, l.cout).double()
        sc, me, rs = ss[0], ss[2], ss[3]
        c1 = -sc * (S2 / n) * rs
        tol_c1 = (sc * rs).abs() / n * tol2 + 4.0 * U * c1.abs()
        c0 = -sc * (S1 / n) - c1 * me
        tol_c0 = sc.abs() / n * tol1 + me.abs() * tol_c1 + 4.0 * U * ((sc * S1 / n).abs() + (c1 * me).abs())
        self.cmp("B3 bc", where + " bc.scale", bc[0], sc, 0.0 * sc, **flat)
        self.cmp("B3 bc", where + " bc.c1", bc[1], c1, tol_c1, **flat)
        self.cmp("B3 bc", where + " bc.c0", bc[2], c0, tol_c0, **flat)

    def dz1(self):
        l, w = self.tab[1], self.wsl[1]
        bc = self.rows(w.bc, 3, l.cout).double()
        a, b, c = self.g32(1).double() * _c(bc[0]), self.z32(1).double() * _c(bc[1]), _c(bc[2])
        got = self.t32(self.wsl[-1].dz1, self.B, w.ho, w.wo, l.cout)
        self.cmp("B dz1", self.where(1), got, a + b + c, 8.0 * U * (a.abs() + b.abs() + c.abs()))

    def wgrad(self, k, dz, dza):
        """B4: dW_k (and the downsample's conv-bias gradient); a term is (scale g + c1 z + c0) x: sum|terms| is taken over the
        three products of dz separately, times the magnitude of the input's own terms."""
        l, w, where = self.tab[k], self.wsl[k], self.where(k)
        X, dX = self.layer_input(k)
        n = dz.numel() // l.cout
        # (likewise the input: where it is rebuilt as act(z scale + shift), |z scale| + |shift| = dX / u is what gets rounded)
        ref, mag = conv_wgrad(dz, X, l), conv_wgrad(dza, torch.maximum(X.abs(), dX / U), l)
        dz32 = self.dz32(k)
        tol = self.long_tol(f"B4 dW {KIND[l.kind]}", ref, conv_wgrad(dz32, self.layer_input32(k), l), mag, n)
        got = self.weight(k, self.grads)
        self.cmp(f"B4 dW {KIND[l.kind]}", where, got, ref, tol + U * ref.abs(), layout="oikk")
        self.cover[l.w_off:l.w_off + got.numel()] += 1
        if l.bias:
            S, A = dz.sum((0, 2, 3)), dza.sum((0, 2, 3))
            tol = self.long_tol("B4 conv bias", S, dz32.sum((0, 2, 3)), A, n)
            self.cmp("B4 conv bias", where, self.vec(l.b_off, l.cout, self.grads), S, tol + U * S.abs(), layout="c")
            self.cover[l.b_off:l.b_off + l.cout] += 1

    # -- entry points ---------------------------------------------------------------------------------------------------------------
    def finish(self):
        if self.fails:
            raise Failure(f"{len(self.fails)} layer-local check(s) failed at (B,M,T,labels)=({self.B},{self.M},{self.T},{self.C}):\n" +
                          "\n".join(self.fails[:12]))
        return dict(ratios=self.ratios, ref_units=self.ref_units, undecided=sum(self.undecided.values()),
                    elements=sum(self.g32(k).numel() for k in self.undecided))


def check_training(cap):
    c = Check(cap)
    c.forward(training=True)
    c.backward()
    if not (c.cover == 1).all():      # B5
        c.fails.append(f"B5: {int((c.cover != 1).sum())} floats of the gradient buffer are not covered exactly once")
    if not np.isfinite(c.grads).all():
        c.fails.append("gradient buffer has non-finite entries")
    return c.finish()


def check_eval(cap):
    """Eval-mode forward: ss from the running buffers (bn_eval_ss_kernel), then F1, F3, F4; the buffers must not move."""
    e = cap["eval"]
    c = Check(e)
    if not np.array_equal(e["bufs_after"], e["bufs1"]):
        c.fails.append("eval-mode forward changed the running statistics")
    c.forward(training=False)
    return c.finish()


def report_text(name, rep):
    lines = [f"[mb_layerwise] {name}: undecided mask elements {rep['undecided']} of {rep['elements']}"]
    for cls in sorted(rep["ratios"]):
        ru = rep["ref_units"].get(cls)
        lines.append(f"[mb_layerwise]   {cls:22s} worst kernel/allowed {rep['ratios'][cls]:.3f}" +
                     (f"   float32 reference error {ru:.2f} u sum|terms|" if ru is not None else ""))
    return "\n".join(lines)


def run_case(lib, mem, B, M, T, C, dropout, layout, eval_too=False):
    """One case end to end; prints the figures before it asserts (visible with ``pytest -s``)."""
    cap = run_kernels(lib, mem, B, M, T, C, dropout=dropout, layout=layout, seed=B * 100 + T, eval_too=eval_too)
    reps, err = {}, None
    for name, fn in (("training", check_training),) + ((("eval", check_eval),) if eval_too else ()):
        try:
            reps[name] = fn(cap)
            print(report_text(f"({B},{M},{T}) labels {C} {layout} {name}", reps[name]), flush=True)
        except Failure as e:
            print(f"[mb_layerwise] ({B},{M},{T}) labels {C} {layout} {name} FAILED\n{e}", flush=True)
            err = err or e
    if err is not None:
        raise err
    return reps


if __name__ == "__main__":
    # child-process body of the emulator tests: ``plan | check B M T labels dropout layout`` on the emulator library, whose device
    # size (HIPEMU_CUS) is read when it is loaded
    import json
    import sys
    from emu_util import emu_lib
    mode, (B, M, T, C, drop), layout = sys.argv[1], (int(a) for a in sys.argv[2:7]), sys.argv[7]
    lib = emu_lib()
    out = {"coverage": sorted(coverage(layer_table(lib), workspace_map(lib, B, M, T, C)))}
    if mode == "check":
        out["reports"] = run_case(lib, HostMem(), B, M, T, C, bool(drop), layout)
    print("RESULT" + json.dumps(out))
