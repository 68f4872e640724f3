"""ctypes binding of the C ABI declared in ``include/howl_hip.h``.

``SIGNATURES`` is the single table of entry points (name -> argtypes); ``tests/test_cabi.py`` checks it against the
header and against the symbols the built library exports.  ``get()`` loads the in-tree ``libhowl_hip.so`` and fails
loudly when it is absent -- there is no fallback path.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p
from pathlib import Path

# HOWL_HIP_LIBRARY selects another build of the same C ABI (diagnostic kernel variants, tools/variants.py)
LIB_PATH = Path(os.environ.get("HOWL_HIP_LIBRARY") or Path(__file__).resolve().parent / "libhowl_hip.so")
MAX_MELS = 96                                                                       # HOWL_MAX_MELS
FB_COLS = 48
FB_PACKED_FLOATS = 260 * FB_COLS + 17 * 64 * 4 + 17 * (FB_COLS // 4) * 64 + 32      # HOWL_FB_PACKED_FLOATS: one bank


def fb_packed_floats(n_mels: int) -> int:
    """``howl_fb_packed_floats``: a packed filterbank is one bank of up to 48 mel bins, or two back to back."""
    return FB_PACKED_FLOATS * (1 if n_mels <= FB_COLS else 2)


P = c_void_p  # device pointer
STREAM = c_void_p


class HowlMelPoints(ctypes.Structure):
    _fields_ = [("f", c_float * (MAX_MELS + 2))]


class HowlRes8Params(ctypes.Structure):
    _fields_ = [("conv0_w", P), ("conv_w", P * 6), ("bn_running_mean", P * 6), ("bn_running_var", P * 6),
                ("bn_num_batches", P * 6), ("out_w", P), ("out_b", P)]


class HowlRes8Grads(ctypes.Structure):
    _fields_ = [("conv0_w", P), ("conv_w", P * 6), ("out_w", P), ("out_b", P)]


class HowlRes8Saved(ctypes.Structure):
    _fields_ = [("s", P * 7), ("bn_stats", P), ("pooled", P), ("mask0", P)]


class HowlLstmParams(ctypes.Structure):
    _fields_ = [("w_ih", P), ("w_hh", P), ("b_ih", P), ("b_hh", P)]


class HowlLstmGrads(ctypes.Structure):
    _fields_ = [("w_ih", P), ("w_hh", P), ("b_ih", P), ("b_hh", P)]


class HowlHeadParams(ctypes.Structure):
    _fields_ = [("w1", P), ("b1", P), ("w2", P), ("b2", P)]


class HowlHeadGrads(ctypes.Structure):
    _fields_ = [("w1", P), ("b1", P), ("w2", P), ("b2", P)]


class HowlCtcMean(ctypes.Structure):
    _fields_ = [("nll", P), ("target_lengths", P), ("B", c_int), ("loss", P)]


class HowlLogmelArgs(ctypes.Structure):
    _fields_ = [("pcm", P), ("B", c_int), ("L", c_int), ("ld", c_long), ("fbp", P), ("M", c_int), ("log_eps", c_float), ("zmuv", P),
                ("out", P), ("layout", c_int)]


class HowlAdamW(ctypes.Structure):
    _fields_ = [("p", P), ("g", P), ("m", P), ("v", P), ("n", c_size_t), ("lr", c_float), ("beta1", c_float), ("beta2", c_float),
                ("eps", c_float), ("weight_decay", c_float), ("step", c_int), ("grad_scale", c_float)]


class HowlLstmSaved(ctypes.Structure):
    _fields_ = [("gx", P), ("gates", P), ("c", P), ("hseq", P), ("dgates", P), ("t_out", c_int), ("x_frames", c_int)]


class HowlMbLayer(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("kind", "cin", "cout", "stride", "pad_h", "pad_w", "act", "bias", "pool", "res_src",
                                     "feat", "sub", "wrapped")] + \
               [(n, ctypes.c_longlong) for n in ("w_off", "b_off", "gamma_off", "beta_off", "rmean_off", "rvar_off")]


class HowlMbWsLayer(ctypes.Structure):
    _fields_ = [(n, ctypes.c_longlong) for n in ("z", "g", "y", "ss", "bc", "b_ss", "f_yout", "pooled", "pooled_d", "dz1",
                                                 "total_floats")] + \
               [(n, c_int) for n in ("hin", "win", "ho", "wo", "hy", "wy", "f_tile", "f_cx", "f_ry", "d_tile", "d_ry", "d_chunks",
                                     "nslab", "group_rows")]


class HowlGruParams(ctypes.Structure):
    """``HowlGruParams`` / ``HowlGruGrads`` of ``include/howl_hip_gru.h``: the sixteen tensors in ``state_dict`` order."""
    _fields_ = [(n, P) for n in ("conv1_w", "conv1_b", "bn1_w", "bn1_b", "conv2_w", "conv2_b", "bn2_w", "bn2_b", "w_ih", "w_hh", "b_ih",
                                 "b_hh", "w1", "b1", "w2", "b2")]


class HowlGruGrads(ctypes.Structure):
    _fields_ = list(HowlGruParams._fields_)


class HowlGruBuffers(ctypes.Structure):
    _fields_ = [(n, P) for n in ("bn1_mean", "bn1_var", "bn1_batches", "bn2_mean", "bn2_var", "bn2_batches")]


class HowlLasParams(ctypes.Structure):
    """``HowlLasParams`` / ``HowlLasGrads`` of ``include/howl_hip_las.h``: the twenty-five distinct tensors in ``state_dict`` order."""
    _fields_ = [(n, P) for n in ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "w_ih_f", "w_hh_f", "b_ih_f",
                                 "b_hh_f", "w_ih_r", "w_hh_r", "b_ih_r", "b_hh_r", "cv", "v_w", "v_b", "k_w", "k_b", "w1", "b1", "w2", "b2")]


class HowlLasGrads(ctypes.Structure):
    _fields_ = list(HowlLasParams._fields_)


class HowlLasBuffers(ctypes.Structure):
    _fields_ = [(n, P) for n in ("bn1_mean", "bn1_var", "bn1_batches", "bn2_mean", "bn2_var", "bn2_batches")]


class HowlCnnParams(ctypes.Structure):
    """``HowlCnnParams`` / ``HowlCnnGrads`` of ``include/howl_hip_cnn.h``: the twelve tensors in ``state_dict`` order."""
    _fields_ = [(n, P) for n in ("conv0_w", "conv0_b", "bn1_w", "bn1_b", "conv1_w", "conv1_b", "bn2_w", "bn2_b", "w1", "b1", "w2", "b2")]


class HowlCnnGrads(ctypes.Structure):
    _fields_ = list(HowlCnnParams._fields_)


class HowlCnnBuffers(ctypes.Structure):
    _fields_ = [(n, P) for n in ("bn1_mean", "bn1_var", "bn1_batches", "bn2_mean", "bn2_var", "bn2_batches")]


class HowlDenseRowMap(ctypes.Structure):
    """``HowlDenseRowMap`` of ``include/howl_hip_dense.h``; ``inner = DENSE_LIN`` is the plain stride ``s_inner``."""
    _fields_ = [("inner", c_int), ("s_outer", c_long), ("s_inner", c_long)]


class HowlDenseChoice(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("family", "t0", "t1", "t2", "t3", "gx", "gy", "gz", "kps")]


class HowlDenseGemm(ctypes.Structure):
    _fields_ = [("a_major_k", c_int), ("a", P), ("am", HowlDenseRowMap), ("a_ks", c_long), ("ak", HowlDenseRowMap), ("b", P),
                ("bk", HowlDenseRowMap), ("b_ns", c_long), ("M", c_int), ("N", c_int), ("K", c_int), ("splits", c_int), ("bias", P),
                ("relu", c_int), ("c", P), ("c_ms", c_long), ("c_split_stride", c_long), ("c_floats", c_size_t), ("w2", P), ("b2", P),
                ("y2", P), ("thin_out", c_int)]


class HowlDenseWgrad(ctypes.Structure):
    _fields_ = [("dout", P), ("dm", HowlDenseRowMap), ("n_out", c_int), ("in_", P), ("im", HowlDenseRowMap), ("k_in", c_int),
                ("rows", c_int), ("scratch", P), ("scratch_floats", c_size_t), ("dw", P), ("max_splits", c_int),
                ("rows_per_split", c_int), ("in2", P), ("im2", HowlDenseRowMap), ("k2", c_int), ("scratch2", P),
                ("scratch2_floats", c_size_t), ("dw2", P)]


class HowlDenseSlabJob(ctypes.Structure):
    _fields_ = [("part", P), ("nparts", c_int), ("stride", c_long), ("n", c_long), ("out", P), ("out2", P)]


class HowlDecideConfig(ctypes.Structure):
    """``HowlDecideConfig`` of ``include/howl_hip_decide.h``: a host struct; ``weights`` / ``color`` are device pointers."""
    _fields_ = [("mode", c_int), ("C", c_int), ("blank", c_int), ("negative", c_int), ("threshold", c_double), ("smoothing_ms", c_double),
                ("window_ms", c_double), ("tolerance_ms", c_double), ("seq_len", c_int), ("sequence", c_int * 16), ("weights", P),
                ("color", P)]


SIGNATURES = {
    "howl_version": [POINTER(c_int), POINTER(c_int)],
    "howl_profile_enable": [c_int],
    "howl_profile_read": [c_char_p, POINTER(c_double), POINTER(c_int), c_int],
    "howl_profile_read_work": [c_char_p, POINTER(c_double), POINTER(c_int), POINTER(c_double), c_int],
    "howl_shutdown": [],
    "howl_fb_pack": [P, c_int, P, STREAM],
    "howl_fb_from_points": [POINTER(HowlMelPoints), c_int, c_float, P, STREAM],
    "howl_logmel_fwd": [P, c_int, c_int, c_long, P, c_int, c_float, P, P, c_int, STREAM],
    "howl_deltas_fwd": [P, c_int, c_int, c_int, P, P, STREAM],
    "howl_zmuv_update": [P, c_size_t, P, P, P, P, STREAM],
    "howl_zmuv_update_masked": [P, P, c_size_t, c_double, P, P, P, P, STREAM],
    "howl_zmuv_pair": [P, P, P, STREAM],
    "howl_zmuv_apply": [P, c_size_t, P, P, STREAM],
    "howl_collate_augment": [P, c_long, P, P, P, P, P, P, ctypes.c_ulonglong, c_int, c_int, P, STREAM],
    "howl_collate_augment_mix": [P, c_long, P, P, P, P, P, P, ctypes.c_ulonglong, P, c_long, P, P, P, c_int, c_int, P, STREAM],
    "howl_collate_augment_window": [P, c_long, P, P, P, P, P, P, ctypes.c_ulonglong, P, c_long, P, P, P, P, c_int, c_int, P,
                                    STREAM],
    "howl_gather_windows": [P, c_long, P, P, P, P, c_int, c_int, P, STREAM],
    "howl_specaug_mask": [P, c_int, c_int, c_int, c_int, c_long, c_long, c_long, c_long, P, P, P, P, STREAM],
    "howl_res8_fwd": [POINTER(HowlRes8Params), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int,
                      POINTER(HowlRes8Saved), P, P, c_size_t, STREAM],
    "howl_res8_fwd_long": [POINTER(HowlRes8Params), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, P, P, c_size_t, STREAM],
    "howl_res8_bwd": [POINTER(HowlRes8Params), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int,
                      POINTER(HowlRes8Saved), P, POINTER(HowlRes8Grads), P, c_size_t, STREAM],
    "howl_res8_bwd_part": [POINTER(HowlRes8Params), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int,
                           POINTER(HowlRes8Saved), P, POINTER(HowlRes8Grads), P, c_size_t, c_int, STREAM],
    "howl_res8_fwd_xent": [POINTER(HowlRes8Params), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int,
                           POINTER(HowlRes8Saved), P, P, P, P, P, c_size_t, STREAM],
    "howl_res8_bwd_xent": [POINTER(HowlRes8Params), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int,
                           POINTER(HowlRes8Saved), P, P, P, POINTER(HowlRes8Grads), P, c_size_t, c_int, POINTER(HowlAdamW), STREAM],
    "howl_dropout_mask": [P, c_size_t, c_float, ctypes.c_ulonglong, STREAM],
    "howl_xent_fwd_bwd": [P, P, c_int, c_int, P, P, STREAM],
    "howl_ctc_loss": [P, c_long, c_long, c_int, c_int, c_int, P, c_long, c_int, P, P, c_int, P, P, P, c_long, c_long, P, c_size_t,
                      STREAM],
    "howl_lstm_fwd": [POINTER(HowlLstmParams), P, c_int, c_int, c_int, P, P, P, POINTER(HowlLstmSaved), P, P, P, c_size_t,
                      STREAM],
    "howl_lstm_fwd_next": [POINTER(HowlLstmParams), P, c_int, c_int, c_int, P, P, P, POINTER(HowlLstmSaved), P, P, P, c_size_t,
                           POINTER(HowlLogmelArgs), STREAM],
    "howl_lstm_bwd": [POINTER(HowlLstmParams), P, c_int, c_int, c_int, P, P, POINTER(HowlLstmSaved), P, P, P,
                      POINTER(HowlLstmGrads), P, c_size_t, STREAM],
    "howl_head_fwd": [POINTER(HowlHeadParams), P, c_int, c_long, c_long, c_int, c_int, c_int, c_int, P, P, STREAM],
    "howl_head_bwd": [POINTER(HowlHeadParams), P, c_int, c_long, c_long, c_int, c_int, c_int, c_int, P, P, P, P,
                      POINTER(HowlHeadGrads), POINTER(HowlCtcMean), P, c_size_t, STREAM],
    "howl_seq_head_ctc": [POINTER(HowlHeadParams), P, c_long, c_long, c_int, c_int, c_int, c_int, c_int, P, c_long, c_int, P, P, c_int, P, P,
                          P, P, P, c_size_t, STREAM],
    "howl_seq_head_ctc_supported": [c_int, c_int, c_int, c_int, c_int, c_int],
    "howl_seq_lstm_bwd": [POINTER(HowlHeadParams), c_int, c_int, P, P, P, P, POINTER(HowlHeadGrads), POINTER(HowlCtcMean), P,
                          c_size_t, POINTER(HowlLstmParams), P, c_int, c_int, c_int, P, P, POINTER(HowlLstmSaved),
                          POINTER(HowlLstmGrads), P, c_size_t, POINTER(HowlAdamW), STREAM],
    "howl_adamw_step": [P, P, P, P, c_size_t, c_float, c_float, c_float, c_float, c_float, c_int, c_float, STREAM],
    "howl_mobilenet_layer": [c_int, POINTER(HowlMbLayer)],
    "howl_mobilenet_workspace_layer": [c_int, c_int, c_int, c_int, c_int, POINTER(HowlMbWsLayer)],
    "howl_mobilenet_fwd": [P, P, c_int, P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, P, c_float, P, P, c_size_t,
                           STREAM],
    "howl_mobilenet_bwd": [P, c_int, P, c_long, c_long, c_long, c_int, c_int, c_int, P, c_float, P, P, P, c_size_t, STREAM],
}
# entry points that do not return an int status
SIZE_FUNCS = {"howl_fb_packed_floats": [c_int], "howl_res8_workspace_bytes": [c_int, c_int], "howl_res8_long_workspace_bytes": [c_int, c_int],
              "howl_res8_workspace_bytes_mels": [c_int, c_int, c_int], "howl_res8_saved_floats": [c_int, c_int, c_int],
              "howl_res8_eval_workspace_bytes_mels": [c_int, c_int, c_int], "howl_res8_row_strips": [c_int], "howl_res8_long_workspace_bytes_mels": [c_int, c_int, c_int], "howl_lstm_workspace_bytes": [c_int, c_int],
              "howl_lstm_needs_gx": [POINTER(HowlLstmParams), c_int, c_int, c_int, c_int],
              "howl_head_workspace_bytes": [c_int, c_int, c_int],
              "howl_mobilenet_num_layers": [],
              "howl_mobilenet_param_floats": [c_int], "howl_mobilenet_buffer_floats": [],
              "howl_mobilenet_workspace_bytes": [c_int, c_int, c_int, c_int],
              "howl_ctc_supported": [c_int, c_int, c_int], "howl_ctc_workspace_floats": [c_int, c_int]}


# The streaming res8 entry points of ``include/howl_hip_stream.h`` (a table of their own: ``tests/test_emu_res8_stream.py`` checks it
# against that header the way ``tests/test_cabi.py`` checks the tables above against ``howl_hip.h``)
STREAM_SIGNATURES = {
    "howl_res8_stream_prepare": [POINTER(HowlRes8Params), c_int, P, c_size_t, STREAM],
    "howl_res8_stream_windows": [P, P, c_long, c_int, c_int, P, c_int, c_float, P, c_int, P, P, STREAM],
}
STREAM_SIZE_FUNCS = {"howl_res8_stream_supported": [c_int, c_int, c_int], "howl_res8_stream_state_bytes": [c_int]}

# The streaming seq-lstm / lstm entry points of ``include/howl_hip_lstm_stream.h`` (their own tables for the same reason:
# ``tests/test_emu_lstm_stream.py`` checks them against that header)
LSTM_STREAM_SIGNATURES = {
    "howl_lstm_stream_chunks": [POINTER(HowlLstmParams), POINTER(HowlHeadParams), P, c_long, c_int, c_int, P, P, P, c_int, c_float, P,
                                P, P, c_int, c_int, P, P, c_long, STREAM],
}
LSTM_STREAM_SIZE_FUNCS = {"howl_lstm_stream_supported": [c_int, c_int, c_int]}

# The decision-logic entry points of ``include/howl_hip_decide.h`` (their own tables again: ``tests/test_emu_decide.py`` checks
# them against that header)
DECIDE_SIGNATURES = {
    "howl_decide_clips": [POINTER(HowlDecideConfig), P, c_long, c_long, c_int, c_int, P, P, P, P, P, P, P, P, P, c_long, P, STREAM],
}
DECIDE_SIZE_FUNCS = {"howl_decide_supported": [POINTER(HowlDecideConfig), c_int]}

# The long-target CTC entry points of ``include/howl_hip_ctc_long.h`` (their own tables again: ``tests/test_emu_ctc_long.py`` checks
# them against that header); ``howl_ctc_loss_long`` takes ``howl_ctc_loss``'s argument list
CTC_LONG_SIGNATURES = {
    "howl_ctc_loss_long": list(SIGNATURES["howl_ctc_loss"]),
}
CTC_LONG_SIZE_FUNCS = {"howl_ctc_long_supported": [c_int, c_int, c_int], "howl_ctc_long_window_rows": [c_int],
                       "howl_ctc_long_workspace_floats": [c_int, c_int, c_int]}

# The gru model's entry points of ``include/howl_hip_gru.h`` (their own tables again: ``tests/test_emu_gru.py`` checks them
# against that header)
GRU_SIGNATURES = {
    "howl_gru_fwd": [POINTER(HowlGruParams), POINTER(HowlGruBuffers), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, P, c_int, P,
                     c_float, P, P, c_size_t, STREAM],
    "howl_gru_bwd": [POINTER(HowlGruParams), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, P, c_float, P, POINTER(HowlGruGrads),
                     P, c_size_t, STREAM],
}
GRU_SIZE_FUNCS = {"howl_gru_supported": [c_int, c_int, c_int, c_int], "howl_gru_workspace_bytes": [c_int, c_int]}

# The las model's entry points of ``include/howl_hip_las.h`` (``tests/test_emu_las.py`` checks them against that header)
LAS_SIGNATURES = {
    "howl_las_fwd": [POINTER(HowlLasParams), POINTER(HowlLasBuffers), P, c_long, c_long, c_long, c_long, c_int, c_int, c_int, c_int, P, c_int,
                     P, c_float, P, P, c_size_t, STREAM],
    "howl_las_bwd": [POINTER(HowlLasParams), P, c_long, c_long, c_long, c_long, c_int, c_int, c_int, c_int, P, c_float, P,
                     POINTER(HowlLasGrads), P, c_size_t, STREAM],
}
LAS_SIZE_FUNCS = {"howl_las_supported": [c_int, c_int, c_int, c_int], "howl_las_workspace_bytes": [c_int, c_int]}

# The streaming las entry points of ``include/howl_hip_las_stream.h`` (tables of their own: ``tests/test_emu_las_stream.py`` checks
# them against that header)
LAS_STREAM_SIGNATURES = {
    "howl_las_stream_prepare": [POINTER(HowlLasParams), POINTER(HowlLasBuffers), c_int, P, c_size_t, STREAM],
    "howl_las_stream_windows": [P, P, c_long, c_int, c_int, c_int, P, c_int, c_float, P, c_int, P, P, P, c_size_t, STREAM],
}
LAS_STREAM_SIZE_FUNCS = {"howl_las_stream_supported": [c_int, c_int, c_int], "howl_las_stream_state_bytes": [c_int],
                         "howl_las_stream_workspace_bytes": [c_int, c_int]}

# The streaming gru entry points of ``include/howl_hip_gru_stream.h`` (tables of their own: ``tests/test_emu_gru_stream.py`` checks
# them against that header)
GRU_STREAM_SIGNATURES = {
    "howl_gru_stream_windows": [POINTER(HowlGruParams), POINTER(HowlGruBuffers), P, c_long, c_int, c_int, c_int, P, c_int, c_float, P, c_int,
                                P, P, P, c_size_t, STREAM],
}
GRU_STREAM_SIZE_FUNCS = {"howl_gru_stream_supported": [c_int, c_int, c_int], "howl_gru_stream_workspace_bytes": [c_int, c_int]}

# The small-cnn / seq-cnn entry points of ``include/howl_hip_cnn.h`` (``tests/test_emu_cnn.py`` checks them against that header)
CNN_SMALL, CNN_SEQ = 0, 1                                                           # HOWL_CNN_SMALL, HOWL_CNN_SEQ
CNN_SIGNATURES = {
    "howl_cnn_fwd": [c_int, POINTER(HowlCnnParams), POINTER(HowlCnnBuffers), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, P,
                     c_float, P, P, c_size_t, STREAM],
    "howl_cnn_bwd": [c_int, POINTER(HowlCnnParams), P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_float, P, POINTER(HowlCnnGrads),
                     P, c_size_t, STREAM],
}
CNN_SIZE_FUNCS = {"howl_cnn_supported": [c_int, c_int, c_int, c_int, c_int], "howl_cnn_workspace_bytes": [c_int, c_int, c_int, c_int],
                  "howl_cnn_out_rows": [c_int, c_int]}

# The streaming small-cnn / seq-cnn entry points of ``include/howl_hip_cnn_stream.h`` (tables of their own:
# ``tests/test_emu_cnn_stream.py`` checks them against that header)
CNN_STREAM_TILE_ROWS = 8                                                            # HOWL_CNN_STREAM_TILE_ROWS
CNN_STREAM_SIGNATURES = {
    "howl_cnn_stream_windows": [POINTER(HowlCnnParams), POINTER(HowlCnnBuffers), P, c_long, c_int, c_int, P, c_int, c_float, P, c_int, P, P,
                                P, c_size_t, STREAM],
    "howl_cnn_stream_clips": [POINTER(HowlCnnParams), POINTER(HowlCnnBuffers), P, c_long, c_int, c_int, P, P, c_int, c_float, P, c_int, P, P,
                              c_long, P, c_size_t, STREAM],
}
CNN_STREAM_SIZE_FUNCS = {"howl_cnn_stream_supported": [c_int, c_int, c_int, c_int], "howl_cnn_stream_workspace_bytes": [c_int, c_int, c_int],
                         "howl_cnn_stream_rows": [c_int, c_int]}

# The time-stretch entry point of ``include/howl_hip_timestretch.h`` (``tests/test_emu_timestretch.py`` checks the table against that
# header).  ``clips_host`` is a HOST pointer to ``HowlStretchClip`` records (``STRETCH_CLIP_DTYPE``), ``clips_dev`` their device copy.
TIMESTRETCH_SIGNATURES = {
    "howl_timestretch_clips": [P, c_long, c_long, P, c_long, c_long, c_void_p, P, c_int, P, c_long, ctypes.c_uint, STREAM],
}
TIMESTRETCH_SIZE_FUNCS = {}
TIMESTRETCH_NO_COPY = 1                                                             # HOWL_TIMESTRETCH_NO_COPY
TIMESTRETCH_MIN_SAMPLES = 2048                                                      # HOWL_TIMESTRETCH_MIN_SAMPLES
# ``HowlStretchClip`` as a numpy record (48 bytes, no padding)
STRETCH_CLIP_FIELDS = [("rate", "<f8"), ("src_row", "<i8"), ("dst_off", "<i8"), ("len", "<i4"), ("out_len", "<i4"), ("n_out", "<i4"),
                       ("bg_idx", "<i4"), ("bg_off", "<i4"), ("alpha", "<f4")]

# The resampler of ``include/howl_hip_resample.h`` (``tests/test_emu_resample.py`` checks the tables against that header).  ``plan``,
# ``clips_host`` and the bank written by ``howl_resample_bank`` are HOST pointers; ``clips_dev`` is the records' device copy.
class HowlResamplePlan(ctypes.Structure):
    _fields_ = [("sr_in", c_int), ("sr_out", c_int), ("up", c_int), ("down", c_int), ("taps", c_int), ("j_lo", c_int), ("j_hi", c_int),
                ("reserved", c_int), ("s", c_double)]


RESAMPLE_SIGNATURES = {
    "howl_resample_plan": [c_int, c_int, POINTER(HowlResamplePlan)],
    "howl_resample_bank": [POINTER(HowlResamplePlan), c_void_p],
    "howl_resample_clips": [P, c_long, c_int, c_int, P, c_long, POINTER(HowlResamplePlan), c_void_p, P, c_int, P, c_long, STREAM],
}
RESAMPLE_SIZE_FUNCS = {"howl_resample_bank_floats": [POINTER(HowlResamplePlan)], "howl_resample_out_len": [POINTER(HowlResamplePlan), c_long]}
RESAMPLE_F32, RESAMPLE_I16 = 0, 1                                                   # HOWL_RESAMPLE_F32 / _I16
RESAMPLE_MAX_CLIPS = 8192                                                           # HOWL_RESAMPLE_MAX_CLIPS
RESAMPLE_MAX_FRAMES = 1 << 24                                                       # HOWL_RESAMPLE_MAX_FRAMES
# ``HowlResampleClip`` as a numpy record (24 bytes, no padding)
RESAMPLE_CLIP_FIELDS = [("src_off", "<i8"), ("dst_off", "<i8"), ("len", "<i4"), ("out_len", "<i4")]

# The tests' door to the dense kernels of ``howl_gemm.hip.h``: ``include/howl_hip_dense.h`` (``tests/test_emu_dense.py`` checks the
# tables against that header)
DENSE_LIN = 1 << 30                                                                 # HOWL_DENSE_LIN
DENSE_FAMILIES = {1: "gemm_kernel", 2: "gemm_vec_kernel", 3: "rowgemm_kernel", 4: "thin_wgrad_kernel", 5: "wgrad_big_kernel",
                  6: "wgrad_big_multi_kernel.job", 7: "wgrad_big_multi_kernel", 8: "wgrad_w8_body", 9: "sum_slabs_kernel",
                  10: "sum_slabs_multi_kernel", 11: "colsum_kernel", 12: "relu_bwd_kernel"}
DENSE_SIGNATURES = {
    "howl_dense_gemm": [POINTER(HowlDenseGemm), POINTER(c_int), POINTER(c_int), STREAM],
    "howl_dense_wgrad": [c_int, c_int, POINTER(HowlDenseWgrad), STREAM],
    "howl_dense_wgrad_slabs": [POINTER(HowlDenseWgrad), c_int, POINTER(c_int), STREAM],
    "howl_dense_colsum": [P, POINTER(HowlDenseRowMap), c_int, c_int, P, c_size_t, P, P, c_int, c_int, c_int, STREAM],
    "howl_dense_slab_sums": [c_int, POINTER(HowlDenseSlabJob), POINTER(HowlAdamW), POINTER(HowlCtcMean), STREAM],
    "howl_dense_sum_slabs": [P, c_int, c_long, P, STREAM],
    "howl_dense_relu_bwd": [P, P, c_long, P, STREAM],
}
DENSE_SIZE_FUNCS = {"howl_dense_choices": [POINTER(HowlDenseChoice), c_size_t], "howl_dense_num_cus": [],
                    "howl_dense_gemm_splits": [c_int, c_int], "howl_dense_gemm_c_floats": [POINTER(HowlDenseGemm)],
                    "howl_dense_wgrad_splits": [POINTER(HowlDenseWgrad)], "howl_dense_wgrad_scratch_floats": [POINTER(HowlDenseWgrad)],
                    "howl_dense_wgrad_scratch2_floats": [POINTER(HowlDenseWgrad)], "howl_dense_colsum_chunks": [c_int, c_int, c_int]}


class HowlHipError(RuntimeError):
    pass


class Library:
    def __init__(self, path):
        path = Path(path)
        if not path.exists():
            raise HowlHipError(
                f"{path} not found: the HIP extension is not built. Run `python __graft_entry__.py` "
                "(build()) first; howl_amd has no CPU fallback.")
        self.path = path
        self.cdll = ctypes.CDLL(str(path))
        self.cdll.howl_last_error.restype = c_char_p
        self.cdll.howl_last_error.argtypes = []
        for name, argtypes in {**SIGNATURES, **STREAM_SIGNATURES, **LSTM_STREAM_SIGNATURES, **DECIDE_SIGNATURES,
                               **CTC_LONG_SIGNATURES, **GRU_SIGNATURES, **LAS_SIGNATURES, **LAS_STREAM_SIGNATURES,
                               **GRU_STREAM_SIGNATURES, **TIMESTRETCH_SIGNATURES, **RESAMPLE_SIGNATURES, **CNN_SIGNATURES, **CNN_STREAM_SIGNATURES,
                               **DENSE_SIGNATURES}.items():
            fn = getattr(self.cdll, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = c_int
            fn.argtypes = argtypes
        for name, argtypes in {**SIZE_FUNCS, **STREAM_SIZE_FUNCS, **LSTM_STREAM_SIZE_FUNCS, **DECIDE_SIZE_FUNCS,
                               **CTC_LONG_SIZE_FUNCS, **GRU_SIZE_FUNCS, **LAS_SIZE_FUNCS, **LAS_STREAM_SIZE_FUNCS,
                               **GRU_STREAM_SIZE_FUNCS, **TIMESTRETCH_SIZE_FUNCS, **RESAMPLE_SIZE_FUNCS, **CNN_SIZE_FUNCS, **CNN_STREAM_SIZE_FUNCS,
                               **DENSE_SIZE_FUNCS}.items():
            fn = getattr(self.cdll, name)
            fn.restype = c_size_t
            fn.argtypes = argtypes

    def call(self, name, *args):
        rc = getattr(self.cdll, name)(*args)
        if rc != 0:
            raise HowlHipError(f"{name} failed ({rc}): {self.cdll.howl_last_error().decode()}")


_LIB = None


def get() -> Library:
    global _LIB
    if _LIB is None:
        _LIB = Library(LIB_PATH)
        import atexit
        atexit.register(_LIB.cdll.howl_shutdown)     # side HIP queues / events go before the runtime does
    return _LIB
