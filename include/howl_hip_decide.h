/* howl_hip_decide.h -- the engines' frame-by-frame decision logic on the device: one kernel launch from the per-frame class
 * probabilities of N clips to each clip's detection flag and time-stamped label history.
 *
 * Replaces, for a dataset pass (InferenceEngine.infer_many / FrameInferenceEngine.infer_many), the host loops of
 * howl_amd/model/inference.py (_run_frames, _run_fsm) over howl_amd/model/decision.py (ProbabilitySmoother, SequenceMatcher):
 * per-class reweighting and renormalisation, the blank skip of the sequence engine, max-smoothing over a time window, threshold,
 * label colouring, the label history and the sequence matcher with its sliding window.  The arithmetic is the host's, operation
 * for operation (fp32 probabilities, NumPy's summation order, a correctly rounded division, fp64 time stamps), so flags, labels
 * and stamps are the same bits.  One wavefront serves one clip; nothing couples two clips.
 *
 * Range: 1 <= C <= 64 classes, a sequence of 0 .. 16 labels, 1 <= N <= 8192 clips, 0 <= n_frames[n] <= T_max <= 8192, a
 * smoothing window that is finite and not negative and holds at most HOWL_DECIDE_RING_FRAMES frames at a time.  Reported by
 * howl_decide_supported and refused by howl_decide_clips (the ring's occupancy depends on the clips' frame periods, which live on
 * the device: a clip whose ring would overflow is flagged in `status` instead); callers keep the host loops for anything else.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).
 */
#ifndef HOWL_HIP_DECIDE_H
#define HOWL_HIP_DECIDE_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_DECIDE_MAX_CLASSES 64
#define HOWL_DECIDE_MAX_SEQUENCE 16
#define HOWL_DECIDE_MAX_CLIPS 8192
#define HOWL_DECIDE_MAX_FRAMES 8192
#define HOWL_DECIDE_RING_FRAMES 32 /* frames the smoothing window may hold at one time */

/* The engine's settings, a HOST struct (read during the call, not kept). */
typedef struct {
    int mode;            /* 0: sequence engine (_run_frames: time advances before the frame, blank frames are skipped);
                            1: frame engine (_run_fsm: time advances behind the frame's history entry) */
    int C;               /* classes per frame */
    int blank;           /* mode 0: frames whose arg-max is this class are skipped */
    int negative;        /* the label of a frame below the threshold, and of a label the colouring does not map */
    double threshold;    /* compared in fp32, as NumPy 2 compares an fp32 scalar with a Python float */
    double smoothing_ms; /* the smoothing window */
    double window_ms;    /* the matcher's window over the label history */
    double tolerance_ms; /* the matcher's tolerance for foreign labels inside a partial match */
    int seq_len;         /* 0: never present, nothing is dropped from the history */
    int sequence[HOWL_DECIDE_MAX_SEQUENCE];
    const double* weights; /* DEVICE, C doubles; NULL: the probabilities are renormalised as they are */
    const int* color;      /* DEVICE, C entries, -1 = "not in the map"; NULL: no colouring is configured */
} HowlDecideConfig;

/* 1 when the configuration and T_max are inside the kernel's range, else 0. */
int howl_decide_supported(const HowlDecideConfig* cfg, int T_max);

/* ONE launch of ceil(N / 4) workgroups, one wavefront per clip.  Clip n = frames t < n_frames[n] with the probabilities
 * probs[n * s_clip + t * s_frame + c], c < C (strides in floats), walked in order with the host's arithmetic.
 *
 *   n_frames   (N) int.  Contract: 0 <= n_frames[n] <= T_max; a value outside is clamped into that range inside the kernel.
 *   delta_ms   (N) double: the clip's frame period.
 *   present    (N) int: 1 when the sequence was matched (the clip stops at that frame, as the host's loop does), else 0.
 *   status     (N) int: 0, or 1 when the smoothing window would have held more than HOWL_DECIDE_RING_FRAMES frames: the clip
 *              stops there and its other results are not to be used (callers replay such a clip on the host).
 *   n_labels   (N) int: entries appended to the clip's history.
 *   first_kept (N) int: entries [first_kept, n_labels) are the history the matcher's window has left.
 *   end_time   (N) double: the clip's time behind its last frame.
 *   hist_time, hist_label  entry k of clip n at [n * hist_ld + k], k < n_labels[n]; hist_ld >= T_max.  Nothing behind
 *              n_labels[n] is touched.  The caller provides them in full: 12 bytes x N x hist_ld, i.e. 805 MB at N = T_max = 8192 --
 *              the limits bound each dimension, a caller short of memory passes its clips in groups.
 *   weighted   NULL, or (N, T_max, C) floats: the reweighted, renormalised probabilities of every frame the clip looked at.
 */
int howl_decide_clips(const HowlDecideConfig* cfg, const float* probs, long s_clip, long s_frame, int N, int T_max,
                      const int* n_frames, const double* delta_ms, int* present, int* status, int* n_labels, int* first_kept,
                      double* end_time, double* hist_time, int* hist_label, long hist_ld, float* weighted, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
