/* howl_hip_las.h -- the "las" classifier (howl/model/rnn.py:133-215, LASClassifier) as one call per direction:
 *   Conv2d(3,8,3,padding=2) - BatchNorm2d(8) - ReLU - MaxPool(1,2) - Conv2d(8,8,3,padding=2) - BatchNorm2d(8) - ReLU - MaxPool(1,2)
 *   - bidirectional LSTM(352 -> 96), packed - FixedAttentionModule (4 heads over 192 columns) - Linear(192,256) - ReLU - Dropout
 *   - Linear(256, num_labels).
 *
 * x: element (b, channel, mel, t) at x[b*sb + channel*sc + mel*sm + t*st], the three ZMUV-normalised feature channels.  The whole
 * buffer goes through the encoder, padded frames included (they count in the BatchNorm statistics, as in the reference);
 * `lengths` (B, int64, NULL = T for all) only decides how many recurrence steps utterance b runs and the attention sees:
 * n_b = (((len_b + 2) / 2) + 2) / 2, at most T2 = (((T + 2) / 2) + 2) / 2.  The forward direction runs steps 0 .. n_b-1, the
 * reverse direction starts from zero state at step n_b-1.  The attention's softmax runs over the n_b steps of the utterance only
 * (the reference keeps the batch's padded steps with an additive -100: a weight of at most e^-100, which vanishes in fp32), so an
 * utterance's result never depends on its batch neighbours.  Nothing is written to `lengths`.
 *
 * training != 0: batch statistics (biased variance to normalise; the running buffers are updated with momentum 0.1 and the
 * unbiased variance, num_batches_tracked += 1) and, when drop_mask (B, 256 of 0/1) is given, y1 * mask * keep_scale between the
 * head's ReLU and its second layer; everything howl_las_bwd needs stays in `ws`, which must reach that call untouched.
 * training == 0: running statistics; drop_mask must be NULL.
 *
 * howl_las_bwd: dlogits (B, num_labels) -> every entry of `grads` written (no input gradient).  conv1_b, conv2_b (each in front of
 * a batch-statistics BatchNorm) and v_b (a constant under the softmax over time) have identically zero gradients and get exact
 * zeros.  Fixed-order sums everywhere: repeated calls are bit-identical.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names the entry point: null pointers, M != 40,
 * T outside 1..HOWL_LAS_MAX_FRAMES, B < 1, num_labels outside 1..HOWL_LAS_MAX_LABELS, a short workspace (HOWL_E_WORKSPACE).
 */
#ifndef HOWL_HIP_LAS_H
#define HOWL_HIP_LAS_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_LAS_MAX_FRAMES 8192
#define HOWL_LAS_MAX_LABELS 64

typedef struct {
    const float* conv1_w; /* encoder.conv1.weight = encoder.conv_encoder.0.weight (8,3,3,3) */
    const float* conv1_b; /* encoder.conv1.bias (8) */
    const float* conv2_w; /* encoder.conv2.weight = encoder.conv_encoder.4.weight (8,8,3,3) */
    const float* conv2_b; /* encoder.conv2.bias (8) */
    const float* bn1_w;   /* encoder.conv_encoder.1.weight (8) */
    const float* bn1_b;   /* encoder.conv_encoder.1.bias (8) */
    const float* bn2_w;   /* encoder.conv_encoder.5.weight (8) */
    const float* bn2_b;   /* encoder.conv_encoder.5.bias (8) */
    const float* w_ih_f;  /* encoder.lstm_encoder.weight_ih_l0 (384,352), rows i | f | g | o */
    const float* w_hh_f;  /* encoder.lstm_encoder.weight_hh_l0 (384,96) */
    const float* b_ih_f;  /* encoder.lstm_encoder.bias_ih_l0 (384) */
    const float* b_hh_f;  /* encoder.lstm_encoder.bias_hh_l0 (384) */
    const float* w_ih_r;  /* encoder.lstm_encoder.weight_ih_l0_reverse (384,352) */
    const float* w_hh_r;  /* encoder.lstm_encoder.weight_hh_l0_reverse (384,96) */
    const float* b_ih_r;  /* encoder.lstm_encoder.bias_ih_l0_reverse (384) */
    const float* b_hh_r;  /* encoder.lstm_encoder.bias_hh_l0_reverse (384) */
    const float* cv;      /* attn.context_vec (192): element l of head k at 4 l + k */
    const float* v_w;     /* attn.v_proj.weight (192,192): the scores' projection */
    const float* v_b;     /* attn.v_proj.bias (192) */
    const float* k_w;     /* attn.k_proj.weight (192,192): what the scores weigh */
    const float* k_b;     /* attn.k_proj.bias (192) */
    const float* w1;      /* fc.0.weight (256,192) */
    const float* b1;      /* fc.0.bias (256) */
    const float* w2;      /* fc.3.weight (num_labels,256) */
    const float* b2;      /* fc.3.bias (num_labels) */
} HowlLasParams;

/* the same twenty-five tensors, in the same order */
typedef struct {
    float *conv1_w, *conv1_b, *conv2_w, *conv2_b, *bn1_w, *bn1_b, *bn2_w, *bn2_b, *w_ih_f, *w_hh_f, *b_ih_f, *b_hh_f, *w_ih_r, *w_hh_r,
        *b_ih_r, *b_hh_r, *cv, *v_w, *v_b, *k_w, *k_b, *w1, *b1, *w2, *b2;
} HowlLasGrads;

/* BatchNorm buffers, updated in place when training */
typedef struct {
    float* bn1_mean;        /* encoder.conv_encoder.1.running_mean (8) */
    float* bn1_var;         /* encoder.conv_encoder.1.running_var (8) */
    long long* bn1_batches; /* encoder.conv_encoder.1.num_batches_tracked (1) */
    float* bn2_mean;        /* encoder.conv_encoder.5.running_mean (8) */
    float* bn2_var;         /* encoder.conv_encoder.5.running_var (8) */
    long long* bn2_batches; /* encoder.conv_encoder.5.num_batches_tracked (1) */
} HowlLasBuffers;

/* 1 when B >= 1, M == 40, 1 <= T <= 8192 and 1 <= num_labels <= 64, else 0. */
int howl_las_supported(int B, int M, int T, int num_labels);
/* Bytes of `ws` for problem (B, T): saved activations, gradients in flight and partial sums (0 outside the range). */
size_t howl_las_workspace_bytes(int B, int T);
int howl_las_fwd(const HowlLasParams* p, const HowlLasBuffers* buffers, const float* x, long sb, long sc, long sm, long st, int B,
                 int M, int T, int num_labels, const long long* lengths, int training, const float* drop_mask, float keep_scale,
                 float* logits, void* ws, size_t ws_bytes, hipStream_t stream);
int howl_las_bwd(const HowlLasParams* p, const float* x, long sb, long sc, long sm, long st, int B, int M, int T, int num_labels,
                 const long long* lengths, float keep_scale, const float* dlogits, const HowlLasGrads* grads, void* ws,
                 size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
