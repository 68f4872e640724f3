/* howl_hip_resample.h -- clips of any sample rate: what librosa.core.load(path, sr=16000, mono=True) does to a file
 * (howl/utils/audio_utils.py:23, howl/data/dataset/dataset.py) on the device.  B independent, ragged clips of raw interleaved
 * samples are averaged to mono and resampled by a band-limited polyphase FIR in ONE launch, written straight into a clip bank.
 *
 * The filter is this project's own: a Kaiser-windowed sinc with the constants resampy documents for `kaiser_best`, the window
 * evaluated exactly (no interpolated table).  Bit parity with librosa's resampler (resampy or soxr, by version) is NOT claimed.
 *
 *   sr_in -> sr_out,  U / D = sr_out / sr_in reduced,  s = min(1, U / D),  M = max(U, D)
 *   Z = 64 zero crossings,  rolloff = 0.9475937167399596,  beta = 14.769656459379492
 *   h(t)    = rolloff sinc(rolloff t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta)   for |t| < Z, else 0     (sinc(x) = sin(pi x) / (pi x))
 *   c[p][j] = s h(s (p/U - j)) = s h((p - j U) / M)      p = (n D) mod U the phase of output n,  j = k - floor(n D / U) the tap
 *                                                        offset of input frame k;  |t| < Z is decided in integers: |p - j U| < Z M
 *   x[k]    = (((v[k][0] + v[k][1]) + ...) + v[k][C-1]) / C in float32, channel order; int16 samples are v / 32768 (exact);
 *             one channel: x[k] = v[k][0];  x[k] = 0 outside [0, len)
 *   out[n]  = sum_k c[p][j] x[k]      for n < out_len <= ceil(len U / D)      (integer arithmetic; the full length is librosa's)
 * The sum of one output runs over its whole bank row in a fixed order in float32, so a clip's bits depend on nothing but the clip.
 *
 * The bank: c is computed on the host in float64 and rounded once to float32, as [U][taps] floats with c[p][j] at
 * bank[p * taps + (j - j_lo)]; taps = j_hi - j_lo + 1 rounded up to a multiple of 4, the padding and every |t| >= Z entry exactly 0.
 * U = D = 1 is the identity filter: j_lo = j_hi = 0 and one tap of 1.0 (the row is {1, 0, 0, 0}).
 *
 * Supported: sr_in and sr_out in 4000 .. 192000 with reduced U <= 640 and D <= 16 U (8000, 11025, 12000, 22050, 24000, 32000,
 * 44100, 48000, 88200, 96000 -> 16000 among them).
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no allocation,
 * no synchronisation; every refusal happens before the launch).  No workspace.
 */
#ifndef HOWL_HIP_RESAMPLE_H
#define HOWL_HIP_RESAMPLE_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_RESAMPLE_MAX_CLIPS 8192
#define HOWL_RESAMPLE_MAX_FRAMES 16777216     /* input frames of one clip */
#define HOWL_RESAMPLE_MAX_CHANNELS 8
#define HOWL_RESAMPLE_MIN_RATE 4000
#define HOWL_RESAMPLE_MAX_RATE 192000
#define HOWL_RESAMPLE_MAX_UP 640
#define HOWL_RESAMPLE_MAX_DECIMATION 16
#define HOWL_RESAMPLE_ZEROS 64
/* sample formats (interleaved) */
#define HOWL_RESAMPLE_F32 0
#define HOWL_RESAMPLE_I16 1

/* What a rate pair fixes.  40 bytes. */
typedef struct {
    int sr_in, sr_out;
    int up, down;        /* U, D */
    int taps;            /* row width of the bank, a multiple of 4 */
    int j_lo, j_hi;      /* tap offsets with a non-zero coefficient in some phase: j_lo <= j <= j_hi */
    int reserved;        /* 0 */
    double s;            /* min(1, U / D) */
} HowlResamplePlan;

/* One clip.  The same 24-byte record is read on the host (to refuse) and on the device (to run). */
typedef struct {
    long long src_off;   /* the clip's first FRAME in src: its samples are src[(src_off + k) * channels + ch] */
    long long dst_off;   /* the resampled clip is out[dst_off .. dst_off + out_len) */
    int len;             /* input frames */
    int out_len;         /* outputs written: 0 .. ceil(len U / D); fewer than the full length truncates (truncate_length) */
} HowlResampleClip;

/* HOST only.  Fills *plan for sr_in -> sr_out; refuses a pair outside the supported range with a message that names it. */
int howl_resample_plan(int sr_in, int sr_out, HowlResamplePlan* plan);
/* HOST only.  up * taps, the floats of the plan's bank (0 for a plan howl_resample_plan did not make). */
size_t howl_resample_bank_floats(const HowlResamplePlan* plan);
/* HOST only.  Writes the bank's howl_resample_bank_floats(plan) floats to HOST memory. */
int howl_resample_bank(const HowlResamplePlan* plan, float* bank_host);
/* HOST only.  ceil(len * up / down), the full output length of a clip of len frames (0 for len < 0 or a foreign plan). */
size_t howl_resample_out_len(const HowlResamplePlan* plan, long len);

/* ONE launch for B ragged clips: a workgroup per (clip, tile of 256 consecutive outputs).
 *   src, src_elems               the raw samples and their count in ELEMENTS (frames * channels), for the bounds check of every clip
 *   format, channels             HOWL_RESAMPLE_F32 or HOWL_RESAMPLE_I16, interleaved, 1 .. 8 channels
 *   bank_dev, bank_floats        DEVICE, the plan's bank (howl_resample_bank, uploaded by the caller) and its size
 *   plan                         HOST
 *   clips_host                   HOST, B records: validated here, before the launch
 *   clips_dev                    DEVICE, the same B records: what the kernel reads.  Contract: the bytes of clips_host by the time the
 *                                kernel runs (the caller's copy on `stream`, in front of this call)
 *   out, out_floats              flat destination; dst_off is free, so a dense row (dst_off = i * max_len, out_len capped at max_len)
 *                                and a ragged flat bank are the same call.  Clips may not overlap (not checked).  Nothing outside
 *                                [dst_off, dst_off + out_len) is written.
 * Refused: a plan that is not howl_resample_plan's for its pair, bank_floats != up * taps, a format or channel count outside the
 * above, B outside 1 .. 8192, a clip of fewer than 1 or more than HOWL_RESAMPLE_MAX_FRAMES frames, out_len outside 0 .. the full
 * length, a source or destination range outside its buffer. */
int howl_resample_clips(const void* src, long src_elems, int format, int channels, const float* bank_dev, long bank_floats,
                        const HowlResamplePlan* plan, const HowlResampleClip* clips_host, const HowlResampleClip* clips_dev, int B,
                        float* out, long out_floats, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
