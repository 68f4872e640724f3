// The engines' decision logic on the device (include/howl_hip_decide.h): ONE launch from the per-frame class probabilities of N
// clips to each clip's detection flag and label history.  Replaces the host loops InferenceEngine._run_frames /
// FrameInferenceEngine._run_fsm over ProbabilitySmoother.push and SequenceMatcher.present (howl_amd/model/inference.py,
// decision.py) for a dataset pass, with the host's arithmetic operation for operation: same flags, same labels, same fp64 stamps.
//
// One wavefront per clip, four waves per workgroup; lane c holds class c.  Nothing is shared between clips (the workgroup's only
// barrier stands behind the copy of the sequence into LDS), so there is no counter, flag or spin loop.  Every scalar of a clip's
// state (time, ring head, history counts, the matcher's state) is computed by all 64 lanes alike: the control flow is
// wave-uniform throughout, and the cross-lane operations (shuffles, ballot) are never under a divergent branch.
//
// Per frame:
//   1. w_c = (float)((double)p_c * weights[c]); s = sum_c w_c in NumPy's pairwise order for n <= 128 (below eight elements left to
//      right; from eight on eight strided accumulators r[j] = a[j] + a[8 + j] + ..., folded ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
//      the last C mod 8 elements added one by one): lanes 0..7 gather their accumulator with C/8 - 1 shuffles, a three-stage
//      butterfly folds them (x + y == y + x bit for bit, so every lane of the eight holds the fold), <= 7 serial adds; q_c = w_c / s,
//      correctly rounded (the compiler's default for `/`; no fast-math flag in the build).
//   2. first-maximum arg-max = wave max (six butterfly stages) + ballot of the lanes that hold it + count of trailing zeros.
//   3. the smoothing ring: DC_RING frames x 64 classes per wave in LDS, lane c reads and writes column c only; the stamps beside it.
//   4. the history: appended to the caller's arrays by lane 0 and mirrored in an LDS tail of the DC_TAIL latest entries, from which
//      the matcher reads (all lanes the same address: a broadcast).  Entries older than the tail -- a matcher window of more than
//      DC_TAIL frames -- are read back from the caller's arrays: stores and loads of one wavefront are performed in order.
//   5. the matcher: its (matched, anchor, holding) state is carried from frame to frame and the scan continues at the new entry
//      while the window drops nothing (the fold over an unchanged prefix is the same state); a drop rescans from first_kept.
//
// LDS (static): ring 4 x 32 x 64 x 4 = 32,768; ring stamps 1,024; history tail 4 x 256 x 12 = 12,288; sequence 64: 46,144 bytes.
#include "howl_common.hip.h"
#include "../../include/howl_hip_decide.h"

// the host multiplies, adds and compares as separate operations: no multiply-add contraction anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int DC_WAVES = 4;
constexpr int DC_THREADS = 64 * DC_WAVES;
constexpr int DC_RING = HOWL_DECIDE_RING_FRAMES;
constexpr int DC_TAIL = 256;               // latest history entries mirrored in LDS (a power of two)
static_assert((DC_RING & (DC_RING - 1)) == 0 && (DC_TAIL & (DC_TAIL - 1)) == 0, "ring indices are masked");

struct DcArgs {
    int mode, C, blank, negative;
    float threshold;
    double smoothing_ms, window_ms, tolerance_ms;
    int seq_len;
    int sequence[HOWL_DECIDE_MAX_SEQUENCE];
    const double* weights;
    const int* color;
    const float* probs;
    long s_clip, s_frame;
    int N, T_max;
    const int* n_frames;
    const double* delta_ms;
    int *present, *status, *n_labels, *first_kept;
    double *end_time, *hist_time;
    int* hist_label;
    long hist_ld;
    float* weighted;
};

// first-maximum arg-max over the lanes (lanes behind C hold -inf) -> (index, maximum), the same in every lane
__device__ __forceinline__ int wave_argmax(float v, float& vmax) {
    float m = v;
    for (int s = 32; s >= 1; s >>= 1) {
        const float o = __shfl_xor(m, s);
        m = o > m ? o : m;
    }
    const unsigned long long holders = __ballot(v == m);
    vmax = m;
    return holders != 0ull ? __builtin_ctzll(holders) : 0;
}

__global__ __launch_bounds__(DC_THREADS) void decide_kernel(DcArgs a) {
    __shared__ float ring_q[DC_WAVES][DC_RING][HOWL_DECIDE_MAX_CLASSES];
    __shared__ double ring_t[DC_WAVES][DC_RING];
    __shared__ double tail_t[DC_WAVES][DC_TAIL];
    __shared__ int tail_l[DC_WAVES][DC_TAIL];
    __shared__ int seq[HOWL_DECIDE_MAX_SEQUENCE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < HOWL_DECIDE_MAX_SEQUENCE) seq[tid] = a.sequence[tid];
    __syncthreads();
    const int n = blockIdx.x * DC_WAVES + wv;
    if (n >= a.N) return;                         // (wave-uniform; no barrier follows)

    const int C = a.C;
    const bool mine = lane < C;
    int nf = a.n_frames[n];
    nf = nf < 0 ? 0 : (nf > a.T_max ? a.T_max : nf);
    const double delta = a.delta_ms[n];
    const double wt = (a.weights != nullptr && mine) ? a.weights[lane] : 1.0;
    const int colour = (a.color != nullptr && mine) ? a.color[lane] : -1;      // lane c holds the map's entry for label c
    const float* const prow = a.probs + (size_t)n * a.s_clip;
    double* const htime = a.hist_time + (size_t)n * a.hist_ld;
    int* const hlabel = a.hist_label + (size_t)n * a.hist_ld;
    float(*const rq)[HOWL_DECIDE_MAX_CLASSES] = ring_q[wv];
    double* const rt = ring_t[wv];
    double* const tt = tail_t[wv];
    int* const tl = tail_l[wv];
    const float NEG_INF = -__builtin_inff();

    double cur = 0.0;
    int head = 0, cnt = 0;                        // the smoothing ring: oldest slot, frames held
    int nl = 0, fk = 0;                           // history entries appended, first entry the matcher's window has kept
    int matched = 0, holding = 0, scanned = 0;    // the matcher's state behind entries [fk, scanned)
    bool has_hold = false;
    double anchor = 0.0;
    int found = 0, overflow = 0;

    float pnext = (mine && nf > 0) ? prow[lane] : 0.0f;
    for (int t = 0; t < nf; ++t) {
        const float p = pnext;
        if (mine && t + 1 < nf) pnext = prow[(size_t)(t + 1) * a.s_frame + lane];      // in flight while this frame is decided
        // 1. reweighting and renormalisation
        const float w = a.weights != nullptr ? (float)((double)p * wt) : p;
        float s;
        if (C < 8) {
            s = __shfl(w, 0);
            for (int j = 1; j < C; ++j) s += __shfl(w, j);
        } else {
            const int nb = C >> 3;
            float r = w;
            for (int b = 1; b < nb; ++b) r += __shfl(w, 8 * b + (lane & 7));
            r += __shfl_xor(r, 1);
            r += __shfl_xor(r, 2);
            r += __shfl_xor(r, 4);
            s = __shfl(r, 0);
            for (int j = 8 * nb; j < C; ++j) s += __shfl(w, j);
        }
        const float q = w / s;
        if (a.weighted != nullptr && mine) a.weighted[((size_t)n * a.T_max + t) * C + lane] = q;
        const float qm = mine ? q : NEG_INF;
        // 2. time, blank skip
        double now;
        if (a.mode == 0) {
            cur += delta;
            float top;
            if (wave_argmax(qm, top) == a.blank) continue;
            now = cur;
        } else {
            now = cur;
        }
        // 3. smoother: the frames of the last smoothing_ms, per-class maximum, threshold, colouring
        while (cnt > 0 && now - rt[head] > a.smoothing_ms) {
            head = (head + 1) & (DC_RING - 1);
            --cnt;
        }
        if (cnt == DC_RING) {
            overflow = 1;
            break;
        }
        const int slot = (head + cnt) & (DC_RING - 1);
        rq[slot][lane] = qm;
        if (lane == 0) rt[slot] = now;
        ++cnt;
        float env = qm;
        for (int k = 0; k + 1 < cnt; ++k) {
            const float v = rq[(head + k) & (DC_RING - 1)][lane];
            env = v > env ? v : env;
        }
        float top;
        int label = wave_argmax(env, top);
        const bool confident = top >= a.threshold;
        if (a.color != nullptr) {
            const int mapped = __shfl(colour, label);
            label = mapped >= 0 ? mapped : a.negative;
        }
        if (!confident) label = a.negative;
        // 4. history
        if (lane == 0) {
            htime[nl] = now;
            hlabel[nl] = label;
            tt[nl & (DC_TAIL - 1)] = now;
            tl[nl & (DC_TAIL - 1)] = label;
        }
        ++nl;
        wave_lds_sync();                          // lane 0's stamp and tail entry, for every lane
        if (a.mode != 0) cur += delta;
        // 5. matcher at time cur
        if (a.seq_len == 0) continue;
        // (entries behind the LDS tail and entries in it are walked by loops of their own: one loop choosing between the two per entry
        // is compiled to a flat load behind a selected pointer, with a wait for every outstanding store in front of each step)
        const int fk0 = fk;
        const int tail0 = nl - DC_TAIL;           // first entry the tail mirrors
        while (fk < tail0 && cur - htime[fk] > a.window_ms) ++fk;
        if (fk >= tail0)
            while (fk < nl && cur - tt[fk & (DC_TAIL - 1)] > a.window_ms) ++fk;
        if (fk != fk0) {
            matched = 0, anchor = 0.0, has_hold = false, scanned = fk;
        }
        auto step = [&](double stamp, int lb) {      // SequenceMatcher.present's three-way branch on one entry
            if (lb == seq[matched]) {
                if (++matched == a.seq_len) {
                    found = 1;
                    return;
                }
                holding = lb, has_hold = true, anchor = stamp;
            } else if (has_hold && lb == holding) {
                anchor = stamp;
            } else if (anchor + a.tolerance_ms < stamp) {
                matched = 0, anchor = 0.0, has_hold = false;
            }
        };
        for (; !found && scanned < tail0; ++scanned) step(htime[scanned], hlabel[scanned]);
        for (; !found && scanned < nl; ++scanned) step(tt[scanned & (DC_TAIL - 1)], tl[scanned & (DC_TAIL - 1)]);
        if (found) break;
    }
    if (lane == 0) {
        a.present[n] = found;
        a.status[n] = overflow;
        a.n_labels[n] = nl;
        a.first_kept[n] = fk;
        a.end_time[n] = cur;
    }
}

bool dc_supported(const HowlDecideConfig* cfg, int T_max) {
    if (cfg == nullptr) return false;
    if (cfg->mode != 0 && cfg->mode != 1) return false;
    if (cfg->C < 1 || cfg->C > HOWL_DECIDE_MAX_CLASSES) return false;
    if (cfg->seq_len < 0 || cfg->seq_len > HOWL_DECIDE_MAX_SEQUENCE) return false;
    if (T_max < 0 || T_max > HOWL_DECIDE_MAX_FRAMES) return false;
    // a smoothing window that is negative drops the frame it has just taken (the host fails there), one that is not finite never
    // drops anything: neither can be held in the ring.  A NaN anywhere else has no host behaviour worth reproducing either.
    if (!(cfg->smoothing_ms >= 0.0) || !std::isfinite(cfg->smoothing_ms)) return false;
    if (std::isnan(cfg->threshold) || std::isnan(cfg->window_ms) || std::isnan(cfg->tolerance_ms)) return false;
    return true;
}

}  // namespace

extern "C" {

int howl_decide_supported(const HowlDecideConfig* cfg, int T_max) { return dc_supported(cfg, T_max) ? 1 : 0; }

int howl_decide_clips(const HowlDecideConfig* cfg, const float* probs, long s_clip, long s_frame, int N, int T_max,
                      const int* n_frames, const double* delta_ms, int* present, int* status, int* n_labels, int* first_kept,
                      double* end_time, double* hist_time, int* hist_label, long hist_ld, float* weighted, hipStream_t stream) {
    HOWL_REQUIRE(cfg && probs && n_frames && delta_ms && present && status && n_labels && first_kept && end_time && hist_time && hist_label,
                 "howl_decide_clips: null pointer");
    HOWL_REQUIRE(cfg->mode == 0 || cfg->mode == 1, "howl_decide_clips: mode=%d unsupported (0: sequence engine, 1: frame engine)", cfg->mode);
    HOWL_REQUIRE(cfg->C >= 1 && cfg->C <= HOWL_DECIDE_MAX_CLASSES, "howl_decide_clips: C=%d classes unsupported (1..%d)", cfg->C,
                 HOWL_DECIDE_MAX_CLASSES);
    HOWL_REQUIRE(cfg->seq_len >= 0 && cfg->seq_len <= HOWL_DECIDE_MAX_SEQUENCE, "howl_decide_clips: seq_len=%d unsupported (0..%d)",
                 cfg->seq_len, HOWL_DECIDE_MAX_SEQUENCE);
    HOWL_REQUIRE(T_max >= 0 && T_max <= HOWL_DECIDE_MAX_FRAMES, "howl_decide_clips: T_max=%d frames unsupported (0..%d)", T_max,
                 HOWL_DECIDE_MAX_FRAMES);
    HOWL_REQUIRE(N >= 1 && N <= HOWL_DECIDE_MAX_CLIPS, "howl_decide_clips: N=%d clips unsupported (1..%d)", N, HOWL_DECIDE_MAX_CLIPS);
    HOWL_REQUIRE(dc_supported(cfg, T_max),
                 "howl_decide_clips: smoothing_ms=%g, threshold=%g, window_ms=%g, tolerance_ms=%g unsupported (a finite smoothing window "
                 ">= 0, no NaN: howl_decide_supported)", cfg->smoothing_ms, cfg->threshold, cfg->window_ms, cfg->tolerance_ms);
    HOWL_REQUIRE(s_clip >= 0 && s_frame >= 0, "howl_decide_clips: negative stride (s_clip=%ld, s_frame=%ld)", s_clip, s_frame);
    HOWL_REQUIRE(hist_ld >= T_max, "howl_decide_clips: hist_ld=%ld entries per clip, a clip may append %d", hist_ld, T_max);
    DcArgs a;
    a.mode = cfg->mode, a.C = cfg->C, a.blank = cfg->blank, a.negative = cfg->negative;
    a.threshold = (float)cfg->threshold;
    a.smoothing_ms = cfg->smoothing_ms, a.window_ms = cfg->window_ms, a.tolerance_ms = cfg->tolerance_ms;
    a.seq_len = cfg->seq_len;
    for (int i = 0; i < HOWL_DECIDE_MAX_SEQUENCE; ++i) a.sequence[i] = i < cfg->seq_len ? cfg->sequence[i] : 0;
    a.weights = cfg->weights, a.color = cfg->color;
    a.probs = probs, a.s_clip = s_clip, a.s_frame = s_frame, a.N = N, a.T_max = T_max;
    a.n_frames = n_frames, a.delta_ms = delta_ms;
    a.present = present, a.status = status, a.n_labels = n_labels, a.first_kept = first_kept;
    a.end_time = end_time, a.hist_time = hist_time, a.hist_label = hist_label, a.hist_ld = hist_ld, a.weighted = weighted;
    hipLaunchKernelGGL(decide_kernel, dim3((unsigned)((N + DC_WAVES - 1) / DC_WAVES)), dim3(DC_THREADS), 0, stream, a);
    HOWL_CHECK_LAUNCH("howl_decide_clips");
    return HOWL_OK;
}

}  // extern "C"
