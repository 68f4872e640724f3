// Streaming seq-lstm / lstm (include/howl_hip_lstm_stream.h): ONE launch from N independent PCM chunks to their per-frame class
// probabilities and the carried (h, c), four streams per workgroup, no activation ever leaves the compute unit.  Replaces, for
// InferenceEngine.infer's chunk (inference.py:179-211) and a dataset pass of the CTC objective, the chain howl_logmel_fwd ->
// howl_lstm_fwd -> howl_head_fwd -> softmax: four launches, the backward's saved activations (gates (T,512), c, hseq) stored for
// nobody, y1 through HBM.
//
// Workgroup g = streams 4g .. 4g+3 with lstm_fwd4_kernel's mapping (block row of v_mfma_f32_4x4x1 = stream, wave c = hidden units
// 16c .. 16c+15 x four gates); rows past N are copies of the last stream, so no store of the step is conditional.  Workgroup
// barriers only: nothing is shared between workgroups, so there is no counter, flag or spin loop.  The time axis is walked in
// windows of W = 16 frames:
//   1. log-mel + ZMUV of frames [t0, t0 + W) of each (real) stream: logmel_body<8, NG_BANDED> called once per stream with that
//      stream's own L and T (reflect padding at the chunk's true ends only), the window selected as share `w` of `windows` equal
//      shares of the quads, the output pointed at the LDS feature tile.  logmel_body itself is untouched.
//   2. W recurrence steps, arithmetic and operation order of lstm_fwd4_kernel<40>: x_t from the feature tile (times W_ih inside the
//      step), h_{t-1} double-buffered in LDS, one barrier per step, a live mask t < frames[n] per stream; h_t rows into an LDS
//      tile.  No gates / c / hseq stores.
//   3. head on the window's rows, one stream (a 16-row MFMA tile) at a time: y1 = relu(h W1^T + b1) on v_mfma_f32_16x16x4_f32 with
//      W1 stationary in registers (wave c = columns 32c .. 32c+31, 64 registers, loaded once per window) -> LDS; y2 = y1 W2^T + b2
//      as vector work (eight lanes per (row, class), fixed fold order); max-subtracted softmax; stores.
// Weights are loaded at the start of the phase that uses them, per window (W_hh 256 KB + W_ih 80 KB + W1 128 KB per workgroup and
// window, from L2): 128 + 40 recurrence registers, the frontend's working set and the head's 64 are never live together.
//
// LDS plan (bytes).  Static: logmel_body<8> 98,048 (74,752 transpose tiles + 5,888 tables + 17,408 filterbank fragments).
// Dynamic, W = 16:   hbuf  [2][4][132]        4,224     h_{t-1} / h_t
//                    hrow  [4][W][132]       33,792     the window's h_t rows (A operand of the head)
//                    feat  [4][W][44]        11,264     the window's features; dead after the recurrence, so the head's
//                    y1 [16][260] + logits [16][64] = 20,736 lie over it
// = 58,752 dynamic, 156,800 of 163,840 in all.  W = 20 would need 67,200 dynamic and break the one-stream-per-16-row-tile head;
// W = 12 leaves a quarter of every MFMA tile empty: W = 16.
#include "howl_logmel.hip.h"
#include "howl_lstm.hip.h"
#include "../../include/howl_hip_lstm_stream.h"

namespace {

constexpr int LS_HID = 128;
constexpr int LS_MELS = 40;
constexpr int LS_NHID = 256;             // the head's hidden width (2 x hidden size, rnn.py:44-48)
constexpr int LS_THREADS = 512;
constexpr int LS_W = 16;                 // frames per window
constexpr int LS_HS = LS_HID + 4;        // h rows in LDS (16-byte aligned rows for the float4 A-fragment reads)
constexpr int LS_FP = LS_MELS + 4;       // feature rows
constexpr int LS_YS = LS_NHID + 4;       // y1 rows
constexpr int LS_HBUF = 0;
constexpr int LS_HROW = LS_HBUF + 2 * 4 * LS_HS;
constexpr int LS_FEAT = LS_HROW + 4 * LS_W * LS_HS;
constexpr int LS_FEAT_FLOATS = 4 * LS_W * LS_FP;
constexpr int LS_HEAD_FLOATS = 16 * LS_YS + 16 * HOWL_LSTM_STREAM_MAX_CLASSES;
constexpr int LS_LDS_FLOATS = LS_FEAT + (LS_FEAT_FLOATS > LS_HEAD_FLOATS ? LS_FEAT_FLOATS : LS_HEAD_FLOATS);
constexpr int LS_MIN_SAMPLES = 400;
static_assert(LS_W % QUAD == 0 && LS_W == 16, "a window is whole quads of the frontend and one 16-row tile of the head per stream");

struct LsArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh, *w1, *b1, *w2, *b2;
    const float* pcm;
    long ld;
    int N, L_max;
    const long long *n_samples, *frames;
    const float* fbp;
    float log_eps;
    const float* zmuv;
    float *h, *c;
    int C, last_only;
    float *probs, *logits;
    long out_ld;
};

__global__ __launch_bounds__(LS_THREADS) void lstm_stream_kernel(LsArgs a) {
    HIP_DYNAMIC_SHARED(float, lds)
    float* const hbuf = lds + LS_HBUF;
    float* const hrow = lds + LS_HROW;
    float* const feat = lds + LS_FEAT;
    float* const y1t = feat;                       // the head's tiles lie over the features (dead after the recurrence)
    float* const lgt = y1t + 16 * LS_YS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 2, g = lane & 3;
    const int u = 16 * wv + j;                     // hidden unit of this lane's quad
    const int col = g * LS_HID + u;                // MFMA role: its gate column in PyTorch order (i, f, g, o)
    const int s0 = blockIdx.x * 4;
    const int nreal = min(4, a.N - s0);            // streams of this workgroup that exist
    const int C = a.C;
    const int T_max = 1 + a.L_max / HOP;

    // samples, frames of the chunk, frames to run: every value clamped into its contract (workgroup-uniform for a uniform s)
    auto geom = [&](int n, int& L, int& T, int& fr) {
        long long ns = a.n_samples != nullptr ? a.n_samples[n] : (long long)a.L_max;
        ns = ns < LS_MIN_SAMPLES ? LS_MIN_SAMPLES : (ns > a.L_max ? a.L_max : ns);
        L = (int)ns;
        T = 1 + L / HOP;
        long long f = a.frames != nullptr ? a.frames[n] : (long long)T;
        fr = (int)(f < 1 ? 1 : (f > T ? T : f));
    };
    int maxfr = 0;
    for (int s = 0; s < nreal; ++s) {
        int L, T, fr;
        geom(s0 + s, L, T, fr);
        maxfr = max(maxfr, fr);
    }
    maxfr = __builtin_amdgcn_readfirstlane(maxfr);

    // everything a later stage may read without having written it (features of frames nobody computes, the head's unused rows) is
    // finite: zero
    for (int i = tid; i < LS_LDS_FLOATS / 4; i += LS_THREADS) reinterpret_cast<float4*>(lds)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();

    // cell role: stream g of the workgroup (a copy of the last real one behind N), unit u
    const int bc = min(s0 + g, a.N - 1);
    float cst = a.c != nullptr ? a.c[(size_t)bc * LS_HID + u] : 0.0f;
    float hst = a.h != nullptr ? a.h[(size_t)bc * LS_HID + u] : 0.0f;
    int len;
    {
        int L, T;
        geom(bc, L, T, len);
    }
    hbuf[g * LS_HS + u] = hst;
    const int xrow = min(g, nreal - 1);            // feature rows exist for the real streams only
    const int jx = j < LS_MELS / 4 ? j : 0;        // (lanes behind the ten x blocks supply no A operand: any row address will do)
    // sigmoid(x) = 1 / (1 + 2^(-x log2 e)); the cell-candidate gate is tanh(x) = 2 sigmoid(2x) - 1
    const float kneg = g == 2 ? -2.88539008177792681f : -1.44269504088896341f;
    const float amul = g == 2 ? 2.0f : 1.0f, aadd = g == 2 ? -1.0f : 0.0f;

    // ---- the head on one 16-row tile `at` (row pitch LS_HS); dest(row) = float offset of the row in probs / logits or -1.
    // `w1f`: this wave's W1 share, B[k][n] of K index 16 q + 4 k + e in w1f[nt][4 q + e]
    auto head_tile = [&](const float* at, const float (&w1f)[2][32], float b1a, float b1b, auto dest) {
        const int k = lane >> 4, n = lane & 15;
        f32x4 acc[2];
        acc[0] = {0.0f, 0.0f, 0.0f, 0.0f};
        acc[1] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* ap = at + n * LS_HS + 4 * k;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 av = *reinterpret_cast<const float4*>(ap + 16 * q);
            const float ae[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[e], w1f[0][4 * q + e], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[e], w1f[1][4 * q + e], acc[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            y1t[(4 * k + r) * LS_YS + 32 * wv + n] = fmaxf(acc[0][r] + b1a, 0.0f);
            y1t[(4 * k + r) * LS_YS + 32 * wv + 16 + n] = fmaxf(acc[1][r] + b1b, 0.0f);
        }
        __syncthreads();
        // y2[row][cls] = b2[cls] + sum_n y1[row][n] W2[cls][n]: eight lanes per output (n = part + 8 i), folded in a fixed order
        for (int ob = 0; ob < 16 * C; ob += LS_THREADS / 8) {
            const int o = min(ob + (tid >> 3), 16 * C - 1), part = tid & 7;
            const int row = o / C, cls = o - row * C;
            const float* yr = y1t + row * LS_YS + part;
            const float* wr = a.w2 + (size_t)cls * LS_NHID + part;
            float sacc = 0.0f;
#pragma unroll 8
            for (int i = 0; i < LS_NHID / 8; ++i) sacc = fmaf(yr[8 * i], wr[8 * i], sacc);
            sacc += __shfl_xor(sacc, 1);
            sacc += __shfl_xor(sacc, 2);
            sacc += __shfl_xor(sacc, 4);
            if (part == 0) lgt[row * HOWL_LSTM_STREAM_MAX_CLASSES + cls] = sacc + a.b2[cls];
        }
        __syncthreads();
        for (int e = tid; e < 16 * C; e += LS_THREADS) {
            const int row = e / C, cls = e - row * C;
            const long d = dest(row);
            if (d < 0) continue;
            // (every (row, class) folds its row again: C exp per output.  One pass per row through LDS was tried and put 28 bytes of
            // scratch into a kernel that has none at its 256 registers; C is 3..12 for every model of the project)
            const float* lg = lgt + row * HOWL_LSTM_STREAM_MAX_CLASSES;
            float mx = lg[0];
            for (int kk = 1; kk < C; ++kk) mx = fmaxf(mx, lg[kk]);
            float se = 0.0f;
            for (int kk = 0; kk < C; ++kk) se += expf(lg[kk] - mx);
            a.probs[d + cls] = expf(lg[cls] - mx) / se;
            if (a.logits != nullptr) a.logits[d + cls] = lg[cls];
        }
    };
    auto load_w1 = [&](float (&w1f)[2][32], float& b1a, float& b1b) {
        int k4 = 4 * (lane >> 4);
        HOWL_OPAQUE_V(k4);      // per window: hoisted in front of the window loop these 64 registers would be live through every phase
        const int n = lane & 15;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float* wr = a.w1 + (size_t)(32 * wv + 16 * nt + n) * LS_HID + k4;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(wr + 16 * q);
                w1f[nt][4 * q + 0] = v.x;
                w1f[nt][4 * q + 1] = v.y;
                w1f[nt][4 * q + 2] = v.z;
                w1f[nt][4 * q + 3] = v.w;
            }
        }
        b1a = a.b1[32 * wv + n];
        b1b = a.b1[32 * wv + 16 + n];
    };

    const int nwin = (maxfr + LS_W - 1) / LS_W;
#pragma unroll 1
    for (int w = 0; w < nwin; ++w) {
        const int t0 = w * LS_W;
        // ---- 1. features of frames [t0, t0 + W) of every real stream that still runs -> feat[s][t - t0][0:40]
#pragma unroll 1
        for (int s = 0; s < nreal; ++s) {
            int L, T, fr;
            geom(s0 + s, L, T, fr);
            if (t0 >= fr) continue;      // (workgroup-uniform)
            const float* row = a.pcm + (long)(s0 + s) * a.ld;
            const int aligned = (reinterpret_cast<uintptr_t>(row) & 7) == 0 ? 1 : 0;
            const int wins = (fr + LS_W - 1) / LS_W;
            // share w of `wins` equal shares of wins * W / 4 quads = the window's quads; frames >= fr are computed on the chunk's
            // first samples and not stored (total_frames = fr)
            logmel_body<LS_THREADS / 64, NG_BANDED>(row, L, 0, T, fr, a.fbp, LS_MELS, a.log_eps, a.zmuv,
                                                    feat + s * (LS_W * LS_FP) - (long)t0 * LS_FP, 1, wins * (LS_W / QUAD), aligned,
                                                    (unsigned)w, (unsigned)wins, LS_FP);
        }
        __syncthreads();

        // ---- 2. the window's steps (lstm_fwd4_kernel<40>'s step; the weights of this phase from L2)
        {
            int colv = col;
            HOWL_OPAQUE_V(colv);      // per window, as load_w1
            float wB[128];
#pragma unroll
            for (int q = 0; q < 32; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(a.w_hh + (size_t)colv * LS_HID + 4 * q);
                wB[4 * q + 0] = v.x;
                wB[4 * q + 1] = v.y;
                wB[4 * q + 2] = v.z;
                wB[4 * q + 3] = v.w;
            }
            const float bias = a.b_ih[colv] + a.b_hh[colv];
            float wI[LS_MELS];
#pragma unroll
            for (int q = 0; q < LS_MELS / 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(a.w_ih + (size_t)colv * LS_MELS + 4 * q);
                wI[4 * q + 0] = v.x;
                wI[4 * q + 1] = v.y;
                wI[4 * q + 2] = v.z;
                wI[4 * q + 3] = v.w;
            }
            const float* xp = feat + (xrow * LS_W) * LS_FP + 4 * jx;
            float* hr = hrow + (g * LS_W) * LS_HS + u;
            const int nst = min(LS_W, maxfr - t0);
            __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): the fragment loads are not the loop's business (lstm_fwd4_kernel)
            for (int tw = 0; tw < nst; ++tw) {
                const int t = t0 + tw;
                const float* hcur = hbuf + (t & 1) * (4 * LS_HS);
                float* hnxt = hbuf + ((t + 1) & 1) * (4 * LS_HS);
                float pre[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) pre[r] = 0.0f + bias;
                const float4 alo = *reinterpret_cast<const float4*>(hcur + g * LS_HS + 4 * j);
                const float4 ahi = *reinterpret_cast<const float4*>(hcur + g * LS_HS + 64 + 4 * j);
                const float4 ax = *reinterpret_cast<const float4*>(xp + tw * LS_FP);
                f32x4 acc[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = {0.0f, 0.0f, 0.0f, 0.0f};
                bcast_mfma64<0, 0, LS_MELS, LS_MELS / 4>(ax, wI, acc);
                bcast_mfma64<0, 0>(alo, wB, acc);
                bcast_mfma64<0, 64>(ahi, wB, acc);
                const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                float act[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = sum[r] + pre[r];
                    const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kneg * p));
                    act[r] = fmaf(sg, amul, aadd);
                }
                quad_transpose(act, (g & 1) != 0, (g & 2) != 0);        // -> i, f, g, o of (stream g, unit u)
                const bool live = t < len;
                const float cn = act[1] * cst + act[0] * act[2];
                const float hn = act[3] * tanhf_(cn);
                cst = live ? cn : cst;
                hst = live ? hn : hst;
                hnxt[g * LS_HS + u] = hst;
                hr[tw * LS_HS] = hst;      // (last_only never reads the tile; a branch on it here cost ten spilled registers: measured)
                __syncthreads();
            }
        }
        if (a.last_only) continue;

        // ---- 3. head + softmax on the window's rows, stream by stream
        {
            float w1f[2][32], b1a, b1b;
            load_w1(w1f, b1a, b1b);
#pragma unroll 1
            for (int s = 0; s < nreal; ++s) {
                int L, T, fr;
                geom(s0 + s, L, T, fr);
                if (t0 >= fr) continue;      // (workgroup-uniform)
                const long base = (long)(s0 + s) * a.out_ld;
                head_tile(hrow + s * (LS_W * LS_HS), w1f, b1a, b1b,
                          [&](int row) -> long { return t0 + row < fr ? base + (long)(t0 + row) * C : -1L; });
                __syncthreads();      // the next tile's y1 goes over what this one's stores may still be reading
            }
        }
    }

    if (a.last_only) {
        // the head on the final hidden states only: rows 0..3 of one tile = the four streams
        hrow[g * LS_HS + u] = hst;
        __syncthreads();
        float w1f[2][32], b1a, b1b;
        load_w1(w1f, b1a, b1b);
        head_tile(hrow, w1f, b1a, b1b, [&](int row) -> long { return row < nreal ? (long)(s0 + row) * a.out_ld : -1L; });
    } else {
        // rows behind a stream's last frame, up to the launch's T_max: zeros
#pragma unroll 1
        for (int s = 0; s < nreal; ++s) {
            int L, T, fr;
            geom(s0 + s, L, T, fr);
            const long base = (long)(s0 + s) * a.out_ld;
            for (int e = fr * C + tid; e < T_max * C; e += LS_THREADS) {
                a.probs[base + e] = 0.0f;
                if (a.logits != nullptr) a.logits[base + e] = 0.0f;
            }
        }
    }
    if (a.h != nullptr) {
        a.h[(size_t)bc * LS_HID + u] = hst;
        a.c[(size_t)bc * LS_HID + u] = cst;
    }
}

bool ls_supported(int L_max, int M, int C) {
    return M == LS_MELS && C >= 1 && C <= HOWL_LSTM_STREAM_MAX_CLASSES && L_max >= LS_MIN_SAMPLES && L_max <= HOWL_LSTM_STREAM_MAX_SAMPLES;
}

}  // namespace

extern "C" {

int howl_lstm_stream_supported(int L_max, int M, int C) { return ls_supported(L_max, M, C) ? 1 : 0; }

int howl_lstm_stream_chunks(const HowlLstmParams* lstm, const HowlHeadParams* head, const float* pcm, long ld, int N, int L_max,
                            const long long* n_samples, const long long* frames, const float* fbp, int M, float log_eps,
                            const float* zmuv_pair, float* h, float* c, int C, int last_only, float* probs, float* logits,
                            long out_ld, hipStream_t stream) {
    HOWL_REQUIRE(lstm && head && pcm && fbp && probs, "howl_lstm_stream_chunks: null pointer");
    HOWL_REQUIRE(lstm->w_ih && lstm->w_hh && lstm->b_ih && lstm->b_hh, "howl_lstm_stream_chunks: null pointer in HowlLstmParams");
    HOWL_REQUIRE(head->w1 && head->b1 && head->w2 && head->b2, "howl_lstm_stream_chunks: null pointer in HowlHeadParams");
    HOWL_REQUIRE(ls_supported(L_max, M, C),
                 "howl_lstm_stream_chunks: L_max=%d samples, M=%d, C=%d unsupported (M = 40, %d <= L_max <= %d, 1 <= C <= %d: "
                 "howl_lstm_stream_supported)", L_max, M, C, LS_MIN_SAMPLES, HOWL_LSTM_STREAM_MAX_SAMPLES, HOWL_LSTM_STREAM_MAX_CLASSES);
    HOWL_REQUIRE(N >= 1 && N <= HOWL_LSTM_STREAM_MAX_STREAMS, "howl_lstm_stream_chunks: N=%d streams unsupported (1..%d)", N,
                 HOWL_LSTM_STREAM_MAX_STREAMS);
    HOWL_REQUIRE(ld >= 0, "howl_lstm_stream_chunks: negative stream stride %ld", ld);
    HOWL_REQUIRE((h == nullptr) == (c == nullptr), "howl_lstm_stream_chunks: h and c come as a pair (both or neither)");
    const long need = last_only ? (long)C : (long)(1 + L_max / HOP) * C;
    HOWL_REQUIRE(out_ld >= need, "howl_lstm_stream_chunks: out_ld=%ld floats per stream, this call writes %ld", out_ld, need);
    HOWL_REQUIRE(((reinterpret_cast<uintptr_t>(lstm->w_ih) | reinterpret_cast<uintptr_t>(lstm->w_hh) | reinterpret_cast<uintptr_t>(head->w1)) & 15) == 0,
                 "howl_lstm_stream_chunks: weight_ih, weight_hh and the head's first weight must be 16-byte aligned");
    LsArgs a{lstm->w_ih, lstm->w_hh, lstm->b_ih, lstm->b_hh, head->w1, head->b1, head->w2, head->b2, pcm, ld, N, L_max, n_samples, frames,
             fbp, log_eps, zmuv_pair, h, c, C, last_only ? 1 : 0, probs, logits, out_ld};
    constexpr size_t lds = (size_t)LS_LDS_FLOATS * sizeof(float);
    static thread_local size_t granted[16] = {};
    howl_raise_lds(reinterpret_cast<const void*>(lstm_stream_kernel), lds, granted, "howl_lstm_stream_chunks");
    hipLaunchKernelGGL(lstm_stream_kernel, dim3((unsigned)((N + 3) / 4)), dim3(LS_THREADS), lds, stream, a);
    HOWL_CHECK_LAUNCH("howl_lstm_stream_chunks");
    return HOWL_OK;
}

}  // extern "C"
