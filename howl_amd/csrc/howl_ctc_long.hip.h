// The fused log_softmax + CTC recursion of one utterance on ONE wavefront for targets beyond ctc_wave's 31 labels
// (howl_ctc.hip.h): a lane holds K consecutive states [K * lane, K * lane + K) of the extended label sequence in registers,
// K = 2, 4, 8 for up to 63, 127, 255 labels (S = 2L + 1 <= 64K - 1).  K is even, so a lane's even registers are all the blank
// (one lp[blank] read per step, no skip term) and its odd registers are K / 2 consecutive labels (one LDS read each).  A step
// of the alpha recursion needs ONE value from the neighbour lane (its last state), a step of beta two (the first two states
// of the next lane): DPP wave shifts as in ctc_wave; everything else is lane-local.
//
// Per state the recursion is ctc_alpha_step's / ctc_beta_step's, lse3(own, prev, skip ? prev2 : -inf) + lp with the same
// masks, and per row and class the posteriors are summed in ctc_window_grad's order (the blank states apart, added last), so
// an utterance's nll and gradient rows are the same bits under ctc_wave<65> and under every K that holds it.
//
// LDS of a window of tc rows: [lp | q][tc][65] class-indexed, [alpha | beta][tc][64K + 1] state-indexed, 64K extended labels.
// State s sits in column (s % K) * 64 + s / K of its row: the recursions' stores (lane = s / K) and the gradient phase's reads
// (lane = row, odd pitch) both touch 64 different banks.  The parked alpha rows use the same [t][K][64] order in the workspace.
#pragma once
#include "howl_ctc.hip.h"

namespace {

constexpr int CTC_LONG_MAX_L = 255;
constexpr int CTC_LONG_CP = 65;     // pitch of the class-indexed rows (ctc_stage_rows<65>)

template <int K>
struct CtcLong {
    static_assert(K == 2 || K == 4 || K == 8, "states per lane");
    static constexpr int H = K / 2;                 // labels per lane
    static constexpr int SP = 64 * K + 1;           // pitch of the state-indexed rows
    static constexpr int WIN = K == 2 ? 64 : 32;    // rows per LDS window: 97.5, 81.5 and 146.5 KB
    static constexpr int MAX_L = 32 * K - 1;
    static constexpr size_t lds_floats(int tc) { return (size_t)tc * (2 * CTC_LONG_CP + 2 * SP) + 64 * K; }
    __device__ static __forceinline__ int col(int s) { return (s % K) * 64 + s / K; }
};

// lse3(a, b, -inf): the third exponential is +0 and the maximum is taken over the same two values -- the same bits
__device__ __forceinline__ float ctc_lse2(float a, float b) {
    constexpr float LOG2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;
    float m = fmaxf(a, b);
    if (m == -INFINITY) m = 0.0f;
    const float e = __builtin_amdgcn_exp2f((a - m) * LOG2E) + __builtin_amdgcn_exp2f((b - m) * LOG2E);
    return __builtin_amdgcn_logf(e) * LN2 + m;
}

template <int K>
struct CtcLongLane {
    int lane, S, blank;
    int lab[K / 2];
    bool skip_a[K / 2], skip_b[K / 2];
};

// one time step of alpha for the lane's K states; lprow = the step's log-softmax row
template <int K>
__device__ __forceinline__ void ctc_long_alpha_step(const CtcLongLane<K>& w, float (&a)[K], const float* lprow) {
    const float lpblank = lprow[w.blank];
    const float p1 = wave_shr1(a[K - 1]);           // state K * lane - 1 (lane 0 keeps its own: masked)
    const int s0 = K * w.lane;
    float n[K];
#pragma unroll
    for (int i = 0; i < K; i += 2) {
        const float prev = i == 0 ? (w.lane >= 1 ? p1 : -INFINITY) : a[i > 0 ? i - 1 : 0];
        const float ve = ctc_lse2(a[i], prev) + lpblank;
        n[i] = s0 + i < w.S ? ve : -INFINITY;
        const float vo = lse3(a[i + 1], a[i], w.skip_a[i >> 1] ? prev : -INFINITY) + lprow[w.lab[i >> 1]];
        n[i + 1] = s0 + i + 1 < w.S ? vo : -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = n[i];
}

template <int K>
__device__ __forceinline__ void ctc_long_beta_step(const CtcLongLane<K>& w, float (&b)[K], const float* lprow) {
    const float lpblank = lprow[w.blank];
    const float n1 = wave_shl1(b[0]), n2 = wave_shl1(b[1]);      // states K * lane + K, + K + 1 (lane 63: masked, S <= 64K - 1)
    const int s0 = K * w.lane;
    float n[K];
#pragma unroll
    for (int i = 0; i < K; i += 2) {
        const float ve = ctc_lse2(b[i], s0 + i + 1 < w.S ? b[i + 1] : -INFINITY) + lpblank;
        n[i] = s0 + i < w.S ? ve : -INFINITY;
        const float nx1 = i + 2 < K ? b[i + 2 < K ? i + 2 : 0] : n1;
        const float nx2 = i + 3 < K ? b[i + 3 < K ? i + 3 : 0] : n2;
        const float vo = lse3(b[i + 1], s0 + i + 2 < w.S ? nx1 : -INFINITY, w.skip_b[i >> 1] ? nx2 : -INFINITY) + lprow[w.lab[i >> 1]];
        n[i + 1] = s0 + i + 1 < w.S ? vo : -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) b[i] = n[i];
}

// ctc_window_grad with the state rows at their own pitch and column order
template <int K>
__device__ __forceinline__ void ctc_long_window_grad(const CtcLane& w, int t0, int len, int blank, float nll, float scale,
                                                     float* __restrict__ db, long dst_t) {
    constexpr int SP = CtcLong<K>::SP, CP = CTC_LONG_CP;
    wave_lds_sync();
    const int S = w.S, C = w.C;
    for (int r = w.lane; r < len; r += 64) {
        const float* ar = w.abuf + r * SP;
        const float* br = w.bbuf + r * SP;
        const float* lr = w.lpbuf + r * CP;
        float* qr = w.qbuf + r * CP;
        const float lpblank = lr[blank];
        float qblank = 0.0f;
        for (int s2 = 0; s2 < S; s2 += 2) {
            const int k = CtcLong<K>::col(s2);
            qblank += expf(ar[k] + br[k] - lpblank + nll);
        }
        for (int s2 = 1; s2 < S; s2 += 2) {
            const int c = w.labbuf[s2], k = CtcLong<K>::col(s2);
            qr[c] += expf(ar[k] + br[k] - lr[c] + nll);
        }
        qr[blank] += qblank;
    }
    wave_lds_sync();
    for (int i = w.lane; i < len * C; i += 64) {
        const int r = i / C, c = i - r * C;
        db[(size_t)(t0 + r) * dst_t + c] = (expf(w.lpbuf[r * CP + c]) - w.qbuf[r * CP + c]) * scale;
    }
}

// ctc_wave's walk over the time axis (alpha alone through the leading windows, its rows parked in `aws`; alpha and beta
// interleaved in the last window; beta back through the rest), K states per lane.  aws: [T][K][64] floats of this utterance.
template <int K>
__device__ __forceinline__ void ctc_long_wave(const float* __restrict__ zb, long st_t, int T, int B, int C,
                                              const long long* __restrict__ tgt, int Tb, int L, int Lcap, int blank,
                                              float* __restrict__ nll_out, float* __restrict__ db, long dst_t, int tc,
                                              float* __restrict__ aws, float* __restrict__ lds, int lane) {
    constexpr int H = CtcLong<K>::H, SP = CtcLong<K>::SP, CP = CTC_LONG_CP;
    float* lpbuf = lds;
    float* qbuf = lds + CP * tc;
    float* abuf = lds + 2 * CP * tc;
    float* bbuf = abuf + SP * tc;
    int* labbuf = reinterpret_cast<int*>(bbuf + SP * tc);      // [64 K] extended labels by state
    // the contract of howl_ctc_loss over ALL L labels (ctc_out_of_contract looks at one label per lane)
    bool bad = Tb < 0 || L < 0 || L > Lcap;
    if (!bad) {
        bool out = false;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const int idx = H * lane + j;
            const long long v = idx < L ? tgt[idx] : 0;
            out |= v < 0 || v >= C;
        }
        bad = __ballot(out) != 0;
    }
    if (bad) Tb = 0, L = 0;
    Tb = Tb > T ? T : Tb;
    const int S = 2 * L + 1;
    const bool want_grad = db != nullptr;

    CtcLongLane<K> w;
    w.lane = lane, w.S = S, w.blank = blank;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const int idx = H * lane + j;                           // state K * lane + 2j + 1; live iff idx < L
        w.lab[j] = idx < L ? (int)tgt[idx] : blank;
        labbuf[K * lane + 2 * j] = blank;
        labbuf[K * lane + 2 * j + 1] = w.lab[j];
    }
    // "may skip the blank between two different labels": the label before a lane's first and behind its last cross the lane boundary
    const int lab_before = __shfl(w.lab[H - 1], lane >= 1 ? lane - 1 : 0);
    const int lab_behind = __shfl(w.lab[0], lane < 63 ? lane + 1 : 63);
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const int idx = H * lane + j;
        const int pl = j == 0 ? lab_before : w.lab[j > 0 ? j - 1 : 0];
        const int nl = j == H - 1 ? lab_behind : w.lab[j + 1 < H ? j + 1 : 0];
        w.skip_a[j] = idx < L && idx >= 1 && w.lab[j] != pl;
        w.skip_b[j] = idx + 1 < L && w.lab[j] != nl;
    }
    CtcLane cw;     // what ctc_stage_rows and the gradient phase use
    cw.lane = lane, cw.lab = blank, cw.S = S, cw.C = C;
    cw.live = K * lane < S, cw.skip_a = cw.skip_b = false, cw.want_grad = want_grad;
    cw.lpbuf = lpbuf, cw.abuf = abuf, cw.bbuf = bbuf, cw.qbuf = qbuf;
    cw.labbuf = labbuf;
    const int nwin = Tb > tc ? (Tb + tc - 1) / tc : 1;
    const int s0 = K * lane;

    float a[K], bt[K];
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = bt[i] = -INFINITY;
    // windows 0 .. nwin-2: alpha alone
    for (int j = 0; j + 1 < nwin; ++j) {
        const int t0 = j * tc;
        ctc_stage_rows<CP>(cw, zb, st_t, t0, tc);
        for (int k = 0; k < tc; ++k) {
            const float* lprow = lpbuf + k * CP;
            if (t0 + k == 0) {
#pragma unroll
                for (int i = 0; i < K; ++i) a[i] = (s0 + i < S && s0 + i < 2) ? lprow[(i & 1) ? w.lab[i >> 1] : blank] : -INFINITY;
            } else {
                ctc_long_alpha_step<K>(w, a, lprow);
            }
            if (want_grad) {
#pragma unroll
                for (int i = 0; i < K; ++i) aws[((size_t)(t0 + k) * K + i) * 64 + lane] = a[i];
            }
        }
        wave_lds_sync();     // the window's LDS rows are rewritten by the next stage
    }
    // the last window: alpha forward and beta backward, interleaved
    const int tl0 = (nwin - 1) * tc, tlen = Tb - tl0;
    ctc_stage_rows<CP>(cw, zb, st_t, tl0, tlen);
    for (int k = 0; k < tlen; ++k) {
        const int kb = tlen - 1 - k;
        const float* lpa = lpbuf + k * CP;
        const float* lpb = lpbuf + kb * CP;
        if (tl0 + k == 0) {
#pragma unroll
            for (int i = 0; i < K; ++i) a[i] = (s0 + i < S && s0 + i < 2) ? lpa[(i & 1) ? w.lab[i >> 1] : blank] : -INFINITY;
        } else {
            ctc_long_alpha_step<K>(w, a, lpa);
        }
        if (k == 0) {
#pragma unroll
            for (int i = 0; i < K; ++i) bt[i] = (s0 + i < S && s0 + i >= S - 2) ? lpb[(i & 1) ? w.lab[i >> 1] : blank] : -INFINITY;
        } else if (want_grad) {
            ctc_long_beta_step<K>(w, bt, lpb);
        }
#pragma unroll
        for (int i = 0; i < K; ++i) {
            abuf[k * SP + i * 64 + lane] = a[i];
            if (want_grad) bbuf[kb * SP + i * 64 + lane] = bt[i];
        }
    }
    float nll;
    if (Tb > 0) {
        // states S - 1 and S - 2: register (s % K) of lane (s / K)
        float v1 = a[0], v2 = a[0];
#pragma unroll
        for (int i = 1; i < K; ++i) {
            v1 = (S - 1) % K == i ? a[i] : v1;
            v2 = (S > 1 ? S - 2 : 0) % K == i ? a[i] : v2;
        }
        const float l1 = __shfl(v1, (S - 1) / K), l2 = S > 1 ? __shfl(v2, (S - 2) / K) : -INFINITY;
        nll = -lse3(l1, l2, -INFINITY);
    } else {
        nll = L == 0 && !bad ? 0.0f : INFINITY;
    }
    if (lane == 0) nll_out[0] = nll;
    if (!want_grad) return;
    const float scale = 1.0f / ((float)B * (float)(L > 0 ? L : 1));
    ctc_long_window_grad<K>(cw, tl0, tlen, blank, nll, scale, db, dst_t);
    // windows nwin-2 .. 0: beta alone, on the alpha rows the first sweep left
    for (int j = nwin - 2; j >= 0; --j) {
        const int t0 = j * tc;
        wave_lds_sync();
        for (int x0 = 0; x0 < tc * K; x0 += 8) {       // independent loads, eight 64-float rows in flight (tc * K is a multiple of 8)
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = aws[((size_t)t0 * K + x0 + u) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 8; ++u) abuf[((x0 + u) / K) * SP + ((x0 + u) % K) * 64 + lane] = v[u];
        }
        ctc_stage_rows<CP>(cw, zb, st_t, t0, tc);
        for (int k = tc - 1; k >= 0; --k) {
            ctc_long_beta_step<K>(w, bt, lpbuf + k * CP);
#pragma unroll
            for (int i = 0; i < K; ++i) bbuf[k * SP + i * 64 + lane] = bt[i];
        }
        ctc_long_window_grad<K>(cw, t0, tc, blank, nll, scale, db, dst_t);
    }
    // rows past the utterance's end
    for (int i = lane; i < (T - Tb) * C; i += 64) {
        const int r = i / C, c = i - r * C;
        db[(size_t)(Tb + r) * dst_t + c] = 0.0f;
    }
}

}  // namespace
