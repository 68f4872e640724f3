// The "small-cnn" and "seq-cnn" models for gfx950 (MI355X), howl/model/cnn.py:32-104 (SmallCnn, SequentialCnn): one two-stage conv
// encoder with training-mode BatchNorm, and a Linear - ReLU - Dropout - Linear head on the whole (64, 2, 3) map (small) or on every
// output row (seq).  One call per direction (include/howl_hip_cnn.h), one launch plan per call (cnn_plan).
//
// Forward launches:                                                 backward launches:
//   cnn_conv0_fwd_kernel   conv0 on the fp32 MFMAs; bias, ReLU and    cnn_head_dz_kernel      dz1                 (+ 4 GEMM-path jobs, dXh)
//                          the 2x2 max-pool in the epilogue: the      cnn_bn_bwd_sums_kernel  BN2's batch sums, per utterance
//                          pooled map P, the pool's choice (one       cnn_bn_bwd_fold_kernel  their fold; d gamma2, d beta2
//                          byte), BN1's batch sums per workgroup      cnn_pool_grad_kernel    BN2 - ReLU - un-pool: G2, conv1's bias sums
//   cnn_bn_stats_kernel    fold -> mean, 1/std, running buffers       cnn_conv1_wgrad_kernel  conv1's weight gradient (slabs)
//   cnn_conv1_fwd_kernel   BN1 where P is staged (the padding is      cnn_conv1_dgrad_kernel  d (BN1's output), by the parity of the row
//                          zero AFTER BatchNorm), conv1 on the MFMAs, cnn_bn_bwd_sums_kernel, cnn_bn_bwd_fold_kernel: BN1
//                          the same epilogue: Q, choice, BN2's sums   cnn_conv0_wgrad_kernel  BN1 - ReLU - un-pool, conv0's weight and bias
//   cnn_bn_stats_kernel                                                                       gradient (slabs)
//   cnn_head_in_kernel     BN2 applied: the head's rows Xh            sum_slabs_multi_kernel x 2: every partial sum, fixed order
//   rowgemm / gemm         y1 = relu(Xh W1^T + b1)
//   cnn_head_out_kernel    mask, logits
// The batch-wide BatchNorm reductions are exchanged at launch boundaries only: a launch leaves one partial sum per workgroup, a
// one-workgroup-per-channel launch folds them in a fixed order.  No workgroup waits on another.  The pre-pool tensors never reach
// memory: the MFMA tile's sixteen rows are four pooled outputs times the four members of their window, so that a lane's four
// result registers are one window and the pool is a maximum over registers.
//
// The two convolutions' gradients run on the vector ALUs in the pool-aware form: the gradient in front of a max-pool is non-zero
// at one of four positions, which the weight gradients use (a quarter of the dense contraction's multiply-adds).
#include <math.h>

#include "howl_common.hip.h"
#include "../../include/howl_hip_cnn.h"
#include "howl_gemm.hip.h"

namespace {

constexpr int NF = 40;             // mel bins
constexpr int C1 = 48, C2 = 64;    // channels of the two stages
constexpr int KF = 16;             // conv0's kernel along frequency
constexpr int WP = 6, W2 = 3;      // pooled columns of the two stages
constexpr int K1 = C1 * 25;        // conv1's contraction
constexpr int HID = 128;           // head's hidden width
constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;
constexpr int XS = NF + 1;         // row stride of the input slab in LDS
constexpr int TPR0 = 8;            // pooled rows per workgroup of conv0's kernels: 48 pooled outputs = 12 MFMA row tiles
constexpr int TPR1 = 4;            // pooled rows per workgroup of conv1's forward: 12 pooled outputs = 3 MFMA row tiles
constexpr int PN_RS = 10, PN_ROWS = 19, PN_CS = PN_RS * PN_ROWS;      // conv1's operand slab: (48, 19 rows, 6 + 4 columns)
constexpr int KC1 = 24, WL1 = 80;  // conv1's weight chunk: 24 k of 64 channels, rows 80 floats apart (four k rows on distinct banks)
constexpr int DG_TH = 16;          // rows of P per workgroup of conv1's data gradient
constexpr int DG_ROWS = DG_TH / 2 + 2;
constexpr int HEAD_SPLITS = 32;
constexpr int W1G_SPLITS = 16;     // utterance groups of conv1's weight gradient
constexpr int W0G_TILES = 8, W0G_GROUPS = 32;

__device__ __forceinline__ void bn_affine(float gamma, float beta, float mean, float invstd, float& sc, float& sh) {
    sc = gamma * invstd;
    sh = beta - mean * sc;
}

// the first maximum of a pool window in scan order, then the ReLU
__device__ __forceinline__ float pool_relu(const f32x4& a, float bias, int& which) {
    float best = a[0] + bias;
    which = 0;
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float v = a[r] + bias;
        if (v > best) {
            best = v;
            which = r;
        }
    }
    return fmaxf(best, 0.0f);
}

// conv0 - ReLU - MaxPool on TPR0 pooled rows of one utterance.  M = (pooled output, window member), N = 48 channels, K = KT * 16;
// the weights pass through LDS in chunks of 64 k.  P, I1: (B, 48, Hp, 6); part1[(b, tile)][c | 48 + c] = sum, sum of squares.
template <int KT, int SH, bool TRAIN>
__global__ __launch_bounds__(256) void cnn_conv0_fwd_kernel(const float* __restrict__ x, long sb, long sm, long st, int T, int Hp,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ P, unsigned char* __restrict__ I1,
                                                            double* __restrict__ part1) {
    constexpr int K = KT * KF, XROWS = (2 * TPR0 - 1) * SH + KT;
    __shared__ float xs[XROWS * XS];
    __shared__ float wl[64 * C1];
    __shared__ float pl[C1 * 48];
    __shared__ unsigned char il[C1 * 48];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, b = blockIdx.y;
    const int hp0 = tile * TPR0, t0 = 2 * hp0 * SH - KT / 2;
    const float* xb = x + (long)b * sb;
    const bool f_fast = sm == 1;
    for (int i = tid; i < XROWS * NF; i += 256) {
        int r, f;
        if (f_fast) {
            r = i / NF;
            f = i - r * NF;
        } else {
            f = i / XROWS;
            r = i - f * XROWS;
        }
        const int t = t0 + r;
        xs[r * XS + f] = (t >= 0 && t < T) ? xb[(long)f * sm + (long)t * st] : 0.0f;
    }
    const int kk = lane >> 4;
    int abase[3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        const int i = lane & 15, pp = (wave * 3 + mt) * 4 + (i >> 2);
        const int hl = 2 * (pp / WP) + ((i >> 1) & 1), w0 = 2 * (pp % WP) + (i & 1);
        abase[mt] = hl * SH * XS + 2 * w0 + kk;
    }
    f32x4 acc[3][3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ch = 0; ch < K / 64; ++ch) {
        __syncthreads();
        for (int i = tid; i < 64 * C1; i += 256) {
            const int c = i >> 6, kc = i & 63;
            wl[kc * C1 + c] = w[c * K + 64 * ch + kc];
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int S = 16 * ch + s;
            const int off = (S >> 2) * XS + (S & 3) * 4;
            float bv[3], av[3];
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) bv[nt] = wl[(4 * s + kk) * C1 + nt * 16 + (lane & 15)];
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) av[mt] = xs[abase[mt] + off];
#pragma unroll
            for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) {
            const int c = nt * 16 + (lane & 15), pp = (wave * 3 + mt) * 4 + (lane >> 4);
            int which;
            pl[c * 48 + pp] = pool_relu(acc[mt][nt], bias[c], which);
            il[c * 48 + pp] = (unsigned char)which;
        }
    __syncthreads();
    const int nvalid = min(TPR0, Hp - hp0) * WP;
    const size_t n1 = (size_t)Hp * WP;
    for (int i = tid; i < C1 * 48; i += 256) {
        const int c = i / 48, pp = i - c * 48;
        if (pp < nvalid) {
            const size_t e = ((size_t)b * C1 + c) * n1 + (size_t)hp0 * WP + pp;
            P[e] = pl[i];
            if constexpr (TRAIN) I1[e] = il[i];
        }
    }
    if constexpr (TRAIN) {
        if (tid < 2 * C1) {
            const int c = tid % C1;
            const bool sq = tid >= C1;
            double a = 0.0;
            for (int pp = 0; pp < nvalid; ++pp) {
                const double v = (double)pl[c * 48 + pp];
                a += sq ? v * v : v;
            }
            part1[((size_t)b * gridDim.x + tile) * (2 * C1) + tid] = a;
        }
    }
}

struct CnnBn {      // one BatchNorm of the encoder
    const float *gamma, *beta;
    float *rmean, *rvar;
    long long* batches;
};

// Fold of a BatchNorm's forward sums, one workgroup per channel: part[row][c | C + c] -> stat[c] = mean, stat[C + c] = 1 / std;
// the running buffers move with the unbiased variance.
__global__ __launch_bounds__(256) void cnn_bn_stats_kernel(const double* __restrict__ part, int nparts, int C, double count, CnnBn bn,
                                                           float* __restrict__ stat) {
    __shared__ double red[4][2];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a0 = 0.0, a1 = 0.0;
    for (int i = tid; i < nparts; i += 256) {
        a0 += part[(size_t)i * 2 * C + c];
        a1 += part[(size_t)i * 2 * C + C + c];
    }
    a0 = wave_sum_d(a0);
    a1 = wave_sum_d(a1);
    if (lane == 0) {
        red[wave][0] = a0;
        red[wave][1] = a1;
    }
    __syncthreads();
    if (tid == 0) {
        const double s = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0], ss = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        const double mean = s / count;
        const double var = fmax(ss / count - mean * mean, 0.0);
        const float meanf = (float)mean;
        stat[c] = meanf;
        stat[C + c] = (float)(1.0 / sqrt(var + (double)BN_EPS));
        bn.rmean[c] = (1.0f - BN_MOMENTUM) * bn.rmean[c] + BN_MOMENTUM * meanf;
        bn.rvar[c] = (1.0f - BN_MOMENTUM) * bn.rvar[c] + BN_MOMENTUM * (float)(var * count / (count - 1.0));
        if (c == 0) bn.batches[0] += 1;
    }
}

// BN1 - conv1 - ReLU - MaxPool on TPR1 pooled rows of one utterance.  The operand slab holds the NORMALISED P with conv1's zero
// padding around it.  M = (pooled output, window member), N = 64 channels (wave = 16 of them), K = 1200 in chunks of 24; koff maps
// k = (ci, kh, kw) to its offset in the slab.  Q, I2: (B, 64, H2, 3); part2[(b, tile)][c | 64 + c].
template <bool TRAIN>
__global__ __launch_bounds__(256) void cnn_conv1_fwd_kernel(const float* __restrict__ P, int Hp, int H2, const float* __restrict__ w,
                                                            const float* __restrict__ bias, CnnBn bn1, const float* __restrict__ stat1,
                                                            float* __restrict__ Q, unsigned char* __restrict__ I2,
                                                            double* __restrict__ part2) {
    __shared__ float pn[C1 * PN_CS];
    __shared__ float wl[KC1 * WL1];
    __shared__ int koff[K1];
    __shared__ float ql[C2 * 12];
    __shared__ unsigned char il[C2 * 12];
    __shared__ float sc[C1], sh[C1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, b = blockIdx.y;
    if (tid < C1) {
        if constexpr (TRAIN) bn_affine(bn1.gamma[tid], bn1.beta[tid], stat1[tid], stat1[C1 + tid], sc[tid], sh[tid]);
        else bn_affine(bn1.gamma[tid], bn1.beta[tid], bn1.rmean[tid], 1.0f / sqrtf(bn1.rvar[tid] + BN_EPS), sc[tid], sh[tid]);
    }
    for (int i = tid; i < K1; i += 256) {
        const int ci = i / 25, r = i - ci * 25;
        koff[i] = ci * PN_CS + (r / 5) * PN_RS + r % 5;
    }
    __syncthreads();
    const int hbase = 4 * TPR1 * tile - 2;
    for (int i = tid; i < C1 * PN_CS; i += 256) {
        const int ci = i / PN_CS, rem = i - ci * PN_CS, r = rem / PN_RS, cc = rem - r * PN_RS;
        const int h = hbase + r, wc = cc - 2;
        float v = 0.0f;
        if (h >= 0 && h < Hp && wc >= 0 && wc < WP) v = fmaf(P[(((size_t)b * C1 + ci) * Hp + h) * WP + wc], sc[ci], sh[ci]);
        pn[i] = v;
    }
    const int kk = lane >> 4, co = wave * 16 + (lane & 15);
    int abase[3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        const int i = lane & 15, pp = mt * 4 + (i >> 2);
        const int h1l = 2 * (pp / W2) + ((i >> 1) & 1), w1 = 2 * (pp % W2) + (i & 1);
        abase[mt] = 2 * h1l * PN_RS + w1;
    }
    f32x4 acc[3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) acc[mt] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ch = 0; ch < K1 / KC1; ++ch) {
        __syncthreads();
        for (int i = tid; i < KC1 * C2; i += 256) {
            const int c = i / KC1, kc = i - c * KC1;
            wl[kc * WL1 + c] = w[(size_t)c * K1 + KC1 * ch + kc];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KC1 / 4; ++s) {
            const int ko = koff[KC1 * ch + 4 * s + kk];
            const float bv = wl[(4 * s + kk) * WL1 + co];
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pn[abase[mt] + ko], bv, acc[mt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        const int pp = mt * 4 + (lane >> 4);
        int which;
        ql[co * 12 + pp] = pool_relu(acc[mt], bias[co], which);
        il[co * 12 + pp] = (unsigned char)which;
    }
    __syncthreads();
    const int nvalid = min(TPR1, H2 - TPR1 * tile) * W2;
    const size_t n2 = (size_t)H2 * W2;
    for (int i = tid; i < C2 * 12; i += 256) {
        const int c = i / 12, pp = i - c * 12;
        if (pp < nvalid) {
            const size_t e = ((size_t)b * C2 + c) * n2 + (size_t)TPR1 * tile * W2 + pp;
            Q[e] = ql[i];
            if constexpr (TRAIN) I2[e] = il[i];
        }
    }
    if constexpr (TRAIN) {
        if (tid < 2 * C2) {
            const int c = tid % C2;
            const bool sq = tid >= C2;
            double a = 0.0;
            for (int pp = 0; pp < nvalid; ++pp) {
                const double v = (double)ql[c * 12 + pp];
                a += sq ? v * v : v;
            }
            part2[((size_t)b * gridDim.x + tile) * (2 * C2) + tid] = a;
        }
    }
}

// Where element (channel c, output row t, column j) of utterance b sits in the head's row matrix (rows of F = 64 * per floats):
// small-cnn flattens (c, h, w) into the utterance's one row, seq-cnn (c, w) into row (b, t).
__device__ __forceinline__ size_t head_at(bool seq, int b, int c, int pos, int H2) {
    if (!seq) return ((size_t)b * C2 + c) * (size_t)(H2 * W2) + pos;
    const int t = pos / W2, j = pos - t * W2;
    return (((size_t)b * H2 + t) * C2 + c) * W2 + j;
}

// BN2 applied: Xh (rows, F) from Q
template <bool TRAIN>
__global__ __launch_bounds__(256) void cnn_head_in_kernel(const float* __restrict__ Q, CnnBn bn2, const float* __restrict__ stat2, int B,
                                                          int H2, int seq, float* __restrict__ Xh) {
    __shared__ float sc[C2], sh[C2];
    const int tid = threadIdx.x;
    if (tid < C2) {
        if constexpr (TRAIN) bn_affine(bn2.gamma[tid], bn2.beta[tid], stat2[tid], stat2[C2 + tid], sc[tid], sh[tid]);
        else bn_affine(bn2.gamma[tid], bn2.beta[tid], bn2.rmean[tid], 1.0f / sqrtf(bn2.rvar[tid] + BN_EPS), sc[tid], sh[tid]);
    }
    __syncthreads();
    const int n2 = H2 * W2;
    const size_t n = (size_t)B * C2 * n2;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n; i += (size_t)gridDim.x * 256) {
        const int pos = (int)(i % n2), c = (int)((i / n2) % C2), b = (int)(i / ((size_t)n2 * C2));
        Xh[head_at(seq != 0, b, c, pos, H2)] = fmaf(Q[i], sc[c], sh[c]);
    }
}

// One wave per head row: y1d = y1 * mask * keep_scale (kept in place when training), logits = y1d W2^T + b2.  Row r = (b, t); the
// mask's rows are (t, b).
__global__ __launch_bounds__(256) void cnn_head_out_kernel(float* __restrict__ y1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ mask, float keep_scale, int rows, int B, int H,
                                                           int L, float* __restrict__ logits) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float y[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) y[e] = y1[(size_t)r * HID + lane + 64 * e];
    if (mask != nullptr) {
        const int b = r / H, t = r - b * H;
        const size_t mr = (size_t)t * B + b;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            y[e] = y[e] * mask[mr * HID + lane + 64 * e] * keep_scale;
            y1[(size_t)r * HID + lane + 64 * e] = y[e];
        }
    }
    for (int l = 0; l < L; ++l) {
        const float a = wave_sum(fmaf(w2[l * HID + lane + 64], y[1], w2[l * HID + lane] * y[0]));
        if (lane == 0) logits[(size_t)r * L + l] = a + b2[l];
    }
}

// dz1 = (y1d > 0) keep_scale (dlogits W2)
__global__ __launch_bounds__(256) void cnn_head_dz_kernel(const float* __restrict__ dlogits, const float* __restrict__ y1d,
                                                          const float* __restrict__ w2, float keep_scale, size_t n, int L,
                                                          float* __restrict__ dz1) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t r = i / HID;
        const int u = (int)(i - r * HID);
        float a = 0.0f;
        for (int l = 0; l < L; ++l) a = fmaf(dlogits[r * L + l], w2[l * HID + u], a);
        dz1[i] = y1d[i] > 0.0f ? a * keep_scale : 0.0f;
    }
}

// A BatchNorm's backward batch sums of one utterance, one wave per channel at a time: part[b][c] = sum d, part[b][C + c] = sum d x^n
// over the channel's n positions.  V: the BatchNorm's input (B, C, n); d: the gradient at its output, in V's layout or (HEAD) in
// the head's row matrix.
template <bool HEAD>
__global__ __launch_bounds__(256) void cnn_bn_bwd_sums_kernel(const float* __restrict__ d, const float* __restrict__ V,
                                                              const float* __restrict__ stat, int C, int n, int H2, int seq,
                                                              double* __restrict__ part) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < C; c += 4) {
        const float mean = stat[c], invstd = stat[C + c];
        double a0 = 0.0, a1 = 0.0;
        for (int pos = lane; pos < n; pos += 64) {
            const size_t e = ((size_t)b * C + c) * n + pos;
            const float dv = HEAD ? d[head_at(seq != 0, b, c, pos, H2)] : d[e];
            const float xn = (V[e] - mean) * invstd;
            a0 += (double)dv;
            a1 += (double)dv * (double)xn;
        }
        a0 = wave_sum_d(a0);
        a1 = wave_sum_d(a1);
        if (lane == 0) {
            part[(size_t)b * 2 * C + c] = a0;
            part[(size_t)b * 2 * C + C + c] = a1;
        }
    }
}

// Their fold, one workgroup per channel: m[c] = mean d, m[C + c] = mean d x^n; d beta = sum d, d gamma = sum d x^n
__global__ __launch_bounds__(256) void cnn_bn_bwd_fold_kernel(const double* __restrict__ part, int nparts, int C, double count,
                                                              float* __restrict__ m, float* __restrict__ g_gamma,
                                                              float* __restrict__ g_beta) {
    __shared__ double red[4][2];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a0 = 0.0, a1 = 0.0;
    for (int i = tid; i < nparts; i += 256) {
        a0 += part[(size_t)i * 2 * C + c];
        a1 += part[(size_t)i * 2 * C + C + c];
    }
    a0 = wave_sum_d(a0);
    a1 = wave_sum_d(a1);
    if (lane == 0) {
        red[wave][0] = a0;
        red[wave][1] = a1;
    }
    __syncthreads();
    if (tid == 0) {
        const double s = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0], sx = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        m[c] = (float)(s / count);
        m[C + c] = (float)(sx / count);
        g_beta[c] = (float)s;
        g_gamma[c] = (float)sx;
    }
}

// BN2's input gradient, the ReLU and the pool of one utterance: G2 (B, 64, n2) = the gradient at the window's chosen position of
// conv1's output (zero where the pooled value is 0); bpart[b][c] = its sum over the positions (conv1's bias gradient).
__global__ __launch_bounds__(256) void cnn_pool_grad_kernel(const float* __restrict__ dXh, const float* __restrict__ Q,
                                                            const float* __restrict__ gamma, const float* __restrict__ stat2,
                                                            const float* __restrict__ m2, int H2, int seq, float* __restrict__ G2,
                                                            float* __restrict__ bpart) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n2 = H2 * W2;
    for (int c = wave; c < C2; c += 4) {
        const float mean = stat2[c], invstd = stat2[C2 + c], k = gamma[c] * invstd, md = m2[c], mdx = m2[C2 + c];
        double a = 0.0;
        for (int pos = lane; pos < n2; pos += 64) {
            const size_t e = ((size_t)b * C2 + c) * n2 + pos;
            const float q = Q[e], xn = (q - mean) * invstd;
            const float g = q > 0.0f ? k * (dXh[head_at(seq != 0, b, c, pos, H2)] - md - xn * mdx) : 0.0f;
            G2[e] = g;
            a += (double)g;
        }
        a = wave_sum_d(a);
        if (lane == 0) bpart[(size_t)b * C2 + c] = (float)a;
    }
}

// conv1's weight gradient in the pool-aware form: workgroup (co, s) sums over the utterances b = s, s + S, ... and their pooled
// outputs G2[b, co, h2, w2] x (normalised, zero-padded P around the window's chosen position); a thread owns five of the 1200
// weights of its output channel.  slabs[s][co][k].
__global__ __launch_bounds__(256) void cnn_conv1_wgrad_kernel(const float* __restrict__ G2, const unsigned char* __restrict__ I2,
                                                              const float* __restrict__ P, const float* __restrict__ g1,
                                                              const float* __restrict__ be1, const float* __restrict__ stat1, int B, int Hp,
                                                              int H2, float* __restrict__ slabs) {
    const int co = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, n2 = H2 * W2;
    int ci[5], kh[5], kw[5];
    float sc[5], sh[5], acc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int k = min(tid + 256 * j, K1 - 1);
        ci[j] = k / 25;
        kh[j] = (k % 25) / 5;
        kw[j] = k % 5;
        bn_affine(g1[ci[j]], be1[ci[j]], stat1[ci[j]], stat1[C1 + ci[j]], sc[j], sh[j]);
        acc[j] = 0.0f;
    }
    for (int b = s; b < B; b += gridDim.y) {
        for (int pos = 0; pos < n2; ++pos) {
            const size_t e = ((size_t)b * C2 + co) * n2 + pos;
            const float g = G2[e];
            if (g == 0.0f) continue;      // (the same for every thread of the workgroup)
            const int id = I2[e], h2 = pos / W2, w2 = pos - h2 * W2;
            const int h1 = 2 * h2 + (id >> 1), w1 = 2 * w2 + (id & 1);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int h = 2 * h1 - 2 + kh[j], wc = w1 - 2 + kw[j];
                float v = 0.0f;
                if (h >= 0 && h < Hp && wc >= 0 && wc < WP) v = fmaf(P[(((size_t)b * C1 + ci[j]) * Hp + h) * WP + wc], sc[j], sh[j]);
                acc[j] = fmaf(g, v, acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j)
        if (tid + 256 * j < K1) slabs[((size_t)s * C2 + co) * K1 + tid + 256 * j] = acc[j];
}

// conv1's data gradient on DG_TH rows of BN1's output of one utterance: dPn (B, 48, Hp, 6).  conv1 strides by two along the rows,
// so row h of its input meets kernel rows of h's parity only: kh = h + 2 - 2 h1.  The dense gradient of the tile's conv1 rows
// (G2 at the chosen member, zero elsewhere, two zero columns on either side) is staged in LDS.
__global__ __launch_bounds__(256) void cnn_conv1_dgrad_kernel(const float* __restrict__ G2, const unsigned char* __restrict__ I2,
                                                              const float* __restrict__ w, int Hp, int H2, float* __restrict__ dPn) {
    __shared__ float dz[C2 * DG_ROWS * PN_RS];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, n2 = H2 * W2;
    const int h0 = tile * DG_TH, r0 = h0 / 2 - 1;      // dz row r <-> conv1 row r0 + r
    for (int i = tid; i < C2 * DG_ROWS * PN_RS; i += 256) {
        const int co = i / (DG_ROWS * PN_RS), rem = i - co * (DG_ROWS * PN_RS), r = rem / PN_RS, w1 = rem - r * PN_RS - 2;
        const int h1 = r0 + r;
        float v = 0.0f;
        if (h1 >= 0 && h1 < 2 * H2 && w1 >= 0 && w1 < 2 * W2) {
            const size_t e = ((size_t)b * C2 + co) * n2 + (size_t)(h1 >> 1) * W2 + (w1 >> 1);
            if (I2[e] == (h1 & 1) * 2 + (w1 & 1)) v = G2[e];
        }
        dz[i] = v;
    }
    __syncthreads();
    if (tid >= 2 * DG_TH * WP) return;
    const int half = tid / (DG_TH * WP), pos = tid - half * (DG_TH * WP);
    const int hl = pos / WP, wc = pos - hl * WP, h = h0 + hl;
    if (h >= Hp) return;
    for (int ci = half; ci < C1; ci += 2) {
        float a = 0.0f;
        for (int co = 0; co < C2; ++co) {
            const float* wk = w + ((size_t)co * C1 + ci) * 25;
            const float* dzc = dz + co * (DG_ROWS * PN_RS);
            for (int kh = h & 1; kh < 5; kh += 2) {
                const int r = (h + 2 - kh) / 2 - r0;
#pragma unroll
                for (int kw = 0; kw < 5; ++kw) a = fmaf(dzc[r * PN_RS + wc + 4 - kw], wk[kh * 5 + kw], a);
            }
        }
        dPn[(((size_t)b * C1 + ci) * Hp + h) * WP + wc] = a;
    }
}

// BN1's input gradient, the ReLU, the pool and conv0's weight and bias gradient.  Workgroup (x, y) sums over the tiles x, x + X, ...
// of TPR0 pooled rows of the utterances y, y + Y, ...: G1 = the gradient at the window's chosen position of conv0's output and that
// position's offset in the input slab are staged per (channel, pooled output); thread (kf, channel group of three) owns the KT
// weights of its three channels at frequency offset kf.  cpart[(y, x)][c][kt][kf | 48 K + c].
template <int KT, int SH>
__global__ __launch_bounds__(256) void cnn_conv0_wgrad_kernel(const float* __restrict__ x, long sb, long sm, long st, int T, int Hp, int B,
                                                              int ntile, const float* __restrict__ P, const unsigned char* __restrict__ I1,
                                                              const float* __restrict__ dPn, const float* __restrict__ g1,
                                                              const float* __restrict__ stat1, const float* __restrict__ m1,
                                                              float* __restrict__ cpart) {
    constexpr int K = KT * KF, XROWS = (2 * TPR0 - 1) * SH + KT;
    __shared__ float xs[XROWS * XS];
    __shared__ float gs[C1 * 48];
    __shared__ int gb[C1 * 48];
    const int tid = threadIdx.x, kf = tid & 15, cg = tid >> 4;
    const bool f_fast = sm == 1;
    const size_t n1 = (size_t)Hp * WP;
    float acc[3][KT], bs[3];
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
        bs[cc] = 0.0f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) acc[cc][kt] = 0.0f;
    }
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* xb = x + (long)b * sb;
        for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
            const int hp0 = tile * TPR0, t0 = 2 * hp0 * SH - KT / 2;
            __syncthreads();      // the tile before has been consumed
            for (int i = tid; i < XROWS * NF; i += 256) {
                int r, f;
                if (f_fast) {
                    r = i / NF;
                    f = i - r * NF;
                } else {
                    f = i / XROWS;
                    r = i - f * XROWS;
                }
                const int t = t0 + r;
                xs[r * XS + f] = (t >= 0 && t < T) ? xb[(long)f * sm + (long)t * st] : 0.0f;
            }
            for (int i = tid; i < C1 * 48; i += 256) {
                const int c = i / 48, pp = i - c * 48, hpl = pp / WP, wp = pp - hpl * WP;
                float g = 0.0f;
                int base = 0;
                if (hp0 + hpl < Hp) {
                    const size_t e = ((size_t)b * C1 + c) * n1 + (size_t)hp0 * WP + pp;
                    const float p = P[e];
                    if (p > 0.0f) {
                        const float invstd = stat1[C1 + c], xn = (p - stat1[c]) * invstd;
                        g = g1[c] * invstd * (dPn[e] - m1[c] - xn * m1[C1 + c]);
                        const int id = I1[e];
                        base = (2 * hpl + (id >> 1)) * SH * XS + 2 * (2 * wp + (id & 1));
                    }
                }
                gs[i] = g;
                gb[i] = base;
            }
            __syncthreads();
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const int c = cg * 3 + cc;
                for (int pp = 0; pp < 48; ++pp) {
                    const float g = gs[c * 48 + pp];
                    const float* xp = xs + gb[c * 48 + pp] + kf;
                    bs[cc] += g;
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) acc[cc][kt] = fmaf(g, xp[kt * XS], acc[cc][kt]);
                }
            }
        }
    }
    float* slab = cpart + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(C1 * K + C1);
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
        const int c = cg * 3 + cc;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) slab[c * K + kt * KF + kf] = acc[cc][kt];
        if (kf == 0) slab[C1 * K + c] = bs[cc];
    }
}

// How one problem (kind, B utterances of T frames, num_labels) runs: geometry, the workspace carve-up and the launch shapes,
// decided once per call; `bad` says why a problem is refused.
struct CnnPlan {
    char bad[96];
    bool seq;
    int KT, H0, Hp, H1, H2, F;        // conv0's kernel rows and output rows, pooled rows, conv1's rows, output rows, head's row width
    int ntile0, ntile1, ntiled;       // tiles per utterance of conv0's kernels, of conv1's forward and of its data gradient
    int gx0, gy0, gs1;                // grid of conv0's weight gradient, utterance groups of conv1's
    long rows;                        // head rows: B (small) or B * H2 (seq)
    double count1, count2;            // elements per channel of BN1 and BN2
    double *part1, *part2, *part3, *part4;
    float *stat1, *stat2, *m1, *m2, *P, *Q, *Xh, *y1;
    unsigned char *I1, *I2;
    float *dz1, *dXh, *G2, *bpart, *dPn, *slabs1, *cpart0, *slabs_w1, *slabs_w2, *scratch_b1, *scratch_b2;
    size_t bytes;
};
int cnn_rows(int kind, int T, int* H0p = nullptr, int* Hpp = nullptr, int* H1p = nullptr) {
    if (kind == HOWL_CNN_SMALL ? (T < 26 || T > 41) : kind == HOWL_CNN_SEQ ? (T < 5 || T > HOWL_CNN_MAX_FRAMES) : true) return 0;
    const int H0 = kind == HOWL_CNN_SMALL ? T / 2 + 1 : T + 1, Hp = H0 / 2, H1 = (Hp - 1) / 2 + 1;
    if (H0p != nullptr) *H0p = H0;
    if (Hpp != nullptr) *Hpp = Hp;
    if (H1p != nullptr) *H1p = H1;
    return H1 / 2;
}
CnnPlan cnn_plan(int kind, int B, int M, int T, int num_labels, void* ws = nullptr) {
    CnnPlan q{};
    if (kind != HOWL_CNN_SMALL && kind != HOWL_CNN_SEQ) snprintf(q.bad, sizeof(q.bad), "kind=%d: HOWL_CNN_SMALL or HOWL_CNN_SEQ", kind);
    else if (B < 1) snprintf(q.bad, sizeof(q.bad), "B=%d: at least one utterance", B);
    else if (M != NF) snprintf(q.bad, sizeof(q.bad), "M=%d mel bins: the kernels are specialised for 40", M);
    else if (cnn_rows(kind, T) == 0)
        snprintf(q.bad, sizeof(q.bad), "T=%d frames outside %d..%d", T, kind == HOWL_CNN_SMALL ? 26 : 5, kind == HOWL_CNN_SMALL ? 41 : HOWL_CNN_MAX_FRAMES);
    else if (num_labels < 1 || num_labels > HOWL_CNN_MAX_LABELS)
        snprintf(q.bad, sizeof(q.bad), "num_labels=%d outside 1..%d", num_labels, HOWL_CNN_MAX_LABELS);
    if (q.bad[0] != 0) return q;
    q.seq = kind == HOWL_CNN_SEQ;
    q.KT = q.seq ? 20 : 8;
    q.H2 = cnn_rows(kind, T, &q.H0, &q.Hp, &q.H1);
    q.F = q.seq ? C2 * W2 : C2 * 2 * W2;
    q.rows = q.seq ? (long)B * q.H2 : (long)B;
    if (q.rows > (1L << 20) || B > (1 << 20)) {
        snprintf(q.bad, sizeof(q.bad), "B=%d x %d output rows: beyond 2^20 head rows", B, q.seq ? q.H2 : 1);
        return q;
    }
    q.ntile0 = (q.Hp + TPR0 - 1) / TPR0;
    q.ntile1 = (q.H2 + TPR1 - 1) / TPR1;
    q.ntiled = (q.Hp + DG_TH - 1) / DG_TH;
    q.gx0 = std::min(q.ntile0, W0G_TILES);
    q.gy0 = std::min(B, W0G_GROUPS);
    q.gs1 = std::min(B, W1G_SPLITS);
    q.count1 = (double)B * q.Hp * WP;
    q.count2 = (double)B * q.H2 * W2;
    size_t off = 0;      // in floats; every region starts on a 16-byte boundary
    auto region = [&](size_t floats) {
        const size_t at = off;
        off += (floats + 3) / 4 * 4;
        return ws != nullptr ? static_cast<float*>(ws) + at : nullptr;
    };
    auto dregion = [&](size_t doubles) { return reinterpret_cast<double*>(region(2 * doubles)); };
    auto bregion = [&](size_t bytes) { return reinterpret_cast<unsigned char*>(region((bytes + 3) / 4)); };
    const size_t rows = (size_t)q.rows, np = (size_t)B * C1 * q.Hp * WP, nq = (size_t)B * C2 * q.H2 * W2;
    q.part1 = dregion((size_t)B * q.ntile0 * 2 * C1);
    q.part2 = dregion((size_t)B * q.ntile1 * 2 * C2);
    q.part3 = dregion((size_t)B * 2 * C2);
    q.part4 = dregion((size_t)B * 2 * C1);
    q.stat1 = region(2 * C1);
    q.stat2 = region(2 * C2);
    q.m1 = region(2 * C1);
    q.m2 = region(2 * C2);
    q.P = region(np);
    q.I1 = bregion(np);
    q.Q = region(nq);
    q.I2 = bregion(nq);
    q.Xh = region(rows * q.F);
    q.y1 = region(rows * HID);
    q.dz1 = region(rows * HID);
    q.dXh = region(rows * q.F);
    q.G2 = region(nq);
    q.bpart = region((size_t)B * C2);
    q.dPn = region(np);
    q.slabs1 = region((size_t)q.gs1 * C2 * K1);
    q.cpart0 = region((size_t)q.gx0 * q.gy0 * (C1 * q.KT * KF + C1));
    q.slabs_w1 = region((size_t)HEAD_SPLITS * HID * q.F);
    q.slabs_w2 = region((size_t)HEAD_SPLITS * HOWL_CNN_MAX_LABELS * HID);
    q.scratch_b1 = region((size_t)64 * HID);
    q.scratch_b2 = region((size_t)64 * HOWL_CNN_MAX_LABELS);
    q.bytes = off * sizeof(float) + 64;
    return q;
}

bool all_set(const void* const* p, int n) {
    for (int i = 0; i < n; ++i)
        if (p[i] == nullptr) return false;
    return true;
}

int grid_for(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 4096); }

}  // namespace

extern "C" {

int howl_cnn_supported(int kind, int B, int M, int T, int num_labels) { return cnn_plan(kind, B, M, T, num_labels).bad[0] == 0 ? 1 : 0; }

size_t howl_cnn_workspace_bytes(int kind, int B, int T, int num_labels) { return cnn_plan(kind, B, NF, T, num_labels).bytes; }

size_t howl_cnn_out_rows(int kind, int T) { return (size_t)cnn_rows(kind, T); }

int howl_cnn_fwd(int kind, const HowlCnnParams* p, const HowlCnnBuffers* bf, const float* x, long sb, long sm, long st, int B, int M,
                 int T, int num_labels, int training, const float* drop_mask, float keep_scale, float* logits, void* ws,
                 size_t ws_bytes, hipStream_t stream) {
    HOWL_REQUIRE(p && bf && x && logits && ws && all_set(reinterpret_cast<const void* const*>(p), 12) &&
                     all_set(reinterpret_cast<const void* const*>(bf), 6), "howl_cnn_fwd: null pointer");
    HOWL_REQUIRE(training || drop_mask == nullptr, "howl_cnn_fwd: a dropout mask in eval mode");
    const CnnPlan q = cnn_plan(kind, B, M, T, num_labels, ws);
    HOWL_REQUIRE(q.bad[0] == 0, "howl_cnn_fwd: %s", q.bad);
    if (ws_bytes < q.bytes) {
        howl_set_error("howl_cnn_fwd: workspace too small (%zu < %zu bytes)", ws_bytes, q.bytes);
        return HOWL_E_WORKSPACE;
    }
    const CnnBn bn1{p->bn1_w, p->bn1_b, bf->bn1_mean, bf->bn1_var, bf->bn1_batches};
    const CnnBn bn2{p->bn2_w, p->bn2_b, bf->bn2_mean, bf->bn2_var, bf->bn2_batches};
    const int rows = (int)q.rows;
    {
        HowlProfScope prof("cnn_conv0", stream, 2.0 * C1 * q.KT * KF * 4.0 * q.Hp * WP * B);
        const dim3 grid(q.ntile0, B);
#define HOWL_CNN_CONV0(KT_, SH_)                                                                                                       \
    do {                                                                                                                               \
        if (training)                                                                                                                  \
            hipLaunchKernelGGL((cnn_conv0_fwd_kernel<KT_, SH_, true>), grid, dim3(256), 0, stream, x, sb, sm, st, T, q.Hp, p->conv0_w,   \
                               p->conv0_b, q.P, q.I1, q.part1);                                                                        \
        else                                                                                                                           \
            hipLaunchKernelGGL((cnn_conv0_fwd_kernel<KT_, SH_, false>), grid, dim3(256), 0, stream, x, sb, sm, st, T, q.Hp, p->conv0_w,  \
                               p->conv0_b, q.P, (unsigned char*)nullptr, (double*)nullptr);                                            \
    } while (0)
        if (q.seq) HOWL_CNN_CONV0(20, 1);
        else HOWL_CNN_CONV0(8, 2);
#undef HOWL_CNN_CONV0
        if (training)
            hipLaunchKernelGGL(cnn_bn_stats_kernel, dim3(C1), dim3(256), 0, stream, (const double*)q.part1, B * q.ntile0, C1, q.count1, bn1, q.stat1);
    }
    {
        HowlProfScope prof("cnn_conv1", stream, 2.0 * C2 * K1 * 4.0 * q.H2 * W2 * B);
        if (training) {
            hipLaunchKernelGGL(cnn_conv1_fwd_kernel<true>, dim3(q.ntile1, B), dim3(256), 0, stream, (const float*)q.P, q.Hp, q.H2, p->conv1_w,
                               p->conv1_b, bn1, (const float*)q.stat1, q.Q, q.I2, q.part2);
            hipLaunchKernelGGL(cnn_bn_stats_kernel, dim3(C2), dim3(256), 0, stream, (const double*)q.part2, B * q.ntile1, C2, q.count2, bn2, q.stat2);
        } else {
            hipLaunchKernelGGL(cnn_conv1_fwd_kernel<false>, dim3(q.ntile1, B), dim3(256), 0, stream, (const float*)q.P, q.Hp, q.H2, p->conv1_w,
                               p->conv1_b, bn1, (const float*)nullptr, q.Q, (unsigned char*)nullptr, (double*)nullptr);
        }
    }
    {
        HowlProfScope prof("cnn_head", stream, 2.0 * HID * (q.F + num_labels) * (double)q.rows);
        const int gin = grid_for((size_t)rows * q.F);
        if (training)
            hipLaunchKernelGGL(cnn_head_in_kernel<true>, dim3(gin), dim3(256), 0, stream, (const float*)q.Q, bn2, (const float*)q.stat2, B, q.H2,
                               q.seq ? 1 : 0, q.Xh);
        else
            hipLaunchKernelGGL(cnn_head_in_kernel<false>, dim3(gin), dim3(256), 0, stream, (const float*)q.Q, bn2, (const float*)nullptr, B, q.H2,
                               q.seq ? 1 : 0, q.Xh);
        gemm(stream, true, q.Xh, lin(q.F), 1, lin(0), p->w1, lin(1), q.F, rows, HID, q.F, 1, p->b1, 1, q.y1, HID, 0);
        hipLaunchKernelGGL(cnn_head_out_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, q.y1, p->w2, p->b2, drop_mask, keep_scale, rows, B,
                           q.seq ? q.H2 : 1, num_labels, logits);
    }
    HOWL_CHECK_LAUNCH("howl_cnn_fwd");
    return HOWL_OK;
}

int howl_cnn_bwd(int kind, const HowlCnnParams* p, const float* x, long sb, long sm, long st, int B, int M, int T, int num_labels,
                 float keep_scale, const float* dlogits, const HowlCnnGrads* g, void* ws, size_t ws_bytes, hipStream_t stream) {
    HOWL_REQUIRE(p && x && dlogits && g && ws && all_set(reinterpret_cast<const void* const*>(p), 12) &&
                     all_set(reinterpret_cast<const void* const*>(g), 12), "howl_cnn_bwd: null pointer");
    const CnnPlan q = cnn_plan(kind, B, M, T, num_labels, ws);
    HOWL_REQUIRE(q.bad[0] == 0, "howl_cnn_bwd: %s", q.bad);
    if (ws_bytes < q.bytes) {
        howl_set_error("howl_cnn_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, q.bytes);
        return HOWL_E_WORKSPACE;
    }
    const int rows = (int)q.rows, seq = q.seq ? 1 : 0, n1 = q.Hp * WP, n2 = q.H2 * W2;
    SlabSums sums;
    {
        HowlProfScope prof("cnn_head", stream, 4.0 * HID * (q.F + num_labels) * (double)q.rows);
        hipLaunchKernelGGL(cnn_head_dz_kernel, dim3(grid_for((size_t)rows * HID)), dim3(256), 0, stream, dlogits, (const float*)q.y1, p->w2,
                           keep_scale, (size_t)rows * HID, num_labels, q.dz1);
    }
    wgrad_gemm(stream, dlogits, lin(num_labels), num_labels, q.y1, lin(HID), HID, rows, q.slabs_w2, g->w2, HEAD_SPLITS, 256, &sums);
    colsum(stream, dlogits, lin(num_labels), rows, num_labels, q.scratch_b2, g->b2, nullptr, 64, 256, &sums);
    wgrad_gemm(stream, q.dz1, lin(HID), HID, q.Xh, lin(q.F), q.F, rows, q.slabs_w1, g->w1, HEAD_SPLITS, 256, &sums);
    colsum(stream, q.dz1, lin(HID), rows, HID, q.scratch_b1, g->b1, nullptr, 64, 256, &sums);
    if (!sums.flush(stream)) return HOWL_E_ARG;
    gemm(stream, true, q.dz1, lin(HID), 1, lin(0), p->w1, lin(q.F), 1, rows, q.F, HID, 1, nullptr, 0, q.dXh, q.F, 0);
    {
        HowlProfScope prof("cnn_conv1_bwd", stream, 2.0 * C2 * K1 * (1.0 * q.H2 * W2 + 2.0 * q.Hp * WP / 2.0) * B);
        hipLaunchKernelGGL(cnn_bn_bwd_sums_kernel<true>, dim3(B), dim3(256), 0, stream, (const float*)q.dXh, (const float*)q.Q, (const float*)q.stat2,
                           C2, n2, q.H2, seq, q.part3);
        hipLaunchKernelGGL(cnn_bn_bwd_fold_kernel, dim3(C2), dim3(256), 0, stream, (const double*)q.part3, B, C2, q.count2, q.m2, g->bn2_w, g->bn2_b);
        hipLaunchKernelGGL(cnn_pool_grad_kernel, dim3(B), dim3(256), 0, stream, (const float*)q.dXh, (const float*)q.Q, p->bn2_w,
                           (const float*)q.stat2, (const float*)q.m2, q.H2, seq, q.G2, q.bpart);
        hipLaunchKernelGGL(cnn_conv1_wgrad_kernel, dim3(C2, q.gs1), dim3(256), 0, stream, (const float*)q.G2, (const unsigned char*)q.I2,
                           (const float*)q.P, p->bn1_w, p->bn1_b, (const float*)q.stat1, B, q.Hp, q.H2, q.slabs1);
        hipLaunchKernelGGL(cnn_conv1_dgrad_kernel, dim3(q.ntiled, B), dim3(256), 0, stream, (const float*)q.G2, (const unsigned char*)q.I2,
                           p->conv1_w, q.Hp, q.H2, q.dPn);
    }
    {
        HowlProfScope prof("cnn_conv0_bwd", stream, 2.0 * C1 * q.KT * KF * (double)q.Hp * WP * B);
        hipLaunchKernelGGL(cnn_bn_bwd_sums_kernel<false>, dim3(B), dim3(256), 0, stream, (const float*)q.dPn, (const float*)q.P, (const float*)q.stat1,
                           C1, n1, q.H2, seq, q.part4);
        hipLaunchKernelGGL(cnn_bn_bwd_fold_kernel, dim3(C1), dim3(256), 0, stream, (const double*)q.part4, B, C1, q.count1, q.m1, g->bn1_w, g->bn1_b);
        const dim3 grid(q.gx0, q.gy0);
        if (q.seq)
            hipLaunchKernelGGL((cnn_conv0_wgrad_kernel<20, 1>), grid, dim3(256), 0, stream, x, sb, sm, st, T, q.Hp, B, q.ntile0, (const float*)q.P,
                               (const unsigned char*)q.I1, (const float*)q.dPn, p->bn1_w, (const float*)q.stat1, (const float*)q.m1, q.cpart0);
        else
            hipLaunchKernelGGL((cnn_conv0_wgrad_kernel<8, 2>), grid, dim3(256), 0, stream, x, sb, sm, st, T, q.Hp, B, q.ntile0, (const float*)q.P,
                               (const unsigned char*)q.I1, (const float*)q.dPn, p->bn1_w, (const float*)q.stat1, (const float*)q.m1, q.cpart0);
    }
    const int K0 = C1 * q.KT * KF;
    sums.add(q.slabs1, q.gs1, (long)C2 * K1, g->conv1_w);
    sums.add(q.bpart, B, C2, g->conv1_b);
    sums.add_strided(q.cpart0, q.gx0 * q.gy0, K0 + C1, K0, g->conv0_w);
    sums.add_strided(q.cpart0 + K0, q.gx0 * q.gy0, K0 + C1, C1, g->conv0_b);
    if (!sums.flush(stream)) return HOWL_E_ARG;
    HOWL_CHECK_LAUNCH("howl_cnn_bwd");
    return HOWL_OK;
}

}  // extern "C"
