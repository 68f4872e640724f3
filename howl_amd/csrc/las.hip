// The "las" classifier for gfx950 (MI355X), howl/model/rnn.py:133-215 (LASClassifier): conv encoder with two training-mode
// BatchNorms, bidirectional LSTM(352 -> 96) on a packed batch, four-head fixed attention over the utterance's own steps,
// Linear - ReLU - Dropout - Linear.  One call per direction (include/howl_hip_las.h), one launch plan per call (las_plan).
//
// Forward launches:                                               backward launches:
//   las_conv1_kernel     Z1 = conv1(x), BN1 batch sums              las_head_bwd_kernel      dz1, d ctx          (+ 4 GEMM-path jobs)
//   las_conv2_kernel     BN1-ReLU-pool where Z1 is staged,          las_attn_bwd_kernel      dV, dK, d context_vec per utterance
//                        Z2 = conv2(.), BN2 batch sums              wgrad_gemm x 2, colsum, gemm x 2: dW_v, dW_k, db_k, d rnn_seq
//   las_feat_kernel      BN2-ReLU-pool -> features (B,T2,352)       las_lstm_bwd4_kernel     BPTT of both directions, dG, bias sums
//   gemm x 2             Gx = F W_ih^T, both directions             wgrad_gemm x 4, gemm x 2: dW_ih, dW_hh, dF
//   las_lstm_fwd4_kernel both directions, one launch                las_bn2_sums_kernel      un-pool + ReLU, BN2's batch sums
//   gemm x 2             V = v_proj(h), K = k_proj(h)               las_conv2_bwd_kernel     BN2, conv2 dw / data, un-pool + ReLU, BN1's sums
//   las_attn_fwd_kernel  scores and weighted sum, one pass          las_conv1_bwd_kernel     BN1, conv1 dw
//   las_head_fwd_kernel  the head on (B, 192)                       sum_slabs_multi_kernel x 3: every partial sum, fixed order
// The batch-wide BatchNorm reductions are exchanged at launch boundaries only: a launch leaves one partial sum per workgroup, the
// next one folds them (every workgroup folds the same numbers in the same order).  No workgroup waits on another.
//
// Kept for the backward, per utterance (W1 = T + 2, T1 = W1 / 2, W2 = T1 + 2, T2 = W2 / 2 steps): conv1's output Z1 (8 x 42 x W1)
// 1344 W1 B, conv2's output Z2 (W2, 8 x 44) 1408 W2 B, the features F 1408 T2 B, the input projections Gx 3072 T2 B, the gates
// i, f, g, o and the cell state of both directions 3840 T2 B, the hidden sequence 768 (T2 + 2) B, V and K 1536 T2 B, the attention
// logits 16 T2 B, ctx and the head's masked hidden row.  Recomputed from those: both pooled activations, both ReLU masks and both
// pools' argmax (the same fmaf of the same numbers as the forward: the same bits), tanh(c) and the attention scores.
#include <math.h>

#include "howl_common.hip.h"
#include "../../include/howl_hip_las.h"
#include "howl_gemm.hip.h"
#include "howl_lstm.hip.h"

namespace {

constexpr int LH = 96;             // hidden units per direction
constexpr int L4 = 4 * LH;         // gate rows, PyTorch order i, f, g, o
constexpr int LSV = 5 * LH;        // saved per step and direction: i, f, g, o, c
constexpr int LD = 2 * LH;         // rnn_seq / attention width
constexpr int LM = 40;             // mel bins
constexpr int LXC = 3;             // feature channels
constexpr int LC = 8;              // latent channels
constexpr int LR1 = LM + 2;        // rows of conv1's output
constexpr int LR2 = LM + 4;        // rows of conv2's output
constexpr int LF = LC * LR2;       // LSTM input features, index channel * 44 + mel
constexpr int LHD = 256;           // head's hidden width
constexpr int LHEADS = 4, LHW = LD / LHEADS;
constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;
constexpr int ENC_THREADS = 256;
constexpr int LT = 16;             // columns per workgroup of the encoder kernels (of conv1's or conv2's output) ...
constexpr int LTW = LT + 2;        // ... and with the 3 x 3 halo
constexpr int LPW = LTW + 1;       // LDS row stride of the tiles (odd: rows fastest over the lanes without bank conflicts)
constexpr int FEAT_STEPS = 4;      // steps per workgroup of the feature kernel
constexpr int LAS_WGRAD_SPLITS = 32, LAS_HEAD_SPLITS = 8;

// sums of NS statistics over `nparts` partial rows (doubles), by the first 256 threads of the workgroup in a fixed order; every
// thread of the workgroup must call (two barriers).  scratch: 256 doubles; tot: NS doubles
template <int NS>
__device__ __forceinline__ void fold_parts(const double* __restrict__ part, int nparts, double* scratch, double* tot) {
    constexpr int NCH = 256 / NS;
    const int tid = threadIdx.x;
    if (tid < 256) {
        const int s = tid % NS, ch = tid / NS;
        double a = 0.0;
        int i = ch;
        for (; i + 7 * NCH < nparts; i += 8 * NCH) {      // eight independent loads in flight; the order of the additions is fixed
            double v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = part[(size_t)(i + e * NCH) * NS + s];
#pragma unroll
            for (int e = 0; e < 8; ++e) a += v[e];
        }
        for (; i < nparts; i += NCH) a += part[(size_t)i * NS + s];
        scratch[ch * NS + s] = a;
    }
    __syncthreads();
    if (tid < NS) {
        double a = 0.0;
        for (int ch = 0; ch < NCH; ++ch) a += scratch[ch * NS + tid];
        tot[tid] = a;
    }
    __syncthreads();
}

// N per-thread doubles -> one row of partial sums (four waves, fixed order)
template <int N>
__device__ __forceinline__ void block_sum_d(double (&v)[N], double (*red)[N], double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double s = wave_sum_d(v[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) out[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// y = z * sc + sh of a BatchNorm channel from its mean and 1 / sqrt(var + eps) as fp32 (forward and backward take these two
// numbers from the same place, so both get the same sc / sh)
__device__ __forceinline__ void bn_affine(float gamma, float beta, float mean, float invstd, float& sc, float& sh) {
    sc = gamma * invstd;
    sh = beta - mean * sc;
}

struct LasBn {      // one BatchNorm of the encoder
    const float *gamma, *beta;
    float *rmean, *rvar;
    long long* batches;
};

// Eight channels' BatchNorm from batch sums (TRAIN; `first` also writes stat = mean[8], invstd[8] and updates the running
// buffers) or from the running buffers, by threads 0..7.  tot: sum z [8], sum z^2 [8]
template <bool TRAIN>
__device__ __forceinline__ void bn_setup(const LasBn& bn, const double* tot, double count, bool first, float* __restrict__ stat, float* sc,
                                         float* sh) {
    const int tid = threadIdx.x;
    if (tid >= LC) return;
    if constexpr (TRAIN) {
        const double mean = tot[tid] / count;
        const double var = fmax(tot[8 + tid] / count - mean * mean, 0.0);
        const float meanf = (float)mean, invstd = (float)(1.0 / sqrt(var + (double)BN_EPS));
        bn_affine(bn.gamma[tid], bn.beta[tid], meanf, invstd, sc[tid], sh[tid]);
        if (first) {
            stat[tid] = meanf;
            stat[8 + tid] = invstd;
            bn.rmean[tid] = (1.0f - BN_MOMENTUM) * bn.rmean[tid] + BN_MOMENTUM * meanf;
            bn.rvar[tid] = (1.0f - BN_MOMENTUM) * bn.rvar[tid] + BN_MOMENTUM * (float)(var * count / fmax(count - 1.0, 1.0));
            if (tid == 0) bn.batches[0] += 1;
        }
    } else {
        bn_affine(bn.gamma[tid], bn.beta[tid], bn.rmean[tid], 1.0f / sqrtf(bn.rvar[tid] + BN_EPS), sc[tid], sh[tid]);
    }
}

// recurrence steps of an utterance of `len` frames (clamped to the buffer's T)
__device__ __forceinline__ int las_steps(const long long* __restrict__ lengths, int b, int T) {
    const int len = lengths != nullptr ? (int)max(0LL, min(lengths[b], (long long)T)) : T;
    return (((len + 2) / 2) + 2) / 2;
}

// x tile of one utterance in LDS: xt[ch][r][c] = x(ch, mel r - 2, frame w0 - 2 + c), zero outside (conv1's padding of 2)
__device__ __forceinline__ void load_x_tile(const float* __restrict__ xb, long sc, long sm, long st, int T, int w0, float* xt) {
    const bool m_fast = sm == 1;      // time-major features: the mel index runs fastest over the lanes
    for (int i = threadIdx.x; i < LXC * LR2 * LTW; i += ENC_THREADS) {
        const int ch = i / (LR2 * LTW), j = i - ch * (LR2 * LTW);
        const int r = m_fast ? j % LR2 : j / LTW, c = m_fast ? j / LR2 : j % LTW;
        const int mm = r - 2, tt = w0 - 2 + c;
        xt[(ch * LR2 + r) * LPW + c] = (mm >= 0 && mm < LM && tt >= 0 && tt < T) ? xb[ch * sc + (long)mm * sm + (long)tt * st] : 0.0f;
    }
}

// Z1 (B,8,42,W1) = conv1(x) on one tile of LT columns of one utterance: x tile and weights in LDS, one output position per thread
// and round, eight accumulators.  STATS: part[(b, tile)][c] = sum z_c, [8 + c] = sum z_c^2.
template <bool STATS>
__global__ __launch_bounds__(ENC_THREADS) void las_conv1_kernel(const float* __restrict__ x, long sb, long sc, long sm, long st, int T,
                                                                const float* __restrict__ c1w, const float* __restrict__ c1b,
                                                                float* __restrict__ Z1, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float cw[27 * LC];      // [(ch * 9 + k) * 8 + co]
    __shared__ float cb[LC];
    __shared__ float xt[LXC * LR2 * LPW];
    __shared__ double red[4][16];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int W1 = T + 2, w0 = tile * LT;
    if (tid < 27 * LC) cw[(tid % 27) * LC + tid / 27] = c1w[tid];
    if (tid >= 224 && tid < 224 + LC) cb[tid - 224] = c1b[tid - 224];
    load_x_tile(x + (long)b * sb, sc, sm, st, T, w0, xt);
    __syncthreads();
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
#pragma unroll 1
    for (int i = tid; i < LR1 * LT; i += ENC_THREADS) {
        const int h = i / LT, cc = i - h * LT, w = w0 + cc;
        if (w >= W1) continue;
        int wo = 0;      // opaque per item: the 216 weights stay LDS broadcast reads and are not hoisted into registers of their own
        HOWL_OPAQUE_V(wo);
        float z[LC];
#pragma unroll
        for (int co = 0; co < LC; ++co) z[co] = cb[co];
#pragma unroll
        for (int ch = 0; ch < LXC; ++ch)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = xt[(ch * LR2 + h + dy) * LPW + cc + dx];
                    const float4 wa = *reinterpret_cast<const float4*>(&cw[wo + (ch * 9 + dy * 3 + dx) * LC]);
                    const float4 wb = *reinterpret_cast<const float4*>(&cw[wo + (ch * 9 + dy * 3 + dx) * LC + 4]);
                    z[0] = fmaf(wa.x, v, z[0]);
                    z[1] = fmaf(wa.y, v, z[1]);
                    z[2] = fmaf(wa.z, v, z[2]);
                    z[3] = fmaf(wa.w, v, z[3]);
                    z[4] = fmaf(wb.x, v, z[4]);
                    z[5] = fmaf(wb.y, v, z[5]);
                    z[6] = fmaf(wb.z, v, z[6]);
                    z[7] = fmaf(wb.w, v, z[7]);
                }
#pragma unroll
        for (int co = 0; co < LC; ++co) {
            Z1[(((size_t)b * LC + co) * LR1 + h) * W1 + w] = z[co];
            if constexpr (STATS) {
                acc[co] += (double)z[co];
                acc[8 + co] += (double)z[co] * (double)z[co];
            }
        }
    }
    if constexpr (STATS) block_sum_d<16>(acc, red, part + ((size_t)b * gridDim.x + tile) * 16);
}

// pooled tile of one utterance in LDS: pt[ci][r][c] = max over the column pair of relu(BN1(Z1)) at (row r - 2, pooled column
// w0 - 2 + c), zero outside (conv2's padding of 2)
__device__ __forceinline__ void load_pool_tile(const float* __restrict__ Z1, int b, int W1, int T1, int w0, const float* sc, const float* sh,
                                               float* pt) {
    for (int i = threadIdx.x; i < LC * (LR1 + 4) * LTW; i += ENC_THREADS) {
        const int ci = i / ((LR1 + 4) * LTW), j = i - ci * ((LR1 + 4) * LTW);
        const int r = j / LTW, c = j - r * LTW;
        const int row = r - 2, p = w0 - 2 + c;
        float v = 0.0f;
        if (row >= 0 && row < LR1 && p >= 0 && p < T1) {
            const float* z = Z1 + (((size_t)b * LC + ci) * LR1 + row) * W1 + 2 * p;
            v = fmaxf(fmaxf(fmaf(z[0], sc[ci], sh[ci]), fmaf(z[1], sc[ci], sh[ci])), 0.0f);
        }
        pt[(ci * (LR1 + 4) + r) * LPW + c] = v;
    }
}

// Z2 (B,W2,8,44) = conv2(pool(relu(BN1(Z1)))) on one tile of LT columns of one utterance.  TRAIN: BN1 from the launch before's
// partial sums (workgroup (0, 0) writes stat1 and updates the running buffers) and part2[(b, tile)] = sum z, sum z^2 per channel.
template <bool TRAIN>
__global__ __launch_bounds__(ENC_THREADS) void las_conv2_kernel(const float* __restrict__ Z1, int T, const float* __restrict__ c2w,
                                                                const float* __restrict__ c2b, LasBn bn1, const double* __restrict__ part1,
                                                                int nparts1, double count1, float* __restrict__ stat1,
                                                                float* __restrict__ Z2, double* __restrict__ part2) {
    __shared__ __attribute__((aligned(16))) float cw[72 * LC];      // [(ci * 9 + k) * 8 + co]
    __shared__ float cb[LC], sc[LC], sh[LC];
    __shared__ float pt[LC * (LR1 + 4) * LPW];
    __shared__ double scratch[256], tot[16], red[4][16];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int W1 = T + 2, T1 = W1 / 2, W2 = T1 + 2, w0 = tile * LT;
    for (int i = tid; i < 72 * LC; i += ENC_THREADS) cw[(i % 72) * LC + i / 72] = c2w[i];
    if (tid >= 248) cb[tid - 248] = c2b[tid - 248];
    if constexpr (TRAIN) fold_parts<16>(part1, nparts1, scratch, tot);
    bn_setup<TRAIN>(bn1, tot, count1, tile == 0 && b == 0, stat1, sc, sh);
    __syncthreads();
    load_pool_tile(Z1, b, W1, T1, w0, sc, sh, pt);
    __syncthreads();
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
#pragma unroll 1
    for (int i = tid; i < LR2 * LT; i += ENC_THREADS) {
        const int cc = i / LR2, h = i - cc * LR2, w = w0 + cc;
        if (w >= W2) continue;
        float z[LC];
#pragma unroll
        for (int co = 0; co < LC; ++co) z[co] = cb[co];
#pragma unroll 1
        for (int ci = 0; ci < LC; ++ci) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = pt[(ci * (LR1 + 4) + h + dy) * LPW + cc + dx];
                    const float4 wa = *reinterpret_cast<const float4*>(&cw[(ci * 9 + dy * 3 + dx) * LC]);
                    const float4 wb = *reinterpret_cast<const float4*>(&cw[(ci * 9 + dy * 3 + dx) * LC + 4]);
                    z[0] = fmaf(wa.x, v, z[0]);
                    z[1] = fmaf(wa.y, v, z[1]);
                    z[2] = fmaf(wa.z, v, z[2]);
                    z[3] = fmaf(wa.w, v, z[3]);
                    z[4] = fmaf(wb.x, v, z[4]);
                    z[5] = fmaf(wb.y, v, z[5]);
                    z[6] = fmaf(wb.z, v, z[6]);
                    z[7] = fmaf(wb.w, v, z[7]);
                }
        }
#pragma unroll
        for (int co = 0; co < LC; ++co) {
            Z2[((size_t)b * W2 + w) * LF + co * LR2 + h] = z[co];
            if constexpr (TRAIN) {
                acc[co] += (double)z[co];
                acc[8 + co] += (double)z[co] * (double)z[co];
            }
        }
    }
    if constexpr (TRAIN) block_sum_d<16>(acc, red, part2 + ((size_t)b * gridDim.x + tile) * 16);
}

// F (B,T2,352) = max over the column pair of relu(BN2(Z2)), FEAT_STEPS steps of one utterance per workgroup.  TRAIN: BN2 from the
// launch before's partial sums (workgroup (0, 0) writes stat2 and updates the running buffers).
template <bool TRAIN>
__global__ __launch_bounds__(ENC_THREADS) void las_feat_kernel(const float* __restrict__ Z2, int W2, int T2, LasBn bn2,
                                                               const double* __restrict__ part2, int nparts2, double count2,
                                                               float* __restrict__ stat2, float* __restrict__ F) {
    __shared__ float sc[LC], sh[LC];
    __shared__ double scratch[256], tot[16];
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * FEAT_STEPS;
    if constexpr (TRAIN) fold_parts<16>(part2, nparts2, scratch, tot);
    bn_setup<TRAIN>(bn2, tot, count2, blockIdx.x == 0 && b == 0, stat2, sc, sh);
    __syncthreads();
    const int n = min(FEAT_STEPS, T2 - t0) * LF;
    for (int i = tid; i < n; i += ENC_THREADS) {
        const int tt = i / LF, j = i - tt * LF, c = j / LR2, t = t0 + tt;
        const float* z = Z2 + ((size_t)b * W2 + 2 * t) * LF + j;
        F[((size_t)b * T2 + t) * LF + j] = fmaxf(fmaxf(fmaf(z[0], sc[c], sh[c]), fmaf(z[LF], sc[c], sh[c])), 0.0f);
    }
}

// Forward recurrence of BOTH directions in one launch, FOUR sequences per workgroup on v_mfma_f32_4x4x1 (lstm_fwd4_kernel's scheme:
// block = hidden unit, block row = sequence, the A operand by block broadcast, one barrier per step with h double-buffered in LDS).
// Workgroups 0 .. nrec-1 run the forward direction, nrec .. 2 nrec-1 the reverse one.  Six waves, wave c = units 16c .. 16c+15; the
// four block columns of unit u over K = 96 are the gates i, f, g, o of W_hh.  Lane 4j+g holds gate g of unit 16c+j for the four
// sequences; the in-quad transpose hands it the four gates of (sequence g, unit 16c+j), where the precomputed input projection
// Gx (B,T2,2,384) and b_ih + b_hh are added and the cell is updated once.  The reverse direction walks t = T2-1 .. 0 and a sequence
// joins at its own step n_b - 1 with the zero state it still has (per-sequence masking; nothing is reversed on the host).  hs
// (B,T2+2,192): row t + 1 = (h_fwd, h_rev) of step t, zero for t >= n_b and in the two border rows (h before the first step of
// either direction).  Sequences past the end of the batch are copies of the last one: every store is unconditional.
constexpr int LF_THREADS = 384;
constexpr int LF_HS = LH + 4;     // h rows in LDS (16-byte aligned rows for the float4 A-fragment reads)
constexpr int LF_AHEAD = 3;       // steps whose input projection is in flight
template <bool TRAIN>
__global__ __launch_bounds__(LF_THREADS) void las_lstm_fwd4_kernel(const float* __restrict__ Gx, const float* __restrict__ whh_f,
                                                                   const float* __restrict__ bih_f, const float* __restrict__ bhh_f,
                                                                   const float* __restrict__ whh_r, const float* __restrict__ bih_r,
                                                                   const float* __restrict__ bhh_r, const long long* __restrict__ lengths,
                                                                   float* __restrict__ gates, float* __restrict__ hs, int B, int T, int T2,
                                                                   int nrec) {
    __shared__ __attribute__((aligned(16))) float hbuf[2][4 * LF_HS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 2, g = lane & 3;
    const int u = 16 * c + j;
    const int dir = (int)blockIdx.x >= nrec ? 1 : 0;
    const int b0 = ((int)blockIdx.x - dir * nrec) * 4;
    const float* whh = dir ? whh_r : whh_f;
    const float* b_ih = dir ? bih_r : bih_f;
    const float* b_hh = dir ? bhh_r : bhh_f;
    float wB[LH];      // the lane's weight row, read in place: no packing launch
#pragma unroll
    for (int k = 0; k < LH; ++k) wB[k] = whh[(size_t)(g * LH + u) * LH + k];
    float bias[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bias[k] = b_ih[k * LH + u] + b_hh[k * LH + u];
    // cell role: sequence g of the workgroup, unit u
    const int bc = min(b0 + g, B - 1);
    const int len = min(las_steps(lengths, bc, T), T2);
    float hst = 0.0f, cst = 0.0f;
    hbuf[0][g * LF_HS + u] = 0.0f;
    float* hrow = hs + (size_t)bc * (T2 + 2) * LD + dir * LH + u;
    hrow[0] = 0.0f;
    hrow[(size_t)(T2 + 1) * LD] = 0.0f;
    const float* gxb = Gx + (size_t)bc * T2 * (2 * L4) + dir * L4 + u;
    // the input projections of the next LF_AHEAD steps are in flight: a step is shorter than a trip to memory, so a request made
    // one step ahead would be waited for.  The step loop is unrolled by LF_AHEAD so that slot d is a fixed set of registers.
    float gq[LF_AHEAD][4];
#pragma unroll
    for (int d = 0; d < LF_AHEAD; ++d) {
        const int sn = min(d, T2 - 1), t = dir ? T2 - 1 - sn : sn;
#pragma unroll
        for (int k = 0; k < 4; ++k) gq[d][k] = gxb[(size_t)t * (2 * L4) + k * LH];
    }
    const int jh = j < (LH - 64) / 4 ? j : 0;      // lanes beyond K re-read block 0: never multiplied
    __syncthreads();
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): the weight loads are complete before the loop (see lstm_fwd4_kernel)
    for (int s0 = 0; s0 < T2; s0 += LF_AHEAD)
#pragma unroll
    for (int d = 0; d < LF_AHEAD; ++d) {
        const int s = s0 + d;
        if (s >= T2) break;
        const int t = dir ? T2 - 1 - s : s;
        const float* hcur = hbuf[s & 1];
        float* hnxt = hbuf[(s + 1) & 1];
        float gc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) gc[k] = gq[d][k];
        {
            const int sn = min(s + LF_AHEAD, T2 - 1), tn = dir ? T2 - 1 - sn : sn;
#pragma unroll
            for (int k = 0; k < 4; ++k) gq[d][k] = gxb[(size_t)tn * (2 * L4) + k * LH];
        }
        const float4 alo = *reinterpret_cast<const float4*>(hcur + g * LF_HS + 4 * j);
        const float4 ahi = *reinterpret_cast<const float4*>(hcur + g * LF_HS + 64 + 4 * jh);
        f32x4 acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = {0.0f, 0.0f, 0.0f, 0.0f};
        bcast_mfma64<0, 0, LH, 16>(alo, wB, acc);
        bcast_mfma64<0, 64, LH, (LH - 64) / 4>(ahi, wB, acc);
        const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = sum[r];
        quad_transpose(v, (g & 1) != 0, (g & 2) != 0);      // -> W_hh h of the gates i, f, g, o of (sequence g, unit u)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (v[k] + gc[k]) + bias[k];
        const float ig = sigmoidf_(v[0]), fg = sigmoidf_(v[1]), gg = tanhf_(v[2]), og = sigmoidf_(v[3]);
        const float cn = fmaf(fg, cst, ig * gg);
        const float hn = og * tanhf_(cn);
        const bool active = t < len;
        cst = active ? cn : cst;
        hst = active ? hn : hst;
        hnxt[g * LF_HS + u] = hst;
        hrow[(size_t)(t + 1) * LD] = active ? hn : 0.0f;
        if constexpr (TRAIN) {
            float* go = gates + (((size_t)bc * T2 + t) * 2 + dir) * LSV + u;
            go[0] = ig;
            go[LH] = fg;
            go[2 * LH] = gg;
            go[3 * LH] = og;
            go[4 * LH] = active ? cn : 0.0f;
        }
        __syncthreads();
    }
}

// The attention of one utterance, one wave per head: logit_t = sum_l V[t, 48k+l] context_vec[4l+k], softmax over the utterance's
// n_b steps and ctx[48k+l] = sum_t score_t K[t, 48k+l] in ONE pass over the rows (running maximum and rescaled sums).  Kept when
// given: the logits lgt (B,T2,4) and the softmax's maximum and denominator ms (B,4,2), from which the backward rebuilds the scores.
__global__ __launch_bounds__(256) void las_attn_fwd_kernel(const float* __restrict__ V, const float* __restrict__ K,
                                                           const float* __restrict__ cv, const long long* __restrict__ lengths, int T, int T2,
                                                           float* __restrict__ ctx, float* __restrict__ lgt, float* __restrict__ ms) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int n = min(las_steps(lengths, b, T), T2);
    const bool on = lane < LHW;
    const int col = LHW * k + (on ? lane : 0);
    const float cvl = on ? cv[4 * lane + k] : 0.0f;
    float m = -INFINITY, s = 0.0f, acc = 0.0f;
    for (int t = 0; t < n; ++t) {
        const size_t o = ((size_t)b * T2 + t) * LD + col;
        const float kk = K[o];
        const float lg = wave_sum(V[o] * cvl);
        const float mn = fmaxf(m, lg);
        const float scale = expf(m - mn), p = expf(lg - mn);
        s = fmaf(s, scale, p);
        acc = fmaf(acc, scale, p * kk);
        m = mn;
        if (lgt != nullptr && lane == 0) lgt[((size_t)b * T2 + t) * LHEADS + k] = lg;
    }
    if (on) ctx[(size_t)b * LD + col] = acc / s;
    if (ms != nullptr && lane == 0) {
        ms[((size_t)b * LHEADS + k) * 2] = m;
        ms[((size_t)b * LHEADS + k) * 2 + 1] = s;
    }
}

// The head on the (B, 192) context rows, one workgroup per utterance: y1 = relu(ctx W1^T + b1), y1d = y1 * mask * keep_scale,
// logits = y1d W2^T + b2.  y1d (kept when given) carries both the ReLU's and the dropout's mask for the backward: y1d > 0.
__global__ __launch_bounds__(256) void las_head_fwd_kernel(const float* __restrict__ ctx, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, const float* __restrict__ mask, float keep_scale,
                                                           int C, float* __restrict__ y1d, float* __restrict__ logits) {
    __shared__ float hs[LD], ys[LHD];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < LD) hs[tid] = ctx[(size_t)b * LD + tid];
    __syncthreads();
    {
        float a = b1[tid];
        for (int k = 0; k < LD; ++k) a = fmaf(w1[tid * LD + k], hs[k], a);
        float y = fmaxf(a, 0.0f);
        if (mask != nullptr) y = y * mask[(size_t)b * LHD + tid] * keep_scale;
        ys[tid] = y;
        if (y1d != nullptr) y1d[(size_t)b * LHD + tid] = y;
    }
    __syncthreads();
    for (int cl = wave; cl < C; cl += 4) {
        float a = 0.0f;
        for (int k = lane; k < LHD; k += 64) a = fmaf(w2[(size_t)cl * LHD + k], ys[k], a);
        a = wave_sum(a);
        if (lane == 0) logits[(size_t)b * C + cl] = a + b2[cl];
    }
}

// dz1 = (y1d > 0) keep_scale (dlogits W2), d ctx = dz1 W1; the four weight gradients are reductions over the B rows (GEMM path)
__global__ __launch_bounds__(256) void las_head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ y1d,
                                                           const float* __restrict__ w1, const float* __restrict__ w2, float keep_scale,
                                                           int C, float* __restrict__ dz1, float* __restrict__ dctx) {
    __shared__ float dls[HOWL_LAS_MAX_LABELS], dzs[LHD];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid < C) dls[tid] = dlogits[(size_t)b * C + tid];
    __syncthreads();
    {
        float a = 0.0f;
        for (int cl = 0; cl < C; ++cl) a = fmaf(dls[cl], w2[(size_t)cl * LHD + tid], a);
        const float dz = y1d[(size_t)b * LHD + tid] > 0.0f ? a * keep_scale : 0.0f;
        dzs[tid] = dz;
        dz1[(size_t)b * LHD + tid] = dz;
    }
    __syncthreads();
    if (tid < LD) {
        float a = 0.0f;
        for (int k = 0; k < LHD; ++k) a = fmaf(dzs[k], w1[k * LD + tid], a);
        dctx[(size_t)b * LD + tid] = a;
    }
}

// The attention's backward of one utterance, one wave per head, one pass over its rows: score_t = exp(logit_t - m) / s,
// dK[t] = score_t d ctx, d score_t = d ctx . K[t], d logit_t = score_t (d score_t - d ctx . ctx), dV[t] = d logit_t context_vec,
// cvpart[b] = sum_t d logit_t V[t] (laid out as context_vec).  Rows of steps the utterance did not run are zero.  v_proj's BIAS adds
// the same constant to every step's logit of a head and the softmax over time ignores it: its gradient, the sum of d logit over
// the steps, is identically zero and is written as that zero (by workgroup 0), not as the rounding residue of a cancelling sum.
__global__ __launch_bounds__(256) void las_attn_bwd_kernel(const float* __restrict__ V, const float* __restrict__ K,
                                                           const float* __restrict__ cv, const long long* __restrict__ lengths, int T, int T2,
                                                           const float* __restrict__ ctx, const float* __restrict__ lgt,
                                                           const float* __restrict__ ms, const float* __restrict__ dctx,
                                                           float* __restrict__ dV, float* __restrict__ dK, float* __restrict__ cvpart,
                                                           float* __restrict__ g_vb) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int n = min(las_steps(lengths, b, T), T2);
    const bool on = lane < LHW;
    const int col = LHW * k + (on ? lane : 0);
    const float cvl = on ? cv[4 * lane + k] : 0.0f;
    const float dc = on ? dctx[(size_t)b * LD + col] : 0.0f;
    const float dot = wave_sum(dc * ctx[(size_t)b * LD + col]);
    const float m = ms[((size_t)b * LHEADS + k) * 2], rs = 1.0f / ms[((size_t)b * LHEADS + k) * 2 + 1];
    float dcv = 0.0f;
    for (int t = 0; t < T2; ++t) {
        const size_t o = ((size_t)b * T2 + t) * LD + col;
        float dv = 0.0f, dk = 0.0f;
        if (t < n) {
            const float score = expf(lgt[((size_t)b * T2 + t) * LHEADS + k] - m) * rs;
            const float ds = wave_sum(dc * K[o]);
            const float dl = score * (ds - dot);
            dk = score * dc;
            dv = dl * cvl;
            dcv = fmaf(dl, V[o], dcv);
        }
        if (on) {
            dV[o] = dv;
            dK[o] = dk;
        }
    }
    if (on) cvpart[(size_t)b * LD + 4 * lane + k] = dcv;
    if (b == 0 && threadIdx.x < LD) g_vb[threadIdx.x] = 0.0f;
}

// Backward recurrence of both directions in one launch, four sequences per workgroup (lstm_bwd4_kernel's scheme):
// d h_prev[4][96] = dG_t[4][384] W_hh on v_mfma_f32_4x4x1.  Eight waves: wave w = (hidden-column chunk ch = w & 1 of 64, of which
// the second holds 32 columns and 32 copies of the last; K range kr = w >> 1: the i, f, g or o block of dG, 96 W_hh registers per
// lane); the four K ranges meet in LDS and are summed in a fixed order by the thread that owns the cell, thread (sequence tid / 96,
// unit tid % 96) of the first 384.  The forward direction's gradient walks t = T2-1 .. 0, the reverse direction's t = 0 .. T2-1.
//   dh (2,B,T2,192): the two halves of d rnn_seq (through v_proj and through k_proj), added where they are read
//   dG (B,T2,2,384) = d i~, d f~, d g~, d o~     (for dW_ih, dW_hh, both biases and dF) -- rows of steps not run are zero
// bpart[workgroup][384]: this workgroup's sums over steps and sequences of dG (both bias gradients of its direction).
constexpr int LB_THREADS = 512;
constexpr int LB_DGS = L4 + 4;      // dG rows in LDS (16-byte aligned rows)
constexpr int LB_PS = 128 + 4;
__global__ __launch_bounds__(LB_THREADS) void las_lstm_bwd4_kernel(const float* __restrict__ dh, const float* __restrict__ whh_f,
                                                                   const float* __restrict__ whh_r, const long long* __restrict__ lengths,
                                                                   const float* __restrict__ gates, float* __restrict__ dG,
                                                                   float* __restrict__ bpart, int B, int T, int T2, int nrec) {
    __shared__ __attribute__((aligned(16))) float dgt[4 * LB_DGS];
    __shared__ float partd[4][4 * LB_PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, kr = wave >> 1;
    const int dir = (int)blockIdx.x >= nrec ? 1 : 0;
    const int b0 = ((int)blockIdx.x - dir * nrec) * 4;
    const float* whh = dir ? whh_r : whh_f;
    const int col = min(64 * ch + lane, LH - 1);
    float wk[LH];      // W_hh[96 kr + k][col], read in place (coalesced over the lanes)
#pragma unroll
    for (int kk = 0; kk < LH; ++kk) wk[kk] = whh[(size_t)(LH * kr + kk) * LH + col];
    const bool cell = tid < 4 * LH;
    const int s = cell ? tid / LH : 3, u = cell ? tid - (tid / LH) * LH : LH - 1;
    const int b = min(b0 + s, B - 1);
    const bool dup = b0 + s >= B;
    const int len = min(las_steps(lengths, b, T), T2);
    const size_t half = (size_t)B * T2 * LD;
    float dcs = 0.0f;
    float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = tid; i < 4 * 4 * LB_PS; i += LB_THREADS) (&partd[0][0])[i] = 0.0f;
    struct Step {
        float ig, fg, gg, og, c, cp, d0, d1;
    };
    // a step's saved activations are requested TWO steps ahead, right after the gate gradients of the step that used the slot
    // went out (a step is shorter than a trip to memory); unconditional loads from clamped addresses.  The step loop is unrolled
    // by two so that a slot is a fixed set of registers.
    Step q[2];
    auto request = [&](Step& raw, int si) {
        si = min(si, T2 - 1);
        const int t = dir ? si : T2 - 1 - si;
        const int tp = min(max(dir ? t + 1 : t - 1, 0), T2 - 1);
        const float* go = gates + (((size_t)b * T2 + t) * 2 + dir) * LSV + u;
        raw.ig = go[0];
        raw.fg = go[LH];
        raw.gg = go[2 * LH];
        raw.og = go[3 * LH];
        raw.c = go[4 * LH];
        raw.cp = gates[(((size_t)b * T2 + tp) * 2 + dir) * LSV + 4 * LH + u];
        const size_t o = ((size_t)b * T2 + t) * LD + dir * LH + u;
        raw.d0 = dh[o];
        raw.d1 = dh[half + o];
    };
    request(q[0], 0);
    request(q[1], 1);
    const int jh = (lane >> 2) < (LH - 64) / 4 ? (lane >> 2) : 0;
    __syncthreads();
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
    for (int si0 = 0; si0 < T2; si0 += 2)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int si = si0 + d;
        if (si >= T2) break;
        const int t = dir ? si : T2 - 1 - si;
        if (cell) {
            const Step cur = q[d];
            float dg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (t < len) {
                float dhv = cur.d0 + cur.d1;
#pragma unroll
                for (int r = 0; r < 4; ++r) dhv += partd[r][s * LB_PS + u];
                const bool first = dir ? t + 1 >= len : t == 0;      // the step that started from the zero state
                const float cp = first ? 0.0f : cur.cp;
                const float tc = tanhf_(cur.c);
                const float dc = fmaf(dhv * cur.og, 1.0f - tc * tc, dcs);
                dg[0] = dc * cur.gg * cur.ig * (1.0f - cur.ig);
                dg[1] = dc * cp * cur.fg * (1.0f - cur.fg);
                dg[2] = dc * cur.ig * (1.0f - cur.gg * cur.gg);
                dg[3] = dhv * tc * cur.og * (1.0f - cur.og);
                dcs = dc * cur.fg;
            } else {
                dcs = 0.0f;
            }
            float* dl = dgt + s * LB_DGS + u;
            float* go = dG + (((size_t)b * T2 + t) * 2 + dir) * L4 + u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                dl[k * LH] = dg[k];
                go[k * LH] = dg[k];
                bs[k] += dg[k];
            }
            request(q[d], si + 2);
        }
        __syncthreads();
        f32x4 acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* arow = dgt + (lane & 3) * LB_DGS + LH * kr;
        const float4 alo = *reinterpret_cast<const float4*>(arow + 4 * (lane >> 2)), ahi = *reinterpret_cast<const float4*>(arow + 64 + 4 * jh);
        bcast_mfma64<0, 0, LH, 16>(alo, wk, acc);
        bcast_mfma64<0, 64, LH, (LH - 64) / 4>(ahi, wk, acc);
        const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) partd[kr][r * LB_PS + 64 * ch + lane] = sum[r];
        __syncthreads();
    }
    if (dup) bs[0] = bs[1] = bs[2] = bs[3] = 0.0f;
    // bias gradients: the step sums are in registers, the four sequences meet in LDS (reusing partd: 4 x 4 x 96 floats)
    float* red = &partd[0][0];
    if (cell) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[(s * 4 + k) * LH + u] = bs[k];
    }
    __syncthreads();
    if (tid < L4) {
        const int k = tid / LH, uu = tid - k * LH;
        bpart[(size_t)blockIdx.x * L4 + tid] =
            ((red[(0 * 4 + k) * LH + uu] + red[(1 * 4 + k) * LH + uu]) + red[(2 * 4 + k) * LH + uu]) + red[(3 * 4 + k) * LH + uu];
    }
}

// The gradient at BN2's output of element (b, column w of conv2's output, j = channel * 44 + row): the pool's gradient goes to the
// first of the pair's two columns unless the second is larger, and through the ReLU where BN2's output is positive.  dF: the two
// halves of the features' gradient (through either direction's W_ih).  z: the element itself, returned for x^.
__device__ __forceinline__ float bn2_out_grad(const float* __restrict__ Z2, const float* __restrict__ dF, size_t half, int b, int w, int j,
                                              int W2, int T2, float sc, float sh, float& z) {
    const float* zr = Z2 + ((size_t)b * W2 + w) * LF + j;
    z = zr[0];
    const int t = w >> 1;
    if (t >= T2) return 0.0f;      // the column an odd W2 leaves over
    const bool odd = (w & 1) != 0;
    const float zo = odd ? zr[-LF] : zr[LF];
    const float y = fmaf(z, sc, sh), yo = fmaf(zo, sc, sh);
    const bool second = fmaxf(odd ? y : yo, 0.0f) > fmaxf(odd ? yo : y, 0.0f);
    if (second != odd || !(y > 0.0f)) return 0.0f;
    const size_t o = ((size_t)b * T2 + t) * LF + j;
    return dF[o] + dF[half + o];
}

// BN2's backward batch sums, channel blockIdx.y over a chunk of (utterance, column) pairs: part[chunk][c] = sum dy,
// [8 + c] = sum dy x^ (x^: the normalised conv2 output)
__global__ __launch_bounds__(256) void las_bn2_sums_kernel(const float* __restrict__ Z2, const float* __restrict__ dF, size_t half,
                                                           const float* __restrict__ g2, const float* __restrict__ be2,
                                                           const float* __restrict__ stat2, int B, int W2, int T2, int cols_per_chunk,
                                                           double* __restrict__ part) {
    __shared__ double red[4][2];
    const int c = blockIdx.y;
    const float mean = stat2[c], invstd = stat2[8 + c];
    float sc, sh;
    bn_affine(g2[c], be2[c], mean, invstd, sc, sh);
    const long ncols = (long)B * W2, c0 = (long)blockIdx.x * cols_per_chunk, c1 = min(ncols, c0 + cols_per_chunk);
    double acc[2] = {0.0, 0.0};
    for (long i = c0 * LR2 + threadIdx.x; i < c1 * LR2; i += 256) {
        const long cw = i / LR2;
        const int h = (int)(i - cw * LR2), b = (int)(cw / W2), w = (int)(cw - (long)b * W2);
        float z;
        const float d = bn2_out_grad(Z2, dF, half, b, w, c * LR2 + h, W2, T2, sc, sh, z);
        acc[0] += (double)d;
        acc[1] += (double)d * (double)((z - mean) * invstd);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double s0 = wave_sum_d(acc[0]), s1 = wave_sum_d(acc[1]);
    if (lane == 0) {
        red[wave][0] = s0;
        red[wave][1] = s1;
    }
    __syncthreads();
    if (threadIdx.x < 2) part[(size_t)blockIdx.x * 16 + 8 * threadIdx.x + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Encoder backward from the features' gradient down to the pooled conv1 activation, one tile of LT columns of one utterance: BN2
// (folding the launch before's sums; workgroup (0, 0) writes d gamma2, d beta2 and conv2's zero bias gradient) into a dense tile of
// d Z2 in LDS; conv2's weight gradient with thread = (output channel, input channel) pair x wave = row phase, nine accumulators
// and a sliding 3 x 3 window of the pooled tile (cpart2[(b, tile)][576]); conv2's data gradient with one pooled position per thread
// and eight accumulators; un-pool + ReLU (dA (B,8,42,T1): the gradient at the pool's argmax, zero where the pooled value is 0) and
// BN1's batch sums part4[(b, tile)] = sum dA, sum dA x^ per channel.  conv2's BIAS sits in front of a training-mode BatchNorm: its
// gradient is identically zero and written as that zero.
__global__ __launch_bounds__(ENC_THREADS) void las_conv2_bwd_kernel(const float* __restrict__ Z1, const float* __restrict__ Z2,
                                                                    const float* __restrict__ dF, size_t half, int B, int T,
                                                                    const float* __restrict__ c2w, const float* __restrict__ g1,
                                                                    const float* __restrict__ be1, const float* __restrict__ g2,
                                                                    const float* __restrict__ be2, const float* __restrict__ stat1,
                                                                    const float* __restrict__ stat2, const double* __restrict__ part3,
                                                                    int nparts3, double count2, float* __restrict__ dA,
                                                                    float* __restrict__ cpart2, double* __restrict__ part4,
                                                                    float* __restrict__ g_bn2_w, float* __restrict__ g_bn2_b,
                                                                    float* __restrict__ g_c2b) {
    __shared__ __attribute__((aligned(16))) float wt[72 * LC];      // [(co * 9 + k) * 8 + ci]
    __shared__ float sc1[LC], sh1[LC], sc2[LC], sh2[LC], md[LC], mdx[LC];
    __shared__ float dzt[LC * LR2 * LPW];
    __shared__ float pt[LC * (LR1 + 4) * LPW];      // the pooled tile, then the four waves' weight-gradient sums
    __shared__ double scratch[256], tot[16], red[4][16];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
    const int W1 = T + 2, T1 = W1 / 2, W2 = T1 + 2, T2 = W2 / 2, w0 = tile * LT;
    for (int i = tid; i < 72 * LC; i += ENC_THREADS) {
        const int co = i / 72, ci = (i / 9) % LC, k = i % 9;
        wt[(co * 9 + k) * LC + ci] = c2w[i];
    }
    fold_parts<16>(part3, nparts3, scratch, tot);
    if (tid < LC) {
        bn_affine(g1[tid], be1[tid], stat1[tid], stat1[8 + tid], sc1[tid], sh1[tid]);
        bn_affine(g2[tid], be2[tid], stat2[tid], stat2[8 + tid], sc2[tid], sh2[tid]);
        md[tid] = (float)(tot[tid] / count2);
        mdx[tid] = (float)(tot[8 + tid] / count2);
        if (tile == 0 && b == 0) {
            g_bn2_b[tid] = (float)tot[tid];
            g_bn2_w[tid] = (float)tot[8 + tid];
            g_c2b[tid] = 0.0f;
        }
    }
    __syncthreads();
    // d Z2 at columns w0 .. w0 + LT + 1 (dense: BN2's input gradient is non-zero everywhere, the left-over column included)
    for (int i = tid; i < LC * LR2 * LTW; i += ENC_THREADS) {
        const int cc = i / LF, j = i - cc * LF, co = j / LR2, h = j - co * LR2, w = w0 + cc;
        float v = 0.0f;
        if (w < W2) {
            float z;
            const float d = bn2_out_grad(Z2, dF, half, b, w, j, W2, T2, sc2[co], sh2[co], z);
            v = sc2[co] * (d - md[co] - (z - stat2[co]) * stat2[8 + co] * mdx[co]);
        }
        dzt[(co * LR2 + h) * LPW + cc] = v;
    }
    load_pool_tile(Z1, b, W1, T1, w0, sc1, sh1, pt);
    __syncthreads();
    {
        // conv2's weight gradient over the tile's own columns: dW[co,ci,dy,dx] = sum dZ2[co,h,w] P[ci,h+dy-2,w+dx-2]
        const int co = lane >> 3, ci = lane & 7, ncol = min(LT, W2 - w0);
        float a[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) a[k] = 0.0f;
#pragma unroll 1
        for (int h = wave; h < LR2; h += 4) {
            const float* pr = pt + (ci * (LR1 + 4) + h) * LPW;
            const float* dr = dzt + (co * LR2 + h) * LPW;
            float p[3][3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                p[dy][1] = pr[dy * LPW];
                p[dy][2] = pr[dy * LPW + 1];
            }
#pragma unroll 1
            for (int cc = 0; cc < ncol; ++cc) {
                const float d = dr[cc];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    p[dy][0] = p[dy][1];
                    p[dy][1] = p[dy][2];
                    p[dy][2] = pr[dy * LPW + cc + 2];
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) a[dy * 3 + dx] = fmaf(d, p[dy][dx], a[dy * 3 + dx]);
                }
            }
        }
        __syncthreads();      // every wave is done with the pooled tile
#pragma unroll
        for (int k = 0; k < 9; ++k) pt[wave * 576 + lane * 9 + k] = a[k];
    }
    __syncthreads();
    for (int i = tid; i < 576; i += ENC_THREADS)
        cpart2[((size_t)b * gridDim.x + tile) * 576 + i] = ((pt[i] + pt[576 + i]) + pt[2 * 576 + i]) + pt[3 * 576 + i];
    // conv2's data gradient, un-pool and ReLU at the tile's pooled columns w0 .. w0 + LT - 1
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int i = tid; i < LR1 * LT; i += ENC_THREADS) {
        const int cx = i / LR1, y = i - cx * LR1, xc = w0 + cx;
        if (xc >= T1) continue;
        float dp[LC];
#pragma unroll
        for (int ci = 0; ci < LC; ++ci) dp[ci] = 0.0f;
#pragma unroll 1
        for (int co = 0; co < LC; ++co) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = dzt[(co * LR2 + y + 2 - dy) * LPW + cx + 2 - dx];
                    const float4 wa = *reinterpret_cast<const float4*>(&wt[(co * 9 + dy * 3 + dx) * LC]);
                    const float4 wb = *reinterpret_cast<const float4*>(&wt[(co * 9 + dy * 3 + dx) * LC + 4]);
                    dp[0] = fmaf(wa.x, v, dp[0]);
                    dp[1] = fmaf(wa.y, v, dp[1]);
                    dp[2] = fmaf(wa.z, v, dp[2]);
                    dp[3] = fmaf(wa.w, v, dp[3]);
                    dp[4] = fmaf(wb.x, v, dp[4]);
                    dp[5] = fmaf(wb.y, v, dp[5]);
                    dp[6] = fmaf(wb.z, v, dp[6]);
                    dp[7] = fmaf(wb.w, v, dp[7]);
                }
        }
#pragma unroll
        for (int ci = 0; ci < LC; ++ci) {
            const float* z = Z1 + (((size_t)b * LC + ci) * LR1 + y) * W1 + 2 * xc;
            const float y0 = fmaf(z[0], sc1[ci], sh1[ci]), y1 = fmaf(z[1], sc1[ci], sh1[ci]);
            const bool second = y1 > y0;
            const float gq = fmaxf(y0, y1) > 0.0f ? dp[ci] : 0.0f;
            const float xn = ((second ? z[1] : z[0]) - stat1[ci]) * stat1[8 + ci];
            dA[(((size_t)b * LC + ci) * LR1 + y) * T1 + xc] = gq;
            acc[ci] += (double)gq;
            acc[8 + ci] += (double)gq * (double)xn;
        }
    }
    block_sum_d<16>(acc, red, part4 + ((size_t)b * gridDim.x + tile) * 16);
}

// BN1's backward (folding part4; workgroup (0, 0) writes d gamma1, d beta1) and conv1's weight gradient over one tile of LT
// columns of one utterance: a dense tile of d Z1 = gamma invstd (dA at the pair's argmax, else 0, - mean(dA) - x^ mean(dA x^)) and
// the x tile in LDS; thread = (output channel, input channel) pair x row phase, nine accumulators and a sliding 3 x 3 window of x;
// cpart1[(b, tile)][216].  conv1's BIAS sits in front of a training-mode BatchNorm: the batch mean absorbs it and its gradient, the
// sum of d Z1 over the batch, is identically zero.  It is written as that zero (by workgroup (0, 0)) and not as the rounding residue
// of a sum that cancels: an optimiser that normalises each gradient by its own magnitude would step by the sign of the residue.
constexpr int C1B_PHASES = 10;
__global__ __launch_bounds__(ENC_THREADS) void las_conv1_bwd_kernel(const float* __restrict__ x, long sb, long sc, long sm, long st, int T,
                                                                    const float* __restrict__ Z1, const float* __restrict__ g1,
                                                                    const float* __restrict__ be1, const float* __restrict__ stat1,
                                                                    const double* __restrict__ part4, int nparts4, double count1,
                                                                    const float* __restrict__ dA, float* __restrict__ cpart1,
                                                                    float* __restrict__ g_bn1_w, float* __restrict__ g_bn1_b,
                                                                    float* __restrict__ g_c1b) {
    __shared__ float sc1[LC], sh1[LC], mg[LC], mgx[LC];
    __shared__ float xt[LXC * LR2 * LPW];
    __shared__ float dzt[LC * LR1 * LPW];
    __shared__ float wred[C1B_PHASES * 216];
    __shared__ double scratch[256], tot[16];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int W1 = T + 2, T1 = W1 / 2, w0 = tile * LT;
    fold_parts<16>(part4, nparts4, scratch, tot);
    if (tid < LC) {
        bn_affine(g1[tid], be1[tid], stat1[tid], stat1[8 + tid], sc1[tid], sh1[tid]);
        mg[tid] = (float)(tot[tid] / count1);
        mgx[tid] = (float)(tot[8 + tid] / count1);
        if (tile == 0 && b == 0) {
            g_bn1_b[tid] = (float)tot[tid];
            g_bn1_w[tid] = (float)tot[8 + tid];
            g_c1b[tid] = 0.0f;
        }
    }
    load_x_tile(x + (long)b * sb, sc, sm, st, T, w0, xt);
    __syncthreads();
    for (int i = tid; i < LC * LR1 * LT; i += ENC_THREADS) {
        const int co = i / (LR1 * LT), j = i - co * (LR1 * LT), h = j / LT, cc = j - h * LT, w = w0 + cc;
        float v = 0.0f;
        if (w < W1) {
            const float* zr = Z1 + (((size_t)b * LC + co) * LR1 + h) * W1 + w;
            const float z = zr[0];
            const int p = w >> 1;
            float d = 0.0f;
            if (p < T1) {      // (else: the column an odd W1 leaves over)
                const bool odd = (w & 1) != 0;
                const float zo = odd ? zr[-1] : zr[1];
                const float y = fmaf(z, sc1[co], sh1[co]), yo = fmaf(zo, sc1[co], sh1[co]);
                const bool second = odd ? y > yo : yo > y;
                if (second == odd) d = dA[(((size_t)b * LC + co) * LR1 + h) * T1 + p];
            }
            v = sc1[co] * (d - mg[co] - (z - stat1[co]) * stat1[8 + co] * mgx[co]);
        }
        dzt[(co * LR1 + h) * LPW + cc] = v;
    }
    __syncthreads();
    const int pair = tid % 24, phase = tid / 24;      // pair = co * 3 + ch
    if (phase < C1B_PHASES) {
        const int co = pair / LXC, chn = pair - co * LXC, ncol = min(LT, W1 - w0);
        float a[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) a[k] = 0.0f;
#pragma unroll 1
        for (int h = phase; h < LR1; h += C1B_PHASES) {
            const float* xr = xt + (chn * LR2 + h) * LPW;
            const float* dr = dzt + (co * LR1 + h) * LPW;
            float p[3][3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                p[dy][1] = xr[dy * LPW];
                p[dy][2] = xr[dy * LPW + 1];
            }
#pragma unroll 1
            for (int cc = 0; cc < ncol; ++cc) {
                const float d = dr[cc];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    p[dy][0] = p[dy][1];
                    p[dy][1] = p[dy][2];
                    p[dy][2] = xr[dy * LPW + cc + 2];
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) a[dy * 3 + dx] = fmaf(d, p[dy][dx], a[dy * 3 + dx]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) wred[phase * 216 + pair * 9 + k] = a[k];
    }
    __syncthreads();
    if (tid < 216) {
        float v = 0.0f;
        for (int ph = 0; ph < C1B_PHASES; ++ph) v += wred[ph * 216 + tid];
        cpart1[((size_t)b * gridDim.x + tile) * 216 + tid] = v;
    }
}

// How one problem (B utterances of T frames, num_labels) runs: geometry, the workspace carve-up and the launch shapes, decided
// once per call; `bad` says why a problem is refused.
struct LasPlan {
    char bad[96];
    int W1, T1, W2, T2;        // conv1's columns, pooled, conv2's columns, pooled = recurrence steps
    int ntile1, ntile2, nfeat, nrec;      // encoder tiles per utterance, feature workgroups per utterance, recurrence workgroups per direction
    int nsum3, cols3;          // workgroups of BN2's backward sums per channel and their columns
    long rows;                 // B * T2
    double count1, count2;     // elements per channel of BN1 and BN2
    RowMap hmap;               // rows (b, t) of the hidden sequence inside hs (B,T2+2,192)
    // saved by the forward
    double *part1, *part2;
    float *stat1, *stat2, *Z1, *Z2, *F, *Gx, *gates, *hs, *V, *K, *lgt, *ms, *ctx, *y1d;
    // backward
    double *part3, *part4;
    float *dz1, *dctx, *dV, *dK, *cvpart, *dh, *dG, *bpart, *dF, *dA, *cpart1, *cpart2;
    float *slabs_ih[2], *slabs_hh[2], *slabs_v, *slabs_k, *slabs_w1, *slabs_w2, *scratch_b1, *scratch_b2, *scratch_bk;
    size_t bytes;
};
LasPlan las_plan(int B, int M, int T, int num_labels, void* ws = nullptr) {
    LasPlan q{};
    if (B < 1) snprintf(q.bad, sizeof(q.bad), "B=%d: at least one utterance", B);
    else if (M != LM) snprintf(q.bad, sizeof(q.bad), "M=%d mel bins: the kernels are specialised for 40", M);
    else if (T < 1 || T > HOWL_LAS_MAX_FRAMES) snprintf(q.bad, sizeof(q.bad), "T=%d frames outside 1..%d", T, HOWL_LAS_MAX_FRAMES);
    else if (num_labels < 1 || num_labels > HOWL_LAS_MAX_LABELS)
        snprintf(q.bad, sizeof(q.bad), "num_labels=%d outside 1..%d", num_labels, HOWL_LAS_MAX_LABELS);
    if (q.bad[0] != 0) return q;
    q.W1 = T + 2;
    q.T1 = q.W1 / 2;
    q.W2 = q.T1 + 2;
    q.T2 = q.W2 / 2;
    q.ntile1 = (q.W1 + LT - 1) / LT;
    q.ntile2 = (q.W2 + LT - 1) / LT;
    q.nfeat = (q.T2 + FEAT_STEPS - 1) / FEAT_STEPS;
    q.nrec = (B + 3) / 4;
    q.rows = (long)B * q.T2;
    const long ncols = (long)B * q.W2;
    q.nsum3 = (int)std::min<long>(64, (ncols + 23) / 24);
    q.cols3 = (int)((ncols + q.nsum3 - 1) / q.nsum3);
    q.count1 = (double)B * LR1 * q.W1;
    q.count2 = (double)B * LR2 * q.W2;
    q.hmap = RowMap{q.T2, (long)(q.T2 + 2) * LD, LD};
    size_t off = 0;      // in floats; every region starts on a 16-byte boundary
    auto region = [&](size_t floats) {
        const size_t at = off;
        off += (floats + 3) / 4 * 4;
        return ws != nullptr ? static_cast<float*>(ws) + at : nullptr;
    };
    auto dregion = [&](size_t doubles) { return reinterpret_cast<double*>(region(2 * doubles)); };
    const size_t rows = (size_t)q.rows, nb1 = (size_t)B * q.ntile1, nb2 = (size_t)B * q.ntile2;
    q.part1 = dregion(nb1 * 16);
    q.part2 = dregion(nb2 * 16);
    q.part3 = dregion((size_t)q.nsum3 * 16);
    q.part4 = dregion(nb2 * 16);
    q.stat1 = region(16);
    q.stat2 = region(16);
    q.Z1 = region((size_t)B * LC * LR1 * q.W1);
    q.Z2 = region((size_t)B * q.W2 * LF);
    q.F = region(rows * LF);
    q.Gx = region(rows * 2 * L4);
    q.gates = region(rows * 2 * LSV);
    q.hs = region((size_t)B * (q.T2 + 2) * LD);
    q.V = region(rows * LD);
    q.K = region(rows * LD);
    q.lgt = region(rows * LHEADS);
    q.ms = region((size_t)B * LHEADS * 2);
    q.ctx = region((size_t)B * LD);
    q.y1d = region((size_t)B * LHD);
    q.dz1 = region((size_t)B * LHD);
    q.dctx = region((size_t)B * LD);
    q.dV = region(rows * LD);
    q.dK = region(rows * LD);
    q.cvpart = region((size_t)B * LD);
    q.dh = region(2 * rows * LD);
    q.dG = region(rows * 2 * L4);
    q.bpart = region((size_t)2 * q.nrec * L4);
    q.dF = region(2 * rows * LF);
    q.dA = region((size_t)B * LC * LR1 * q.T1);
    q.cpart1 = region(nb1 * 216);
    q.cpart2 = region(nb2 * 576);
    for (int d = 0; d < 2; ++d) {
        q.slabs_ih[d] = region((size_t)LAS_WGRAD_SPLITS * L4 * LF);
        q.slabs_hh[d] = region((size_t)LAS_WGRAD_SPLITS * L4 * LH);
    }
    q.slabs_v = region((size_t)LAS_WGRAD_SPLITS * LD * LD);
    q.slabs_k = region((size_t)LAS_WGRAD_SPLITS * LD * LD);
    q.slabs_w1 = region((size_t)LAS_HEAD_SPLITS * LHD * LD);
    q.slabs_w2 = region((size_t)LAS_HEAD_SPLITS * HOWL_LAS_MAX_LABELS * LHD);
    q.scratch_b1 = region((size_t)64 * LHD);
    q.scratch_b2 = region((size_t)64 * HOWL_LAS_MAX_LABELS);
    q.scratch_bk = region((size_t)64 * LD);
    q.bytes = off * sizeof(float) + 64;
    return q;
}

bool all_set(const void* const* p, int n) {
    for (int i = 0; i < n; ++i)
        if (p[i] == nullptr) return false;
    return true;
}

}  // namespace

extern "C" {

int howl_las_supported(int B, int M, int T, int num_labels) { return las_plan(B, M, T, num_labels).bad[0] == 0 ? 1 : 0; }

size_t howl_las_workspace_bytes(int B, int T) { return las_plan(B, LM, T, 1).bytes; }

int howl_las_fwd(const HowlLasParams* p, const HowlLasBuffers* bf, const float* x, long sb, long sc, long sm, long st, int B, int M, int T,
                 int num_labels, const long long* lengths, int training, const float* drop_mask, float keep_scale, float* logits,
                 void* ws, size_t ws_bytes, hipStream_t stream) {
    HOWL_REQUIRE(p && bf && x && logits && ws && all_set(reinterpret_cast<const void* const*>(p), 25) &&
                     all_set(reinterpret_cast<const void* const*>(bf), 6), "howl_las_fwd: null pointer");
    HOWL_REQUIRE(training || drop_mask == nullptr, "howl_las_fwd: a dropout mask in eval mode");
    const LasPlan q = las_plan(B, M, T, num_labels, ws);
    HOWL_REQUIRE(q.bad[0] == 0, "howl_las_fwd: %s", q.bad);
    if (ws_bytes < q.bytes) {
        howl_set_error("howl_las_fwd: workspace too small (%zu < %zu bytes)", ws_bytes, q.bytes);
        return HOWL_E_WORKSPACE;
    }
    const LasBn bn1{p->bn1_w, p->bn1_b, bf->bn1_mean, bf->bn1_var, bf->bn1_batches};
    const LasBn bn2{p->bn2_w, p->bn2_b, bf->bn2_mean, bf->bn2_var, bf->bn2_batches};
    const int np1 = B * q.ntile1, np2 = B * q.ntile2, rows = (int)q.rows;
    {
        HowlProfScope prof("las_enc_fwd", stream, 2.0 * 9 * LC * ((double)LXC * LR1 * q.W1 + (double)LC * LR2 * q.W2) * B);
        if (training) {
            hipLaunchKernelGGL(las_conv1_kernel<true>, dim3(q.ntile1, B), dim3(ENC_THREADS), 0, stream, x, sb, sc, sm, st, T, p->conv1_w,
                               p->conv1_b, q.Z1, q.part1);
            hipLaunchKernelGGL(las_conv2_kernel<true>, dim3(q.ntile2, B), dim3(ENC_THREADS), 0, stream, (const float*)q.Z1, T, p->conv2_w,
                               p->conv2_b, bn1, (const double*)q.part1, np1, q.count1, q.stat1, q.Z2, q.part2);
            hipLaunchKernelGGL(las_feat_kernel<true>, dim3(q.nfeat, B), dim3(ENC_THREADS), 0, stream, (const float*)q.Z2, q.W2, q.T2, bn2,
                               (const double*)q.part2, np2, q.count2, q.stat2, q.F);
        } else {
            hipLaunchKernelGGL(las_conv1_kernel<false>, dim3(q.ntile1, B), dim3(ENC_THREADS), 0, stream, x, sb, sc, sm, st, T, p->conv1_w,
                               p->conv1_b, q.Z1, (double*)nullptr);
            hipLaunchKernelGGL(las_conv2_kernel<false>, dim3(q.ntile2, B), dim3(ENC_THREADS), 0, stream, (const float*)q.Z1, T, p->conv2_w,
                               p->conv2_b, bn1, (const double*)nullptr, 0, q.count1, (float*)nullptr, q.Z2, (double*)nullptr);
            hipLaunchKernelGGL(las_feat_kernel<false>, dim3(q.nfeat, B), dim3(ENC_THREADS), 0, stream, (const float*)q.Z2, q.W2, q.T2, bn2,
                               (const double*)nullptr, 0, q.count2, (float*)nullptr, q.F);
        }
    }
    // the input projections of every step at once, per direction (K is never split: a row's bits do not depend on the row count)
    gemm(stream, true, q.F, lin(LF), 1, lin(0), p->w_ih_f, lin(1), LF, rows, L4, LF, 1, nullptr, 0, q.Gx, 2 * L4, 0);
    gemm(stream, true, q.F, lin(LF), 1, lin(0), p->w_ih_r, lin(1), LF, rows, L4, LF, 1, nullptr, 0, q.Gx + L4, 2 * L4, 0);
    {
        HowlProfScope prof("las_lstm_fwd", stream, 2.0 * 2 * L4 * LH * (double)q.rows);
        if (training)
            hipLaunchKernelGGL(las_lstm_fwd4_kernel<true>, dim3(2 * q.nrec), dim3(LF_THREADS), 0, stream, (const float*)q.Gx, p->w_hh_f, p->b_ih_f,
                               p->b_hh_f, p->w_hh_r, p->b_ih_r, p->b_hh_r, lengths, q.gates, q.hs, B, T, q.T2, q.nrec);
        else
            hipLaunchKernelGGL(las_lstm_fwd4_kernel<false>, dim3(2 * q.nrec), dim3(LF_THREADS), 0, stream, (const float*)q.Gx, p->w_hh_f, p->b_ih_f,
                               p->b_hh_f, p->w_hh_r, p->b_ih_r, p->b_hh_r, lengths, (float*)nullptr, q.hs, B, T, q.T2, q.nrec);
    }
    gemm(stream, true, q.hs + LD, q.hmap, 1, lin(0), p->v_w, lin(1), LD, rows, LD, LD, 1, p->v_b, 0, q.V, LD, 0);
    gemm(stream, true, q.hs + LD, q.hmap, 1, lin(0), p->k_w, lin(1), LD, rows, LD, LD, 1, p->k_b, 0, q.K, LD, 0);
    {
        HowlProfScope prof("las_attn", stream, 4.0 * LD * (double)q.rows);
        hipLaunchKernelGGL(las_attn_fwd_kernel, dim3(B), dim3(256), 0, stream, (const float*)q.V, (const float*)q.K, p->cv, lengths, T, q.T2,
                           q.ctx, training ? q.lgt : (float*)nullptr, training ? q.ms : (float*)nullptr);
    }
    {
        HowlProfScope prof("las_head", stream, 2.0 * LHD * (LD + num_labels) * (double)B);
        hipLaunchKernelGGL(las_head_fwd_kernel, dim3(B), dim3(256), 0, stream, (const float*)q.ctx, p->w1, p->b1, p->w2, p->b2, drop_mask,
                           keep_scale, num_labels, training ? q.y1d : (float*)nullptr, logits);
    }
    HOWL_CHECK_LAUNCH("howl_las_fwd");
    return HOWL_OK;
}

int howl_las_bwd(const HowlLasParams* p, const float* x, long sb, long sc, long sm, long st, int B, int M, int T, int num_labels,
                 const long long* lengths, float keep_scale, const float* dlogits, const HowlLasGrads* g, void* ws, size_t ws_bytes,
                 hipStream_t stream) {
    HOWL_REQUIRE(p && x && dlogits && g && ws && all_set(reinterpret_cast<const void* const*>(p), 25) &&
                     all_set(reinterpret_cast<const void* const*>(g), 25), "howl_las_bwd: null pointer");
    const LasPlan q = las_plan(B, M, T, num_labels, ws);
    HOWL_REQUIRE(q.bad[0] == 0, "howl_las_bwd: %s", q.bad);
    if (ws_bytes < q.bytes) {
        howl_set_error("howl_las_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, q.bytes);
        return HOWL_E_WORKSPACE;
    }
    const int rows = (int)q.rows, np2 = B * q.ntile2;
    const size_t hhalf = (size_t)q.rows * LD, fhalf = (size_t)q.rows * LF;
    SlabSums sums;
    {
        HowlProfScope prof("las_head", stream, 4.0 * LHD * (LD + num_labels) * (double)B);
        hipLaunchKernelGGL(las_head_bwd_kernel, dim3(B), dim3(256), 0, stream, dlogits, (const float*)q.y1d, p->w1, p->w2, keep_scale, num_labels,
                           q.dz1, q.dctx);
    }
    wgrad_gemm(stream, dlogits, lin(num_labels), num_labels, q.y1d, lin(LHD), LHD, B, q.slabs_w2, g->w2, LAS_HEAD_SPLITS, 512, &sums);
    colsum(stream, dlogits, lin(num_labels), B, num_labels, q.scratch_b2, g->b2, nullptr, 64, 256, &sums);
    wgrad_gemm(stream, q.dz1, lin(LHD), LHD, q.ctx, lin(LD), LD, B, q.slabs_w1, g->w1, LAS_HEAD_SPLITS, 512, &sums);
    colsum(stream, q.dz1, lin(LHD), B, LHD, q.scratch_b1, g->b1, nullptr, 64, 256, &sums);
    {
        HowlProfScope prof("las_attn", stream, 8.0 * LD * (double)q.rows);
        hipLaunchKernelGGL(las_attn_bwd_kernel, dim3(B), dim3(256), 0, stream, (const float*)q.V, (const float*)q.K, p->cv, lengths, T, q.T2,
                           (const float*)q.ctx, (const float*)q.lgt, (const float*)q.ms, (const float*)q.dctx, q.dV, q.dK, q.cvpart, g->v_b);
    }
    // dW_v = dV^T H, dW_k = dK^T H, db_k, d context_vec; d rnn_seq = dV W_v (first half of dh) + dK W_k (second half)
    wgrad_gemm(stream, q.dV, lin(LD), LD, q.hs + LD, q.hmap, LD, rows, q.slabs_v, g->v_w, LAS_WGRAD_SPLITS, 256, &sums);
    wgrad_gemm(stream, q.dK, lin(LD), LD, q.hs + LD, q.hmap, LD, rows, q.slabs_k, g->k_w, LAS_WGRAD_SPLITS, 256, &sums);
    colsum(stream, q.dK, lin(LD), rows, LD, q.scratch_bk, g->k_b, nullptr, 64, 256, &sums);
    sums.add(q.cvpart, B, LD, g->cv);
    if (!sums.flush(stream)) return HOWL_E_ARG;
    gemm(stream, true, q.dV, lin(LD), 1, lin(0), p->v_w, lin(LD), 1, rows, LD, LD, 1, nullptr, 0, q.dh, LD, 0);
    gemm(stream, true, q.dK, lin(LD), 1, lin(0), p->k_w, lin(LD), 1, rows, LD, LD, 1, nullptr, 0, q.dh + hhalf, LD, 0);
    {
        HowlProfScope prof("las_lstm_bwd", stream, 2.0 * 2 * L4 * LH * (double)q.rows);
        hipLaunchKernelGGL(las_lstm_bwd4_kernel, dim3(2 * q.nrec), dim3(LB_THREADS), 0, stream, (const float*)q.dh, p->w_hh_f, p->w_hh_r, lengths,
                           (const float*)q.gates, q.dG, q.bpart, B, T, q.T2, q.nrec);
    }
    // per direction: dW_ih = dG^T F, dW_hh = dG^T H_prev (the hidden sequence one row earlier / later), both biases from the
    // recurrence's per-workgroup sums; dF = dG W_ih, one half per direction
    const float* w_ih[2] = {p->w_ih_f, p->w_ih_r};
    float* g_ih[2] = {g->w_ih_f, g->w_ih_r};
    float* g_hh[2] = {g->w_hh_f, g->w_hh_r};
    float* g_bi[2] = {g->b_ih_f, g->b_ih_r};
    float* g_bh[2] = {g->b_hh_f, g->b_hh_r};
    for (int d = 0; d < 2; ++d) {
        const float* dGd = q.dG + d * L4;
        wgrad_gemm(stream, dGd, lin(2 * L4), L4, q.F, lin(LF), LF, rows, q.slabs_ih[d], g_ih[d], LAS_WGRAD_SPLITS, 256, &sums);
        wgrad_gemm(stream, dGd, lin(2 * L4), L4, q.hs + (d ? 2 * LD + LH : 0), q.hmap, LH, rows, q.slabs_hh[d], g_hh[d], LAS_WGRAD_SPLITS, 256,
                   &sums);
        sums.add(q.bpart + (size_t)d * q.nrec * L4, q.nrec, L4, g_bi[d], g_bh[d]);
        gemm(stream, true, dGd, lin(2 * L4), 1, lin(0), w_ih[d], lin(LF), 1, rows, LF, L4, 1, nullptr, 0, q.dF + d * fhalf, LF, 0);
    }
    if (!sums.flush(stream)) return HOWL_E_ARG;
    {
        HowlProfScope prof("las_enc_bwd", stream, 2.0 * 9 * LC * ((double)LXC * LR1 * q.W1 + 2.0 * LC * LR2 * q.W2) * B);
        hipLaunchKernelGGL(las_bn2_sums_kernel, dim3(q.nsum3, LC), dim3(256), 0, stream, (const float*)q.Z2, (const float*)q.dF, fhalf, p->bn2_w,
                           p->bn2_b, (const float*)q.stat2, B, q.W2, q.T2, q.cols3, q.part3);
        hipLaunchKernelGGL(las_conv2_bwd_kernel, dim3(q.ntile2, B), dim3(ENC_THREADS), 0, stream, (const float*)q.Z1, (const float*)q.Z2,
                           (const float*)q.dF, fhalf, B, T, p->conv2_w, p->bn1_w, p->bn1_b, p->bn2_w, p->bn2_b, (const float*)q.stat1,
                           (const float*)q.stat2, (const double*)q.part3, q.nsum3, q.count2, q.dA, q.cpart2, q.part4, g->bn2_w, g->bn2_b,
                           g->conv2_b);
        hipLaunchKernelGGL(las_conv1_bwd_kernel, dim3(q.ntile1, B), dim3(ENC_THREADS), 0, stream, x, sb, sc, sm, st, T, (const float*)q.Z1,
                           p->bn1_w, p->bn1_b, (const float*)q.stat1, (const double*)q.part4, np2, q.count1, (const float*)q.dA, q.cpart1,
                           g->bn1_w, g->bn1_b, g->conv1_b);
    }
    sums.add(q.cpart2, np2, 576, g->conv2_w);
    sums.add(q.cpart1, B * q.ntile1, 216, g->conv1_w);
    if (!sums.flush(stream)) return HOWL_E_ARG;
    HOWL_CHECK_LAUNCH("howl_las_bwd");
    return HOWL_OK;
}

}  // extern "C"
