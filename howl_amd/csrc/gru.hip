// The "gru" classifier for gfx950 (MI355X), howl/model/rnn.py:94-130 (SimpleGru): conv encoder with training-mode BatchNorm,
// GRU(40 -> 96) on the final hidden state of a packed batch, Linear - ReLU - Dropout - Linear.  One call per direction
// (include/howl_hip_gru.h), one launch plan per call (gru_plan).
//
// Forward launches (training):                                  backward launches:
//   gru_conv1_stats_kernel   BN1 batch sums of conv1(x)           gru_head_bwd_kernel     dz1, d h_T         (+ 4 GEMM-path jobs)
//   gru_enc_fwd_kernel       conv1-BN1-ReLU-pool-conv2-ReLU,      gru_bwd4_kernel         BPTT, dGx / dGh, bias partial sums
//                            BN2 batch sums                       wgrad_gemm x 2, gemm    dW_ih, dW_hh, dX^ = dGx W_ih
//   gru_fwd4_kernel          BN2 applied where x_t is read,       gru_bn2_bwd_sums_kernel batch sums of dX^ and dX^ x^
//                            the recurrence                       gru_enc_bwd2_kernel     BN2, ReLU, conv2 (dw, db, data), un-pool,
//   gru_head_fwd_kernel      the head on (B, 96)                                          ReLU, BN1 batch sums
//   (eval: no statistics launch)                                  gru_enc_bwd1_kernel     BN1, conv1 dw (db = 0)
//                                                                 sum_slabs_multi_kernel x 2: every partial sum, fixed order
// The batch-wide BatchNorm reductions are exchanged at launch boundaries only: a launch leaves one partial sum per workgroup, the
// next one folds them (every workgroup folds the same numbers in the same order).  No workgroup waits on another.
//
// Kept for the backward, per utterance of T1 = (T + 4) / 2 recurrence steps: the pooled encoder activation P (8 x 40 x T1) 1280 T1 B,
// relu(conv2) Y (T1,40) 160 T1 B, x^ (T1,40) 160 T1 B, the gates r, z, n and W_hn h + b_hn (T1,384) 1536 T1 B, the hidden
// sequence (T1+1,96) 384 (T1+1) B, h_T and the head's masked hidden row.  Recomputed from x: conv1's output (needed dense for
// BN1's backward and at the pool's argmax) and the argmax itself (the same fmaf chain as the forward: the same bits).
#include <math.h>

#include "howl_common.hip.h"
#include "../../include/howl_hip_gru.h"
#include "howl_gemm.hip.h"
#include "howl_lstm.hip.h"

namespace {

constexpr int GH = 96;             // hidden units
constexpr int G3 = 3 * GH;         // gate rows of the parameters, PyTorch order r, z, n
constexpr int GSV = 4 * GH;        // saved per step: r, z, n, W_hn h + b_hn
constexpr int GM = 40;             // mel bins = GRU input features
constexpr int GC = 8;              // latent channels
constexpr int GHD = 2 * GH;        // head's hidden width
constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;
constexpr int ENC_THREADS = 256;
constexpr int ENC_TP = 32;         // pooled columns per workgroup of the encoder kernels ...
constexpr int ENC_PW = ENC_TP + 2; // ... and with conv2's halo
constexpr int ENC_ROWS = GM + 2;   // mel rows with conv2's zero padding
constexpr int ST_TP = 128;         // column PAIRS (2p, 2p+1) of conv1's output per workgroup of the statistic / conv1-gradient kernels
constexpr int GRU_WGRAD_SPLITS = 32, GRU_HEAD_SPLITS = 8;

// conv1 at (mel m, column w) of the (40, T + 4) output for all eight channels: one fmaf chain per channel in a fixed order, so
// that the backward's recomputation gives the forward's bits.  cw: 72 weights + 8 biases; xv: the 3 x 3 input window.
__device__ __forceinline__ void conv1_at(const float* __restrict__ xb, long sm, long st, int T, int m, int w,
                                         const float* cw, float (&xv)[9], float (&z)[GC]) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int mm = m + dy - 1, tt = w + dx - 3;
            xv[dy * 3 + dx] = (mm >= 0 && mm < GM && tt >= 0 && tt < T) ? xb[(long)mm * sm + (long)tt * st] : 0.0f;
        }
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        float a = cw[72 + c];
#pragma unroll
        for (int k = 0; k < 9; ++k) a = fmaf(cw[c * 9 + k], xv[k], a);
        z[c] = a;
    }
}

// Item i of a (40 mel rows x n columns) tile -> (m, column): the mel index runs fastest over the lanes when the features are
// time-major (sm == 1: the (B, T, 40) buffer the fused frontend leaves), the column when they are mel-major ((B, C, 40, T)):
// either way a wave's loads of x fall into a few cache lines.  The pooled activation P and its gradient dA take the matching
// layout (pool_at): (B, 8, T1, 40) or (B, 8, 40, T1).
__device__ __forceinline__ void tile_item(int i, int n, bool m_fast, int& m, int& col) {
    if (m_fast) {
        col = i / GM;
        m = i - col * GM;
    } else {
        m = i / n;
        col = i - m * n;
    }
}
__device__ __forceinline__ size_t pool_at(int b, int c, int m, int p, int T1, bool m_fast) {
    return m_fast ? (((size_t)b * GC + c) * T1 + p) * GM + m : (((size_t)b * GC + c) * GM + m) * T1 + p;
}

// sums of NS statistics over `nparts` partial rows (doubles), by the first 256 threads of the workgroup in a fixed order; every
// thread of the workgroup must call (two barriers).  scratch: 256 doubles; tot: NS doubles
template <int NS>
__device__ __forceinline__ void fold_parts(const double* __restrict__ part, int nparts, double* scratch, double* tot) {
    constexpr int NCH = 256 / NS;
    const int tid = threadIdx.x;
    if (tid < 256) {
        const int s = tid % NS, ch = tid / NS;
        // eight independent loads in flight per round trip (every workgroup of the launch folds the same rows out of L2: the
        // fold is latency, not bandwidth); the order of the additions is fixed all the same
        double a = 0.0;
        int i = ch;
        for (; i + 7 * NCH < nparts; i += 8 * NCH) {
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

// BN1's batch sums: part[(b, tile)][c] = sum z_c, [8 + c] = sum z_c^2 over the tile's columns of conv1(x)
__global__ __launch_bounds__(ENC_THREADS) void gru_conv1_stats_kernel(const float* __restrict__ x, long sb, long sm, long st, int T,
                                                                      const float* __restrict__ c1w, const float* __restrict__ c1b,
                                                                      double* __restrict__ part) {
    __shared__ float cw[80];
    __shared__ double red[4][16];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int W1 = T + 4, np = (W1 + 1) / 2;
    if (tid < 72) cw[tid] = c1w[tid];
    else if (tid < 80) cw[tid] = c1b[tid - 72];
    __syncthreads();
    const int p0 = tile * ST_TP, n = min(ST_TP, np - p0);
    const float* xb = x + (long)b * sb;
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    const bool m_fast = sm == 1;
    for (int i = tid; i < GM * n; i += ENC_THREADS) {
        int m, p;
        tile_item(i, n, m_fast, m, p);
        p += p0;
        for (int h = 0; h < 2; ++h) {
            const int w = 2 * p + h;
            if (w >= W1) break;
            float xv[9], z[GC];
            conv1_at(xb, sm, st, T, m, w, cw, xv, z);
#pragma unroll
            for (int c = 0; c < GC; ++c) {
                acc[c] += (double)z[c];
                acc[8 + c] += (double)z[c] * (double)z[c];
            }
        }
    }
    block_sum_d<16>(acc, red, part + ((size_t)b * gridDim.x + tile) * 16);
}

struct GruBn {      // one BatchNorm of the encoder
    const float *gamma, *beta;
    float *rmean, *rvar;
    long long* batches;
};

// conv1 - BN1 - ReLU - MaxPool(1,2) - conv2 - ReLU on one tile of ENC_TP pooled columns of one utterance.  TRAIN: BN1 from the
// statistic launch's partial sums (workgroup (0, 0) also writes stat1 = mean[8], invstd[8] and updates the running buffers), the
// pooled activation P (pool_at) is kept and part2[(b, tile)] = sum y, sum y^2 goes to the next launch.  Y: (B,T1,40).
template <bool TRAIN>
__global__ __launch_bounds__(ENC_THREADS) void gru_enc_fwd_kernel(const float* __restrict__ x, long sb, long sm, long st, int T, int T1,
                                                                  const float* __restrict__ c1w, const float* __restrict__ c1b, GruBn bn1,
                                                                  const float* __restrict__ c2w, const float* __restrict__ c2b,
                                                                  const double* __restrict__ part1, int nparts1, double count1,
                                                                  float* __restrict__ stat1, float* __restrict__ P, float* __restrict__ Y,
                                                                  double* __restrict__ part2) {
    __shared__ float cw[80], w2s[73], sc[GC], sh[GC];
    __shared__ float pt[GC * ENC_ROWS * ENC_PW];
    __shared__ double scratch[256], tot[16], red[4][2];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    if (tid < 72) cw[tid] = c1w[tid];
    else if (tid < 80) cw[tid] = c1b[tid - 72];
    if (tid >= 128 && tid < 128 + 72) w2s[tid - 128] = c2w[tid - 128];
    if (tid == 255) w2s[72] = c2b[0];
    if constexpr (TRAIN) {
        fold_parts<16>(part1, nparts1, scratch, tot);
        if (tid < GC) {
            const double mean = tot[tid] / count1;
            const double var = fmax(tot[8 + tid] / count1 - mean * mean, 0.0);
            const float meanf = (float)mean, invstd = (float)(1.0 / sqrt(var + (double)BN_EPS));
            bn_affine(bn1.gamma[tid], bn1.beta[tid], meanf, invstd, sc[tid], sh[tid]);
            if (tile == 0 && b == 0) {
                stat1[tid] = meanf;
                stat1[8 + tid] = invstd;
                bn1.rmean[tid] = (1.0f - BN_MOMENTUM) * bn1.rmean[tid] + BN_MOMENTUM * meanf;
                bn1.rvar[tid] = (1.0f - BN_MOMENTUM) * bn1.rvar[tid] + BN_MOMENTUM * (float)(var * count1 / (count1 - 1.0));
                if (tid == 0) bn1.batches[0] += 1;
            }
        }
    } else {
        if (tid < GC) bn_affine(bn1.gamma[tid], bn1.beta[tid], bn1.rmean[tid], 1.0f / sqrtf(bn1.rvar[tid] + BN_EPS), sc[tid], sh[tid]);
    }
    // conv2's zero rows above and below the mel axis
    for (int i = tid; i < GC * 2 * ENC_PW; i += ENC_THREADS) {
        const int c = i / (2 * ENC_PW), r = (i / ENC_PW) & 1, pc = i % ENC_PW;
        pt[(c * ENC_ROWS + r * (ENC_ROWS - 1)) * ENC_PW + pc] = 0.0f;
    }
    __syncthreads();
    const int p0 = tile * ENC_TP;
    const float* xb = x + (long)b * sb;
    const bool m_fast = sm == 1;
    for (int i = tid; i < GM * ENC_PW; i += ENC_THREADS) {
        int m, pc;
        tile_item(i, ENC_PW, m_fast, m, pc);
        const int p = p0 - 1 + pc;
        float v[GC];
        if (p >= 0 && p < T1) {
            float xv[9], z0[GC], z1[GC];
            conv1_at(xb, sm, st, T, m, 2 * p, cw, xv, z0);
            conv1_at(xb, sm, st, T, m, 2 * p + 1, cw, xv, z1);
#pragma unroll
            for (int c = 0; c < GC; ++c) v[c] = fmaxf(fmaxf(fmaf(z0[c], sc[c], sh[c]), fmaf(z1[c], sc[c], sh[c])), 0.0f);
        } else {
#pragma unroll
            for (int c = 0; c < GC; ++c) v[c] = 0.0f;
        }
#pragma unroll
        for (int c = 0; c < GC; ++c) {
            pt[(c * ENC_ROWS + m + 1) * ENC_PW + pc] = v[c];
            if constexpr (TRAIN)
                if (pc >= 1 && pc <= ENC_TP && p < T1) P[pool_at(b, c, m, p, T1, m_fast)] = v[c];
        }
    }
    __syncthreads();
    double acc[2] = {0.0, 0.0};
    for (int i = tid; i < GM * ENC_TP; i += ENC_THREADS) {
        const int m = i % GM, pc = i / GM, p = p0 + pc;
        if (p >= T1) continue;
        float a = w2s[72];
#pragma unroll
        for (int c = 0; c < GC; ++c)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) a = fmaf(w2s[c * 9 + dy * 3 + dx], pt[(c * ENC_ROWS + m + dy) * ENC_PW + pc + dx], a);
        const float y = fmaxf(a, 0.0f);
        Y[((size_t)b * T1 + p) * GM + m] = y;
        acc[0] += (double)y;
        acc[1] += (double)y * (double)y;
    }
    if constexpr (TRAIN) block_sum_d<2>(acc, red, part2 + ((size_t)b * gridDim.x + tile) * 2);
}

// Forward recurrence, FOUR sequences per workgroup on v_mfma_f32_4x4x1 (lstm_fwd4_kernel's scheme: block = hidden unit, block row
// = sequence, the A operand by block broadcast, one barrier per step with h double-buffered in LDS).  Six waves, wave c = units
// 16c .. 16c+15; the four block columns of unit u over K = 96 + 40 are
//   0: W_hr h + W_ir x     1: W_hz h + W_iz x     2: W_hn h (its x weights are zero)     3: W_in x (its h weights are zero)
// -- the two halves of n stay apart because r multiplies only the first.  Lane 4j+g holds column g of unit 16c+j for the four
// sequences; the in-quad transpose hands it the four columns of (sequence g, unit 16c+j), where r, z, n and h' are computed once.
// BN2 is one scale and one shift, applied where x_t is staged (TRAIN: folded from the encoder launch's partial sums; workgroup 0
// writes stat2 = mean, invstd and updates the running buffers; x^ is kept for dW_ih).  Sequences past the end of the batch are
// copies of the last one: every store is unconditional.
constexpr int GF_THREADS = 384;
constexpr int GF_HS = GH + 4;     // h rows in LDS (16-byte aligned rows for the float4 A-fragment reads)
constexpr int GF_XS = 64 + 4;     // x rows in LDS
template <bool TRAIN>
__global__ __launch_bounds__(GF_THREADS) void gru_fwd4_kernel(const float* __restrict__ Y, float* __restrict__ xhat,
                                                              const float* __restrict__ wih, const float* __restrict__ whh,
                                                              const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                              const long long* __restrict__ lengths, GruBn bn2,
                                                              const double* __restrict__ part2, int nparts2, double count2,
                                                              float* __restrict__ stat2, float* __restrict__ gates, float* __restrict__ hseq,
                                                              float* __restrict__ hT, int B, int T1) {
    __shared__ __attribute__((aligned(16))) float hbuf[2][4 * GF_HS];
    __shared__ __attribute__((aligned(16))) float xbuf[2][4 * GF_XS];
    __shared__ double scratch[256], tot[2];
    __shared__ float aff[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane >> 2, g = lane & 3;
    const int u = 16 * c + j;
    const int b0 = blockIdx.x * 4;
    if constexpr (TRAIN) {
        fold_parts<2>(part2, nparts2, scratch, tot);
        if (tid == 0) {
            const double mean = tot[0] / count2;
            const double var = fmax(tot[1] / count2 - mean * mean, 0.0);
            const float meanf = (float)mean, invstd = (float)(1.0 / sqrt(var + (double)BN_EPS));
            bn_affine(bn2.gamma[0], bn2.beta[0], meanf, invstd, aff[0], aff[1]);
            if (blockIdx.x == 0) {
                stat2[0] = meanf;
                stat2[1] = invstd;
                bn2.rmean[0] = (1.0f - BN_MOMENTUM) * bn2.rmean[0] + BN_MOMENTUM * meanf;
                bn2.rvar[0] = (1.0f - BN_MOMENTUM) * bn2.rvar[0] + BN_MOMENTUM * (float)(var * count2 / (count2 - 1.0));
                bn2.batches[0] += 1;
            }
        }
    } else {
        if (tid == 0) bn_affine(bn2.gamma[0], bn2.beta[0], bn2.rmean[0], 1.0f / sqrtf(bn2.rvar[0] + BN_EPS), aff[0], aff[1]);
    }
    // the lane's weight rows, read in place: no packing launch
    const int hrow = (g < 3 ? g : 2) * GH + u, xrow = (g == 3 ? 2 : g) * GH + u;
    const bool has_h = g < 3, has_x = g != 2;
    float wB[GH], wI[GM];
#pragma unroll
    for (int k = 0; k < GH; ++k) {
        const float v = whh[(size_t)hrow * GH + k];
        wB[k] = has_h ? v : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < GM; ++k) {
        const float v = wih[(size_t)xrow * GM + k];
        wI[k] = has_x ? v : 0.0f;
    }
    const float bias = g < 2 ? b_ih[g * GH + u] + b_hh[g * GH + u] : g == 2 ? b_hh[2 * GH + u] : b_ih[2 * GH + u];
    // cell role: sequence g of the workgroup, unit u
    const int bc = min(b0 + g, B - 1);
    const int len = lengths != nullptr ? max(0, min((int)((lengths[bc] + 4) / 2), T1)) : T1;
    float hst = 0.0f;
    hbuf[0][g * GF_HS + u] = 0.0f;
    if constexpr (TRAIN) hseq[((size_t)bc * (T1 + 1)) * GH + u] = 0.0f;
    // thread (sequence xr, feature xm) of the first 160 carries x_t of the NEXT step into xbuf (requested a step ahead)
    const bool xthread = tid < 4 * GM;
    const int xr = min(tid / GM, 3), xm = tid - (tid / GM) * GM;
    const size_t xo = ((size_t)min(b0 + xr, B - 1) * T1) * GM + xm;
    __syncthreads();      // aff
    const float s2 = aff[0], t2 = aff[1];
    float xn = 0.0f;
    if (xthread) {
        const float x0 = fmaf(Y[xo], s2, t2);
        xbuf[0][xr * GF_XS + xm] = x0;
        if constexpr (TRAIN) xhat[xo] = x0;
        xn = Y[xo + (size_t)(T1 > 1 ? 1 : 0) * GM];
    }
    const int jx = j < GM / 4 ? j : 0, jh = j < (GH - 64) / 4 ? j : 0;      // lanes beyond K re-read block 0: never multiplied
    size_t go = ((size_t)bc * T1) * GSV + u, ho = ((size_t)bc * (T1 + 1) + 1) * GH + u;
    __syncthreads();
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): the weight loads are complete before the loop (see lstm_fwd4_kernel)
    for (int t = 0; t < T1; ++t) {
        const float* hcur = hbuf[t & 1];
        float* hnxt = hbuf[(t + 1) & 1];
        const float xw = fmaf(xn, s2, t2);      // x^_{t+1}, requested a step ago; goes to LDS at the end of this step
        if (xthread) xn = Y[xo + (size_t)min(t + 2, T1 - 1) * GM];
        const float4 ax = *reinterpret_cast<const float4*>(&xbuf[t & 1][g * GF_XS + 4 * jx]);
        const float4 alo = *reinterpret_cast<const float4*>(hcur + g * GF_HS + 4 * j);
        const float4 ahi = *reinterpret_cast<const float4*>(hcur + g * GF_HS + 64 + 4 * jh);
        f32x4 acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = {0.0f, 0.0f, 0.0f, 0.0f};
        bcast_mfma64<0, 0, GM, GM / 4>(ax, wI, acc);
        bcast_mfma64<0, 0, GH, 16>(alo, wB, acc);
        bcast_mfma64<0, 64, GH, (GH - 64) / 4>(ahi, wB, acc);
        const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = sum[r] + bias;
        quad_transpose(v, (g & 1) != 0, (g & 2) != 0);      // -> r, z, W_hn h + b_hn, W_in x + b_in of (sequence g, unit u)
        const float rg = sigmoidf_(v[0]), zg = sigmoidf_(v[1]);
        const float ng = tanhf_(fmaf(rg, v[2], v[3]));
        const float hn = fmaf(zg, hst - ng, ng);            // (1 - z) n + z h
        hst = t < len ? hn : hst;
        hnxt[g * GF_HS + u] = hst;
        if (xthread && t + 1 < T1) {
            xbuf[(t + 1) & 1][xr * GF_XS + xm] = xw;
            if constexpr (TRAIN) xhat[xo + (size_t)(t + 1) * GM] = xw;
        }
        if constexpr (TRAIN) {
            gates[go] = rg;
            gates[go + GH] = zg;
            gates[go + 2 * GH] = ng;
            gates[go + 3 * GH] = v[2];
            hseq[ho] = hst;
            go += GSV;
            ho += GH;
        }
        __syncthreads();
    }
    hT[(size_t)bc * GH + u] = hst;
}

// The head on the (B, 96) final states, one workgroup per utterance: y1 = relu(h W1^T + b1), y1d = y1 * mask * keep_scale, logits =
// y1d W2^T + b2.  y1d (kept when given) carries both the ReLU's and the dropout's mask for the backward: y1d > 0.
__global__ __launch_bounds__(256) void gru_head_fwd_kernel(const float* __restrict__ hT, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, const float* __restrict__ mask, float keep_scale,
                                                           int C, float* __restrict__ y1d, float* __restrict__ logits) {
    __shared__ float hs[GH], ys[GHD];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < GH) hs[tid] = hT[(size_t)b * GH + tid];
    __syncthreads();
    if (tid < GHD) {
        float a = b1[tid];
        for (int k = 0; k < GH; ++k) a = fmaf(w1[tid * GH + k], hs[k], a);
        float y = fmaxf(a, 0.0f);
        if (mask != nullptr) y = y * mask[(size_t)b * GHD + tid] * keep_scale;
        ys[tid] = y;
        if (y1d != nullptr) y1d[(size_t)b * GHD + tid] = y;
    }
    __syncthreads();
    for (int cl = wave; cl < C; cl += 4) {
        float a = 0.0f;
        for (int k = lane; k < GHD; k += 64) a = fmaf(w2[(size_t)cl * GHD + k], ys[k], a);
        a = wave_sum(a);
        if (lane == 0) logits[(size_t)b * C + cl] = a + b2[cl];
    }
}

// dz1 = (y1d > 0) keep_scale (dlogits W2), d h_T = dz1 W1; the four weight gradients are reductions over the B rows (GEMM path)
__global__ __launch_bounds__(256) void gru_head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ y1d,
                                                           const float* __restrict__ w1, const float* __restrict__ w2, float keep_scale,
                                                           int C, float* __restrict__ dz1, float* __restrict__ dhT) {
    __shared__ float dls[HOWL_GRU_MAX_LABELS], dzs[GHD];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid < C) dls[tid] = dlogits[(size_t)b * C + tid];
    __syncthreads();
    if (tid < GHD) {
        float a = 0.0f;
        for (int cl = 0; cl < C; ++cl) a = fmaf(dls[cl], w2[(size_t)cl * GHD + tid], a);
        const float dz = y1d[(size_t)b * GHD + tid] > 0.0f ? a * keep_scale : 0.0f;
        dzs[tid] = dz;
        dz1[(size_t)b * GHD + tid] = dz;
    }
    __syncthreads();
    if (tid < GH) {
        float a = 0.0f;
        for (int k = 0; k < GHD; ++k) a = fmaf(dzs[k], w1[k * GH + tid], a);
        dhT[(size_t)b * GH + tid] = a;
    }
}

// Backward recurrence from d h_T, four sequences per workgroup (lstm_bwd4_kernel's scheme): d h_{t-1}[4][96] = z d h_t + dGh_t[4][288]
// W_hh on v_mfma_f32_4x4x1.  Six waves: wave w = (hidden-column chunk ch = w & 1 of 64, of which the second holds 32 columns and
// 32 copies of the last; K range kr = w >> 1: the r, z or n block of dGh, 96 W_hh registers per lane); the three K ranges meet in
// LDS and are summed in a fixed order by the thread that owns the cell, thread (sequence tid / 96, unit tid % 96).
//   dGx (B,T1,288) = d r~, d z~, d n~            (for dW_ih, db_ih and dX^)
//   dGh (B,T1,288) = d r~, d z~, d n~ * r        (for dW_hh, db_hh)      -- rows of steps an utterance did not run are zero
// bpart[workgroup][576]: this workgroup's sums over steps and sequences of dGx | dGh (the bias gradients).
constexpr int GB_THREADS = 384;
constexpr int GB_DGS = G3 + 4;      // dGh rows in LDS (16-byte aligned rows)
constexpr int GB_PS = 128 + 4;
__global__ __launch_bounds__(GB_THREADS) void gru_bwd4_kernel(const float* __restrict__ dhT, const float* __restrict__ whh,
                                                              const long long* __restrict__ lengths, const float* __restrict__ gates,
                                                              const float* __restrict__ hseq, float* __restrict__ dGx,
                                                              float* __restrict__ dGh, float* __restrict__ bpart, int B, int T1) {
    __shared__ __attribute__((aligned(16))) float dgt[4 * GB_DGS];
    __shared__ float partd[3][4 * GB_PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, kr = wave >> 1;
    const int b0 = blockIdx.x * 4;
    const int col = min(64 * ch + lane, GH - 1);
    float wk[GH];      // W_hh[96 kr + k][col], read in place (coalesced over the lanes)
#pragma unroll
    for (int kk = 0; kk < GH; ++kk) wk[kk] = whh[(size_t)(GH * kr + kk) * GH + col];
    const int s = tid / GH, u = tid - (tid / GH) * GH;
    const int b = min(b0 + s, B - 1);
    const bool dup = b0 + s >= B;
    const int len = lengths != nullptr ? max(0, min((int)((lengths[b] + 4) / 2), T1)) : T1;
    float dhp = dhT[(size_t)b * GH + u];
    float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = tid; i < 3 * 4 * GB_PS; i += GB_THREADS) (&partd[0][0])[i] = 0.0f;
    struct Step {
        float rg, zg, ng, hn, hp;
    };
    // a step's saved activations are requested right after the previous step's gate gradients went out and taken (masked) after
    // that step's matrix work (see lstm_bwd4_kernel)
    Step raw;
    auto request = [&](int t) {      // unconditional loads from clamped addresses
        const size_t o = (size_t)b * T1 + (t >= 0 ? t : 0);
        raw.rg = gates[o * GSV + u];
        raw.zg = gates[o * GSV + GH + u];
        raw.ng = gates[o * GSV + 2 * GH + u];
        raw.hn = gates[o * GSV + 3 * GH + u];
        raw.hp = hseq[((size_t)b * (T1 + 1) + (t >= 0 ? t : 0)) * GH + u];
    };
    Step cur;
    request(T1 - 1);
    cur = raw;
    const int jh = (lane >> 2) < (GH - 64) / 4 ? (lane >> 2) : 0;
    __syncthreads();
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
    for (int t = T1 - 1; t >= 0; --t) {
        {
            float dh = dhp;
#pragma unroll
            for (int r = 0; r < 3; ++r) dh += partd[r][s * GB_PS + u];
            float dr = 0.0f, dz = 0.0f, dn = 0.0f, dnr = 0.0f;
            if (t < len) {
                dn = dh * (1.0f - cur.zg) * (1.0f - cur.ng * cur.ng);
                dz = dh * (cur.hp - cur.ng) * cur.zg * (1.0f - cur.zg);
                dr = dn * cur.hn * cur.rg * (1.0f - cur.rg);
                dnr = dn * cur.rg;
                dhp = dh * cur.zg;
            } else {
                dhp = dh;      // frozen step: h_t = h_{t-1}
            }
            float* dl = dgt + s * GB_DGS + u;
            dl[0] = dr;
            dl[GH] = dz;
            dl[2 * GH] = dnr;
            bs[0] += dr;
            bs[1] += dz;
            bs[2] += dn;
            bs[3] += dnr;
            const size_t o = ((size_t)b * T1 + t) * G3 + u;
            dGx[o] = dr;
            dGx[o + GH] = dz;
            dGx[o + 2 * GH] = dn;
            dGh[o] = dr;
            dGh[o + GH] = dz;
            dGh[o + 2 * GH] = dnr;
            request(t - 1);
        }
        __syncthreads();
        f32x4 acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* arow = dgt + (lane & 3) * GB_DGS + GH * kr;
        const float4 alo = *reinterpret_cast<const float4*>(arow + 4 * (lane >> 2)), ahi = *reinterpret_cast<const float4*>(arow + 64 + 4 * jh);
        bcast_mfma64<0, 0, GH, 16>(alo, wk, acc);
        bcast_mfma64<0, 64, GH, (GH - 64) / 4>(ahi, wk, acc);
        const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) partd[kr][r * GB_PS + 64 * ch + lane] = sum[r];
        HOWL_SCHED_PIN();      // the saved activations are not touched before this point
        cur = raw;
        __syncthreads();
    }
    if (dup) bs[0] = bs[1] = bs[2] = bs[3] = 0.0f;
    // bias gradients: the step sums are in registers, the four sequences meet in LDS (reusing partd: 4 x 96 x 4 floats)
    float* red = &partd[0][0];
    red[(s * 4 + 0) * GH + u] = bs[0];
    red[(s * 4 + 1) * GH + u] = bs[1];
    red[(s * 4 + 2) * GH + u] = bs[2];
    red[(s * 4 + 3) * GH + u] = bs[3];
    __syncthreads();
    if (tid < GSV) {
        const int k = tid / GH, uu = tid - k * GH;      // k: 0 dr, 1 dz, 2 dn, 3 dn * r
        const float v = ((red[(0 * 4 + k) * GH + uu] + red[(1 * 4 + k) * GH + uu]) + red[(2 * 4 + k) * GH + uu]) + red[(3 * 4 + k) * GH + uu];
        float* bp = bpart + (size_t)blockIdx.x * (2 * G3);
        if (k < 3) bp[k * GH + uu] = v;                  // db_ih = sums of dGx
        if (k < 2) bp[G3 + k * GH + uu] = v;             // db_hh = sums of dGh
        if (k == 3) bp[G3 + 2 * GH + uu] = v;
    }
}

// BN2's backward batch sums over the B * T1 * 40 elements: part[chunk] = sum dX^, sum dX^ x^n (x^n: the normalised relu(conv2))
__global__ __launch_bounds__(256) void gru_bn2_bwd_sums_kernel(const float* __restrict__ dxhat, const float* __restrict__ Y,
                                                               const float* __restrict__ stat2, size_t n, double* __restrict__ part) {
    __shared__ double red[4][2];
    const float mean = stat2[0], invstd = stat2[1];
    double acc[2] = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float d = dxhat[i], xn = (Y[i] - mean) * invstd;
        acc[0] += (double)d;
        acc[1] += (double)d * (double)xn;
    }
    block_sum_d<2>(acc, red, part + (size_t)blockIdx.x * 2);
}

// Encoder backward down to BN1's output, one tile of ENC_TP pooled columns of one utterance: BN2 (folding the launch before's
// sums; workgroup (0, 0) writes d gamma2, d beta2) - ReLU - conv2's weight / bias gradient (cpart2[(b, tile)][0..71 | 72]) and
// data gradient - un-pool + ReLU (dA, laid out as P: the gradient at the pool's argmax, zero where the pooled value is 0) and BN1's
// batch sums part4[(b, tile)] = sum dA, sum dA x^n per channel (conv1 recomputed at both columns of the pair).
__global__ __launch_bounds__(ENC_THREADS) void gru_enc_bwd2_kernel(const float* __restrict__ x, long sb, long sm, long st, int T, int T1,
                                                                   const float* __restrict__ c1w, const float* __restrict__ c1b,
                                                                   const float* __restrict__ g1, const float* __restrict__ be1,
                                                                   const float* __restrict__ c2w, const float* __restrict__ g2,
                                                                   const float* __restrict__ stat1, const float* __restrict__ stat2,
                                                                   const double* __restrict__ part3, int nparts3, double count2,
                                                                   const float* __restrict__ P, const float* __restrict__ Y,
                                                                   const float* __restrict__ dxhat, float* __restrict__ dA,
                                                                   float* __restrict__ cpart2, double* __restrict__ part4,
                                                                   float* __restrict__ g_bn2_w, float* __restrict__ g_bn2_b) {
    __shared__ float cw[80], w2s[72], sc[GC], sh[GC];
    __shared__ float pt[GC * ENC_ROWS * ENC_PW];
    __shared__ float dc[ENC_ROWS * ENC_PW];
    __shared__ double scratch[256], tot[2], red[4][16];
    __shared__ float redf[4][73];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
    if (tid < 72) cw[tid] = c1w[tid];
    else if (tid < 80) cw[tid] = c1b[tid - 72];
    if (tid >= 128 && tid < 128 + 72) w2s[tid - 128] = c2w[tid - 128];
    if (tid >= 200 && tid < 200 + GC) bn_affine(g1[tid - 200], be1[tid - 200], stat1[tid - 200], stat1[8 + tid - 200], sc[tid - 200], sh[tid - 200]);
    fold_parts<2>(part3, nparts3, scratch, tot);
    if (tile == 0 && b == 0 && tid == 0) {
        g_bn2_b[0] = (float)tot[0];
        g_bn2_w[0] = (float)tot[1];
    }
    const float mean2 = stat2[0], invstd2 = stat2[1];
    const float md = (float)(tot[0] / count2), mdx = (float)(tot[1] / count2), k2 = g2[0] * invstd2;
    const int p0 = tile * ENC_TP;
    for (int i = tid; i < 2 * ENC_PW; i += ENC_THREADS) dc[(i / ENC_PW) * (ENC_ROWS - 1) * ENC_PW + i % ENC_PW] = 0.0f;
    for (int i = tid; i < GC * 2 * ENC_PW; i += ENC_THREADS) {
        const int c = i / (2 * ENC_PW), r = (i / ENC_PW) & 1, pc = i % ENC_PW;
        pt[(c * ENC_ROWS + r * (ENC_ROWS - 1)) * ENC_PW + pc] = 0.0f;
    }
    for (int i = tid; i < GM * ENC_PW; i += ENC_THREADS) {
        const int m = i % GM, pc = i / GM, p = p0 - 1 + pc;
        float v = 0.0f;
        if (p >= 0 && p < T1) {
            const size_t o = ((size_t)b * T1 + p) * GM + m;
            const float y = Y[o], xn = (y - mean2) * invstd2;
            v = y > 0.0f ? k2 * (dxhat[o] - md - xn * mdx) : 0.0f;
        }
        dc[(m + 1) * ENC_PW + pc] = v;
    }
    const bool m_fast = sm == 1;
    for (int i = tid; i < GC * GM * ENC_PW; i += ENC_THREADS) {
        const int c = i / (ENC_PW * GM);
        int m, pc;
        tile_item(i - c * (ENC_PW * GM), ENC_PW, m_fast, m, pc);
        const int p = p0 - 1 + pc;
        pt[(c * ENC_ROWS + m + 1) * ENC_PW + pc] = (p >= 0 && p < T1) ? P[pool_at(b, c, m, p, T1, m_fast)] : 0.0f;
    }
    __syncthreads();
    const float* xb = x + (long)b * sb;
    // conv2's weight and bias gradient: 73 sums per thread over its items, then over the workgroup (a loop of its own, so that its
    // accumulators are not live across the un-pool loop below: two waves per SIMD instead of one)
    {
        float wacc[73];
#pragma unroll
        for (int k = 0; k < 73; ++k) wacc[k] = 0.0f;
        for (int i = tid; i < GM * ENC_TP; i += ENC_THREADS) {
            int m, pc;
            tile_item(i, ENC_TP, m_fast, m, pc);
            pc += 1;
            if (p0 - 1 + pc >= T1) continue;
            const float d = dc[(m + 1) * ENC_PW + pc];
            wacc[72] += d;
#pragma unroll
            for (int c = 0; c < GC; ++c)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx)
                        wacc[c * 9 + dy * 3 + dx] = fmaf(d, pt[(c * ENC_ROWS + m + dy) * ENC_PW + pc - 1 + dx], wacc[c * 9 + dy * 3 + dx]);
        }
#pragma unroll
        for (int k = 0; k < 73; ++k) {
            const float v = wave_sum(wacc[k]);
            if (lane == 0) redf[wave][k] = v;
        }
    }
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    for (int i = tid; i < GM * ENC_TP; i += ENC_THREADS) {
        int m, pc;
        tile_item(i, ENC_TP, m_fast, m, pc);
        pc += 1;
        const int p = p0 - 1 + pc;
        if (p >= T1) continue;
        // the pair of conv1 columns behind pooled column p, for the argmax and x^n there
        float xv[9], z0[GC], z1[GC];
        conv1_at(xb, sm, st, T, m, 2 * p, cw, xv, z0);
        conv1_at(xb, sm, st, T, m, 2 * p + 1, cw, xv, z1);
#pragma unroll
        for (int c = 0; c < GC; ++c) {
            float dp = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) dp = fmaf(w2s[c * 9 + dy * 3 + dx], dc[(m + 2 - dy) * ENC_PW + pc + 1 - dx], dp);
            const float gq = pt[(c * ENC_ROWS + m + 1) * ENC_PW + pc] > 0.0f ? dp : 0.0f;
            dA[pool_at(b, c, m, p, T1, m_fast)] = gq;
            const bool second = fmaf(z1[c], sc[c], sh[c]) > fmaf(z0[c], sc[c], sh[c]);
            const float xn = ((second ? z1[c] : z0[c]) - stat1[c]) * stat1[8 + c];
            acc[c] += (double)gq;
            acc[8 + c] += (double)gq * (double)xn;
        }
    }
    block_sum_d<16>(acc, red, part4 + ((size_t)b * gridDim.x + tile) * 16);      // (its barrier covers redf)
    if (tid < 73) cpart2[((size_t)b * gridDim.x + tile) * 80 + tid] = ((redf[0][tid] + redf[1][tid]) + redf[2][tid]) + redf[3][tid];
}

// BN1's backward (folding part4; workgroup (0, 0) writes d gamma1, d beta1) and conv1's weight gradient over one tile of ST_TP
// column pairs of one utterance: cpart1[(b, tile)][0..71].  conv1's output is recomputed; BN1's input gradient is dense:
// d z = gamma invstd (dA at the pair's argmax, else 0, - mean(dA) - x^n mean(dA x^n)).  conv1's BIAS sits in front of a
// training-mode BatchNorm: the batch mean absorbs it and its gradient, the sum of d z over the batch, is identically zero.  It is
// written as that zero (by workgroup (0, 0)) and not as the rounding residue of a sum that cancels: an optimiser that normalises
// each gradient by its own magnitude would step by the sign of the residue.
__global__ __launch_bounds__(ENC_THREADS) void gru_enc_bwd1_kernel(const float* __restrict__ x, long sb, long sm, long st, int T, int T1,
                                                                   const float* __restrict__ c1w, const float* __restrict__ c1b,
                                                                   const float* __restrict__ g1, const float* __restrict__ be1,
                                                                   const float* __restrict__ stat1, const double* __restrict__ part4,
                                                                   int nparts4, double count1, const float* __restrict__ dA,
                                                                   float* __restrict__ cpart1, float* __restrict__ g_bn1_w,
                                                                   float* __restrict__ g_bn1_b, float* __restrict__ g_c1b) {
    __shared__ float cw[80], sc[GC], sh[GC], mg[GC], mgx[GC];
    __shared__ double scratch[256], tot[16];
    __shared__ float redf[4][72];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
    const int W1 = T + 4, np = (W1 + 1) / 2;
    if (tid < 72) cw[tid] = c1w[tid];
    else if (tid < 80) cw[tid] = c1b[tid - 72];
    fold_parts<16>(part4, nparts4, scratch, tot);
    if (tid < GC) {
        bn_affine(g1[tid], be1[tid], stat1[tid], stat1[8 + tid], sc[tid], sh[tid]);
        mg[tid] = (float)(tot[tid] / count1);
        mgx[tid] = (float)(tot[8 + tid] / count1);
        if (tile == 0 && b == 0) {
            g_bn1_b[tid] = (float)tot[tid];
            g_bn1_w[tid] = (float)tot[8 + tid];
            g_c1b[tid] = 0.0f;
        }
    }
    __syncthreads();
    const int p0 = tile * ST_TP, n = min(ST_TP, np - p0);
    const float* xb = x + (long)b * sb;
    float wacc[72];
#pragma unroll
    for (int k = 0; k < 72; ++k) wacc[k] = 0.0f;
    const bool m_fast = sm == 1;
    for (int i = tid; i < GM * n; i += ENC_THREADS) {
        int m, p;
        tile_item(i, n, m_fast, m, p);
        p += p0;
        const bool pair = 2 * p + 1 < W1;      // (p == T1 with T + 4 odd: the column the pool dropped)
        float xv0[9], xv1[9], z0[GC], z1[GC];
        conv1_at(xb, sm, st, T, m, 2 * p, cw, xv0, z0);
        conv1_at(xb, sm, st, T, m, pair ? 2 * p + 1 : 2 * p, cw, xv1, z1);
#pragma unroll
        for (int c = 0; c < GC; ++c) {
            const float gq = p < T1 ? dA[pool_at(b, c, m, p, T1, m_fast)] : 0.0f;
            const bool second = pair && fmaf(z1[c], sc[c], sh[c]) > fmaf(z0[c], sc[c], sh[c]);
            const float k1 = sc[c];      // gamma invstd
            const float xn0 = (z0[c] - stat1[c]) * stat1[8 + c], xn1 = (z1[c] - stat1[c]) * stat1[8 + c];
            const float d0 = k1 * ((second ? 0.0f : gq) - mg[c] - xn0 * mgx[c]);
            const float d1 = pair ? k1 * ((second ? gq : 0.0f) - mg[c] - xn1 * mgx[c]) : 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) wacc[c * 9 + k] = fmaf(d1, xv1[k], fmaf(d0, xv0[k], wacc[c * 9 + k]));
        }
    }
#pragma unroll
    for (int k = 0; k < 72; ++k) {
        const float v = wave_sum(wacc[k]);
        if (lane == 0) redf[wave][k] = v;
    }
    __syncthreads();
    if (tid < 72) cpart1[((size_t)b * gridDim.x + tile) * 72 + tid] = ((redf[0][tid] + redf[1][tid]) + redf[2][tid]) + redf[3][tid];
}

// How one problem (B utterances of T frames, num_labels) runs: geometry, the workspace carve-up and the launch shapes, decided
// once per call; `bad` says why a problem is refused.
struct GruPlan {
    char bad[96];
    int W1, T1, np;            // conv1's columns, pooled columns = recurrence steps, column pairs
    int ntile1, ntile2, nrec;  // tiles per utterance of the statistic / conv1-gradient kernels and of the encoder kernels; recurrence workgroups
    int nsum3;                 // workgroups of BN2's backward sums
    long rows;                 // B * T1
    double count1, count2;     // elements per channel of BN1 and BN2
    // saved by the forward
    double *part1, *part2;
    float *stat1, *stat2, *P, *Y, *xhat, *gates, *hseq, *hT, *y1d;
    // backward
    double *part3, *part4;
    float *dz1, *dhT, *dGx, *dGh, *bpart, *dxhat, *dA, *cpart1, *cpart2;
    float *slabs_ih, *slabs_hh, *slabs_w1, *slabs_w2, *scratch_b1, *scratch_b2;
    size_t bytes;
};
GruPlan gru_plan(int B, int M, int T, int num_labels, void* ws = nullptr) {
    GruPlan q{};
    if (B < 1) snprintf(q.bad, sizeof(q.bad), "B=%d: at least one utterance", B);
    else if (M != GM) snprintf(q.bad, sizeof(q.bad), "M=%d mel bins: the kernels are specialised for 40", M);
    else if (T < 1 || T > HOWL_GRU_MAX_FRAMES) snprintf(q.bad, sizeof(q.bad), "T=%d frames outside 1..%d", T, HOWL_GRU_MAX_FRAMES);
    else if (num_labels < 1 || num_labels > HOWL_GRU_MAX_LABELS)
        snprintf(q.bad, sizeof(q.bad), "num_labels=%d outside 1..%d", num_labels, HOWL_GRU_MAX_LABELS);
    if (q.bad[0] != 0) return q;
    q.W1 = T + 4;
    q.T1 = q.W1 / 2;
    q.np = (q.W1 + 1) / 2;
    q.ntile1 = (q.np + ST_TP - 1) / ST_TP;
    q.ntile2 = (q.T1 + ENC_TP - 1) / ENC_TP;
    q.nrec = (B + 3) / 4;
    q.rows = (long)B * q.T1;
    q.nsum3 = (int)std::min<long>(256, (q.rows * GM + 1023) / 1024);
    q.count1 = (double)B * GM * q.W1;
    q.count2 = (double)B * GM * q.T1;
    size_t off = 0;      // in floats; every region starts on a 16-byte boundary
    auto region = [&](size_t floats) {
        const size_t at = off;
        off += (floats + 3) / 4 * 4;
        return ws != nullptr ? static_cast<float*>(ws) + at : nullptr;
    };
    auto dregion = [&](size_t doubles) { return reinterpret_cast<double*>(region(2 * doubles)); };
    const size_t rows = (size_t)q.rows, nb1 = (size_t)B * q.ntile1, nb2 = (size_t)B * q.ntile2;
    q.part1 = dregion(nb1 * 16);
    q.part2 = dregion(nb2 * 2);
    q.part3 = dregion((size_t)q.nsum3 * 2);
    q.part4 = dregion(nb2 * 16);
    q.stat1 = region(16);
    q.stat2 = region(4);
    q.P = region(rows * GC * GM);
    q.Y = region(rows * GM);
    q.xhat = region(rows * GM);
    q.gates = region(rows * GSV);
    q.hseq = region((size_t)B * (q.T1 + 1) * GH);
    q.hT = region((size_t)B * GH);
    q.y1d = region((size_t)B * GHD);
    q.dz1 = region((size_t)B * GHD);
    q.dhT = region((size_t)B * GH);
    q.dGx = region(rows * G3);
    q.dGh = region(rows * G3);
    q.bpart = region((size_t)q.nrec * 2 * G3);
    q.dxhat = region(rows * GM);
    q.dA = region(rows * GC * GM);
    q.cpart1 = region(nb1 * 72);
    q.cpart2 = region(nb2 * 80);
    q.slabs_ih = region((size_t)GRU_WGRAD_SPLITS * G3 * GM);
    q.slabs_hh = region((size_t)GRU_WGRAD_SPLITS * G3 * GH);
    q.slabs_w1 = region((size_t)GRU_HEAD_SPLITS * GHD * GH);
    q.slabs_w2 = region((size_t)GRU_HEAD_SPLITS * HOWL_GRU_MAX_LABELS * GHD);
    q.scratch_b1 = region((size_t)64 * GHD);
    q.scratch_b2 = region((size_t)64 * HOWL_GRU_MAX_LABELS);
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

int howl_gru_supported(int B, int M, int T, int num_labels) { return gru_plan(B, M, T, num_labels).bad[0] == 0 ? 1 : 0; }

size_t howl_gru_workspace_bytes(int B, int T) { return gru_plan(B, GM, T, 1).bytes; }

int howl_gru_fwd(const HowlGruParams* p, const HowlGruBuffers* bf, const float* x, long sb, long sm, long st, int B, int M, int T,
                 int num_labels, const long long* lengths, int training, const float* drop_mask, float keep_scale, float* logits,
                 void* ws, size_t ws_bytes, hipStream_t stream) {
    HOWL_REQUIRE(p && bf && x && logits && ws && all_set(reinterpret_cast<const void* const*>(p), 16) &&
                     all_set(reinterpret_cast<const void* const*>(bf), 6), "howl_gru_fwd: null pointer");
    HOWL_REQUIRE(training || drop_mask == nullptr, "howl_gru_fwd: a dropout mask in eval mode");
    const GruPlan q = gru_plan(B, M, T, num_labels, ws);
    HOWL_REQUIRE(q.bad[0] == 0, "howl_gru_fwd: %s", q.bad);
    if (ws_bytes < q.bytes) {
        howl_set_error("howl_gru_fwd: workspace too small (%zu < %zu bytes)", ws_bytes, q.bytes);
        return HOWL_E_WORKSPACE;
    }
    const GruBn bn1{p->bn1_w, p->bn1_b, bf->bn1_mean, bf->bn1_var, bf->bn1_batches};
    const GruBn bn2{p->bn2_w, p->bn2_b, bf->bn2_mean, bf->bn2_var, bf->bn2_batches};
    const int np1 = B * q.ntile1, np2 = B * q.ntile2;
    {
        HowlProfScope prof("gru_enc_fwd", stream, 2.0 * 9 * GC * GM * ((training ? 2.0 : 1.0) * q.W1 + q.T1) * B);
        if (training) {
            hipLaunchKernelGGL(gru_conv1_stats_kernel, dim3(q.ntile1, B), dim3(ENC_THREADS), 0, stream, x, sb, sm, st, T, p->conv1_w, p->conv1_b,
                               q.part1);
            hipLaunchKernelGGL(gru_enc_fwd_kernel<true>, dim3(q.ntile2, B), dim3(ENC_THREADS), 0, stream, x, sb, sm, st, T, q.T1, p->conv1_w,
                               p->conv1_b, bn1, p->conv2_w, p->conv2_b, (const double*)q.part1, np1, q.count1, q.stat1, q.P, q.Y, q.part2);
        } else {
            hipLaunchKernelGGL(gru_enc_fwd_kernel<false>, dim3(q.ntile2, B), dim3(ENC_THREADS), 0, stream, x, sb, sm, st, T, q.T1, p->conv1_w,
                               p->conv1_b, bn1, p->conv2_w, p->conv2_b, (const double*)nullptr, 0, q.count1, (float*)nullptr, (float*)nullptr, q.Y,
                               (double*)nullptr);
        }
    }
    {
        HowlProfScope prof("gru_fwd", stream, 2.0 * GSV * (GH + GM) * (double)q.rows);
        if (training)
            hipLaunchKernelGGL(gru_fwd4_kernel<true>, dim3(q.nrec), dim3(GF_THREADS), 0, stream, (const float*)q.Y, q.xhat, p->w_ih, p->w_hh, p->b_ih,
                               p->b_hh, lengths, bn2, (const double*)q.part2, np2, q.count2, q.stat2, q.gates, q.hseq, q.hT, B, q.T1);
        else
            hipLaunchKernelGGL(gru_fwd4_kernel<false>, dim3(q.nrec), dim3(GF_THREADS), 0, stream, (const float*)q.Y, (float*)nullptr, p->w_ih,
                               p->w_hh, p->b_ih, p->b_hh, lengths, bn2, (const double*)nullptr, 0, q.count2, (float*)nullptr, (float*)nullptr,
                               (float*)nullptr, q.hT, B, q.T1);
    }
    {
        HowlProfScope prof("gru_head", stream, 2.0 * GHD * (GH + num_labels) * (double)B);
        hipLaunchKernelGGL(gru_head_fwd_kernel, dim3(B), dim3(256), 0, stream, (const float*)q.hT, p->w1, p->b1, p->w2, p->b2, drop_mask,
                           keep_scale, num_labels, training ? q.y1d : (float*)nullptr, logits);
    }
    HOWL_CHECK_LAUNCH("howl_gru_fwd");
    return HOWL_OK;
}

int howl_gru_bwd(const HowlGruParams* p, const float* x, long sb, long sm, long st, int B, int M, int T, int num_labels,
                 const long long* lengths, float keep_scale, const float* dlogits, const HowlGruGrads* g, void* ws, size_t ws_bytes,
                 hipStream_t stream) {
    HOWL_REQUIRE(p && x && dlogits && g && ws && all_set(reinterpret_cast<const void* const*>(p), 16) &&
                     all_set(reinterpret_cast<const void* const*>(g), 16), "howl_gru_bwd: null pointer");
    const GruPlan q = gru_plan(B, M, T, num_labels, ws);
    HOWL_REQUIRE(q.bad[0] == 0, "howl_gru_bwd: %s", q.bad);
    if (ws_bytes < q.bytes) {
        howl_set_error("howl_gru_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, q.bytes);
        return HOWL_E_WORKSPACE;
    }
    const int rows = (int)q.rows, np2 = B * q.ntile2;
    SlabSums sums;
    {
        HowlProfScope prof("gru_head", stream, 4.0 * GHD * (GH + num_labels) * (double)B);
        hipLaunchKernelGGL(gru_head_bwd_kernel, dim3(B), dim3(256), 0, stream, dlogits, (const float*)q.y1d, p->w1, p->w2, keep_scale, num_labels,
                           q.dz1, q.dhT);
    }
    wgrad_gemm(stream, dlogits, lin(num_labels), num_labels, q.y1d, lin(GHD), GHD, B, q.slabs_w2, g->w2, GRU_HEAD_SPLITS, 512, &sums);
    colsum(stream, dlogits, lin(num_labels), B, num_labels, q.scratch_b2, g->b2, nullptr, 64, 256, &sums);
    wgrad_gemm(stream, q.dz1, lin(GHD), GHD, q.hT, lin(GH), GH, B, q.slabs_w1, g->w1, GRU_HEAD_SPLITS, 512, &sums);
    colsum(stream, q.dz1, lin(GHD), B, GHD, q.scratch_b1, g->b1, nullptr, 64, 256, &sums);
    {
        HowlProfScope prof("gru_bwd", stream, 2.0 * G3 * GH * (double)q.rows);
        hipLaunchKernelGGL(gru_bwd4_kernel, dim3(q.nrec), dim3(GB_THREADS), 0, stream, (const float*)q.dhT, p->w_hh, lengths, (const float*)q.gates,
                           (const float*)q.hseq, q.dGx, q.dGh, q.bpart, B, q.T1);
    }
    // dW_ih = dGx^T X^, dW_hh = dGh^T H_prev (rows t = 0 .. T1-1 of each utterance's hidden sequence), the biases from the
    // recurrence's per-workgroup sums, dX^ = dGx W_ih: howl_gemm.hip.h
    wgrad_gemm(stream, q.dGx, lin(G3), G3, q.xhat, lin(GM), GM, rows, q.slabs_ih, g->w_ih, GRU_WGRAD_SPLITS, 256, &sums);
    wgrad_gemm(stream, q.dGh, lin(G3), G3, q.hseq, RowMap{q.T1, (long)(q.T1 + 1) * GH, GH}, GH, rows, q.slabs_hh, g->w_hh, GRU_WGRAD_SPLITS, 256,
               &sums);
    sums.add_strided(q.bpart, q.nrec, 2 * G3, G3, g->b_ih);
    sums.add_strided(q.bpart + G3, q.nrec, 2 * G3, G3, g->b_hh);
    if (!sums.flush(stream)) return HOWL_E_ARG;
    gemm(stream, true, q.dGx, lin(G3), 1, lin(0), p->w_ih, lin(GM), 1, rows, GM, G3, 1, nullptr, 0, q.dxhat, GM, 0);
    {
        HowlProfScope prof("gru_enc_bwd", stream, 2.0 * 9 * GC * GM * (3.0 * q.W1 + 2.0 * q.T1) * B);
        hipLaunchKernelGGL(gru_bn2_bwd_sums_kernel, dim3(q.nsum3), dim3(256), 0, stream, (const float*)q.dxhat, (const float*)q.Y,
                           (const float*)q.stat2, (size_t)q.rows * GM, q.part3);
        hipLaunchKernelGGL(gru_enc_bwd2_kernel, dim3(q.ntile2, B), dim3(ENC_THREADS), 0, stream, x, sb, sm, st, T, q.T1, p->conv1_w, p->conv1_b,
                           p->bn1_w, p->bn1_b, p->conv2_w, p->bn2_w, (const float*)q.stat1, (const float*)q.stat2, (const double*)q.part3, q.nsum3,
                           q.count2, (const float*)q.P, (const float*)q.Y, (const float*)q.dxhat, q.dA, q.cpart2, q.part4, g->bn2_w, g->bn2_b);
        hipLaunchKernelGGL(gru_enc_bwd1_kernel, dim3(q.ntile1, B), dim3(ENC_THREADS), 0, stream, x, sb, sm, st, T, q.T1, p->conv1_w, p->conv1_b,
                           p->bn1_w, p->bn1_b, (const float*)q.stat1, (const double*)q.part4, np2, q.count1, (const float*)q.dA, q.cpart1, g->bn1_w,
                           g->bn1_b, g->conv1_b);
    }
    sums.add_strided(q.cpart2, np2, 80, 72, g->conv2_w);
    sums.add_strided(q.cpart2 + 72, np2, 80, 1, g->conv2_b);
    sums.add(q.cpart1, B * q.ntile1, 72, g->conv1_w);
    if (!sums.flush(stream)) return HOWL_E_ARG;
    HOWL_CHECK_LAUNCH("howl_gru_bwd");
    return HOWL_OK;
}

}  // extern "C"
