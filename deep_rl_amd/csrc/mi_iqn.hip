// mi_iqn.hip — libmirl_iqn.so: IQN (reference iqn.py) re-targeted to CartPole-v1, for gfx950.  C ABI, numerics and RNG contract: include/mi_iqn.h.
//
// One 256-thread workgroup evaluates one observation with up to 64 taus at a time.  Thread (lane i, wave c) owns TAU ROW i: the row's Hadamard product prod[64] lives
// in its registers, and wave c walks the hidden units of S_c = { u : (u >> 3) & 3 == c } (the header's split).  The weights of a hidden unit are therefore the same
// for every lane of a wave: they come through the scalar cache as SGPR operands of the k-ascending fmaf chain, and the head needs no LDS traffic at all.
//   iqn_forward_kernel   features, tau embedding, head; quantiles and / or their mean
//   iqn_act_kernel       a workgroup walks its envs, each through all steps of the chunk (the structure of c51_act_kernel); exploring steps skip the networks
//   iqn_target_kernel    next actions + target quantiles
//   iqn_grad_kernel      per batch row: targets (target networks), online forward, the 64 x 64 quantile-Huber loss inside the workgroup, backward.  The backward
//                        recomputes the hidden layer in blocks of 32 units: the block's dz / h go through LDS transposed to threads that own (unit, 8 embedding
//                        columns) and reduce over the 64 tau rows; every row's gradient is added to the workgroup's slab by a fixed owner thread.
//   iqn_reduce_kernel    fixed-order slab sum (+ Adam).
//   iqn_huber_kernel     the loss stage alone.
// All arithmetic on the VALU in fp32 with the chains of the header (the chains are what the f32 MFMA forms compute, so a matrix-core version keeps the bits);
// no floating-point atomics.  Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"

#include "../../include/mi_iqn.h"

#define IQ_E MI_IQN_EMB
#define IQ_H MI_IQN_HID
#define IQ_NP MI_IQN_NPARAMS
#define IQ_STRIDE MI_IQN_SLAB_STRIDE
#define IQ_FW1 MI_IQN_FW1
#define IQ_FB1 MI_IQN_FB1
#define IQ_FW2 MI_IQN_FW2
#define IQ_FB2 MI_IQN_FB2
#define IQ_FW3 MI_IQN_FW3
#define IQ_FB3 MI_IQN_FB3
#define IQ_CW MI_IQN_CW
#define IQ_CB MI_IQN_CB
#define IQ_QW1 MI_IQN_QW1
#define IQ_QB1 MI_IQN_QB1
#define IQ_QW2 MI_IQN_QW2
#define IQ_QB2 MI_IQN_QB2
#define IQ_BLK 32              // hidden units per backward block (8 per wave)
#define IQ_STREAM_ACT_TAU 9u
#define IQ_STREAM_TAU 10u
#define IQ_STREAM_NEXT_TAU 11u
#define IQ_STREAM_TAU_DASH 12u
static_assert(MI_IQN_OK == RG_OK && MI_IQN_EINVAL == RG_EINVAL && MI_IQN_EHIP == RG_EHIP && MI_IQN_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");

#ifndef MI_IQN_SOURCE_ID
#define MI_IQN_SOURCE_ID "unknown"
#endif
extern "C" int mi_iqn_version(void) { return MI_IQN_VERSION; }
extern "C" const char* mi_iqn_last_error(void) { return rg_err; }
extern "C" const char* mi_iqn_source_id(void) { return MI_IQN_SOURCE_ID; }
static int iq_slabs(int batch) { return rg_slabs(batch, MI_IQN_MAX_SLABS); }
extern "C" size_t mi_iqn_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)iq_slabs(batch) * IQ_STRIDE * sizeof(float);
}

__constant__ uint32_t iq_ipi_bits[MI_IQN_NCOS] = {MI_IQN_I_PI_BITS};
__device__ __forceinline__ float iq_ipi(int k) { return __uint_as_float(iq_ipi_bits[k]); }

struct iq_smem {
    float teT[64][64];            // te[e][i]; at the end of the backward the cosines c[i][k]
    float prT[64][64];            // tau embedding: cosines c[k][i]; backward: prod[e][i], then dte[e][i]
    float blk[2][IQ_BLK][65];     // backward: dz / h of one hidden block [unit][i] (padded rows: written by lane i, read by lane unit); then dprod[e][i] as float[64][64]
    float part[4][2][64];         // the four partial chains of the head / of the loss
    float out[64][2];             // quantiles [i][a]
    float emb[64], h2[64], h1[32];
    float tau[64], cur[64], tgt[64], dout[64], li[64];
    float dz3[64], dz2[64], dz1[32];
    float q[2];
    float rowloss;
};

// FeaturesExtractor of one observation: sm.h1, sm.h2, sm.emb valid for every thread on return
__device__ __forceinline__ void iq_features(const float* __restrict__ P, const float4 x, iq_smem& sm, int t) {
    if (t < 32) {
        const float4 w = reinterpret_cast<const float4*>(P + IQ_FW1)[t];
        float z = P[IQ_FB1 + t];
        z = __builtin_fmaf(w.x, x.x, z); z = __builtin_fmaf(w.y, x.y, z); z = __builtin_fmaf(w.z, x.z, z); z = __builtin_fmaf(w.w, x.w, z);
        sm.h1[t] = fmaxf(z, 0.0f);
    }
    __syncthreads();
    if (t < 64) {
        const float4* row = reinterpret_cast<const float4*>(P + IQ_FW2 + 32 * t);
        float z = P[IQ_FB2 + t];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 w = row[k];
            z = __builtin_fmaf(w.x, sm.h1[4 * k], z); z = __builtin_fmaf(w.y, sm.h1[4 * k + 1], z);
            z = __builtin_fmaf(w.z, sm.h1[4 * k + 2], z); z = __builtin_fmaf(w.w, sm.h1[4 * k + 3], z);
        }
        sm.h2[t] = fmaxf(z, 0.0f);
    }
    __syncthreads();
    if (t < 64) {
        const float4* row = reinterpret_cast<const float4*>(P + IQ_FW3 + 64 * t);
        float z = P[IQ_FB3 + t];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4 w = row[k];
            z = __builtin_fmaf(w.x, sm.h2[4 * k], z); z = __builtin_fmaf(w.y, sm.h2[4 * k + 1], z);
            z = __builtin_fmaf(w.z, sm.h2[4 * k + 2], z); z = __builtin_fmaf(w.w, sm.h2[4 * k + 3], z);
        }
        sm.emb[t] = fmaxf(z, 0.0f);
    }
    __syncthreads();
}

// CosineEmbeddingNetwork of this lane's tau: sm.teT[e][lane] valid for every thread on return.  Wave c forms cosines 16 c .. 16 c + 15 of its rows, then
// embedding columns 16 c .. 16 c + 15 (C.W's rows are wave-uniform).
__device__ __forceinline__ void iq_tau_embed(const float* __restrict__ P, const float tau, iq_smem& sm, int lane, int c) {
    __syncthreads();   // earlier readers of prT / teT are done
#pragma unroll
    for (int q = 0; q < 16; ++q) sm.prT[16 * c + q][lane] = cosf(tau * iq_ipi(16 * c + q));
    __syncthreads();
    float cs[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) cs[k] = sm.prT[k][lane];
    for (int q = 0; q < 16; ++q) {
        const int e = 16 * c + q;
        const float* __restrict__ row = P + IQ_CW + 64 * e;
        float z = P[IQ_CB + e];
#pragma unroll
        for (int k = 0; k < 64; ++k) z = __builtin_fmaf(row[k], cs[k], z);
        sm.teT[e][lane] = fmaxf(z, 0.0f);
    }
    __syncthreads();
}

__device__ __forceinline__ void iq_load_prod(const iq_smem& sm, int lane, float (&prod)[64]) {
#pragma unroll
    for (int e = 0; e < 64; ++e) prod[e] = sm.emb[e] * sm.teT[e][lane];
}

// QuantileNetwork of the row held in prod: sm.out[lane][0 .. 1] valid for every thread on return
__device__ __forceinline__ void iq_head(const float* __restrict__ P, const float (&prod)[64], iq_smem& sm, int t, int lane, int c) {
    float o0 = c == 0 ? P[IQ_QB2] : 0.0f, o1 = c == 0 ? P[IQ_QB2 + 1] : 0.0f;
    for (int nb = 0; nb < IQ_H / IQ_BLK; ++nb) {
        for (int j = 0; j < 8; ++j) {
            const int u = IQ_BLK * nb + 8 * c + j;
            const float* __restrict__ w = P + IQ_QW1 + 64 * u;
            float z = P[IQ_QB1 + u];
#pragma unroll
            for (int e = 0; e < 64; ++e) z = __builtin_fmaf(w[e], prod[e], z);
            const float h = fmaxf(z, 0.0f);
            o0 = __builtin_fmaf(P[IQ_QW2 + u], h, o0);
            o1 = __builtin_fmaf(P[IQ_QW2 + IQ_H + u], h, o1);
        }
    }
    sm.part[c][0][lane] = o0; sm.part[c][1][lane] = o1;
    __syncthreads();
    if (t < 128) {
        const int a = t >> 6, i = t & 63;
        sm.out[i][a] = ((sm.part[0][a][i] + sm.part[1][a][i]) + sm.part[2][a][i]) + sm.part[3][a][i];
    }
    __syncthreads();
}

// action values over the first K rows of sm.out -> sm.q
__device__ __forceinline__ void iq_mean(iq_smem& sm, int K, int t) {
    if (t < 2) {
        float s = 0.0f;
        for (int i = 0; i < K; ++i) s = s + sm.out[i][t];
        sm.q[t] = s / (float)K;
    }
    __syncthreads();
}

__device__ __forceinline__ float iq_tau_draw(uint64_t seed, uint64_t key, uint64_t block, int word, uint32_t stream) {
    uint32_t r[4];
    mi_philox(seed, key, block, stream, r);
    const uint32_t w = word == 0 ? r[0] : (word == 1 ? r[1] : (word == 2 ? r[2] : r[3]));
    return mi_u32_to_uniform(w);
}

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) iqn_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, const float* __restrict__ taus, int n, int K,
                                                          float* __restrict__ quantiles, float* __restrict__ q) {
    __shared__ iq_smem sm;
    const int t = threadIdx.x, lane = t & 63, c = __builtin_amdgcn_readfirstlane(t >> 6);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        const float tau = taus[(size_t)row * K + (lane < K ? lane : K - 1)];
        iq_features(params, x, sm, t);
        iq_tau_embed(params, tau, sm, lane, c);
        float prod[64];
        iq_load_prod(sm, lane, prod);
        iq_head(params, prod, sm, t, lane, c);
        if (quantiles && t < 128 && (t >> 1) < K) quantiles[((size_t)row * K + (t >> 1)) * 2 + (t & 1)] = sm.out[t >> 1][t & 1];
        if (q) {
            iq_mean(sm, K, t);
            if (t < 2) q[2 * (size_t)row + t] = sm.q[t];
        }
        __syncthreads();
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the step's 32 taus (drawn or forced, reported through taus_out), then the mean of their quantiles
template <bool FORCED>
struct iq_policy {
    const float* __restrict__ params;
    const float* forced_taus;
    float* taus_out;
    uint64_t seed;
    int N;
    iq_smem& sm;
    int t, lane, c;
    __device__ __forceinline__ int greedy(const float4& x, int s, int n, uint64_t env_id, uint64_t ctr) {
        const int j = lane & 31;
        const float tau = (FORCED && forced_taus) ? forced_taus[((size_t)s * N + n) * MI_IQN_N_QUANT + j]
                                                  : iq_tau_draw(seed, env_id, ctr * 8 + (uint64_t)(j >> 2), j & 3, IQ_STREAM_ACT_TAU);
        if (taus_out && t < MI_IQN_N_QUANT) taus_out[((size_t)s * N + n) * MI_IQN_N_QUANT + t] = tau;
        iq_features(params, x, sm, t);
        iq_tau_embed(params, tau, sm, lane, c);
        float prod[64];
        iq_load_prod(sm, lane, prod);
        iq_head(params, prod, sm, t, lane, c);
        iq_mean(sm, MI_IQN_N_QUANT, t);
        const int a = sm.q[1] > sm.q[0] ? 1 : 0;   // torch.argmax: the first index on a tie
        __syncthreads();
        return a;
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) iqn_act_kernel(mi_env e, mi_iqn_ring_t ring, mi_iqn_act_t a_, rg_eps_tab eps) {
    __shared__ iq_smem sm;
    const int t = threadIdx.x, lane = t & 63, c = __builtin_amdgcn_readfirstlane(t >> 6);
    iq_policy<FORCED> policy{a_.params, a_.forced_taus, a_.taus_out, e.seed, e.n, sm, t, lane, c};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// next_actions[b] and target[b][:] of ring row i from the target networks TP; sm.tgt valid for every thread on return
__device__ __forceinline__ void iq_target_row(const float* __restrict__ TP, const mi_iqn_ring_t& ring, const mi_iqn_batch_t& bt, int b, long long i, iq_smem& sm, int t,
                                              int lane, int c) {
    const long long N = ring.n_envs, total = ring.slots * N;
    const long long nx = i + N >= total ? i + N - total : i + N;   // ((slot + 1) % slots) * N + env
    const float4 x = reinterpret_cast<const float4*>(ring.observations)[nx];
    const float r = ring.rewards[nx];
    const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
    iq_features(TP, x, sm, t);
    float prod[64];
    {
        const int j = lane & 31;
        const float tau = bt.forced_next_taus ? bt.forced_next_taus[(size_t)b * MI_IQN_N_QUANT + j]
                                              : iq_tau_draw(bt.seed, bt.update, (uint64_t)b * 16 + (uint64_t)(j >> 2), j & 3, IQ_STREAM_NEXT_TAU);
        iq_tau_embed(TP, tau, sm, lane, c);
        iq_load_prod(sm, lane, prod);
        iq_head(TP, prod, sm, t, lane, c);
        iq_mean(sm, MI_IQN_N_QUANT, t);
    }
    const int a = __builtin_amdgcn_readfirstlane(sm.q[1] > sm.q[0] ? 1 : 0);
    {
        const float tau = bt.forced_tau_dashes ? bt.forced_tau_dashes[(size_t)b * MI_IQN_N_TAU_PRIME + lane]
                                               : iq_tau_draw(bt.seed, bt.update, (uint64_t)b * 16 + (uint64_t)(lane >> 2), lane & 3, IQ_STREAM_TAU_DASH);
        iq_tau_embed(TP, tau, sm, lane, c);
        iq_load_prod(sm, lane, prod);
        iq_head(TP, prod, sm, t, lane, c);
    }
    if (t < 64) {
        const float tg = r + lg * sm.out[t][a];
        sm.tgt[t] = tg;
        bt.target[(size_t)b * MI_IQN_N_TAU_PRIME + t] = tg;
    }
    if (t == 0) bt.next_actions[b] = a;
    __syncthreads();
}

__global__ void __launch_bounds__(256) iqn_target_kernel(mi_iqn_ring_t ring, mi_iqn_batch_t bt) {
    __shared__ iq_smem sm;
    const int t = threadIdx.x, lane = t & 63, c = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long total = ring.slots * (long long)ring.n_envs;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);
        iq_target_row(bt.target_params, ring, bt, b, i, sm, t, lane, c);
    }
}

// the 64 x 64 quantile-Huber loss of one row from sm.cur / sm.tgt / sm.tau: sm.dout, sm.li, sm.rowloss valid for every thread on return
__device__ __forceinline__ void iq_loss_row(iq_smem& sm, const float inv, int t, int lane, int c) {
    {
        const float cur = sm.cur[lane], tau = sm.tau[lane];
        float T = 0.0f, S = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float d = sm.tgt[16 * c + q] - cur;
            const float ad = fabsf(d);
            const bool quad = ad <= 1.0f;
            const float huber = quad ? d * d : ad - 0.5f;
            const float g = quad ? 2.0f * d : (d > 0.0f ? 1.0f : -1.0f);
            const float w = fabsf(tau - (d < 0.0f ? 1.0f : 0.0f));
            T = T + w * huber;
            S = S + w * g;
        }
        sm.part[c][0][lane] = T; sm.part[c][1][lane] = S;
    }
    __syncthreads();
    if (t < 64) {
        const float L = ((sm.part[0][0][t] + sm.part[1][0][t]) + sm.part[2][0][t]) + sm.part[3][0][t];
        const float G = ((sm.part[0][1][t] + sm.part[1][1][t]) + sm.part[2][1][t]) + sm.part[3][1][t];
        sm.li[t] = L;
        sm.dout[t] = -(G * inv);
    }
    __syncthreads();
    if (t == 0) {
        float s = 0.0f;
        for (int i = 0; i < 64; ++i) s = s + sm.li[i];
        sm.rowloss = s;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) iqn_huber_kernel(const float* __restrict__ current, const float* __restrict__ target, const float* __restrict__ taus, int batch,
                                                        float* __restrict__ loss, float* __restrict__ dcurrent) {
    __shared__ iq_smem sm;
    const int t = threadIdx.x, lane = t & 63, c = __builtin_amdgcn_readfirstlane(t >> 6);
    const float inv = 1.0f / (float)(batch * 64);
    float total = 0.0f;
    for (int b = 0; b < batch; ++b) {
        if (t < 64) { sm.cur[t] = current[(size_t)b * 64 + t]; sm.tgt[t] = target[(size_t)b * 64 + t]; sm.tau[t] = taus[(size_t)b * 64 + t]; }
        __syncthreads();
        iq_loss_row(sm, inv, t, lane, c);
        if (t < 64) dcurrent[(size_t)b * 64 + t] = sm.dout[t];
        if (t == 0) total = total + sm.rowloss;
        __syncthreads();
    }
    if (t == 0) loss[0] = total * inv;
}

__global__ void __launch_bounds__(256) iqn_grad_kernel(mi_iqn_ring_t ring, mi_iqn_batch_t bt, float* __restrict__ slabs) {
    __shared__ iq_smem sm;
    const int t = threadIdx.x, lane = t & 63, c = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long total = ring.slots * (long long)ring.n_envs;
    const float* __restrict__ P = bt.params;
    const float inv = 1.0f / (float)(bt.batch * 64);
    float* const slab = slabs + (size_t)blockIdx.x * IQ_STRIDE;
    for (int k = t; k < IQ_STRIDE / 4; k += 256) reinterpret_cast<float4*>(slab)[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // 44,900 = 4 * 11,225
    __threadfence_block();   // other threads of the workgroup add to what this one has zeroed
    __syncthreads();
    float (*X)[64] = reinterpret_cast<float (*)[64]>(&sm.blk[0][0][0]);   // dprod[e][i] once the block loop is over
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.seed, bt.update, bt.sample_upper, bt.idx, b, total, t == 0);
        // ---- targets, with the target networks ----
        iq_target_row(bt.target_params, ring, bt, b, i, sm, t, lane, c);
        // ---- online forward ----
        const float4 x = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = __builtin_amdgcn_readfirstlane(ring.actions[i] != 0 ? 1 : 0);
        const float tau = bt.forced_taus ? bt.forced_taus[(size_t)b * MI_IQN_N_TAU + lane]
                                         : iq_tau_draw(bt.seed, bt.update, (uint64_t)b * 16 + (uint64_t)(lane >> 2), lane & 3, IQ_STREAM_TAU);
        if (c == 0) { sm.tau[lane] = tau; bt.taus[(size_t)b * MI_IQN_N_TAU + lane] = tau; }
        iq_features(P, x, sm, t);
        iq_tau_embed(P, tau, sm, lane, c);
        float prod[64];
        iq_load_prod(sm, lane, prod);
        iq_head(P, prod, sm, t, lane, c);
        if (t < 64) {
            const float v = sm.out[t][a];
            sm.cur[t] = v;
            bt.current[(size_t)b * MI_IQN_N_TAU + t] = v;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) sm.prT[16 * c + q][lane] = prod[16 * c + q];   // prod[e][i] for the block loop (the cosines in prT are spent)
        __syncthreads();
        // ---- loss ----
        iq_loss_row(sm, inv, t, lane, c);
        // ---- backward through the head, hidden units in blocks of 32 ----
        const float dout = sm.dout[lane];
        float dprod[64];
#pragma unroll
        for (int e = 0; e < 64; ++e) dprod[e] = 0.0f;
        for (int nb = 0; nb < IQ_H / IQ_BLK; ++nb) {
            for (int j = 0; j < 8; ++j) {
                const int ul = 8 * c + j, u = IQ_BLK * nb + ul;
                const float* __restrict__ w = P + IQ_QW1 + 64 * u;
                float z = P[IQ_QB1 + u];
#pragma unroll
                for (int e = 0; e < 64; ++e) z = __builtin_fmaf(w[e], prod[e], z);
                const float dz = z > 0.0f ? dout * P[IQ_QW2 + IQ_H * a + u] : 0.0f;
#pragma unroll
                for (int e = 0; e < 64; ++e) dprod[e] = __builtin_fmaf(dz, w[e], dprod[e]);
                sm.blk[0][ul][lane] = dz;
                sm.blk[1][ul][lane] = fmaxf(z, 0.0f);
            }
            __syncthreads();
            {   // thread (unit ul, half hf, wave c) owns dQ.W1[u][16 c + 8 hf .. + 7]: chains over the 64 tau rows
                const int ul = lane & 31, hf = lane >> 5, u = IQ_BLK * nb + ul, e0 = 16 * c + 8 * hf;
                float acc[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] = 0.0f;
                for (int r = 0; r < 64; r += 4) {
                    const float d0 = sm.blk[0][ul][r], d1 = sm.blk[0][ul][r + 1], d2 = sm.blk[0][ul][r + 2], d3 = sm.blk[0][ul][r + 3];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const float4 p = *reinterpret_cast<const float4*>(&sm.prT[e0 + q][r]);
                        acc[q] = __builtin_fmaf(d0, p.x, acc[q]); acc[q] = __builtin_fmaf(d1, p.y, acc[q]);
                        acc[q] = __builtin_fmaf(d2, p.z, acc[q]); acc[q] = __builtin_fmaf(d3, p.w, acc[q]);
                    }
                }
                float4* const dst = reinterpret_cast<float4*>(slab + IQ_QW1 + 64 * u + e0);
                float4 v0 = dst[0], v1 = dst[1];
                v0.x = v0.x + acc[0]; v0.y = v0.y + acc[1]; v0.z = v0.z + acc[2]; v0.w = v0.w + acc[3];
                v1.x = v1.x + acc[4]; v1.y = v1.y + acc[5]; v1.z = v1.z + acc[6]; v1.w = v1.w + acc[7];
                dst[0] = v0; dst[1] = v1;
                if (hf == 0 && c == 0) {
                    float s = 0.0f;
                    for (int r = 0; r < 64; ++r) s = s + sm.blk[0][ul][r];
                    slab[IQ_QB1 + u] = slab[IQ_QB1 + u] + s;
                }
                if (hf == 0 && c == 1) {
                    float s = 0.0f;
                    for (int r = 0; r < 64; ++r) s = __builtin_fmaf(sm.dout[r], sm.blk[1][ul][r], s);
                    slab[IQ_QW2 + IQ_H * a + u] = slab[IQ_QW2 + IQ_H * a + u] + s;
                }
            }
            __syncthreads();
        }
        // ---- dprod = ((R_0 + R_1) + R_2) + R_3 ----
        for (int w = 0; w < 4; ++w) {
            if (c == w) {
#pragma unroll
                for (int e = 0; e < 64; ++e) X[e][lane] = w == 0 ? dprod[e] : X[e][lane] + dprod[e];
            }
            __syncthreads();
        }
        // ---- into the features (demb) and the cosine net (dte) ----
        if (t < 64) {
            float acc = 0.0f;
            for (int r = 0; r < 64; ++r) acc = __builtin_fmaf(X[t][r], sm.teT[t][r], acc);
            sm.dz3[t] = sm.emb[t] > 0.0f ? acc : 0.0f;
        }
        if (t == 64) {
            float s = 0.0f;
            for (int r = 0; r < 64; ++r) s = s + sm.dout[r];
            slab[IQ_QB2 + a] = slab[IQ_QB2 + a] + s;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = 16 * c + q;
            sm.prT[e][lane] = sm.teT[e][lane] > 0.0f ? X[e][lane] * sm.emb[e] : 0.0f;   // dte[e][i]
        }
        __syncthreads();
        for (int q = 0; q < 16; ++q) sm.teT[16 * c + q][lane] = cosf(sm.tau[16 * c + q] * iq_ipi(lane));   // c[i][k], k = lane: the forward's values again
        __syncthreads();
        {   // thread (k = lane, wave c) owns dC.W[16 c .. 16 c + 15][k]; every lane forms dC.b redundantly, lane 0 adds it
            float acc[16], bacc[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) { acc[q] = 0.0f; bacc[q] = 0.0f; }
            for (int r = 0; r < 64; r += 4) {
                const float c0 = sm.teT[r][lane], c1 = sm.teT[r + 1][lane], c2 = sm.teT[r + 2][lane], c3 = sm.teT[r + 3][lane];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float4 d = *reinterpret_cast<const float4*>(&sm.prT[16 * c + q][r]);
                    acc[q] = __builtin_fmaf(d.x, c0, acc[q]); acc[q] = __builtin_fmaf(d.y, c1, acc[q]);
                    acc[q] = __builtin_fmaf(d.z, c2, acc[q]); acc[q] = __builtin_fmaf(d.w, c3, acc[q]);
                    bacc[q] = bacc[q] + d.x; bacc[q] = bacc[q] + d.y; bacc[q] = bacc[q] + d.z; bacc[q] = bacc[q] + d.w;
                }
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                float* const dst = slab + IQ_CW + 64 * (16 * c + q) + lane;
                *dst = *dst + acc[q];
                if (lane == 0) slab[IQ_CB + 16 * c + q] = slab[IQ_CB + 16 * c + q] + bacc[q];
            }
        }
        // ---- features extractor (one row: the weight gradients are outer products) ----
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int idx = 16 * t + m;
            slab[IQ_FW3 + idx] = slab[IQ_FW3 + idx] + sm.dz3[idx >> 6] * sm.h2[idx & 63];
        }
        if (t < 64) {
            slab[IQ_FB3 + t] = slab[IQ_FB3 + t] + sm.dz3[t];
            float acc = 0.0f;
            for (int e = 0; e < 64; ++e) acc = __builtin_fmaf(sm.dz3[e], P[IQ_FW3 + 64 * e + t], acc);
            sm.dz2[t] = sm.h2[t] > 0.0f ? acc : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int idx = 8 * t + m;
            slab[IQ_FW2 + idx] = slab[IQ_FW2 + idx] + sm.dz2[idx >> 5] * sm.h1[idx & 31];
        }
        if (t < 64) slab[IQ_FB2 + t] = slab[IQ_FB2 + t] + sm.dz2[t];
        if (t < 32) {
            float acc = 0.0f;
            for (int o = 0; o < 64; ++o) acc = __builtin_fmaf(sm.dz2[o], P[IQ_FW2 + 32 * o + t], acc);
            sm.dz1[t] = sm.h1[t] > 0.0f ? acc : 0.0f;
        }
        __syncthreads();
        if (t < 128) {
            const int k = t & 3;
            const float xk = k == 0 ? x.x : (k == 1 ? x.y : (k == 2 ? x.z : x.w));
            slab[IQ_FW1 + t] = slab[IQ_FW1 + t] + sm.dz1[t >> 2] * xk;
        }
        if (t < 32) slab[IQ_FB1 + t] = slab[IQ_FB1 + t] + sm.dz1[t];
        if (t == 0) slab[IQ_NP] = slab[IQ_NP] + sm.rowloss;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) iqn_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                         float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                         rg_adam_consts k, int adam) {
    rg_reduce<IQ_NP, IQ_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_iqn_forward(const float* params, const float* obs, const float* taus, int n, int k, float* quantiles, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && taus && n > 0 && (quantiles || q), "bad arguments");
    RG_CHECK_ARG(k >= 1 && k <= MI_IQN_N_TAU, "k must be in [1, 64]");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    iqn_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, taus, n, k, quantiles, q);
    RG_HIP(hipGetLastError());
    return MI_IQN_OK;
}

extern "C" int mi_iqn_act_steps(void* handle, const mi_iqn_ring_t* ring, const mi_iqn_act_t* a, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    RG_CHECK_ARG(e != nullptr && a != nullptr, "NULL pointer");
    RG_CHECK_ARG(a->global_step >= 0 && a->learning_starts >= 0, "global_step < 0 or learning_starts < 0");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, a->slope, 1.0, a->final_epsilon);   // epsilon = max(1 + slope * step, final_epsilon)
    int grid;
    const int rc = rg_act_prelude(e, ring, a->params, a->obs_cur, a->n_steps, a->max_ep, a->episodes, a->episode_stats, s, grid);
    if (rc != MI_IQN_OK) return rc;
    if (a->forced_actions || a->forced_resets || a->forced_taus)
        iqn_act_kernel<true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    else
        iqn_act_kernel<false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    RG_HIP(hipGetLastError());
    return MI_IQN_OK;
}

extern "C" int mi_iqn_target(const mi_iqn_ring_t* ring, const mi_iqn_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_IQN_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->batch > 0, "batch <= 0");
    RG_CHECK_ARG(b->target_params && b->idx && b->next_actions && b->target, "a batch buffer is NULL");
    RG_CHECK_ARG(rg_aligned(b->target_params), "target_params must be 16-byte aligned");
    iqn_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_IQN_OK;
}

extern "C" int mi_iqn_quantile_huber(const float* current, const float* target, const float* taus, int batch, float* loss, float* dcurrent, void* stream) {
    RG_CHECK_ARG(current && target && taus && loss && dcurrent, "NULL pointer");
    RG_CHECK_ARG(batch > 0 && batch <= (1 << 24), "batch must be in [1, 2^24]");
    iqn_huber_kernel<<<1, 256, 0, (hipStream_t)stream>>>(current, target, taus, batch, loss, dcurrent);
    RG_HIP(hipGetLastError());
    return MI_IQN_OK;
}

// mi_iqn_grad (update false: opt is not looked at) and mi_iqn_update
static int iq_grad(const mi_iqn_ring_t* ring, const mi_iqn_batch_t* b, const mi_iqn_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, 1 << 24, "batch must be in [1, 2^24]", [](const mi_iqn_batch_t& bt) { return bt.taus && bt.current && bt.target; });
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<IQ_NP>(iqn_grad_kernel, iqn_reduce_kernel, ring, b, iq_slabs(b->batch), 1.0f / (float)(b->batch * 64), update ? opt : nullptr, s);
}
extern "C" int mi_iqn_grad(const mi_iqn_ring_t* ring, const mi_iqn_batch_t* b, void* stream) { return iq_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_iqn_update(const mi_iqn_ring_t* ring, const mi_iqn_batch_t* b, const mi_iqn_adam_t* opt, void* stream) {
    return iq_grad(ring, b, opt, true, (hipStream_t)stream);
}
