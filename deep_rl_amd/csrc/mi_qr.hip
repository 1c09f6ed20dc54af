// mi_qr.hip — libmirl_qr.so: QR-DQN on CartPole-v1 for gfx950.  C ABI, numerics and RNG contract: include/mi_qr.h.
//
// The form of mi_c51.hip: one 256-thread workgroup evaluates one network row at a time with the network in its registers (thread c * 84 + o a 40-wide third of row o
// of W2, thread u < 120 row u of W1, and — in the kernels that need quantiles — thread r < 128 row r of W3), loaded once per launch.  Every launch first forms the
// collapsed head (wbar, bbar: the mean over the 64 quantile rows of each action) in LDS; action values are two 84-long chains on it.
//   qr_act_kernel       a workgroup walks its envs, each through all steps of the chunk.  It never loads W3: every thread keeps wbar / bbar in registers and forms both
//                       action values itself, so a greedy step costs the torso's three barriers and none for the head.
//   qr_grad_kernel      a workgroup walks its batch rows twice: with the TARGET network it writes next_actions / target (the greedy action's 64 rows by one wave), then
//                       with the ONLINE network forward (the stored action's 64 rows), the 64 x 64 quantile-Huber loss on all four waves, and the backward into register
//                       accumulators — one slab per workgroup.
//   qr_reduce_kernel    fixed-order slab sum (+ Adam).
//   qr_huber_kernel     the loss stage alone.
// The torso (layout, loader, ts_row, ts_backward, ts_store) is mi_torso.h's, shared with mi_c51.hip and mi_ddqn.hip; the host side of acting and of the gradient entry
// points is mi_ring.h's.  All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"

#include "../../include/mi_qr.h"

#define QR_H1 MI_QR_H1
#define QR_H2 MI_QR_H2
#define QR_NQ MI_QR_N_QUANT
#define QR_NL (2 * MI_QR_N_QUANT)
#define QR_W3 MI_QR_W3
#define QR_B3 MI_QR_B3
#define QR_NP MI_QR_NPARAMS
#define QR_STRIDE MI_QR_SLAB_STRIDE
#define QR_DH2C 22             // quantiles per partial chain of dh2 (three threads per column: 22, 22, 20)
static_assert(MI_QR_OK == RG_OK && MI_QR_EINVAL == RG_EINVAL && MI_QR_EHIP == RG_EHIP && MI_QR_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_QR_W1 == TS_W1 && MI_QR_B1 == TS_B1 && MI_QR_W2 == TS_W2 && MI_QR_B2 == TS_B2 && MI_QR_H1 == TS_H1 && MI_QR_H2 == TS_H2, "mi_torso.h holds this torso");

#ifndef MI_QR_SOURCE_ID
#define MI_QR_SOURCE_ID "unknown"
#endif
extern "C" int mi_qr_version(void) { return MI_QR_VERSION; }
extern "C" const char* mi_qr_last_error(void) { return rg_err; }
extern "C" const char* mi_qr_source_id(void) { return MI_QR_SOURCE_ID; }
static int qr_slabs(int batch) { return rg_slabs(batch, MI_QR_MAX_SLABS); }
extern "C" size_t mi_qr_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)qr_slabs(batch) * QR_STRIDE * sizeof(float);
}

// ---- the network as one workgroup holds it ------------------------------------------------------------
struct qr_head { float w3[QR_H2]; float b3; };   // thread r < 128: row r of W3
struct qr_smem {
    float h1[QR_H1];
    float p2[3][QR_H2];                 // layer 2's partial chains; the backward's partial chains of dh2
    float h2[QR_H2];
    float wbar[2][QR_H2];               // the collapsed head of the network the workgroup currently holds
    float bbar[2];
    float cur[QR_NQ], tgt[QR_NQ];
    float part[4][2][QR_NQ];            // the loss's partial sums T_c, S_c
    float li[QR_NQ], dout[QR_NQ];
    float rowloss;
    float dz2[QR_H2];
    float ph[2][QR_H1];                 // the backward's partial chains of dh1
};

__device__ __forceinline__ void qr_load_head(qr_head& w, const float* __restrict__ P, int t) {
    const int r = t < QR_NL ? t : QR_NL - 1;
    const float4* src = reinterpret_cast<const float4*>(P + QR_W3 + (size_t)r * QR_H2);   // 10,764 and 84 are multiples of 4
#pragma unroll
    for (int k = 0; k < QR_H2 / 4; ++k) { const float4 v = src[k]; w.w3[4 * k] = v.x; w.w3[4 * k + 1] = v.y; w.w3[4 * k + 2] = v.z; w.w3[4 * k + 3] = v.w; }
    w.b3 = P[QR_B3 + r];
}

// the collapsed head of the parameters P into sm.wbar / sm.bbar (mi_qr.h: the serial sums over ascending i, scaled by 1 / 64); ends in a barrier
__device__ __forceinline__ void qr_collapse(const float* __restrict__ P, qr_smem& sm, int t) {
    if (t < 2 * QR_H2) {   // thread a * 84 + k: column k of action a's 64 rows (consecutive threads, consecutive addresses)
        const int a = t / QR_H2, k = t - a * QR_H2;
        const float* const col = P + QR_W3 + (size_t)(a * QR_NQ) * QR_H2 + k;
        float s = 0.0f;
#pragma unroll 16
        for (int i = 0; i < QR_NQ; ++i) s = s + col[(size_t)i * QR_H2];
        sm.wbar[a][k] = s * (1.0f / 64.0f);
    } else if (t < 2 * QR_H2 + 2) {
        const int a = t - 2 * QR_H2;
        float s = 0.0f;
#pragma unroll 16
        for (int i = 0; i < QR_NQ; ++i) s = s + P[QR_B3 + a * QR_NQ + i];
        sm.bbar[a] = s * (1.0f / 64.0f);
    }
    __syncthreads();
}

// both action values from sm.h2 and the collapsed head in LDS, in every thread (two independent chains; the reads are workgroup-uniform broadcasts)
__device__ __forceinline__ void qr_values(const qr_smem& sm, float& q0, float& q1) {
    q0 = sm.bbar[0]; q1 = sm.bbar[1];
#pragma unroll
    for (int k = 0; k < QR_H2; ++k) {
        const float h = sm.h2[k];
        q0 = __builtin_fmaf(sm.wbar[0][k], h, q0);
        q1 = __builtin_fmaf(sm.wbar[1][k], h, q1);
    }
}
// theta_{r / 64, r % 64} of the row in sm.h2 by thread r < 128
__device__ __forceinline__ float qr_quantile(const qr_head& w, const qr_smem& sm) {
    float acc = w.b3;
#pragma unroll
    for (int k = 0; k < QR_H2; ++k) acc = __builtin_fmaf(w.w3[k], sm.h2[k], acc);
    return acc;
}

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) qr_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, float* __restrict__ quantiles,
                                                         float* __restrict__ q) {
    __shared__ qr_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    qr_head hd;
    ts_load(w, params, t);
    qr_load_head(hd, params, t);
    qr_collapse(params, sm, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        ts_row(w, x, sm, t);
        if (quantiles && t < QR_NL) quantiles[(size_t)row * QR_NL + t] = qr_quantile(hd, sm);
        if (q) {
            float q0, q1;
            qr_values(sm, q0, q1);
            if (t == 0) { q[2 * (size_t)row] = q0; q[2 * (size_t)row + 1] = q1; }
        }
        __syncthreads();
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the torso in `w`, the collapsed head in every thread's registers
struct qr_policy {
    const ts_torso& w;
    const float (&wb0)[QR_H2], (&wb1)[QR_H2];
    float bb0, bb1;
    qr_smem& sm;
    int t;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t, uint64_t) {
        ts_row(w, x, sm, t);
        float q0 = bb0, q1 = bb1;
#pragma unroll
        for (int k = 0; k < QR_H2; ++k) {
            const float h = sm.h2[k];
            q0 = __builtin_fmaf(wb0[k], h, q0);
            q1 = __builtin_fmaf(wb1[k], h, q1);
        }
        // no barrier here: sm.h2 is next written behind two barriers of the next ts_row, which no wave passes before all have read it
        return q1 > q0 ? 1 : 0;   // torch.argmax: the first index on a tie
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) qr_act_kernel(mi_env e, mi_qr_ring_t ring, mi_qr_act_t a_, rg_eps_tab eps) {
    __shared__ qr_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, a_.params, t);
    qr_collapse(a_.params, sm, t);
    float wb0[QR_H2], wb1[QR_H2];   // the collapsed head in every thread's registers
#pragma unroll
    for (int k = 0; k < QR_H2; ++k) { wb0[k] = sm.wbar[0][k]; wb1[k] = sm.wbar[1][k]; }
    qr_policy policy{w, wb0, wb1, sm.bbar[0], sm.bbar[1], sm, t};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, 0, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// next_actions[b] and target[b][:] of ring row `i` (flat index) from the target network held in `w`, `hd` and sm.wbar / sm.bbar
__device__ __forceinline__ void qr_target_row(const ts_torso& w, const qr_head& hd, const mi_qr_ring_t& ring, long long i, float gamma, qr_smem& sm, int t,
                                              int32_t* __restrict__ next_action, float* __restrict__ tgt_out) {
    const long long N = ring.n_envs, total = ring.slots * N;
    const long long nx = i + N >= total ? i + N - total : i + N;   // ((slot + 1) % slots) * N + env
    const float4 x = reinterpret_cast<const float4*>(ring.observations)[nx];
    const float r = ring.rewards[nx];
    const float lg = ring.terminated[nx] ? 0.0f : gamma;
    ts_row(w, x, sm, t);
    float q0, q1;
    qr_values(sm, q0, q1);
    const int a = q1 > q0 ? 1 : 0;
    if ((t >> 6) == a) tgt_out[t & 63] = r + lg * qr_quantile(hd, sm);   // one wave: the greedy action's 64 rows (-ffp-contract=off: a product, then a sum)
    if (t == 0) *next_action = a;
    __syncthreads();
}

__global__ void __launch_bounds__(256) qr_target_kernel(mi_qr_ring_t ring, mi_qr_batch_t bt) {
    __shared__ qr_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso w;
    qr_head hd;
    ts_load(w, bt.target_params, t);
    qr_load_head(hd, bt.target_params, t);
    qr_collapse(bt.target_params, sm, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        qr_target_row(w, hd, ring, i, bt.gamma, sm, t, bt.next_actions + b, bt.target + (size_t)b * QR_NQ);
    }
}

// the 64 x 64 quantile-Huber loss of one row from sm.cur / sm.tgt: sm.dout, sm.li, sm.rowloss valid for every thread on return.  Wave c takes targets 16 c .. 16 c + 15,
// lane i the quantile i.
__device__ __forceinline__ void qr_loss_row(qr_smem& sm, const float inv, int t, int lane, int c) {
    {
        const float cur = sm.cur[lane], tau = (float)(2 * lane + 1) * (1.0f / 128.0f);
        float T = 0.0f, S = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float u = sm.tgt[16 * c + q] - cur;
            const float au = fabsf(u);
            const float L = au <= 1.0f ? (0.5f * u) * u : au - 0.5f;
            const float g = fminf(fmaxf(u, -1.0f), 1.0f);
            const float wt = fabsf(tau - (u < 0.0f ? 1.0f : 0.0f));
            T = T + wt * L;
            S = S + wt * g;
        }
        sm.part[c][0][lane] = T; sm.part[c][1][lane] = S;
    }
    __syncthreads();
    if (t < QR_NQ) {
        const float L = ((sm.part[0][0][t] + sm.part[1][0][t]) + sm.part[2][0][t]) + sm.part[3][0][t];
        const float G = ((sm.part[0][1][t] + sm.part[1][1][t]) + sm.part[2][1][t]) + sm.part[3][1][t];
        sm.li[t] = L;
        sm.dout[t] = -(G * inv);
    }
    __syncthreads();
    if (t == 0) {
        float s = 0.0f;
        for (int i = 0; i < QR_NQ; ++i) s = s + sm.li[i];
        sm.rowloss = s;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) qr_huber_kernel(const float* __restrict__ current, const float* __restrict__ target, int batch, float* __restrict__ loss,
                                                       float* __restrict__ dcurrent) {
    __shared__ qr_smem sm;
    const int t = threadIdx.x, lane = t & 63, c = __builtin_amdgcn_readfirstlane(t >> 6);
    const float inv = 1.0f / (float)(batch * QR_NQ);
    float total = 0.0f;
    for (int b = 0; b < batch; ++b) {
        if (t < QR_NQ) { sm.cur[t] = current[(size_t)b * QR_NQ + t]; sm.tgt[t] = target[(size_t)b * QR_NQ + t]; }
        __syncthreads();
        qr_loss_row(sm, inv, t, lane, c);
        if (t < QR_NQ) dcurrent[(size_t)b * QR_NQ + t] = sm.dout[t];
        if (t == 0) total = total + sm.rowloss;
        __syncthreads();
    }
    if (t == 0) loss[0] = total * inv;
}

__global__ void __launch_bounds__(256) qr_grad_kernel(mi_qr_ring_t ring, mi_qr_batch_t bt, float* __restrict__ slabs) {
    __shared__ qr_smem sm;
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso w;
    qr_head hd;
    // ---- pass 1, target network: indices, next_actions, target of this workgroup's rows ----
    ts_load(w, bt.target_params, t);
    qr_load_head(hd, bt.target_params, t);
    qr_collapse(bt.target_params, sm, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        qr_target_row(w, hd, ring, i, bt.gamma, sm, t, bt.next_actions + b, bt.target + (size_t)b * QR_NQ);
    }
    __threadfence_block();   // pass 2 reads the targets this workgroup wrote (qr_target_row ends in a barrier)
    __syncthreads();
    // ---- pass 2, online network: forward, loss, backward into register accumulators (the stored action is given: no action values, no collapsed head) ----
    ts_load(w, bt.params, t);
    qr_load_head(hd, bt.params, t);
    float g3[QR_H2], gb3 = 0.0f, loss = 0.0f;
    ts_grads g;
#pragma unroll
    for (int k = 0; k < QR_H2; ++k) g3[k] = 0.0f;
    ts_zero(g);
    const float inv = 1.0f / (float)(bt.batch * QR_NQ);
    const float* __restrict__ P = bt.params;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, false);   // recomputed, not re-read
        const float4 x = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        ts_row(w, x, sm, t);
        if (wv == a) {   // one wave: the stored action's 64 rows
            const float th = qr_quantile(hd, sm);
            sm.cur[lane] = th;
            sm.tgt[lane] = bt.target[(size_t)b * QR_NQ + lane];
            if (bt.current) bt.current[(size_t)b * QR_NQ + lane] = th;
        }
        __syncthreads();
        qr_loss_row(sm, inv, t, lane, wv);
        if (t == 0) loss += sm.rowloss;
        // layer 3: thread r owns row r of dW3
        if (wv == a) {
            const float d = sm.dout[lane];
            gb3 += d;
#pragma unroll
            for (int k = 0; k < QR_H2; ++k) g3[k] = __builtin_fmaf(d, sm.h2[k], g3[k]);
        }
        // dh2: thread c * 84 + k sums its third of the quantiles; W3's column k comes from memory (consecutive threads, consecutive addresses)
        if (t < 3 * QR_H2) {
            const int c = t / QR_H2, k = t - c * QR_H2;
            const int i0 = QR_DH2C * c, i1 = i0 + QR_DH2C < QR_NQ ? i0 + QR_DH2C : QR_NQ;
            const float* const col = P + QR_W3 + (size_t)(a * QR_NQ) * QR_H2 + k;
            float acc = 0.0f;
            for (int q = i0; q < i1; ++q) acc = __builtin_fmaf(sm.dout[q], col[(size_t)q * QR_H2], acc);
            sm.p2[c][k] = acc;
        }
        __syncthreads();
        if (t < QR_H2) sm.dz2[t] = sm.h2[t] > 0.0f ? (sm.p2[0][t] + sm.p2[1][t]) + sm.p2[2][t] : 0.0f;
        __syncthreads();
        ts_backward(g, sm.h1, sm.dz2, sm.ph, x, P, t);
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * QR_STRIDE;
    if (t < QR_NL) {
        float4* const dst = reinterpret_cast<float4*>(slab + QR_W3 + (size_t)t * QR_H2);
#pragma unroll
        for (int k = 0; k < QR_H2 / 4; ++k) dst[k] = make_float4(g3[4 * k], g3[4 * k + 1], g3[4 * k + 2], g3[4 * k + 3]);
        slab[QR_B3 + t] = gb3;
    }
    ts_store(g, slab, t);
    if (t == 0) { slab[QR_NP] = loss; slab[QR_NP + 1] = 0.0f; slab[QR_NP + 2] = 0.0f; slab[QR_NP + 3] = 0.0f; }
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) qr_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                        float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                        rg_adam_consts k, int adam) {
    rg_reduce<QR_NP, QR_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_qr_forward(const float* params, const float* obs, int n, float* quantiles, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && n > 0 && (quantiles || q), "bad arguments");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    qr_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, n, quantiles, q);
    RG_HIP(hipGetLastError());
    return MI_QR_OK;
}

extern "C" int mi_qr_act_steps(void* handle, const mi_qr_ring_t* ring, const mi_qr_act_t* a, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    RG_CHECK_ARG(e != nullptr && a != nullptr, "NULL pointer");
    RG_CHECK_ARG(a->global_step >= 0 && a->total_timesteps > 0 && a->exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, (a->end_e - a->start_e) / (a->exploration_fraction * (double)a->total_timesteps), a->start_e, a->end_e);
    int grid;
    const int rc = rg_act_prelude(e, ring, a->params, a->obs_cur, a->n_steps, a->max_ep, a->episodes, a->episode_stats, s, grid);
    if (rc != MI_QR_OK) return rc;
    if (a->forced_actions || a->forced_resets)
        qr_act_kernel<true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    else
        qr_act_kernel<false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    RG_HIP(hipGetLastError());
    return MI_QR_OK;
}

extern "C" int mi_qr_target(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_QR_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->target_params && b->idx && b->next_actions && b->target && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->target_params), "target_params must be 16-byte aligned");
    qr_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_QR_OK;
}

extern "C" int mi_qr_quantile_huber(const float* current, const float* target, int batch, float* loss, float* dcurrent, void* stream) {
    RG_CHECK_ARG(current && target && loss && dcurrent && batch > 0, "bad arguments");
    qr_huber_kernel<<<1, 256, 0, (hipStream_t)stream>>>(current, target, batch, loss, dcurrent);
    RG_HIP(hipGetLastError());
    return MI_QR_OK;
}

// mi_qr_grad (update false: opt is not looked at) and mi_qr_update
static int qr_grad(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, const mi_qr_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_qr_batch_t& bt) { return bt.target != nullptr; });
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<QR_NP>(qr_grad_kernel, qr_reduce_kernel, ring, b, qr_slabs(b->batch), 1.0f / (float)(b->batch * QR_NQ), update ? opt : nullptr, s);
}
extern "C" int mi_qr_grad(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, void* stream) { return qr_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_qr_update(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, const mi_qr_adam_t* opt, void* stream) {
    return qr_grad(ring, b, opt, true, (hipStream_t)stream);
}
