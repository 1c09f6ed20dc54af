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
// All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"

#include "../../include/mi_qr.h"

#define QR_H1 MI_QR_H1
#define QR_H2 MI_QR_H2
#define QR_NQ MI_QR_N_QUANT
#define QR_NL (2 * MI_QR_N_QUANT)
#define QR_W1 MI_QR_W1
#define QR_B1 MI_QR_B1
#define QR_W2 MI_QR_W2
#define QR_B2 MI_QR_B2
#define QR_W3 MI_QR_W3
#define QR_B3 MI_QR_B3
#define QR_NP MI_QR_NPARAMS
#define QR_STRIDE MI_QR_SLAB_STRIDE
#define QR_W2C 40              // columns of W2 per thread (three threads per row)
#define QR_DH2C 22             // quantiles per partial chain of dh2 (three threads per column: 22, 22, 20)
static_assert(MI_QR_OK == RG_OK && MI_QR_EINVAL == RG_EINVAL && MI_QR_EHIP == RG_EHIP && MI_QR_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");

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
struct qr_torso {
    float w2[QR_W2C]; float b2;         // thread c * 84 + o < 252: W2[o][40 c .. 40 c + 39]; b2 is the chain's start (the bias for c = 0, else 0)
    float w1[4]; float b1;              // thread u < 120
};
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

__device__ __forceinline__ void qr_load_torso(qr_torso& w, const float* __restrict__ P, int t) {
    {
        const int tt = t < 3 * QR_H2 ? t : 3 * QR_H2 - 1;
        const int c = tt / QR_H2, o = tt - c * QR_H2;
        const float4* src = reinterpret_cast<const float4*>(P + QR_W2 + (size_t)o * QR_H1 + QR_W2C * c);   // 600, 120 and 40 are multiples of 4
#pragma unroll
        for (int k = 0; k < QR_W2C / 4; ++k) { const float4 v = src[k]; w.w2[4 * k] = v.x; w.w2[4 * k + 1] = v.y; w.w2[4 * k + 2] = v.z; w.w2[4 * k + 3] = v.w; }
        w.b2 = c == 0 ? P[QR_B2 + o] : 0.0f;
    }
    {
        const int u = t < QR_H1 ? t : QR_H1 - 1;
        const float4 v = reinterpret_cast<const float4*>(P + QR_W1)[u];
        w.w1[0] = v.x; w.w1[1] = v.y; w.w1[2] = v.z; w.w1[3] = v.w;
        w.b1 = P[QR_B1 + u];
    }
}
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

// layers 1 and 2 of one row: sm.h1 and sm.h2 are valid for every thread when it returns
__device__ __forceinline__ void qr_torso_row(const qr_torso& w, const float4 x, qr_smem& sm, int t) {
    if (t < QR_H1) {
        float z = w.b1;
        z = __builtin_fmaf(w.w1[0], x.x, z); z = __builtin_fmaf(w.w1[1], x.y, z);
        z = __builtin_fmaf(w.w1[2], x.z, z); z = __builtin_fmaf(w.w1[3], x.w, z);
        sm.h1[t] = fmaxf(z, 0.0f);
    }
    __syncthreads();
    if (t < 3 * QR_H2) {
        const int c = t / QR_H2, o = t - c * QR_H2;
        float acc = w.b2;
#pragma unroll
        for (int k = 0; k < QR_W2C; ++k) acc = __builtin_fmaf(w.w2[k], sm.h1[QR_W2C * c + k], acc);
        sm.p2[c][o] = acc;
    }
    __syncthreads();
    if (t < QR_H2) sm.h2[t] = fmaxf((sm.p2[0][t] + sm.p2[1][t]) + sm.p2[2][t], 0.0f);
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
    qr_torso w;
    qr_head hd;
    qr_load_torso(w, params, t);
    qr_load_head(hd, params, t);
    qr_collapse(params, sm, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        qr_torso_row(w, x, sm, t);
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
    const qr_torso& w;
    const float (&wb0)[QR_H2], (&wb1)[QR_H2];
    float bb0, bb1;
    qr_smem& sm;
    int t;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t, uint64_t) {
        qr_torso_row(w, x, sm, t);
        float q0 = bb0, q1 = bb1;
#pragma unroll
        for (int k = 0; k < QR_H2; ++k) {
            const float h = sm.h2[k];
            q0 = __builtin_fmaf(wb0[k], h, q0);
            q1 = __builtin_fmaf(wb1[k], h, q1);
        }
        // no barrier here: sm.h2 is next written behind two barriers of the next qr_torso_row, which no wave passes before all have read it
        return q1 > q0 ? 1 : 0;   // torch.argmax: the first index on a tie
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) qr_act_kernel(mi_env e, mi_qr_ring_t ring, mi_qr_act_t a_, rg_eps_tab eps) {
    __shared__ qr_smem sm;
    const int t = threadIdx.x;
    qr_torso w;
    qr_load_torso(w, a_.params, t);
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
__device__ __forceinline__ void qr_target_row(const qr_torso& w, const qr_head& hd, const mi_qr_ring_t& ring, long long i, float gamma, qr_smem& sm, int t,
                                              int32_t* __restrict__ next_action, float* __restrict__ tgt_out) {
    const long long N = ring.n_envs, total = ring.slots * N;
    const long long nx = i + N >= total ? i + N - total : i + N;   // ((slot + 1) % slots) * N + env
    const float4 x = reinterpret_cast<const float4*>(ring.observations)[nx];
    const float r = ring.rewards[nx];
    const float lg = ring.terminated[nx] ? 0.0f : gamma;
    qr_torso_row(w, x, sm, t);
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
    qr_torso w;
    qr_head hd;
    qr_load_torso(w, bt.target_params, t);
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
    qr_torso w;
    qr_head hd;
    // ---- pass 1, target network: indices, next_actions, target of this workgroup's rows ----
    qr_load_torso(w, bt.target_params, t);
    qr_load_head(hd, bt.target_params, t);
    qr_collapse(bt.target_params, sm, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        qr_target_row(w, hd, ring, i, bt.gamma, sm, t, bt.next_actions + b, bt.target + (size_t)b * QR_NQ);
    }
    __threadfence_block();   // pass 2 reads the targets this workgroup wrote (qr_target_row ends in a barrier)
    __syncthreads();
    // ---- pass 2, online network: forward, loss, backward into register accumulators (the stored action is given: no action values, no collapsed head) ----
    qr_load_torso(w, bt.params, t);
    qr_load_head(hd, bt.params, t);
    float g3[QR_H2], g2[QR_W2C], g1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float gb3 = 0.0f, gb2 = 0.0f, gb1 = 0.0f, loss = 0.0f;
#pragma unroll
    for (int k = 0; k < QR_H2; ++k) g3[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < QR_W2C; ++k) g2[k] = 0.0f;
    const float inv = 1.0f / (float)(bt.batch * QR_NQ);
    const float* __restrict__ P = bt.params;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, false);   // recomputed, not re-read
        const float4 x = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        qr_torso_row(w, x, sm, t);
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
        if (t < 3 * QR_H2) {
            const int c = t / QR_H2, o = t - c * QR_H2;
            const float d = sm.dz2[o];
            if (c == 0) gb2 += d;
#pragma unroll
            for (int k = 0; k < QR_W2C; ++k) g2[k] = __builtin_fmaf(d, sm.h1[QR_W2C * c + k], g2[k]);
        }
        if (t < 2 * QR_H1) {
            const int c = t / QR_H1, k = t - c * QR_H1;
            const float* const col = P + QR_W2 + k;
            float acc = 0.0f;
            for (int o = 42 * c; o < 42 * c + 42; ++o) acc = __builtin_fmaf(sm.dz2[o], col[(size_t)o * QR_H1], acc);
            sm.ph[c][k] = acc;
        }
        __syncthreads();
        if (t < QR_H1) {
            const float d = sm.h1[t] > 0.0f ? sm.ph[0][t] + sm.ph[1][t] : 0.0f;
            gb1 += d;
            g1[0] = __builtin_fmaf(d, x.x, g1[0]); g1[1] = __builtin_fmaf(d, x.y, g1[1]);
            g1[2] = __builtin_fmaf(d, x.z, g1[2]); g1[3] = __builtin_fmaf(d, x.w, g1[3]);
        }
        __syncthreads();
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * QR_STRIDE;
    if (t < QR_NL) {
        float4* const dst = reinterpret_cast<float4*>(slab + QR_W3 + (size_t)t * QR_H2);
#pragma unroll
        for (int k = 0; k < QR_H2 / 4; ++k) dst[k] = make_float4(g3[4 * k], g3[4 * k + 1], g3[4 * k + 2], g3[4 * k + 3]);
        slab[QR_B3 + t] = gb3;
    }
    if (t < 3 * QR_H2) {
        const int c = t / QR_H2, o = t - c * QR_H2;
        float4* const dst = reinterpret_cast<float4*>(slab + QR_W2 + (size_t)o * QR_H1 + QR_W2C * c);
#pragma unroll
        for (int k = 0; k < QR_W2C / 4; ++k) dst[k] = make_float4(g2[4 * k], g2[4 * k + 1], g2[4 * k + 2], g2[4 * k + 3]);
        if (c == 0) slab[QR_B2 + o] = gb2;
    }
    if (t < QR_H1) {
        reinterpret_cast<float4*>(slab + QR_W1)[t] = make_float4(g1[0], g1[1], g1[2], g1[3]);
        slab[QR_B1 + t] = gb1;
    }
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
    RG_CHECK_ARG(a->params && a->obs_cur, "params or obs_cur is NULL");
    RG_CHECK_ARG(rg_aligned(a->params) && rg_aligned(a->obs_cur), "params and obs_cur must be 16-byte aligned");
    const int rc = rg_check_ring(ring);
    if (rc != MI_QR_OK) return rc;
    RG_CHECK_ARG(e->kind == MI_ENV_CARTPOLE_V1 && e->n > 0, "env is not a CartPole-v1 handle");
    RG_CHECK_ARG(e->n == ring->n_envs, "the ring's n_envs is not the handle's");
    RG_CHECK_ARG(a->n_steps > 0 && a->n_steps <= MI_QR_MAX_STEPS_PER_CALL, "n_steps must be in [1, 64]");
    RG_CHECK_ARG(a->global_step >= 0 && a->total_timesteps > 0 && a->exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    RG_CHECK_ARG(a->max_ep >= 0 && (a->max_ep == 0 || (a->episodes && a->episode_stats)), "episodes / episode_stats buffer missing");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, (a->end_e - a->start_e) / (a->exploration_fraction * (double)a->total_timesteps), a->start_e, a->end_e);
    if (a->episode_stats) RG_HIP(hipMemsetAsync(a->episode_stats, 0, 4 * sizeof(int32_t), s));
    const int grid = e->n < 1024 ? e->n : 1024;
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

static int qr_check_batch(const mi_qr_ring_t* ring, const mi_qr_batch_t* b) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_QR_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->batch > 0, "batch <= 0");
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->target && b->next_actions && b->grads && b->loss && b->workspace, "a batch buffer is NULL");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params) && rg_aligned(b->workspace), "params, target_params and workspace must be 16-byte aligned");
    RG_CHECK_ARG(b->sample_upper >= 0 && b->sample_upper <= ring->slots * (int64_t)ring->n_envs, "sample_upper outside [0, slots * n_envs]");
    return MI_QR_OK;
}
static int qr_launch_grad(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, float* p, float* m, float* v, const rg_adam_consts& k, int adam, hipStream_t s) {
    const int slabs = qr_slabs(b->batch);
    qr_grad_kernel<<<slabs, 256, 0, s>>>(*ring, *b, (float*)b->workspace);
    RG_HIP(hipGetLastError());
    if (b->mid_event) RG_HIP(hipEventRecord((hipEvent_t)b->mid_event, s));
    qr_reduce_kernel<<<(QR_NP + 1 + 31) / 32, 32 * RG_RED_GROUPS, 0, s>>>((const float*)b->workspace, slabs, 1.0f / (float)(b->batch * QR_NQ), b->grads, b->loss, p, m, v, k,
                                                                        adam);
    RG_HIP(hipGetLastError());
    return MI_QR_OK;
}

extern "C" int mi_qr_grad(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, void* stream) {
    const int rc = qr_check_batch(ring, b);
    if (rc != MI_QR_OK) return rc;
    return qr_launch_grad(ring, b, nullptr, nullptr, nullptr, rg_adam_consts{}, 0, (hipStream_t)stream);
}

extern "C" int mi_qr_update(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, const mi_qr_adam_t* opt, void* stream) {
    const int rc = qr_check_batch(ring, b);
    if (rc != MI_QR_OK) return rc;
    RG_CHECK_ARG(opt != nullptr, "opt is NULL");
    RG_CHECK_ARG(opt->exp_avg && opt->exp_avg_sq && opt->step >= 1, "an optimizer buffer is NULL or step < 1");
    return qr_launch_grad(ring, b, (float*)b->params, opt->exp_avg, opt->exp_avg_sq, rg_adam_host(opt->step, opt->lr, opt->beta1, opt->beta2, opt->eps), 1, (hipStream_t)stream);
}
