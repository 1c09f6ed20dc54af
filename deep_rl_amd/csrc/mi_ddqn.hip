// mi_ddqn.hip — libmirl_ddqn.so: Double DQN on CartPole-v1 for gfx950.  C ABI, numerics and RNG contract: include/mi_ddqn.h.
//
// The form of mi_c51.hip / mi_qr.hip: one 256-thread workgroup evaluates one row at a time with the torso in its registers (thread c * 84 + o a 40-wide third of row
// o of W2, thread u < 120 row u of W1), loaded once per launch; the two-row heads lie in LDS and every thread forms both action values itself from workgroup-uniform
// broadcasts, so a forward pass costs the torso's three barriers and none for the head.  The gradient launch holds BOTH networks' torsos (2 x 46 floats per thread)
// beside its accumulators and evaluates the three torsos of a batch row — online at obs[i], online at obs[nx], target at obs[nx] — between the same three barriers.
//   ddqn_act_kernel      a workgroup walks its envs, each through all steps of the chunk; exploring and pre-learning_starts steps skip the network.
//   ddqn_grad_kernel     a workgroup walks its batch rows: pass 1 on obs[nx] (online argmax a*, the target network's value of a* -> next_actions / target), pass 2 on
//                        obs[i] (online forward -> current, loss, backward into register accumulators) — one slab per workgroup.
//   ddqn_reduce_kernel   fixed-order slab sum (+ Adam).
//   ddqn_target_kernel   pass 1 alone.
//   ddqn_forward_kernel  the action values of n observations.
// All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"

#include "../../include/mi_ddqn.h"

#define DD_H1 MI_DDQN_H1
#define DD_H2 MI_DDQN_H2
#define DD_W1 MI_DDQN_W1
#define DD_B1 MI_DDQN_B1
#define DD_W2 MI_DDQN_W2
#define DD_B2 MI_DDQN_B2
#define DD_W3 MI_DDQN_W3
#define DD_B3 MI_DDQN_B3
#define DD_NP MI_DDQN_NPARAMS
#define DD_STRIDE MI_DDQN_SLAB_STRIDE
#define DD_W2C 40              // columns of W2 per thread (three threads per row)
static_assert(MI_DDQN_OK == RG_OK && MI_DDQN_EINVAL == RG_EINVAL && MI_DDQN_EHIP == RG_EHIP && MI_DDQN_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(DD_W2 % 4 == 0 && DD_H1 % 4 == 0 && DD_W2C % 4 == 0 && DD_STRIDE % 4 == 0 && DD_STRIDE > DD_NP, "float4 loads and stores");

#ifndef MI_DDQN_SOURCE_ID
#define MI_DDQN_SOURCE_ID "unknown"
#endif
extern "C" int mi_ddqn_version(void) { return MI_DDQN_VERSION; }
extern "C" const char* mi_ddqn_last_error(void) { return rg_err; }
extern "C" const char* mi_ddqn_source_id(void) { return MI_DDQN_SOURCE_ID; }
static int dd_slabs(int batch) { return rg_slabs(batch, MI_DDQN_MAX_SLABS); }
extern "C" size_t mi_ddqn_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)dd_slabs(batch) * DD_STRIDE * sizeof(float);
}

// ---- the network as one workgroup holds it ------------------------------------------------------------
struct dd_torso {
    float w2[DD_W2C]; float b2;         // thread c * 84 + o < 252: W2[o][40 c .. 40 c + 39]; b2 is the chain's start (the bias for c = 0, else 0)
    float w1[4]; float b1;              // thread u < 120
};
// the evaluations a workgroup keeps side by side: ROW the online network at obs[i], NEXT the online network at obs[nx], TGT the target network at obs[nx]
enum { DD_ROW = 0, DD_NEXT = 1, DD_TGT = 2, DD_EVALS = 3 };
enum { DD_ONLINE = 0, DD_TARGET = 1 };
struct dd_smem {
    float h1[DD_EVALS][DD_H1];
    float p2[DD_EVALS][3][DD_H2];       // layer 2's partial chains
    float h2[DD_EVALS][DD_H2];
    float w3[2][2][DD_H2];              // [network][action]: the heads
    float b3[2][2];
    float dz2[DD_H2];
    float ph[2][DD_H1];                 // the backward's partial chains of dh1
};

__device__ __forceinline__ void dd_load_torso(dd_torso& w, const float* __restrict__ P, int t) {
    {
        const int tt = t < 3 * DD_H2 ? t : 3 * DD_H2 - 1;
        const int c = tt / DD_H2, o = tt - c * DD_H2;
        const float4* src = reinterpret_cast<const float4*>(P + DD_W2 + (size_t)o * DD_H1 + DD_W2C * c);   // 600, 120 and 40 are multiples of 4
#pragma unroll
        for (int k = 0; k < DD_W2C / 4; ++k) { const float4 v = src[k]; w.w2[4 * k] = v.x; w.w2[4 * k + 1] = v.y; w.w2[4 * k + 2] = v.z; w.w2[4 * k + 3] = v.w; }
        w.b2 = c == 0 ? P[DD_B2 + o] : 0.0f;
    }
    {
        const int u = t < DD_H1 ? t : DD_H1 - 1;
        const float4 v = reinterpret_cast<const float4*>(P + DD_W1)[u];
        w.w1[0] = v.x; w.w1[1] = v.y; w.w1[2] = v.z; w.w1[3] = v.w;
        w.b1 = P[DD_B1 + u];
    }
}
// the head of the parameters P into sm.w3[net] / sm.b3[net]; the caller's next barrier (every torso evaluation has three) publishes it
__device__ __forceinline__ void dd_load_head(dd_smem& sm, int net, const float* __restrict__ P, int t) {
    if (t < 2 * DD_H2) sm.w3[net][t / DD_H2][t % DD_H2] = P[DD_W3 + t];
    else if (t < 2 * DD_H2 + 2) sm.b3[net][t - 2 * DD_H2] = P[DD_B3 + t - 2 * DD_H2];
}

__device__ __forceinline__ float dd_z1(const dd_torso& w, const float4 x) {
    float z = w.b1;
    z = __builtin_fmaf(w.w1[0], x.x, z); z = __builtin_fmaf(w.w1[1], x.y, z);
    z = __builtin_fmaf(w.w1[2], x.z, z); z = __builtin_fmaf(w.w1[3], x.w, z);
    return fmaxf(z, 0.0f);
}
__device__ __forceinline__ float dd_p2(const dd_torso& w, const float* __restrict__ h1c) {
    float acc = w.b2;
#pragma unroll
    for (int k = 0; k < DD_W2C; ++k) acc = __builtin_fmaf(w.w2[k], h1c[k], acc);
    return acc;
}
// layers 1 and 2: with ROW the online torso `on` at xi (-> sm.h1 / sm.h2 [DD_ROW]), with NEXT the online torso at xn (-> [DD_NEXT]) and the target torso `tg` at xn
// (-> [DD_TGT]), all between the same three barriers; the results are valid for every thread when it returns
template <bool ROW, bool NEXT>
__device__ __forceinline__ void dd_torso_rows(const dd_torso& on, const dd_torso& tg, const float4 xi, const float4 xn, dd_smem& sm, int t) {
    if (t < DD_H1) {
        if (ROW) sm.h1[DD_ROW][t] = dd_z1(on, xi);
        if (NEXT) { sm.h1[DD_NEXT][t] = dd_z1(on, xn); sm.h1[DD_TGT][t] = dd_z1(tg, xn); }
    }
    __syncthreads();
    if (t < 3 * DD_H2) {
        const int c = t / DD_H2, o = t - c * DD_H2;
        if (ROW) sm.p2[DD_ROW][c][o] = dd_p2(on, &sm.h1[DD_ROW][DD_W2C * c]);
        if (NEXT) { sm.p2[DD_NEXT][c][o] = dd_p2(on, &sm.h1[DD_NEXT][DD_W2C * c]); sm.p2[DD_TGT][c][o] = dd_p2(tg, &sm.h1[DD_TGT][DD_W2C * c]); }
    }
    __syncthreads();
    if (t < DD_H2) {
        if (ROW) sm.h2[DD_ROW][t] = fmaxf((sm.p2[DD_ROW][0][t] + sm.p2[DD_ROW][1][t]) + sm.p2[DD_ROW][2][t], 0.0f);
        if (NEXT) {
            sm.h2[DD_NEXT][t] = fmaxf((sm.p2[DD_NEXT][0][t] + sm.p2[DD_NEXT][1][t]) + sm.p2[DD_NEXT][2][t], 0.0f);
            sm.h2[DD_TGT][t] = fmaxf((sm.p2[DD_TGT][0][t] + sm.p2[DD_TGT][1][t]) + sm.p2[DD_TGT][2][t], 0.0f);
        }
    }
    __syncthreads();
}

// THE two action values (mi_ddqn.h) of evaluation `ev` through the head of network `net`, in every thread (two independent chains; the reads are workgroup-uniform
// broadcasts)
__device__ __forceinline__ void dd_values(const dd_smem& sm, int ev, int net, float& q0, float& q1) {
    q0 = sm.b3[net][0]; q1 = sm.b3[net][1];
#pragma unroll
    for (int k = 0; k < DD_H2; ++k) {
        const float h = sm.h2[ev][k];
        q0 = __builtin_fmaf(sm.w3[net][0][k], h, q0);
        q1 = __builtin_fmaf(sm.w3[net][1][k], h, q1);
    }
}
__device__ __forceinline__ int dd_argmax(float q0, float q1) { return q1 > q0 ? 1 : 0; }   // torch.argmax: the first index on a tie

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) ddqn_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, float* __restrict__ q) {
    __shared__ dd_smem sm;
    const int t = threadIdx.x;
    dd_torso w;
    dd_load_torso(w, params, t);
    dd_load_head(sm, DD_ONLINE, params, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        dd_torso_rows<true, false>(w, w, x, x, sm, t);
        float q0, q1;
        dd_values(sm, DD_ROW, DD_ONLINE, q0, q1);
        if (t == 0) { q[2 * (size_t)row] = q0; q[2 * (size_t)row + 1] = q1; }
        // no barrier here: sm.h2 is next written behind two barriers of the next dd_torso_rows, which no wave passes before all have read it
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the online torso in `w`, its head in LDS
struct dd_policy {
    const dd_torso& w;
    dd_smem& sm;
    int t;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t, uint64_t) {
        dd_torso_rows<true, false>(w, w, x, x, sm, t);
        float q0, q1;
        dd_values(sm, DD_ROW, DD_ONLINE, q0, q1);
        // no barrier here: sm.h2 is next written behind two barriers of the next dd_torso_rows, which no wave passes before all have read it
        return dd_argmax(q0, q1);
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) ddqn_act_kernel(mi_env e, mi_ddqn_ring_t ring, mi_ddqn_act_t a_, rg_eps_tab eps) {
    __shared__ dd_smem sm;
    const int t = threadIdx.x;
    dd_torso w;
    dd_load_torso(w, a_.params, t);
    dd_load_head(sm, DD_ONLINE, a_.params, t);
    __syncthreads();
    dd_policy policy{w, sm, t};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// the successor of flat ring index i: ((slot + 1) % slots) * N + env
__device__ __forceinline__ long long dd_successor(const mi_ddqn_ring_t& ring, long long i, long long total) {
    const long long N = ring.n_envs;
    return i + N >= total ? i + N - total : i + N;
}
// pass 1 of a row whose evaluations DD_NEXT / DD_TGT are in sm: a* by the online head, the target network's value of a* (every thread holds both)
__device__ __forceinline__ void dd_target_value(const dd_smem& sm, float r, float lg, int& a_star, float& tgt) {
    float q0, q1, t0, t1;
    dd_values(sm, DD_NEXT, DD_ONLINE, q0, q1);
    dd_values(sm, DD_TGT, DD_TARGET, t0, t1);
    a_star = dd_argmax(q0, q1);
    tgt = r + lg * (a_star ? t1 : t0);   // -ffp-contract=off: a product, then a sum
}

__global__ void __launch_bounds__(256) ddqn_target_kernel(mi_ddqn_ring_t ring, mi_ddqn_batch_t bt) {
    __shared__ dd_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    dd_torso on, tg;
    dd_load_torso(on, bt.params, t);
    dd_load_torso(tg, bt.target_params, t);
    dd_load_head(sm, DD_ONLINE, bt.params, t);
    dd_load_head(sm, DD_TARGET, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        const long long nx = dd_successor(ring, i, total);
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        dd_torso_rows<false, true>(on, tg, xn, xn, sm, t);
        int a_star; float tgt;
        dd_target_value(sm, r, lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; }
    }
}

__global__ void __launch_bounds__(256) ddqn_grad_kernel(mi_ddqn_ring_t ring, mi_ddqn_batch_t bt, float* __restrict__ slabs) {
    __shared__ dd_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    dd_torso on, tg;   // the online network is loaded once and serves both online passes
    dd_load_torso(on, bt.params, t);
    dd_load_torso(tg, bt.target_params, t);
    dd_load_head(sm, DD_ONLINE, bt.params, t);
    dd_load_head(sm, DD_TARGET, bt.target_params, t);
    float g2[DD_W2C], g1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float g3 = 0.0f, gb3 = 0.0f, gb2 = 0.0f, gb1 = 0.0f, loss = 0.0f;
#pragma unroll
    for (int k = 0; k < DD_W2C; ++k) g2[k] = 0.0f;
    const float inv = 1.0f / (float)bt.batch;
    const float* __restrict__ P = bt.params;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        const long long nx = dd_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        dd_torso_rows<true, true>(on, tg, xi, xn, sm, t);
        // ---- pass 1, obs[nx]: the online argmax, the target network's value of it ----
        int a_star; float tgt;
        dd_target_value(sm, r, lg, a_star, tgt);
        // ---- pass 2, obs[i]: the stored action's online value, the loss, the backward into register accumulators ----
        float c0, c1;
        dd_values(sm, DD_ROW, DD_ONLINE, c0, c1);
        const float cur = a ? c1 : c0;
        const float td = tgt - cur;
        const float d = -((2.0f * td) * inv);
        if (t == 0) {
            bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.current[b] = cur;
            loss += td * td;
        }
        // layer 3: thread a' * 84 + k owns dW3[a'][k], thread 168 + a' db3[a']; the other action's row is not touched
        if (t < 2 * DD_H2) {
            if (t / DD_H2 == a) g3 = __builtin_fmaf(d, sm.h2[DD_ROW][t % DD_H2], g3);
        } else if (t - 2 * DD_H2 == a) {
            gb3 += d;
        }
        if (t < DD_H2) sm.dz2[t] = sm.h2[DD_ROW][t] > 0.0f ? d * sm.w3[DD_ONLINE][a][t] : 0.0f;
        __syncthreads();
        if (t < 3 * DD_H2) {
            const int c = t / DD_H2, o = t - c * DD_H2;
            const float dz = sm.dz2[o];
            if (c == 0) gb2 += dz;
#pragma unroll
            for (int k = 0; k < DD_W2C; ++k) g2[k] = __builtin_fmaf(dz, sm.h1[DD_ROW][DD_W2C * c + k], g2[k]);
        }
        if (t < 2 * DD_H1) {   // dh1: W2's column k comes from memory (consecutive threads, consecutive addresses)
            const int c = t / DD_H1, k = t - c * DD_H1;
            const float* const col = P + DD_W2 + k;
            float acc = 0.0f;
            for (int o = 42 * c; o < 42 * c + 42; ++o) acc = __builtin_fmaf(sm.dz2[o], col[(size_t)o * DD_H1], acc);
            sm.ph[c][k] = acc;
        }
        __syncthreads();
        if (t < DD_H1) {
            const float dz = sm.h1[DD_ROW][t] > 0.0f ? sm.ph[0][t] + sm.ph[1][t] : 0.0f;
            gb1 += dz;
            g1[0] = __builtin_fmaf(dz, xi.x, g1[0]); g1[1] = __builtin_fmaf(dz, xi.y, g1[1]);
            g1[2] = __builtin_fmaf(dz, xi.z, g1[2]); g1[3] = __builtin_fmaf(dz, xi.w, g1[3]);
        }
        __syncthreads();   // sm.h1 / sm.ph / sm.dz2 are the next row's
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * DD_STRIDE;
    if (t < 2 * DD_H2) slab[DD_W3 + t] = g3;
    else if (t < 2 * DD_H2 + 2) slab[DD_B3 + t - 2 * DD_H2] = gb3;
    if (t < 3 * DD_H2) {
        const int c = t / DD_H2, o = t - c * DD_H2;
        float4* const dst = reinterpret_cast<float4*>(slab + DD_W2 + (size_t)o * DD_H1 + DD_W2C * c);
#pragma unroll
        for (int k = 0; k < DD_W2C / 4; ++k) dst[k] = make_float4(g2[4 * k], g2[4 * k + 1], g2[4 * k + 2], g2[4 * k + 3]);
        if (c == 0) slab[DD_B2 + o] = gb2;
    }
    if (t < DD_H1) {
        reinterpret_cast<float4*>(slab + DD_W1)[t] = make_float4(g1[0], g1[1], g1[2], g1[3]);
        slab[DD_B1 + t] = gb1;
    }
    if (t == 0) { slab[DD_NP] = loss; slab[DD_NP + 1] = 0.0f; }
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) ddqn_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                          float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                          rg_adam_consts k, int adam) {
    rg_reduce<DD_NP, DD_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_ddqn_forward(const float* params, const float* obs, int n, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && n > 0 && q, "bad arguments");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    ddqn_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, n, q);
    RG_HIP(hipGetLastError());
    return MI_DDQN_OK;
}

extern "C" int mi_ddqn_act_steps(void* handle, const mi_ddqn_ring_t* ring, const mi_ddqn_act_t* a, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    RG_CHECK_ARG(e != nullptr && a != nullptr, "NULL pointer");
    RG_CHECK_ARG(a->params && a->obs_cur, "params or obs_cur is NULL");
    RG_CHECK_ARG(rg_aligned(a->params) && rg_aligned(a->obs_cur), "params and obs_cur must be 16-byte aligned");
    const int rc = rg_check_ring(ring);
    if (rc != MI_DDQN_OK) return rc;
    RG_CHECK_ARG(e->kind == MI_ENV_CARTPOLE_V1 && e->n > 0, "env is not a CartPole-v1 handle");
    RG_CHECK_ARG(e->n == ring->n_envs, "the ring's n_envs is not the handle's");
    RG_CHECK_ARG(a->n_steps > 0 && a->n_steps <= MI_DDQN_MAX_STEPS_PER_CALL, "n_steps must be in [1, 64]");
    RG_CHECK_ARG(a->global_step >= 0 && a->total_timesteps > 0 && a->exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    RG_CHECK_ARG(a->learning_starts >= 0, "learning_starts < 0");
    RG_CHECK_ARG(a->max_ep >= 0 && (a->max_ep == 0 || (a->episodes && a->episode_stats)), "episodes / episode_stats buffer missing");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, (a->end_e - a->start_e) / (a->exploration_fraction * (double)a->total_timesteps), a->start_e, a->end_e);
    for (int k = 0; k < RG_MAX_STEPS; ++k) tab.v[k] = (double)(float)tab.v[k];   // DQN compares the draw with epsilon as an f32 (mi_dqn_act_steps)
    if (a->episode_stats) RG_HIP(hipMemsetAsync(a->episode_stats, 0, 4 * sizeof(int32_t), s));
    const int grid = e->n < 1024 ? e->n : 1024;
    if (a->forced_actions || a->forced_resets)
        ddqn_act_kernel<true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    else
        ddqn_act_kernel<false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    RG_HIP(hipGetLastError());
    return MI_DDQN_OK;
}

extern "C" int mi_ddqn_target(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_DDQN_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->next_actions && b->target && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params), "params and target_params must be 16-byte aligned");
    ddqn_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_DDQN_OK;
}

static int dd_check_batch(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_DDQN_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->batch > 0, "batch <= 0");
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->current && b->target && b->next_actions && b->grads && b->loss && b->workspace, "a batch buffer is NULL");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params) && rg_aligned(b->workspace), "params, target_params and workspace must be 16-byte aligned");
    RG_CHECK_ARG(b->sample_upper >= 0 && b->sample_upper <= ring->slots * (int64_t)ring->n_envs, "sample_upper outside [0, slots * n_envs]");
    return MI_DDQN_OK;
}
static int dd_launch_grad(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, float* p, float* m, float* v, const rg_adam_consts& k, int adam, hipStream_t s) {
    const int slabs = dd_slabs(b->batch);
    ddqn_grad_kernel<<<slabs, 256, 0, s>>>(*ring, *b, (float*)b->workspace);
    RG_HIP(hipGetLastError());
    if (b->mid_event) RG_HIP(hipEventRecord((hipEvent_t)b->mid_event, s));
    ddqn_reduce_kernel<<<(DD_NP + 1 + 31) / 32, 32 * RG_RED_GROUPS, 0, s>>>((const float*)b->workspace, slabs, 1.0f / (float)b->batch, b->grads, b->loss, p, m, v, k, adam);
    RG_HIP(hipGetLastError());
    return MI_DDQN_OK;
}

extern "C" int mi_ddqn_grad(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, void* stream) {
    const int rc = dd_check_batch(ring, b);
    if (rc != MI_DDQN_OK) return rc;
    return dd_launch_grad(ring, b, nullptr, nullptr, nullptr, rg_adam_consts{}, 0, (hipStream_t)stream);
}

extern "C" int mi_ddqn_update(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, const mi_ddqn_adam_t* opt, void* stream) {
    const int rc = dd_check_batch(ring, b);
    if (rc != MI_DDQN_OK) return rc;
    RG_CHECK_ARG(opt != nullptr, "opt is NULL");
    RG_CHECK_ARG(opt->exp_avg && opt->exp_avg_sq && opt->step >= 1, "an optimizer buffer is NULL or step < 1");
    return dd_launch_grad(ring, b, (float*)b->params, opt->exp_avg, opt->exp_avg_sq, rg_adam_host(opt->step, opt->lr, opt->beta1, opt->beta2, opt->eps), 1, (hipStream_t)stream);
}
