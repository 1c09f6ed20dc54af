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
// The torso's layout, loader, per-thread pieces, backward and slab store are mi_torso.h's, shared with mi_c51.hip and mi_qr.hip; the host side of acting and of the
// gradient entry points is mi_ring.h's.  All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"

#include "../../include/mi_ddqn.h"

#define DD_H1 MI_DDQN_H1
#define DD_H2 MI_DDQN_H2
#define DD_W3 MI_DDQN_W3
#define DD_B3 MI_DDQN_B3
#define DD_NP MI_DDQN_NPARAMS
#define DD_STRIDE MI_DDQN_SLAB_STRIDE
static_assert(MI_DDQN_OK == RG_OK && MI_DDQN_EINVAL == RG_EINVAL && MI_DDQN_EHIP == RG_EHIP && MI_DDQN_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_DDQN_W1 == TS_W1 && MI_DDQN_B1 == TS_B1 && MI_DDQN_W2 == TS_W2 && MI_DDQN_B2 == TS_B2 && MI_DDQN_H1 == TS_H1 && MI_DDQN_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(DD_STRIDE % 4 == 0 && DD_STRIDE > DD_NP, "float4 stores");

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

// the head of the parameters P into sm.w3[net] / sm.b3[net]; the caller's next barrier (every torso evaluation has three) publishes it
__device__ __forceinline__ void dd_load_head(dd_smem& sm, int net, const float* __restrict__ P, int t) {
    if (t < 2 * DD_H2) sm.w3[net][t / DD_H2][t % DD_H2] = P[DD_W3 + t];
    else if (t < 2 * DD_H2 + 2) sm.b3[net][t - 2 * DD_H2] = P[DD_B3 + t - 2 * DD_H2];
}

// layers 1 and 2: with ROW the online torso `on` at xi (-> sm.h1 / sm.h2 [DD_ROW]), with NEXT the online torso at xn (-> [DD_NEXT]) and the target torso `tg` at xn
// (-> [DD_TGT]), all between the same three barriers; the results are valid for every thread when it returns
template <bool ROW, bool NEXT>
__device__ __forceinline__ void dd_torso_rows(const ts_torso& on, const ts_torso& tg, const float4 xi, const float4 xn, dd_smem& sm, int t) {
    if (t < DD_H1) {
        if (ROW) sm.h1[DD_ROW][t] = ts_h1(on, xi);
        if (NEXT) { sm.h1[DD_NEXT][t] = ts_h1(on, xn); sm.h1[DD_TGT][t] = ts_h1(tg, xn); }
    }
    __syncthreads();
    if (t < 3 * DD_H2) {
        const int c = t / DD_H2, o = t - c * DD_H2;
        if (ROW) sm.p2[DD_ROW][c][o] = ts_p2(on, &sm.h1[DD_ROW][TS_W2C * c]);
        if (NEXT) { sm.p2[DD_NEXT][c][o] = ts_p2(on, &sm.h1[DD_NEXT][TS_W2C * c]); sm.p2[DD_TGT][c][o] = ts_p2(tg, &sm.h1[DD_TGT][TS_W2C * c]); }
    }
    __syncthreads();
    if (t < DD_H2) {
        if (ROW) sm.h2[DD_ROW][t] = ts_h2(sm.p2[DD_ROW], t);
        if (NEXT) { sm.h2[DD_NEXT][t] = ts_h2(sm.p2[DD_NEXT], t); sm.h2[DD_TGT][t] = ts_h2(sm.p2[DD_TGT], t); }
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
    ts_torso w;
    ts_load(w, params, t);
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
    const ts_torso& w;
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
    ts_torso w;
    ts_load(w, a_.params, t);
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
    ts_torso on, tg;
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
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
    ts_torso on, tg;   // the online network is loaded once and serves both online passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    dd_load_head(sm, DD_ONLINE, bt.params, t);
    dd_load_head(sm, DD_TARGET, bt.target_params, t);
    float g3 = 0.0f, gb3 = 0.0f, loss = 0.0f;
    ts_grads g;
    ts_zero(g);
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
        ts_backward(g, sm.h1[DD_ROW], sm.dz2, sm.ph, xi, P, t);   // sm.h1 / sm.ph / sm.dz2 are then the next row's
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * DD_STRIDE;
    if (t < 2 * DD_H2) slab[DD_W3 + t] = g3;
    else if (t < 2 * DD_H2 + 2) slab[DD_B3 + t - 2 * DD_H2] = gb3;
    ts_store(g, slab, t);
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
    RG_CHECK_ARG(a->global_step >= 0 && a->total_timesteps > 0 && a->exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    RG_CHECK_ARG(a->learning_starts >= 0, "learning_starts < 0");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, (a->end_e - a->start_e) / (a->exploration_fraction * (double)a->total_timesteps), a->start_e, a->end_e);
    for (int k = 0; k < RG_MAX_STEPS; ++k) tab.v[k] = (double)(float)tab.v[k];   // DQN compares the draw with epsilon as an f32 (mi_dqn_act_steps)
    int grid;
    const int rc = rg_act_prelude(e, ring, a->params, a->obs_cur, a->n_steps, a->max_ep, a->episodes, a->episode_stats, s, grid);
    if (rc != MI_DDQN_OK) return rc;
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

// mi_ddqn_grad (update false: opt is not looked at) and mi_ddqn_update
static int dd_grad(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, const mi_ddqn_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_ddqn_batch_t& bt) { return bt.current && bt.target; });
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<DD_NP>(ddqn_grad_kernel, ddqn_reduce_kernel, ring, b, dd_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_ddqn_grad(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, void* stream) { return dd_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_ddqn_update(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, const mi_ddqn_adam_t* opt, void* stream) {
    return dd_grad(ring, b, opt, true, (hipStream_t)stream);
}
