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
// The torso's layout, loader, per-thread pieces, backward and slab store are mi_torso.h's, shared with mi_c51.hip and mi_qr.hip; the head, the three evaluations of
// a row and pass 2 of a gradient row are mi_qhead.h's, shared with mi_mdqn.hip; the host side of acting and of the gradient entry points is mi_ring.h's. All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_qhead.h"

#include "../../include/mi_ddqn.h"

static_assert(MI_DDQN_OK == RG_OK && MI_DDQN_EINVAL == RG_EINVAL && MI_DDQN_EHIP == RG_EHIP && MI_DDQN_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_DDQN_W1 == TS_W1 && MI_DDQN_B1 == TS_B1 && MI_DDQN_W2 == TS_W2 && MI_DDQN_B2 == TS_B2 && MI_DDQN_H1 == TS_H1 && MI_DDQN_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_DDQN_W3 == QH_W3 && MI_DDQN_B3 == QH_B3 && MI_DDQN_NPARAMS == QH_NP && MI_DDQN_SLAB_STRIDE == QH_STRIDE, "mi_qhead.h holds this head");

#ifndef MI_DDQN_SOURCE_ID
#define MI_DDQN_SOURCE_ID "unknown"
#endif
extern "C" int mi_ddqn_version(void) { return MI_DDQN_VERSION; }
extern "C" const char* mi_ddqn_last_error(void) { return rg_err; }
extern "C" const char* mi_ddqn_source_id(void) { return MI_DDQN_SOURCE_ID; }
static int dd_slabs(int batch) { return rg_slabs(batch, MI_DDQN_MAX_SLABS); }
extern "C" size_t mi_ddqn_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)dd_slabs(batch) * QH_STRIDE * sizeof(float);
}

// the evaluations a workgroup keeps beside QH_ROW (the online network at obs[i]): NEXT the online network at obs[nx], TGT the target network at obs[nx]
enum { DD_NEXT = 1, DD_TGT = 2 };

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) ddqn_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, float* __restrict__ q) {
    __shared__ qh_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, params, t);
    qh_load_head(sm, QH_ONLINE, params, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        qh_torso_rows<true, false>(w, x, w, x, w, x, sm, t);
        float q0, q1;
        qh_values(sm, QH_ROW, QH_ONLINE, q0, q1);
        if (t == 0) { q[2 * (size_t)row] = q0; q[2 * (size_t)row + 1] = q1; }
        // no barrier here: sm.h2 is next written behind two barriers of the next qh_torso_rows, which no wave passes before all have read it
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the online torso in `w`, its head in LDS
struct dd_policy {
    const ts_torso& w;
    qh_smem& sm;
    int t;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t, uint64_t) {
        qh_torso_rows<true, false>(w, x, w, x, w, x, sm, t);
        float q0, q1;
        qh_values(sm, QH_ROW, QH_ONLINE, q0, q1);
        // no barrier here: sm.h2 is next written behind two barriers of the next qh_torso_rows, which no wave passes before all have read it
        return qh_argmax(q0, q1);
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) ddqn_act_kernel(mi_env e, mi_ddqn_ring_t ring, mi_ddqn_act_t a_, rg_eps_tab eps) {
    __shared__ qh_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, a_.params, t);
    qh_load_head(sm, QH_ONLINE, a_.params, t);
    __syncthreads();
    dd_policy policy{w, sm, t};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// pass 1 of a row whose evaluations DD_NEXT / DD_TGT are in sm: a* by the online head, the target network's value of a* (every thread holds both)
__device__ __forceinline__ void dd_target_value(const qh_smem& sm, float r, float lg, int& a_star, float& tgt) {
    float q0, q1, t0, t1;
    qh_values(sm, DD_NEXT, QH_ONLINE, q0, q1);
    qh_values(sm, DD_TGT, QH_TARGET, t0, t1);
    a_star = qh_argmax(q0, q1);
    tgt = r + lg * (a_star ? t1 : t0);   // -ffp-contract=off: a product, then a sum
}

__global__ void __launch_bounds__(256) ddqn_target_kernel(mi_ddqn_ring_t ring, mi_ddqn_batch_t bt) {
    __shared__ qh_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    qh_load_head(sm, QH_ONLINE, bt.params, t);
    qh_load_head(sm, QH_TARGET, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = qh_clamp_index(bt.idx[b], total);
        const long long nx = qh_successor(ring, i, total);
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        qh_torso_rows<false, true>(on, xn, on, xn, tg, xn, sm, t);
        int a_star; float tgt;
        dd_target_value(sm, r, lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; }
    }
}

__global__ void __launch_bounds__(256) ddqn_grad_kernel(mi_ddqn_ring_t ring, mi_ddqn_batch_t bt, float* __restrict__ slabs) {
    __shared__ qh_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;   // the online network is loaded once and serves both online passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    qh_load_head(sm, QH_ONLINE, bt.params, t);
    qh_load_head(sm, QH_TARGET, bt.target_params, t);
    qh_grads G;
    qh_zero(G);
    const float inv = 1.0f / (float)bt.batch;
    const float* __restrict__ P = bt.params;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        const long long nx = qh_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        qh_torso_rows<true, true>(on, xi, on, xn, tg, xn, sm, t);
        // ---- pass 1, obs[nx]: the online argmax, the target network's value of it ----
        int a_star; float tgt;
        dd_target_value(sm, r, lg, a_star, tgt);
        // ---- pass 2, obs[i]: the stored action's online value, the loss, the backward into register accumulators ----
        qh_grad_row(G, sm, a, tgt, inv, xi, P, t, [&](float cur, float) { bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.current[b] = cur; });
    }
    qh_store(G, slabs + (size_t)blockIdx.x * QH_STRIDE, t);
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) ddqn_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                          float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                          rg_adam_consts k, int adam) {
    rg_reduce<QH_NP, QH_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
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
    return rg_launch_grad<QH_NP>(ddqn_grad_kernel, ddqn_reduce_kernel, ring, b, dd_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_ddqn_grad(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, void* stream) { return dd_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_ddqn_update(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, const mi_ddqn_adam_t* opt, void* stream) {
    return dd_grad(ring, b, opt, true, (hipStream_t)stream);
}
