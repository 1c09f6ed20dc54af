// mi_pdd.hip — libmirl_pdd.so: prioritized dueling Double DQN on CartPole-v1 for gfx950.  C ABI, numerics and RNG contract: include/mi_pdd.h.
//
// The form of mi_ddqn.hip: one 256-thread workgroup evaluates one row at a time with the torso in its registers (thread c * 84 + o a 40-wide third of row o of W2,
// thread u < 120 row u of W1), loaded once per launch; the 255-element dueling heads (value row, advantage rows, three biases) lie in LDS in parameter order and every
// thread forms both action values itself from workgroup-uniform broadcasts, so a forward pass costs the torso's three barriers and none for the head.  The gradient
// launch holds BOTH networks' torsos (2 x 46 floats per thread) beside its accumulators and evaluates the three torsos of a batch row — online at obs[i], online at
// obs[nx], target at obs[nx] — between the same three barriers.  The head's gradient is ONE accumulator per thread: thread t < 255 owns element 10,764 + t.
//   pdd_act_kernel      a workgroup walks its envs, each through all steps of the chunk; exploring and pre-learning_starts steps skip the network.
//   pdd_grad_kernel     a workgroup walks its batch rows: pass 1 on obs[nx] (online argmax a*, the target network's value of a* -> next_actions / target), pass 2 on
//                       obs[i] (online forward -> current, |td|, weighted loss, backward into register accumulators) — one slab per workgroup.
//   pdd_reduce_kernel   fixed-order slab sum (+ Adam).
//   pdd_target_kernel   pass 1 alone.
//   pdd_forward_kernel  the action values of n observations.
// The torso's layout, loader, per-thread pieces, backward and slab store are mi_torso.h's; the host side of acting and of the gradient entry points is mi_ring.h's.
// The dueling head in LDS, the three-evaluation torso rows, the action values, the gradient row and the slab epilogue are mi_dueling.h's, which mi_nstep.hip and
// mi_noisy.hip include too.  All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"
#include "mi_dueling.h"

#include "../../include/mi_pdd.h"

#define PD_NP MI_PDD_NPARAMS
#define PD_STRIDE MI_PDD_SLAB_STRIDE
static_assert(MI_PDD_OK == RG_OK && MI_PDD_EINVAL == RG_EINVAL && MI_PDD_EHIP == RG_EHIP && MI_PDD_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_PDD_W1 == TS_W1 && MI_PDD_B1 == TS_B1 && MI_PDD_W2 == TS_W2 && MI_PDD_B2 == TS_B2 && MI_PDD_H1 == TS_H1 && MI_PDD_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_PDD_WV == DU_HEAD + DU_WV && MI_PDD_BV == DU_HEAD + DU_BV && MI_PDD_WA == DU_HEAD + DU_WA && MI_PDD_BA == DU_HEAD + DU_BA && PD_NP == DU_HEAD + DU_NHEAD,
              "mi_dueling.h holds this head");
static_assert(PD_STRIDE % 4 == 0 && PD_STRIDE > PD_NP, "float4 stores");

#ifndef MI_PDD_SOURCE_ID
#define MI_PDD_SOURCE_ID "unknown"
#endif
extern "C" int mi_pdd_version(void) { return MI_PDD_VERSION; }
extern "C" const char* mi_pdd_last_error(void) { return rg_err; }
extern "C" const char* mi_pdd_source_id(void) { return MI_PDD_SOURCE_ID; }
static int pd_slabs(int batch) { return rg_slabs(batch, MI_PDD_MAX_SLABS); }
extern "C" size_t mi_pdd_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)pd_slabs(batch) * PD_STRIDE * sizeof(float);
}

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) pdd_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, float* __restrict__ q) {
    __shared__ du_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, params, t);
    du_load_head(sm, DU_ONLINE, params, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        du_torso_rows<true, false>(w, w, x, x, sm, t);
        float q0, q1;
        du_values(sm, DU_ROW, DU_ONLINE, q0, q1);
        if (t == 0) { q[2 * (size_t)row] = q0; q[2 * (size_t)row + 1] = q1; }
        // no barrier here: sm.h2 is next written behind two barriers of the next du_torso_rows, which no wave passes before all have read it
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the online torso in `w`, its head in LDS
struct pd_policy {
    const ts_torso& w;
    du_smem& sm;
    int t;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t, uint64_t) {
        du_torso_rows<true, false>(w, w, x, x, sm, t);
        float q0, q1;
        du_values(sm, DU_ROW, DU_ONLINE, q0, q1);
        // no barrier here: sm.h2 is next written behind two barriers of the next du_torso_rows, which no wave passes before all have read it
        return du_argmax(q0, q1);
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) pdd_act_kernel(mi_env e, mi_pdd_ring_t ring, mi_pdd_act_t a_, rg_eps_tab eps) {
    __shared__ du_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, a_.params, t);
    du_load_head(sm, DU_ONLINE, a_.params, t);
    __syncthreads();
    pd_policy policy{w, sm, t};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// the successor of flat ring index i: ((slot + 1) % slots) * N + env
__device__ __forceinline__ long long pd_successor(const mi_pdd_ring_t& ring, long long i, long long total) {
    const long long N = ring.n_envs;
    return i + N >= total ? i + N - total : i + N;
}

__global__ void __launch_bounds__(256) pdd_target_kernel(mi_pdd_ring_t ring, mi_pdd_batch_t bt) {
    __shared__ du_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    du_load_head(sm, DU_ONLINE, bt.params, t);
    du_load_head(sm, DU_TARGET, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        const long long nx = pd_successor(ring, i, total);
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        du_torso_rows<false, true>(on, tg, xn, xn, sm, t);
        int a_star; float tgt;
        du_target_value(sm, r, lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; }
    }
}

__global__ void __launch_bounds__(256) pdd_grad_kernel(mi_pdd_ring_t ring, mi_pdd_batch_t bt, float* __restrict__ slabs) {
    __shared__ du_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;   // the online network is loaded once and serves both online passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    du_load_head(sm, DU_ONLINE, bt.params, t);
    du_load_head(sm, DU_TARGET, bt.target_params, t);
    du_grads G;
    du_zero(G);
    const float inv = 1.0f / (float)bt.batch;
    const du_elem he = du_classify(t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        const long long nx = pd_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        const float wb = bt.weights ? bt.weights[b] : 1.0f;
        du_grad_row(G, sm, on, tg, xi, xn, a, r, lg, wb, inv, he, bt.params, t, [&](int a_star, float tgt, float cur, float td) {
            bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.current[b] = cur; bt.td_abs[b] = fabsf(td);
        });
    }
    du_store(G, slabs + (size_t)blockIdx.x * PD_STRIDE, PD_NP, t);
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) pdd_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                         float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                         rg_adam_consts k, int adam) {
    rg_reduce<PD_NP, PD_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_pdd_forward(const float* params, const float* obs, int n, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && n > 0 && q, "bad arguments");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    pdd_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, n, q);
    RG_HIP(hipGetLastError());
    return MI_PDD_OK;
}

extern "C" int mi_pdd_act_steps(void* handle, const mi_pdd_ring_t* ring, const mi_pdd_act_t* a, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    DU_ACT_EPSILON(e, a, tab);
    int grid;
    const int rc = rg_act_prelude(e, ring, a->params, a->obs_cur, a->n_steps, a->max_ep, a->episodes, a->episode_stats, s, grid);
    if (rc != MI_PDD_OK) return rc;
    if (a->forced_actions || a->forced_resets)
        pdd_act_kernel<true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    else
        pdd_act_kernel<false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    RG_HIP(hipGetLastError());
    return MI_PDD_OK;
}

extern "C" int mi_pdd_target(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_PDD_OK) return rc;
    DU_CHECK_TARGET(b);
    pdd_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_PDD_OK;
}

// mi_pdd_grad (update false: opt is not looked at) and mi_pdd_update
static int pd_grad(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, const mi_pdd_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_pdd_batch_t& bt) { return bt.current && bt.target && bt.td_abs; });
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<PD_NP>(pdd_grad_kernel, pdd_reduce_kernel, ring, b, pd_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_pdd_grad(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, void* stream) { return pd_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_pdd_update(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, const mi_pdd_adam_t* opt, void* stream) {
    return pd_grad(ring, b, opt, true, (hipStream_t)stream);
}
