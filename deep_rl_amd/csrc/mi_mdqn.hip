// mi_mdqn.hip — libmirl_mdqn.so: Munchausen DQN on CartPole-v1 for gfx950.  C ABI and numerics contract: include/mi_mdqn.h.
//
// The form of mi_ddqn.hip, mirrored: one 256-thread workgroup evaluates one batch row at a time with BOTH networks' torsos in its registers (2 x 46 floats per thread,
// loaded once per launch) and both two-row heads in LDS, and evaluates the three torsos of a row — online at obs[i], target at obs[i], target at obs[nx] — between
// the same three barriers.  Every thread then forms the action values and the soft-max quantities itself from workgroup-uniform LDS broadcasts, so the Munchausen
// target costs no barrier of its own.
//   mdqn_grad_kernel     a workgroup walks its batch rows: pass 1 on the target network (its log-policy of the stored action at obs[i] -> bonus, its soft value at
//                        obs[nx] -> soft_value / next_actions / target), pass 2 on obs[i] (online forward -> current, loss, backward into register accumulators) — one
//                        slab per workgroup.
//   mdqn_reduce_kernel   fixed-order slab sum (+ Adam).
//   mdqn_target_kernel   pass 1 alone.
// No acting and no forward kernel: those are libmirl_ddqn.so's.  The torso is mi_torso.h's; the head, the three evaluations of a row and pass 2 of a gradient row
// are mi_qhead.h's, shared with mi_ddqn.hip; the host side of the gradient entry points is mi_ring.h's.  All arithmetic on the VALU in fp32 with the summation
// orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_qhead.h"

#include "../../include/mi_mdqn.h"

static_assert(MI_MD_OK == RG_OK && MI_MD_EINVAL == RG_EINVAL && MI_MD_EHIP == RG_EHIP, "mi_ring.h returns these");
static_assert(MI_MD_W1 == TS_W1 && MI_MD_B1 == TS_B1 && MI_MD_W2 == TS_W2 && MI_MD_B2 == TS_B2 && MI_MD_H1 == TS_H1 && MI_MD_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_MD_W3 == QH_W3 && MI_MD_B3 == QH_B3 && MI_MD_NPARAMS == QH_NP && MI_MD_SLAB_STRIDE == QH_STRIDE, "mi_qhead.h holds this head");

#ifndef MI_MD_SOURCE_ID
#define MI_MD_SOURCE_ID "unknown"
#endif
extern "C" int mi_md_version(void) { return MI_MD_VERSION; }
extern "C" const char* mi_md_last_error(void) { return rg_err; }
extern "C" const char* mi_md_source_id(void) { return MI_MD_SOURCE_ID; }
static int md_slabs(int batch) { return rg_slabs(batch, MI_MD_MAX_SLABS); }
extern "C" size_t mi_md_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)md_slabs(batch) * QH_STRIDE * sizeof(float);
}

// the evaluations a workgroup keeps beside QH_ROW (the online network at obs[i]): TROW the target network at obs[i], TGT the target network at obs[nx]
enum { MD_TROW = 1, MD_TGT = 2 };

// the soft-max quantities of (q0, q1) (mi_mdqn.h): v the maximum, u0 / u1 the scaled distances to it, lse = ln(e^u0 + e^u1); -ffp-contract=off keeps every
// product and sum its own
__device__ __forceinline__ void md_softmax(float q0, float q1, float it, float& v, float& u0, float& u1, float& lse) {
    v = fmaxf(q0, q1);
    u0 = (q0 - v) * it;
    u1 = (q1 - v) * it;
    lse = logf(expf(u0) + expf(u1));
}

// pass 1 of a row whose evaluations MD_TROW / MD_TGT are in sm, all through the TARGET head (every thread holds every result)
struct md_row_target { float bonus, soft, tgt; int next_action; };
__device__ __forceinline__ md_row_target md_target_value(const qh_smem& sm, int a, float r, float lg, float alpha, float tau, float it, float clip_lo) {
    md_row_target o;
    float q0, q1, v, u0, u1, lse;
    qh_values(sm, MD_TROW, QH_TARGET, q0, q1);
    md_softmax(q0, q1, it, v, u0, u1, lse);
    const float slp = tau * ((a ? u1 : u0) - lse);
    o.bonus = fminf(fmaxf(slp, clip_lo), 0.0f);
    qh_values(sm, MD_TGT, QH_TARGET, q0, q1);
    md_softmax(q0, q1, it, v, u0, u1, lse);
    o.soft = v + tau * lse;
    o.next_action = qh_argmax(q0, q1);
    o.tgt = (r + alpha * o.bonus) + lg * o.soft;
    return o;
}

__global__ void __launch_bounds__(256) mdqn_target_kernel(mi_md_ring_t ring, mi_md_batch_t bt) {
    __shared__ qh_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso tg;
    ts_load(tg, bt.target_params, t);
    qh_load_head(sm, QH_TARGET, bt.target_params, t);
    const float it = 1.0f / bt.tau;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = qh_clamp_index(bt.idx[b], total);
        const long long nx = qh_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        qh_torso_rows<false, true>(tg, xi, tg, xi, tg, xn, sm, t);
        const md_row_target o = md_target_value(sm, a, r, lg, bt.alpha, bt.tau, it, bt.clip_lo);
        if (t == 0) { bt.next_actions[b] = o.next_action; bt.target[b] = o.tgt; bt.bonus[b] = o.bonus; bt.soft_value[b] = o.soft; }
        // no barrier here: sm.h2 is next written behind two barriers of the next qh_torso_rows, which no wave passes before all have read it
    }
}

__global__ void __launch_bounds__(256) mdqn_grad_kernel(mi_md_ring_t ring, mi_md_batch_t bt, float* __restrict__ slabs) {
    __shared__ qh_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;   // the target network is loaded once and serves both of its passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    qh_load_head(sm, QH_ONLINE, bt.params, t);
    qh_load_head(sm, QH_TARGET, bt.target_params, t);
    qh_grads G;
    qh_zero(G);
    const float inv = 1.0f / (float)bt.batch;
    const float it = 1.0f / bt.tau;
    const float* __restrict__ P = bt.params;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        const long long nx = qh_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        qh_torso_rows<true, true>(on, xi, tg, xi, tg, xn, sm, t);
        // ---- pass 1, the target network: the stored action's clipped log-policy at obs[i], the soft value at obs[nx] ----
        const md_row_target o = md_target_value(sm, a, r, lg, bt.alpha, bt.tau, it, bt.clip_lo);
        // ---- pass 2, obs[i]: the stored action's online value, the loss, the backward into register accumulators ----
        qh_grad_row(G, sm, a, o.tgt, inv, xi, P, t, [&](float cur, float) {
            bt.next_actions[b] = o.next_action; bt.target[b] = o.tgt; bt.bonus[b] = o.bonus; bt.soft_value[b] = o.soft; bt.current[b] = cur;
        });
    }
    qh_store(G, slabs + (size_t)blockIdx.x * QH_STRIDE, t);
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) mdqn_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                          float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                          rg_adam_consts k, int adam) {
    rg_reduce<QH_NP, QH_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
// the three hyper-parameters: tau and its reciprocal finite and positive (a subnormal tau would make 0 * inf of a tie), alpha finite, clip_lo <= 0 (NaN fails all)
template <class BATCH>
static int md_check_knobs(const BATCH* b) {
    RG_CHECK_ARG(b->tau > 0.0f && std::isfinite(b->tau) && std::isfinite(1.0f / b->tau), "tau must be > 0 and finite, and so must 1 / tau");
    RG_CHECK_ARG(std::isfinite(b->alpha), "alpha must be finite");
    RG_CHECK_ARG(b->clip_lo <= 0.0f, "clip_lo must be <= 0");
    return RG_OK;
}

extern "C" int mi_md_target(const mi_md_ring_t* ring, const mi_md_batch_t* b, void* stream) {
    int rc = rg_check_ring(ring);
    if (rc != MI_MD_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->target_params && b->idx && b->next_actions && b->target && b->bonus && b->soft_value && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->target_params), "target_params must be 16-byte aligned");
    rc = md_check_knobs(b);
    if (rc != MI_MD_OK) return rc;
    mdqn_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_MD_OK;
}

// mi_md_grad (update false: opt is not looked at) and mi_md_update
static int md_grad(const mi_md_ring_t* ring, const mi_md_batch_t* b, const mi_md_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_md_batch_t& bt) { return bt.current && bt.target && bt.bonus && bt.soft_value; });
    if (rc == RG_OK) rc = md_check_knobs(b);
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<QH_NP>(mdqn_grad_kernel, mdqn_reduce_kernel, ring, b, md_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_md_grad(const mi_md_ring_t* ring, const mi_md_batch_t* b, void* stream) { return md_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_md_update(const mi_md_ring_t* ring, const mi_md_batch_t* b, const mi_md_adam_t* opt, void* stream) {
    return md_grad(ring, b, opt, true, (hipStream_t)stream);
}
