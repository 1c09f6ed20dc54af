// mi_nstep.hip — libmirl_nstep.so: n-step returns under prioritized dueling Double DQN on CartPole-v1 for gfx950.  C ABI and numerics contract: include/mi_nstep.h
// (and include/mi_pdd.h, which it refers to for everything but the target).
//
// The form of mi_pdd.hip: one 256-thread workgroup evaluates one batch row at a time with BOTH networks' torsos in its registers, the two 255-element dueling heads
// in LDS, and a row's three torso evaluations — online at obs[i], online at obs[s_m], target at obs[s_m] — between the same three barriers; the head's gradient is
// ONE accumulator per thread.  The kernels differ from mi_pdd.hip's only in where xn, r and lg come from: the walk of mi_nwalk.h, computed ahead of the row's first
// barrier by the two waves that need the bootstrap observation there (lane k loads step k + 1: one flag load and one reward load per walk; the observation at s_m is
// the one dependent load) and handed to the other waves through three LDS words that the row's first barrier publishes — it adds no barrier — and in the int32
// horizon they write out.  (The walk in every thread, with its 2 x 16 unrolled loads, spilled to scratch beside the two resident torsos: mi_nwalk.h.)
//   ns_target_kernel   pass 1 alone.
//   ns_grad_kernel     a workgroup walks its batch rows: the ring walk, pass 1 on obs[s_m], pass 2 on obs[i] — one slab per workgroup.
//   ns_reduce_kernel   fixed-order slab sum (+ Adam).
// There is no acting and no forward kernel: n-step returns change neither, an engine acts and evaluates through libmirl_pdd.so.
// The dueling head in LDS, the three-evaluation torso rows, the action values, the gradient row, the slab epilogue and the walk's hand-off (du_walk_row) are
// mi_dueling.h's, shared with mi_pdd.hip and mi_noisy.hip.  The torso's layout, loader, per-thread pieces, backward and slab store are mi_torso.h's; the host side
// of the gradient entry points is mi_ring.h's.  All arithmetic on the VALU in fp32 with the summation orders of mi_pdd.h; no floating-point atomics, no inline
// assembly, no device-wide hand-off inside a launch.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"
#include "mi_nwalk.h"
#include "mi_dueling.h"

#include "../../include/mi_nstep.h"

#define PD_NP MI_NS_NPARAMS
#define PD_STRIDE MI_NS_SLAB_STRIDE
static_assert(MI_NS_OK == RG_OK && MI_NS_EINVAL == RG_EINVAL && MI_NS_EHIP == RG_EHIP, "mi_ring.h returns these");
static_assert(MI_NS_W1 == TS_W1 && MI_NS_B1 == TS_B1 && MI_NS_W2 == TS_W2 && MI_NS_B2 == TS_B2 && MI_NS_H1 == TS_H1 && MI_NS_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_NS_WV == DU_HEAD + DU_WV && MI_NS_BV == DU_HEAD + DU_BV && MI_NS_WA == DU_HEAD + DU_WA && MI_NS_BA == DU_HEAD + DU_BA && PD_NP == DU_HEAD + DU_NHEAD,
              "mi_dueling.h holds this head");
static_assert(PD_STRIDE % 4 == 0 && PD_STRIDE > PD_NP, "float4 stores");
static_assert(MI_NS_MAX_N == NW_MAX_N, "mi_nwalk.h walks this far");

#ifndef MI_NS_SOURCE_ID
#define MI_NS_SOURCE_ID "unknown"
#endif
extern "C" int mi_ns_version(void) { return MI_NS_VERSION; }
extern "C" const char* mi_ns_last_error(void) { return rg_err; }
extern "C" const char* mi_ns_source_id(void) { return MI_NS_SOURCE_ID; }
static int ns_slabs(int batch) { return rg_slabs(batch, MI_NS_MAX_SLABS); }
extern "C" size_t mi_ns_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)ns_slabs(batch) * PD_STRIDE * sizeof(float);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
__global__ void __launch_bounds__(256) ns_target_kernel(mi_ns_ring_t ring, mi_ns_batch_t bt) {
    __shared__ du_smem sm;
    __shared__ du_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
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
        const float4 xn = du_walk_row(ring, bt, i, total, wk[par], t);
        du_torso_rows<false, true>(on, tg, xn, xn, sm, t);
        int a_star; float tgt;
        du_target_value(sm, wk[par].R, wk[par].lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.horizon[b] = wk[par].m; }
        par ^= 1;
    }
}

__global__ void __launch_bounds__(256) ns_grad_kernel(mi_ns_ring_t ring, mi_ns_batch_t bt, float* __restrict__ slabs) {
    __shared__ du_smem sm;
    __shared__ du_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
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
        const float4 xn = du_walk_row(ring, bt, i, total, wk[par], t);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float wb = bt.weights ? bt.weights[b] : 1.0f;
        du_grad_row(G, sm, on, tg, xi, xn, a, wk[par].R, wk[par].lg, wb, inv, he, bt.params, t, [&](int a_star, float tgt, float cur, float td) {
            bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.current[b] = cur; bt.td_abs[b] = fabsf(td); bt.horizon[b] = wk[par].m;
        });
        par ^= 1;
    }
    du_store(G, slabs + (size_t)blockIdx.x * PD_STRIDE, PD_NP, t);
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) ns_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                        float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                        rg_adam_consts k, int adam) {
    rg_reduce<PD_NP, PD_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_ns_target(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_NS_OK) return rc;
    DU_CHECK_TARGET(b);
    DU_CHECK_WALK(ring, b);
    ns_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_NS_OK;
}

// mi_ns_grad (update false: opt is not looked at) and mi_ns_update
static int ns_grad(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, const mi_ns_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_ns_batch_t& bt) { return bt.current && bt.target && bt.td_abs; });
    if (rc != RG_OK) return rc;
    DU_CHECK_WALK(ring, b);
    if (update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<PD_NP>(ns_grad_kernel, ns_reduce_kernel, ring, b, ns_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_ns_grad(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, void* stream) { return ns_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_ns_update(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, const mi_ns_adam_t* opt, void* stream) {
    return ns_grad(ring, b, opt, true, (hipStream_t)stream);
}
