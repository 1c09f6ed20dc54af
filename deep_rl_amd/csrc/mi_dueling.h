// mi_dueling.h — the dueling head and the batch row of the gradient launch as one 256-thread workgroup holds them, shared by mi_pdd.hip, mi_nstep.hip and
// mi_noisy.hip: the head's layout, the LDS state of a row's three torso evaluations, the head loader, the two action values, the argmax, the pass-1 target value,
// what head element a thread owns, ONE gradient row (pass 1, pass 2, loss term, head gradient, dz2, the torso's backward), the slab epilogue, the hand-off of the
// n-step walk (for a library that included mi_nwalk.h ahead of this header) and the host-side argument checks the three libraries have in common.  Every
// `__global__`, every C entry point, the noise and each library's own output stores stay in the library; nothing here knows which library includes it and nothing
// is exported: every entity is static or inline, and the host pieces are macros because RG_CHECK_ARG names the entry point it stands in.
// Each library static_asserts its own MI_X_WV .. BA against the offsets below.  Every sum keeps the order include/mi_pdd.h states; FMAs are explicit.
#pragma once
#include "mi_torso.h"

#define DU_HEAD 10764          // the head's first element: Wv[84] bv Wa[2][84] ba[2] behind the torso
#define DU_NHEAD 255
#define DU_WV 0                // offsets inside the head
#define DU_BV 84
#define DU_WA 85
#define DU_BA 253
static_assert(DU_HEAD == TS_B2 + TS_H2 && DU_BV == DU_WV + TS_H2 && DU_WA == DU_BV + 1 && DU_BA == DU_WA + 2 * TS_H2 && DU_NHEAD == DU_BA + 2, "the head");
static_assert(DU_NHEAD <= 256, "one head element per thread");

// ---- the network as one workgroup holds it ------------------------------------------------------------
// the evaluations a workgroup keeps side by side: ROW the online network at obs[i], NEXT the online network at the bootstrap observation, TGT the target network there
enum { DU_ROW = 0, DU_NEXT = 1, DU_TGT = 2, DU_EVALS = 3 };
enum { DU_ONLINE = 0, DU_TARGET = 1 };
// SM below is this struct or one derived from it
struct du_smem {
    float h1[DU_EVALS][TS_H1];
    float p2[DU_EVALS][3][TS_H2];       // layer 2's partial chains
    float h2[DU_EVALS][TS_H2];
    float hd[2][256];                   // [network]: the head in parameter order (DU_WV, DU_BV, DU_WA, DU_BA); element 255 is never touched
    float dz2[TS_H2];
    float ph[2][TS_H1];                 // the backward's partial chains of dh1
};

// the head of the parameters P into sm.hd[net], element by element (it starts at an odd offset); the caller's next barrier (every torso evaluation has three)
// publishes it
template <class SM>
__device__ __forceinline__ void du_load_head(SM& sm, int net, const float* __restrict__ P, int t) {
    if (t < DU_NHEAD) sm.hd[net][t] = P[DU_HEAD + t];
}

// layers 1 and 2: with ROW the online torso `on` at xi (-> sm.h1 / sm.h2 [DU_ROW]), with NEXT the online torso at xn (-> [DU_NEXT]) and the target torso `tg` at xn
// (-> [DU_TGT]), all between the same three barriers; the results are valid for every thread when it returns
template <bool ROW, bool NEXT, class SM>
__device__ __forceinline__ void du_torso_rows(const ts_torso& on, const ts_torso& tg, const float4 xi, const float4 xn, SM& sm, int t) {
    if (t < TS_H1) {
        if (ROW) sm.h1[DU_ROW][t] = ts_h1(on, xi);
        if (NEXT) { sm.h1[DU_NEXT][t] = ts_h1(on, xn); sm.h1[DU_TGT][t] = ts_h1(tg, xn); }
    }
    __syncthreads();
    if (t < 3 * TS_H2) {
        const int c = t / TS_H2, o = t - c * TS_H2;
        if (ROW) sm.p2[DU_ROW][c][o] = ts_p2(on, &sm.h1[DU_ROW][TS_W2C * c]);
        if (NEXT) { sm.p2[DU_NEXT][c][o] = ts_p2(on, &sm.h1[DU_NEXT][TS_W2C * c]); sm.p2[DU_TGT][c][o] = ts_p2(tg, &sm.h1[DU_TGT][TS_W2C * c]); }
    }
    __syncthreads();
    if (t < TS_H2) {
        if (ROW) sm.h2[DU_ROW][t] = ts_h2(sm.p2[DU_ROW], t);
        if (NEXT) { sm.h2[DU_NEXT][t] = ts_h2(sm.p2[DU_NEXT], t); sm.h2[DU_TGT][t] = ts_h2(sm.p2[DU_TGT], t); }
    }
    __syncthreads();
}

// THE two action values (mi_pdd.h) of evaluation `ev` through the head sm.hd[net], in every thread (three independent chains; the reads are workgroup-uniform
// broadcasts)
template <class SM>
__device__ __forceinline__ void du_values(const SM& sm, int ev, int net, float& q0, float& q1) {
    const float* const hd = sm.hd[net];
    float v = hd[DU_BV], a0 = hd[DU_BA], a1 = hd[DU_BA + 1];
#pragma unroll
    for (int k = 0; k < TS_H2; ++k) {
        const float h = sm.h2[ev][k];
        v = __builtin_fmaf(hd[DU_WV + k], h, v);
        a0 = __builtin_fmaf(hd[DU_WA + k], h, a0);
        a1 = __builtin_fmaf(hd[DU_WA + TS_H2 + k], h, a1);
    }
    const float m = (a0 + a1) * 0.5f;
    q0 = v + (a0 - m);
    q1 = v + (a1 - m);
}
__device__ __forceinline__ int du_argmax(float q0, float q1) { return q1 > q0 ? 1 : 0; }   // torch.argmax: the first index on a tie

// pass 1 of a row whose evaluations DU_NEXT / DU_TGT are in sm: a* by the online head, the target network's value of a* (every thread holds both); r is the reward
// (the walk's reward sum R), lg the bootstrap's factor
template <class SM>
__device__ __forceinline__ void du_target_value(const SM& sm, float r, float lg, int& a_star, float& tgt) {
    float q0, q1, t0, t1;
    du_values(sm, DU_NEXT, DU_ONLINE, q0, q1);
    du_values(sm, DU_TGT, DU_TARGET, t0, t1);
    a_star = du_argmax(q0, q1);
    tgt = r + lg * (a_star ? t1 : t0);   // -ffp-contract=off: a product, then a sum
}

// ---- the gradient launch --------------------------------------------------------------------------------
// what head element t is: a value weight, the value bias, an advantage weight of action `act`, or an advantage bias of action `act`; k its h2 index
struct du_elem { bool is_wv, is_bv, is_wa, is_ba; int act, k; };
__device__ __forceinline__ du_elem du_classify(int t) {
    du_elem h;
    const int rel = t - DU_WA;
    h.is_wv = t < DU_BV; h.is_bv = t == DU_BV; h.is_wa = t >= DU_WA && t < DU_BA; h.is_ba = t >= DU_BA && t < DU_NHEAD;
    h.act = h.is_wa ? rel / TS_H2 : t - DU_BA;
    h.k = h.is_wv ? t : (h.is_wa ? rel - h.act * TS_H2 : 0);
    return h;
}
// a workgroup's register accumulators: the torso's, the gradient of head element t (t < 255) and, in thread 0, the loss
struct du_grads { ts_grads g; float gh, loss; };
__device__ __forceinline__ void du_zero(du_grads& G) { G.gh = 0.0f; G.loss = 0.0f; ts_zero(G.g); }

// One batch row into G: the three torso evaluations; pass 1 on xn (the online argmax a*, the target network's value of it); pass 2 on xi (the stored action a's
// online value, td, the weighted loss term); the head's gradient; dz2; the torso's backward.  r and lg are READ BEHIND the torso's barriers, so they may lie in LDS
// words that the row's first barrier publishes (the walk's hand-off below).  Thread 0 calls store(a_star, tgt, cur, td) where a row's outputs are written.
// `he` is du_classify(t), `inv` 1 / batch, `wb` the row's weight, P the online parameters.  Six barriers (the torso rows' three, one behind dz2, ts_backward's
// two), the last ends it: sm's h1 / ph / dz2 are then the next row's.
template <class SM, class STORE>
__device__ __forceinline__ void du_grad_row(du_grads& G, SM& sm, const ts_torso& on, const ts_torso& tg, const float4 xi, const float4 xn, int a, const float& r,
                                            const float& lg, float wb, float inv, const du_elem& he, const float* __restrict__ P, int t, STORE store) {
    du_torso_rows<true, true>(on, tg, xi, xn, sm, t);
    // ---- pass 1, xn: the online argmax, the target network's value of it ----
    int a_star; float tgt;
    du_target_value(sm, r, lg, a_star, tgt);
    // ---- pass 2, xi: the stored action's online value, |td|, the weighted loss, the backward into register accumulators ----
    float c0, c1;
    du_values(sm, DU_ROW, DU_ONLINE, c0, c1);
    const float cur = a ? c1 : c0;
    const float td = tgt - cur;
    const float d = -(((2.0f * td) * wb) * inv);
    const float e = 0.5f * d;
    if (t == 0) {
        store(a_star, tgt, cur, td);
        G.loss += wb * (td * td);
    }
    // the head: q_a = v + 0.5 A_a - 0.5 A_{1 - a}
    {
        const float h = sm.h2[DU_ROW][he.k];
        const float es = he.act == a ? e : -e;
        if (he.is_wv) G.gh = __builtin_fmaf(d, h, G.gh);
        else if (he.is_wa) G.gh = __builtin_fmaf(es, h, G.gh);
        else if (he.is_bv) G.gh += d;
        else if (he.is_ba) G.gh += es;
    }
    if (t < TS_H2) {
        const float* const hd = sm.hd[DU_ONLINE];
        const float wa_a = hd[DU_WA + a * TS_H2 + t], wa_o = hd[DU_WA + (1 - a) * TS_H2 + t];
        sm.dz2[t] = sm.h2[DU_ROW][t] > 0.0f ? (d * hd[DU_WV + t]) + (e * (wa_a - wa_o)) : 0.0f;
    }
    __syncthreads();
    ts_backward(G.g, sm.h1[DU_ROW], sm.dz2, sm.ph, xi, P, t);
}

// the workgroup's slab: the head's 255 elements, the torso, the loss at element `np`
__device__ __forceinline__ void du_store(const du_grads& G, float* __restrict__ slab, int np, int t) {
    if (t < DU_NHEAD) slab[DU_HEAD + t] = G.gh;
    ts_store(G.g, slab, t);
    if (t == 0) slab[np] = G.loss;
}

// ---- the walk's hand-off (mi_nwalk.h, included ahead of this header by the libraries that walk) -----------
#ifdef NW_MAX_N
// what the walk of a row hands to the waves that do not compute it
struct du_walk_lds { float R, lg; int m; int pad; };
// The walk of ring row i (mi_nwalk.h) in waves 0 and 1 — the waves whose threads t < TS_H1 read the bootstrap observation in layer 1 — and that observation, the
// one dependent load, for them (the other waves get zeros and never look at them).  Thread 0 leaves R, lg and m in `out`, which the first of the row's three torso
// barriers publishes; every thread reads them behind the third.  `out` alternates between two copies from row to row: a wave that is already past row b's last
// barrier writes the other copy, and the copy of row b is next written behind the three barriers of row b + 1, which no wave passes before all have read it.
template <class RING, class BATCH>
__device__ __forceinline__ float4 du_walk_row(const RING& ring, const BATCH& bt, long long i, long long total, du_walk_lds& out, int t) {
    float4 xn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t < 128) {
        const nw_walk_t w = nw_walk(ring, i, total, bt.n_step, bt.head_slot, bt.gamma);
        xn = reinterpret_cast<const float4*>(ring.observations)[w.at];
        if (t == 0) { out.R = w.R; out.lg = w.lg; out.m = w.m; }
    }
    return xn;
}
// the members only the walk needs
#define DU_CHECK_WALK(ring, b)                                                                                                                      \
    do {                                                                                                                                            \
        RG_CHECK_ARG((b)->horizon != nullptr, "horizon is NULL");                                                                                   \
        RG_CHECK_ARG((b)->n_step >= 1 && (b)->n_step <= NW_MAX_N && (int64_t)(b)->n_step < (ring)->slots, "n_step must be in [1, 16] and below slots"); \
        RG_CHECK_ARG((b)->head_slot >= 0 && (b)->head_slot < (ring)->slots, "head_slot outside [0, slots)");                                        \
    } while (0)
#endif

// ---- host: the checks of mi_x_target's batch and the epsilon table of mi_x_act_steps (mi_ring.h's RG_CHECK_ARG: they return from the entry point) -------------
#define DU_CHECK_TARGET(b)                                                                                                                          \
    do {                                                                                                                                            \
        RG_CHECK_ARG((b) != nullptr, "batch is NULL");                                                                                              \
        RG_CHECK_ARG((b)->params && (b)->target_params && (b)->idx && (b)->next_actions && (b)->target && (b)->batch > 0, "bad arguments");         \
        RG_CHECK_ARG(rg_aligned((b)->params) && rg_aligned((b)->target_params), "params and target_params must be 16-byte aligned");                \
    } while (0)
// the handle e, the act arguments a and the schedule; tab: epsilon(global_step + k) rounded to f32, as DQN compares the draw with epsilon (mi_dqn_act_steps)
#define DU_ACT_EPSILON(e, a, tab)                                                                                                                   \
    do {                                                                                                                                            \
        RG_CHECK_ARG((e) != nullptr && (a) != nullptr, "NULL pointer");                                                                             \
        RG_CHECK_ARG((a)->global_step >= 0 && (a)->total_timesteps > 0 && (a)->exploration_fraction > 0.0,                                          \
                     "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");                                                         \
        RG_CHECK_ARG((a)->learning_starts >= 0, "learning_starts < 0");                                                                             \
        rg_eps_fill(tab, (a)->global_step, ((a)->end_e - (a)->start_e) / ((a)->exploration_fraction * (double)(a)->total_timesteps), (a)->start_e, (a)->end_e); \
        for (int k_ = 0; k_ < RG_MAX_STEPS; ++k_) (tab).v[k_] = (double)(float)(tab).v[k_];                                                         \
    } while (0)
