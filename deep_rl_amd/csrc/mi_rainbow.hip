// mi_rainbow.hip — libmirl_rainbow.so: Rainbow (distributional noisy n-step dueling Double DQN with the row loss as the replay priority) on CartPole-v1 for gfx950.
// C ABI, numerics and RNG contract: include/mi_rainbow.h.
//
// One 256-thread workgroup evaluates one row at a time.  The torso is mi_torso.h's register layout; thread r < 153 owns head ROW r (51 value rows, 2 x 51 advantage
// rows): its 84 effective weights and its bias in registers, as mi_c51.hip holds W3.  A noise sample's 321 factors are drawn by the workgroup (thread t draws c = t
// and c = t + 256: at most two Philox calls) into LDS, because a row owner needs all 84 input factors of its stream; the owner then forms mu + sigma * (fout * fin_k).
//   rb_act_kernel      rg_act_loop as it is, instantiated with and without the noise.  The row owner keeps mu and sigma (2 x 84 registers) and forms the effective
//                      weight inside the 84-term chain of every greedy step; the step's draw is published by the torso's three barriers.
//   rb_forward_kernel  probs / q of n observations under one sample, or the mean network.
//   rb_target_kernel   passes 1 and 2 below.
//   rb_grad_kernel     a workgroup walks its batch rows in THREE passes with one network resident each (mi_c51.hip's two passes and the double rule's extra one):
//                      1. online at obs[s_m]: a* -> next_actions, horizon;  2. target at obs[s_m]: the projection -> target_probs;  3. online at obs[i]: forward,
//                      loss, backward into register accumulators.  The effective rows are formed once per pass; eps is recomputed from the LDS factors at the slab
//                      store.  dh2 needs a COLUMN of the effective head: it is recomputed from mu, sigma (memory, consecutive threads consecutive addresses) and the
//                      LDS factors with the expression that formed the rows.
//   rb_reduce_kernel   fixed-order slab sum (+ Adam) over 36,774 elements.
//   rb_noise_kernel    one sample written out as the kernels form it (the tests' view of the draw).
// Head rows start at offsets that are not all multiples of 4 (Wa's means at 15,099, Wv's sigmas at 23,769): a row is read as 22 aligned float4s around it and taken
// out at a compile-time shift.  rb_normal / rb_xi are copies of mi_noisy.hip's expressions (that library's source is pinned by its id) with the counter b * 512 + c.
// All arithmetic on the VALU in fp32; no floating-point atomics, no inline assembly, no device-wide hand-off inside a launch.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"
#include "mi_nwalk.h"

#include "../../include/mi_rainbow.h"

#include <math.h>

#define RB_H1 MI_RB_H1
#define RB_H2 MI_RB_H2
#define RB_NA MI_RB_N_ATOMS
#define RB_NR MI_RB_NROWS                     // 153 head rows
#define RB_HEAD MI_RB_WV
#define RB_SIGMA MI_RB_SIGMA
#define RB_BV (MI_RB_BV - MI_RB_WV)           // offsets inside the head
#define RB_WA (MI_RB_WA - MI_RB_WV)
#define RB_BA (MI_RB_BA - MI_RB_WV)
#define RB_NP MI_RB_NPARAMS
#define RB_STRIDE MI_RB_SLAB_STRIDE
#define RB_XI_VIN 0                           // the meaning of c
#define RB_XI_VOUT RB_H2
#define RB_XI_AIN (RB_H2 + RB_NA)
#define RB_XI_AOUT (2 * RB_H2 + RB_NA)
static_assert(MI_RB_OK == RG_OK && MI_RB_EINVAL == RG_EINVAL && MI_RB_EHIP == RG_EHIP && MI_RB_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_RB_W1 == TS_W1 && MI_RB_B1 == TS_B1 && MI_RB_W2 == TS_W2 && MI_RB_B2 == TS_B2 && MI_RB_H1 == TS_H1 && MI_RB_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_RB_WV == TS_B2 + TS_H2 && MI_RB_BV == MI_RB_WV + RB_NA * RB_H2 && MI_RB_WA == MI_RB_BV + RB_NA && MI_RB_BA == MI_RB_WA + 2 * RB_NA * RB_H2, "the head");
static_assert(MI_RB_SIGMA == MI_RB_BA + 2 * RB_NA && MI_RB_NHEAD == MI_RB_SIGMA - MI_RB_WV && RB_NP == MI_RB_SIGMA + MI_RB_NHEAD, "mu and then sigma");
static_assert(RB_NR == 3 * RB_NA && RB_NR <= 256 && RB_NA <= 64, "one head row per thread, one atom per lane");
static_assert(MI_RB_NXI == RB_XI_AOUT + 2 * RB_NA && MI_RB_NXI <= 512, "b * 512 + c keys them; two draws per thread at the most");
static_assert(RB_STRIDE % 4 == 0 && RB_STRIDE > RB_NP, "float4 stores");
static_assert(MI_RB_MAX_N == NW_MAX_N, "mi_nwalk.h walks this far");
static_assert(MI_RB_STREAM_ACT < 16 && MI_RB_STREAM_LEARN < 16, "the stream tag has 4 bits");

#ifndef MI_RB_SOURCE_ID
#define MI_RB_SOURCE_ID "unknown"
#endif
extern "C" int mi_rb_version(void) { return MI_RB_VERSION; }
extern "C" const char* mi_rb_last_error(void) { return rg_err; }
extern "C" const char* mi_rb_source_id(void) { return MI_RB_SOURCE_ID; }
static int rb_slabs(int batch) { return rg_slabs(batch, MI_RB_MAX_SLABS); }
extern "C" size_t mi_rb_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)rb_slabs(batch) * RB_STRIDE * sizeof(float);
}

// ---- the noise ----------------------------------------------------------------------------------------
struct rb_key { uint64_t seed, a, b; uint32_t stream; };
// z_c of the sample `k`: mi_noisy.hip's expression, the counter b * 512 + c
__device__ __forceinline__ float rb_normal(const rb_key& k, int c) {
    uint32_t r[4];
    mi_philox(k.seed, k.a, k.b * 512ull + (uint64_t)c, k.stream, r);
    const float u1 = ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}
// xi_c = sgn(z) * sqrtf(|z|)
__device__ __forceinline__ float rb_xi(const rb_key& k, int c) {
    const float z = rb_normal(k, c);
    const float s = sqrtf(fabsf(z));
    return z > 0.0f ? s : (z < 0.0f ? -s : 0.0f);
}
#define RB_XI_LEN 324
// the sample's 321 factors into xi[]; the caller's next barrier publishes them
__device__ __forceinline__ void rb_draw(float* xi, const rb_key& k, int t) {
    xi[t] = rb_xi(k, t);
    if (t + 256 < MI_RB_NXI) xi[t + 256] = rb_xi(k, t + 256);
}

// ---- the network as one workgroup holds it -----------------------------------------------------------
struct rb_smem {
    float h1[RB_H1];
    float p2[3][RB_H2];                 // layer 2's partial chains; the backward's partial chains of dh2
    float h2[RB_H2];
    float xi[2][RB_XI_LEN];             // [network] the sample's factors (acting: one sample, redrawn per greedy step)
    float y[RB_NR + 3];                 // the head rows' outputs: v[51], A[0][51], A[1][51]
    float q[2];
    float rowloss;
    float R, lg; int m;                 // the walk's result
    float wl[RB_NA], wu[RB_NA];         // the projection's image
    int li[RB_NA], ui[RB_NA];
    float dl[RB_NA];                    // dlogit of the stored action
    float dz2[RB_H2];
    float ph[2][RB_H1];                 // the backward's partial chains of dh1
};
// where head row r lies: its weights' and its bias's offset inside the head, its input factors' first index and its output factor's index
__device__ __forceinline__ int rb_row_w(int r) { return r < RB_NA ? r * RB_H2 : RB_WA + (r - RB_NA) * RB_H2; }
__device__ __forceinline__ int rb_row_b(int r) { return r < RB_NA ? RB_BV + r : RB_BA + (r - RB_NA); }
__device__ __forceinline__ int rb_row_in(int r) { return r < RB_NA ? RB_XI_VIN : RB_XI_AIN; }
__device__ __forceinline__ int rb_row_out(int r) { return r < RB_NA ? RB_XI_VOUT + r : RB_XI_AOUT + (r - RB_NA); }

// 84 floats at P + off as 22 aligned float4s around them: off % 4 is SHV for a value row and SHA for an advantage row, and ONE code path serves both (a select
// per element; two branches kept both rows' registers alive and spilled).  Every address is inside the parameter vector: the first row starts at 10,764, the last
// ends 102 floats before its end.
template <int SHV, int SHA>
__device__ __forceinline__ void rb_load84(float (&w)[RB_H2], const float* __restrict__ P, int off, bool value) {
    const float4* src = reinterpret_cast<const float4*>(P + (off - (value ? SHV : SHA)));
    float buf[RB_H2 + 4];
#pragma unroll
    for (int k = 0; k < (RB_H2 + 4) / 4; ++k) { const float4 v = src[k]; buf[4 * k] = v.x; buf[4 * k + 1] = v.y; buf[4 * k + 2] = v.z; buf[4 * k + 3] = v.w; }
#pragma unroll
    for (int k = 0; k < RB_H2; ++k) w[k] = value ? buf[k + SHV] : buf[k + SHA];
}
static_assert(MI_RB_WV % 4 == 0 && MI_RB_WA % 4 == 3 && MI_RB_SIGMA % 4 == 1 && (MI_RB_SIGMA + RB_WA) % 4 == 0 && RB_H2 % 4 == 0, "the shifts of rb_load_mu / rb_load_sigma / rb_store84");
// the means / the sigmas of row r's weights
__device__ __forceinline__ void rb_load_mu(float (&w)[RB_H2], const float* __restrict__ P, int r) { rb_load84<0, 3>(w, P, RB_HEAD + rb_row_w(r), r < RB_NA); }
__device__ __forceinline__ void rb_load_sigma(float (&w)[RB_H2], const float* __restrict__ P, int r) { rb_load84<1, 0>(w, P, RB_SIGMA + rb_row_w(r), r < RB_NA); }

struct rb_row { float w[RB_H2]; float b; };   // thread r < 153: head row r
// the EFFECTIVE row of thread t under the factors xi (noisy == 0: the mean row, xi is not read)
__device__ __forceinline__ void rb_form_row(rb_row& row, const float* __restrict__ P, const float* xi, int noisy, int t) {
    const int r = t < RB_NR ? t : RB_NR - 1;
    rb_load_mu(row.w, P, r);
    row.b = P[RB_HEAD + rb_row_b(r)];
    if (noisy) {
        float sg[RB_H2];
        rb_load_sigma(sg, P, r);
        const float fo = xi[rb_row_out(r)];
        const float* const fin = xi + rb_row_in(r);
#pragma unroll
        for (int k = 0; k < RB_H2; ++k) row.w[k] = row.w[k] + sg[k] * (fo * fin[k]);   // -ffp-contract=off: products, then a sum
        row.b = row.b + P[RB_SIGMA + rb_row_b(r)] * fo;
    }
}

// the balanced pairwise sum over the 64 lanes in natural order, result in every lane, VALU only (mi_c51.hip's)
__device__ __forceinline__ float rb_wave_sum(float v) {
    v += dpp_xor1(v);
    v += dpp_xor2(v);
    v += dpp_half_mirror(v);
    v += dpp_mirror(v);
    return groups_sum(v);
}
__device__ __forceinline__ float rb_wave_max(float v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s));
    return v;
}
struct rb_support { float v_min, v_max, dz; };
__device__ __forceinline__ rb_support rb_make_support(float v_min, float v_max) { return rb_support{v_min, v_max, (v_max - v_min) / (float)(RB_NA - 1)}; }
__device__ __forceinline__ float rb_atom(const rb_support& z, int j) { return z.v_min + z.dz * (float)j; }   // a product, then a sum

// the head rows' outputs of sm.h2 through the resident effective rows -> sm.y; one barrier, which ends it
__device__ __forceinline__ void rb_head(const rb_row& row, rb_smem& sm, int t) {
    if (t < RB_NR) {
        float acc = row.b;
#pragma unroll
        for (int k = 0; k < RB_H2; ++k) acc = __builtin_fmaf(row.w[k], sm.h2[k], acc);
        sm.y[t] = acc;
    }
    __syncthreads();
}
// dueling combine + softmax of both actions from sm.y: wave a < 2 returns its action's p_lane (0 past atom 50); sm.q valid for every thread on return (one barrier)
__device__ __forceinline__ float rb_softmax(rb_smem& sm, const rb_support& z, int t) {
    const int wv = t >> 6, lane = t & 63;
    float p = 0.0f;
    if (wv < 2) {
        const bool valid = lane < RB_NA;
        const int j = valid ? lane : RB_NA - 1;   // the tail repeats atom 50 in the max and is 0 in every sum
        const float v = sm.y[j], a0 = sm.y[RB_NA + j], a1 = sm.y[2 * RB_NA + j];
        const float l = v + ((wv ? a1 : a0) - 0.5f * (a0 + a1));
        const float m = rb_wave_max(l);
        const float e = valid ? expf(l - m) : 0.0f;
        const float s = rb_wave_sum(e);
        p = e / s;
        const float q = rb_wave_sum(p * rb_atom(z, lane));
        if (lane == 0) sm.q[wv] = q;
    }
    __syncthreads();
    return p;
}
__device__ __forceinline__ int rb_argmax(const rb_smem& sm) { return sm.q[1] > sm.q[0] ? 1 : 0; }   // torch.argmax: the first index on a tie

// =====================================================================================================
// the sample, written out
// =====================================================================================================
__global__ void __launch_bounds__(256) rb_noise_kernel(rb_key k, float* __restrict__ xi_out, float* __restrict__ fin_out, float* __restrict__ fout_out) {
    __shared__ float xi[RB_XI_LEN];
    const int t = threadIdx.x;
    rb_draw(xi, k, t);
    __syncthreads();
    for (int c = t; c < MI_RB_NXI; c += 256) xi_out[c] = xi[c];
    if (t < RB_NR) {
        fout_out[t] = xi[rb_row_out(t)];
        for (int c = 0; c < RB_H2; ++c) fin_out[t * RB_H2 + c] = xi[rb_row_in(t) + c];
    }
}

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) rb_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, rb_key key, int noisy, float v_min,
                                                         float v_max, float* __restrict__ probs, float* __restrict__ q) {
    __shared__ rb_smem sm;
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const rb_support z = rb_make_support(v_min, v_max);
    if (noisy) {
        rb_draw(sm.xi[0], key, t);
        __syncthreads();
    }
    rb_row row;
    rb_form_row(row, params, sm.xi[0], noisy, t);
    ts_torso w;
    ts_load(w, params, t);
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[r];
        ts_row(w, x, sm, t);
        rb_head(row, sm, t);
        const float p = rb_softmax(sm, z, t);
        if (wv < 2) {
            if (probs && lane < RB_NA) probs[((size_t)r * 2 + wv) * RB_NA + lane] = p;
            if (q && lane == 0) q[2 * (size_t)r + wv] = sm.q[wv];
        }
        // no barrier here: sm.q is next written behind the four barriers of the next row
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the online torso in `w`, mu and sigma of this thread's head row in registers, the step's factors in LDS
template <bool NOISY>
struct rb_policy {
    const ts_torso& w;
    rb_smem& sm;
    int t;
    uint64_t seed;
    rb_support z;
    const float (&mu)[RB_H2];
    const float (&sg)[RB_H2];
    float bmu, bsg;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t env_id, uint64_t ctr) {
        // the last readers of sm.xi (the previous greedy step's chains) are two barriers back; ts_row's three publish the new factors
        if (NOISY) rb_draw(sm.xi[0], rb_key{seed, env_id, ctr, MI_RB_STREAM_ACT}, t);
        ts_row(w, x, sm, t);
        if (t < RB_NR) {
            float acc;
            if (NOISY) {
                const float fo = sm.xi[0][rb_row_out(t)];
                const float* const fin = sm.xi[0] + rb_row_in(t);
                acc = bmu + bsg * fo;
#pragma unroll
                for (int k = 0; k < RB_H2; ++k) acc = __builtin_fmaf(mu[k] + sg[k] * (fo * fin[k]), sm.h2[k], acc);
            } else {
                acc = bmu;
#pragma unroll
                for (int k = 0; k < RB_H2; ++k) acc = __builtin_fmaf(mu[k], sm.h2[k], acc);
            }
            sm.y[t] = acc;
        }
        __syncthreads();
        rb_softmax(sm, z, t);
        return rb_argmax(sm);   // sm.q is next written behind the next step's five barriers
    }
};

// NOISY false: the draw's code and the sigmas' registers are not in that instantiation at all
template <bool FORCED, bool NOISY>
__global__ void __launch_bounds__(256) rb_act_kernel(mi_env e, mi_rb_ring_t ring, mi_rb_act_t a_, rg_eps_tab eps) {
    __shared__ rb_smem sm;
    const int t = threadIdx.x;
    const int r = t < RB_NR ? t : RB_NR - 1;
    const float* __restrict__ P = a_.params;
    float mu[RB_H2], sg[RB_H2];
    rb_load_mu(mu, P, r);
    const float bmu = P[RB_HEAD + rb_row_b(r)];
    float bsg = 0.0f;
    if (NOISY) {
        rb_load_sigma(sg, P, r);
        bsg = P[RB_SIGMA + rb_row_b(r)];
    } else {
#pragma unroll
        for (int k = 0; k < RB_H2; ++k) sg[k] = 0.0f;   // never read
    }
    ts_torso w;
    ts_load(w, P, t);
    rb_policy<NOISY> policy{w, sm, t, e.seed, rb_make_support(a_.v_min, a_.v_max), mu, sg, bmu, bsg};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// the walk of ring row i by waves 0 and 1 (mi_nstep.hip's hand-off): the bootstrap observation for t < 128, the result in sm behind the caller's next barrier
__device__ __forceinline__ float4 rb_walk_row(const mi_rb_ring_t& ring, const mi_rb_batch_t& bt, long long i, long long total, rb_smem& sm, int t) {
    float4 xn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t < 128) {
        const nw_walk_t w = nw_walk(ring, i, total, bt.n_step, bt.head_slot, bt.gamma);
        xn = reinterpret_cast<const float4*>(ring.observations)[w.at];
        if (t == 0) { sm.R = w.R; sm.lg = w.lg; sm.m = w.m; }
    }
    return xn;
}

// pass 1, the ONLINE network resident: a* and the horizon of this workgroup's rows (and their drawn indices)
__device__ __forceinline__ void rb_pass_astar(const mi_rb_ring_t& ring, const mi_rb_batch_t& bt, const rb_support& z, int64_t upper, rb_smem& sm, int t) {
    const long long total = ring.slots * (long long)ring.n_envs;
    rb_row row;
    rb_form_row(row, bt.params, sm.xi[0], bt.noisy, t);
    ts_torso w;
    ts_load(w, bt.params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, upper, bt.idx, b, total, t == 0);
        const float4 xn = rb_walk_row(ring, bt, i, total, sm, t);
        ts_row(w, xn, sm, t);
        rb_head(row, sm, t);
        rb_softmax(sm, z, t);
        if (t == 0) { bt.next_actions[b] = rb_argmax(sm); bt.horizon[b] = sm.m; }
        // no barrier here: sm.R / sm.m / sm.q are thread 0's until then, and next written by it
    }
}

// pass 2, the TARGET network resident: the projection of its distribution of a* into target_probs
__device__ __forceinline__ void rb_pass_project(const mi_rb_ring_t& ring, const mi_rb_batch_t& bt, const rb_support& z, int64_t upper, rb_smem& sm, int t) {
    const long long total = ring.slots * (long long)ring.n_envs;
    const int wv = t >> 6, lane = t & 63;
    rb_row row;
    rb_form_row(row, bt.target_params, sm.xi[1], bt.noisy, t);
    ts_torso w;
    ts_load(w, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, upper, bt.idx, b, total, false);   // recomputed, not re-read
        const float4 xn = rb_walk_row(ring, bt, i, total, sm, t);
        const int a = bt.next_actions[b] != 0 ? 1 : 0;   // pass 1 of this workgroup wrote it
        ts_row(w, xn, sm, t);
        rb_head(row, sm, t);
        const float p = rb_softmax(sm, z, t);
        if (wv == a && lane < RB_NA) {
            const float tz = fminf(fmaxf(sm.R + sm.lg * rb_atom(z, lane), z.v_min), z.v_max);
            const float bj = (tz - z.v_min) / z.dz;
            const float l = floorf(bj), u = ceilf(bj);
            sm.li[lane] = (int)l; sm.ui[lane] = (int)u;
            sm.wl[lane] = ((u + (l == u ? 1.0f : 0.0f)) - bj) * p;
            sm.wu[lane] = (bj - l) * p;
        }
        __syncthreads();
        if (t < RB_NA) {   // per target atom: the lower contributions in ascending j, then the upper ones
            float m = 0.0f;
            for (int j = 0; j < RB_NA; ++j) if (sm.li[j] == t) m += sm.wl[j];
            for (int j = 0; j < RB_NA; ++j) if (sm.ui[j] == t) m += sm.wu[j];
            bt.target_probs[(size_t)b * RB_NA + t] = m;
        }
        __syncthreads();   // sm.R / sm.lg and the image are the next row's
    }
}

__global__ void __launch_bounds__(256) rb_target_kernel(mi_rb_ring_t ring, mi_rb_batch_t bt) {
    __shared__ rb_smem sm;
    const int t = threadIdx.x;
    const rb_support z = rb_make_support(bt.v_min, bt.v_max);
    if (bt.noisy) {
        rb_draw(sm.xi[0], rb_key{bt.sample_seed, bt.sample_update, 0, MI_RB_STREAM_LEARN}, t);
        rb_draw(sm.xi[1], rb_key{bt.sample_seed, bt.sample_update, 1, MI_RB_STREAM_LEARN}, t);
        __syncthreads();
    }
    rb_pass_astar(ring, bt, z, 0, sm, t);   // the given indices: a bad one reads a valid row, never past the ring
    __threadfence_block();   // pass 2 reads the next_actions this workgroup wrote
    __syncthreads();
    rb_pass_project(ring, bt, z, 0, sm, t);
}

// the slab store of a head row's 84 accumulators (times eps for the sigmas) at a compile-time alignment
template <int SH>
__device__ __forceinline__ void rb_store84(float* __restrict__ dst, const float (&g)[RB_H2]) {
    if (SH == 0) {
#pragma unroll
        for (int k = 0; k < RB_H2 / 4; ++k) reinterpret_cast<float4*>(dst)[k] = make_float4(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < RB_H2; ++k) dst[k] = g[k];
    }
}

__global__ void __launch_bounds__(256) rb_grad_kernel(mi_rb_ring_t ring, mi_rb_batch_t bt, float* __restrict__ slabs) {
    __shared__ rb_smem sm;
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const long long total = ring.slots * (long long)ring.n_envs;
    const rb_support z = rb_make_support(bt.v_min, bt.v_max);
    if (bt.noisy) {
        rb_draw(sm.xi[0], rb_key{bt.sample_seed, bt.sample_update, 0, MI_RB_STREAM_LEARN}, t);
        rb_draw(sm.xi[1], rb_key{bt.sample_seed, bt.sample_update, 1, MI_RB_STREAM_LEARN}, t);
        __syncthreads();
    }
    rb_pass_astar(ring, bt, z, bt.sample_upper, sm, t);
    __threadfence_block();
    __syncthreads();
    rb_pass_project(ring, bt, z, bt.sample_upper, sm, t);
    __threadfence_block();   // pass 3 reads the target_probs this workgroup wrote (rb_pass_project ends in a barrier)
    __syncthreads();
    // ---- pass 3, online network at obs[i]: forward + backward into register accumulators ----
    const float* __restrict__ P = bt.params;
    const float* const xi = sm.xi[0];
    rb_row row;
    rb_form_row(row, P, xi, bt.noisy, t);
    ts_torso w;
    ts_load(w, P, t);
    float gw[RB_H2], gb = 0.0f, loss = 0.0f;
    ts_grads g;
#pragma unroll
    for (int k = 0; k < RB_H2; ++k) gw[k] = 0.0f;
    ts_zero(g);
    const float invB = 1.0f / (float)bt.batch;
    // what this thread is in the head: row `hr` = atom hj of the value stream (hs == 0) or of action hs - 1's advantage
    const int hr = t < RB_NR ? t : RB_NR - 1;
    const int hs = hr / RB_NA, hj = hr - hs * RB_NA;
    // and in dh2: column ck of stream cs
    const int cs = (t < 3 * RB_H2 ? t : 3 * RB_H2 - 1) / RB_H2, ck = (t < 3 * RB_H2 ? t : 3 * RB_H2 - 1) - cs * RB_H2;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, false);
        const float4 x = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float wb = bt.weights ? bt.weights[b] : 1.0f;
        ts_row(w, x, sm, t);
        rb_head(row, sm, t);
        const float p = rb_softmax(sm, z, t);
        if (wv == a) {   // one wave, all lanes active
            const bool valid = lane < RB_NA;
            const float mk = valid ? bt.target_probs[(size_t)b * RB_NA + lane] : 0.0f;
            const float d = p + 1e-8f;
            const float rowloss = -rb_wave_sum(valid ? mk * logf(d) : 0.0f);
            const float gk = valid ? -mk / d : 0.0f;
            const float S = rb_wave_sum(p * gk);
            if (valid) {
                sm.dl[lane] = (p * (gk - S)) * (wb * invB);
                if (bt.probs) bt.probs[(size_t)b * RB_NA + lane] = p;
            }
            if (lane == 0) sm.rowloss = rowloss;
        }
        __syncthreads();
        if (t == 0) {
            const float rl = sm.rowloss;
            loss += wb * rl;
            bt.prio[b] = fmaxf(rl, 0.0f);
        }
        // the head: thread r owns row r of the effective head's gradient
        if (t < RB_NR) {
            const float dl = sm.dl[hj];
            const float e = 0.5f * dl;
            const float d = hs == 0 ? dl : (hs - 1 == a ? e : -e);
            gb += d;
#pragma unroll
            for (int k = 0; k < RB_H2; ++k) gw[k] = __builtin_fmaf(d, sm.h2[k], gw[k]);
        }
        // dh2: thread cs * 84 + ck sums stream cs's 51 rows of column ck; the effective column is formed again from mu, sigma and the factors
        if (t < 3 * RB_H2) {
            const int w0 = cs == 0 ? 0 : RB_WA + (cs - 1) * RB_NA * RB_H2;
            const float* const mu = P + RB_HEAD + w0 + ck;
            const float* const sg = P + RB_SIGMA + w0 + ck;
            const float fin = xi[(cs == 0 ? RB_XI_VIN : RB_XI_AIN) + ck];
            const float* const fo = xi + (cs == 0 ? RB_XI_VOUT : RB_XI_AOUT + (cs - 1) * RB_NA);
            const float sign = cs == 0 ? 1.0f : (cs - 1 == a ? 0.5f : -0.5f);   // 0.5f * dl and its negation are exact
            float acc = 0.0f;
            if (bt.noisy) {
#pragma unroll 3
                for (int j = 0; j < RB_NA; ++j) acc = __builtin_fmaf(sign * sm.dl[j], mu[(size_t)j * RB_H2] + sg[(size_t)j * RB_H2] * (fo[j] * fin), acc);
            } else {
#pragma unroll 3
                for (int j = 0; j < RB_NA; ++j) acc = __builtin_fmaf(sign * sm.dl[j], mu[(size_t)j * RB_H2], acc);
            }
            sm.p2[cs][ck] = acc;
        }
        __syncthreads();
        if (t < RB_H2) sm.dz2[t] = sm.h2[t] > 0.0f ? (sm.p2[0][t] + sm.p2[1][t]) + sm.p2[2][t] : 0.0f;
        __syncthreads();
        ts_backward(g, sm.h1, sm.dz2, sm.ph, x, P, t);
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * RB_STRIDE;
    if (t < RB_NR) {
        const int ow = rb_row_w(t), ob = rb_row_b(t);
        if (t < RB_NA) rb_store84<0>(slab + RB_HEAD + ow, gw); else rb_store84<3>(slab + RB_HEAD + ow, gw);
        slab[RB_HEAD + ob] = gb;
        float fo = 0.0f;
        if (bt.noisy) {
            fo = xi[rb_row_out(t)];
            const float* const fin = xi + rb_row_in(t);
#pragma unroll
            for (int k = 0; k < RB_H2; ++k) gw[k] = gw[k] * (fo * fin[k]);   // one product with eps, itself the product that formed the row
        } else {
#pragma unroll
            for (int k = 0; k < RB_H2; ++k) gw[k] = 0.0f;   // off: exact zeros
        }
        if (t < RB_NA) rb_store84<1>(slab + RB_SIGMA + ow, gw); else rb_store84<0>(slab + RB_SIGMA + ow, gw);
        slab[RB_SIGMA + ob] = bt.noisy ? gb * fo : 0.0f;
    }
    ts_store(g, slab, t);
    if (t == 0) { slab[RB_NP] = loss; slab[RB_NP + 1] = 0.0f; }
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) rb_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                        float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                        rg_adam_consts k, int adam) {
    rg_reduce<RB_NP, RB_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
static bool rb_support_ok(float v_min, float v_max) { return isfinite(v_min) && isfinite(v_max) && v_min < v_max && isfinite(v_max - v_min); }
#define RB_CHECK_SUPPORT(lo, hi) RG_CHECK_ARG(rb_support_ok((lo), (hi)), "the support needs finite v_min < v_max")

extern "C" int mi_rb_noise(uint64_t seed, uint64_t a, uint64_t b, uint32_t stream, float* xi_out, float* fin_out, float* fout_out, void* hip_stream) {
    RG_CHECK_ARG(xi_out && fin_out && fout_out, "xi_out, fin_out or fout_out is NULL");
    RG_CHECK_ARG(stream < 16u, "stream must be in [0, 16)");
    rb_noise_kernel<<<1, 256, 0, (hipStream_t)hip_stream>>>(rb_key{seed, a, b, stream}, xi_out, fin_out, fout_out);
    RG_HIP(hipGetLastError());
    return MI_RB_OK;
}

extern "C" int mi_rb_forward(const float* params, const float* obs, int n, const mi_rb_key_t* key, float v_min, float v_max, float* probs, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && n > 0 && (probs || q), "bad arguments");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    RG_CHECK_ARG(key == nullptr || key->stream < 16u, "the key's stream must be in [0, 16)");
    RB_CHECK_SUPPORT(v_min, v_max);
    const rb_key k = key ? rb_key{key->seed, key->a, key->b, key->stream} : rb_key{0, 0, 0, 0};
    rb_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, n, k, key ? 1 : 0, v_min, v_max, probs, q);
    RG_HIP(hipGetLastError());
    return MI_RB_OK;
}

extern "C" int mi_rb_act_steps(void* handle, const mi_rb_ring_t* ring, const mi_rb_act_t* a, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    RG_CHECK_ARG(e != nullptr && a != nullptr, "NULL pointer");
    RG_CHECK_ARG(a->global_step >= 0 && a->total_timesteps > 0 && a->exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    RG_CHECK_ARG(a->learning_starts >= 0, "learning_starts < 0");
    RB_CHECK_SUPPORT(a->v_min, a->v_max);
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, (a->end_e - a->start_e) / (a->exploration_fraction * (double)a->total_timesteps), a->start_e, a->end_e);
    for (int k = 0; k < RG_MAX_STEPS; ++k) tab.v[k] = (double)(float)tab.v[k];   // DQN compares the draw with epsilon as an f32 (mi_pdd_act_steps)
    int grid;
    const int rc = rg_act_prelude(e, ring, a->params, a->obs_cur, a->n_steps, a->max_ep, a->episodes, a->episode_stats, s, grid);
    if (rc != MI_RB_OK) return rc;
    const bool forced = a->forced_actions || a->forced_resets;
    if (a->noisy) {
        if (forced) rb_act_kernel<true, true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
        else rb_act_kernel<false, true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    } else {
        if (forced) rb_act_kernel<true, false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
        else rb_act_kernel<false, false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    }
    RG_HIP(hipGetLastError());
    return MI_RB_OK;
}

// the members only the walk needs (a macro: the error text names the entry point that was called); mi_nstep.hip's three checks
#define RB_CHECK_WALK(ring, b)                                                                                                                          \
    do {                                                                                                                                                \
        RG_CHECK_ARG((b)->horizon != nullptr, "horizon is NULL");                                                                                       \
        RG_CHECK_ARG((b)->n_step >= 1 && (b)->n_step <= MI_RB_MAX_N && (int64_t)(b)->n_step < (ring)->slots, "n_step must be in [1, 16] and below slots"); \
        RG_CHECK_ARG((b)->head_slot >= 0 && (b)->head_slot < (ring)->slots, "head_slot outside [0, slots)");                                            \
    } while (0)

extern "C" int mi_rb_target(const mi_rb_ring_t* ring, const mi_rb_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_RB_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->next_actions && b->target_probs && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params), "params and target_params must be 16-byte aligned");
    RB_CHECK_WALK(ring, b);
    RB_CHECK_SUPPORT(b->v_min, b->v_max);
    rb_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_RB_OK;
}

// mi_rb_grad (update false: opt is not looked at) and mi_rb_update
static int rb_grad(const mi_rb_ring_t* ring, const mi_rb_batch_t* b, const mi_rb_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_rb_batch_t& bt) { return bt.target_probs && bt.prio; });
    if (rc != RG_OK) return rc;
    RB_CHECK_WALK(ring, b);
    RB_CHECK_SUPPORT(b->v_min, b->v_max);
    if (update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<RB_NP>(rb_grad_kernel, rb_reduce_kernel, ring, b, rb_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_rb_grad(const mi_rb_ring_t* ring, const mi_rb_batch_t* b, void* stream) { return rb_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_rb_update(const mi_rb_ring_t* ring, const mi_rb_batch_t* b, const mi_rb_adam_t* opt, void* stream) {
    return rb_grad(ring, b, opt, true, (hipStream_t)stream);
}
