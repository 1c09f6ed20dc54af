// mi_ring.h — what the ring-replay libraries (libmirl_c51.so, libmirl_iqn.so, libmirl_qr.so, libmirl_ddqn.so) have in common: the error plumbing, the argument checks
// of the replay ring, of an acting call, of a batch and of the optimizer state, the epsilon table, the acting loop, the minibatch row index, the gradient launch and
// the fixed-order slab sum (+ Adam).  Each library is ONE translation unit that includes this header once, so every `static` / `static thread_local` below is that
// library's own copy; nothing here is exported.
//
// A library supplies its network (layout, loaders, forward / target / loss / gradient kernels), the argument checks that are its own, its `__global__` entry points
// and a POLICY struct for rg_act_loop; its MI_X_OK / MI_X_EINVAL / MI_X_EHIP must be 0 / -1 / -2 and its MI_X_MAX_STEPS_PER_CALL must be RG_MAX_STEPS (static_assert
// them).  Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#pragma once
#include "mi_common.h"

#include <stdarg.h>

#define RG_OK 0
#define RG_EINVAL (-1)
#define RG_EHIP (-2)
#define RG_MAX_STEPS 64        // steps of one acting launch: the length of rg_eps_tab
#define RG_STREAM_EXPLORE 3u
#define RG_STREAM_SAMPLE 4u

// ---- error plumbing of the including library --------------------------------------------------------
static thread_local char rg_err[512] = "";
static void rg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(rg_err, sizeof(rg_err), fmt, ap);
    va_end(ap);
}
#define RG_CHECK_ARG(cond, msg)                                       \
    do {                                                              \
        if (!(cond)) {                                                \
            rg_set_error("%s: invalid argument: %s", __func__, msg);  \
            return RG_EINVAL;                                         \
        }                                                             \
    } while (0)
#define RG_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            rg_set_error("%s: %s failed: %s", __func__, #call, hipGetErrorString(e_));    \
            return RG_EHIP;                                                               \
        }                                                                                 \
    } while (0)

static bool rg_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }   // parameters, observations and slabs are read and written as float4
static int rg_slabs(int batch, int max_slabs) { return batch < max_slabs ? batch : max_slabs; }
// RING: mi_c51_ring_t / mi_iqn_ring_t / mi_qr_ring_t / mi_ddqn_ring_t, and BATCH / ADAM below likewise (the same members; every use below is by name, so nothing is cast between them)
template <class RING>
static int rg_check_ring(const RING* r) {
    RG_CHECK_ARG(r != nullptr, "ring is NULL");
    RG_CHECK_ARG(r->observations && r->actions && r->rewards && r->terminated, "a ring buffer is NULL");
    RG_CHECK_ARG(r->slots >= 2 && r->n_envs >= 1, "slots must be >= 2 and n_envs >= 1");
    RG_CHECK_ARG(rg_aligned(r->observations), "observations must be 16-byte aligned");
    return RG_OK;
}

// ---- acting -----------------------------------------------------------------------------------------
struct rg_eps_tab { double v[RG_MAX_STEPS]; };   // epsilon(global_step + k) in the reference's double arithmetic, passed by value
// v[k] = max(slope * (global_step + k) + start_e, end_e): one product, one sum, one compare, in double.  C51 / QR-DQN form the slope from their schedule; IQN's
// epsilon 1 + slope * step is the same product and the same sum (IEEE addition commutes) with start_e = 1.
static void rg_eps_fill(rg_eps_tab& tab, int64_t global_step, double slope, double start_e, double end_e) {
    for (int k = 0; k < RG_MAX_STEPS; ++k) {
        const double ev = slope * (double)(global_step + k) + start_e;
        tab.v[k] = ev > end_e ? ev : end_e;
    }
}

struct rg_act_args {
    float* obs_cur;                  // [N][4] carried in / out
    const int64_t* forced_actions;   // [n_steps][N] nullable
    const double* forced_resets;     // [n_steps][N][4] nullable
    mi_episode_t* episodes;          // [max_ep]
    int32_t* episode_stats;          // [4] nullable
    long long global_step;
    long long learning_starts;       // steps before it explore whatever epsilon says (0: no such steps)
    int n_steps, max_ep;
};

// The acting loop of one launch: a workgroup walks its envs (n = g, g + G, ...), each through all steps of the chunk; fp64 physics in every thread (same cost as in
// one), exploring steps skip the network.  POLICY::greedy(x, s, n, env_id, ctr) returns the greedy action of observation x (step s of env n, whose step counter is
// ctr); it is called by the whole workgroup at once and owns every barrier of the greedy branch, the one that ends it (or its absence) included.
template <bool FORCED, class RING, class POLICY>
__device__ __forceinline__ void rg_act_loop(const mi_env& e, const RING& ring, const rg_act_args& a_, const rg_eps_tab& eps, POLICY& policy) {
    const int t = threadIdx.x;
    const int N = e.n;
    const long long slots = ring.slots, slot0 = a_.global_step % slots;   // (a 64-bit division: once per launch, not once per env)
    int st_cnt = 0, st_len = 0, st_max = 0;
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        // the env's state lives in every thread's registers (uniform across the workgroup); thread 0 does the stores
        const uint64_t env_id = e.env_id_base + (uint64_t)n;
        double s0 = e.x[n], s1 = e.x_dot[n], s2 = e.theta[n], s3 = e.theta_dot[n];
        int elapsed = e.elapsed[n], eplen = e.ep_len[n];
        float epret = e.ep_ret[n];
        uint64_t episode = e.episode[n], ctr = e.step_ctr[n];
        float4 x = reinterpret_cast<const float4*>(a_.obs_cur)[n];
        // every wave holds env n's state before thread 0 may store the advanced one below: a chunk of exploring or teacher-forced steps has no other barrier, and a
        // wave that read the advanced step counter would take the greedy branch (and its barriers) apart from the rest of the workgroup
        __syncthreads();
        long long slot = slot0;
        for (int s = 0; s < a_.n_steps; ++s) {
            int a;
            if (FORCED && a_.forced_actions) {
                a = a_.forced_actions[(size_t)s * N + n] != 0 ? 1 : 0;
            } else {
                uint32_t r[4];
                mi_philox(e.seed, env_id, ctr, RG_STREAM_EXPLORE, r);
                if ((a_.learning_starts > 0 && a_.global_step + s < a_.learning_starts) || (double)mi_u32_to_uniform(r[0]) < eps.v[s]) {
                    a = (int)(r[1] & 1u);
                } else {   // uniform branch: the whole workgroup works on this env
                    a = policy.greedy(x, s, n, env_id, ctr);
                }
            }
            int term;
            mi_cartpole_step(s0, s1, s2, s3, a, term);
            elapsed += 1; eplen += 1; epret += 1.0f;
            const bool trunc = !term && elapsed >= CP_MAX_STEPS;
            const bool done = term || trunc;
            const int fin_len = eplen; const float fin_ret = epret;
            if (done) {
                double rs[4];
                if (FORCED && a_.forced_resets) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) rs[k] = a_.forced_resets[4 * ((size_t)s * N + n) + k];
                } else {
                    mi_reset_noise(e.seed, env_id, episode, rs);
                }
                episode += 1;
                s0 = rs[0]; s1 = rs[1]; s2 = rs[2]; s3 = rs[3];
                elapsed = 0; eplen = 0; epret = 0.0f;
            }
            x = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
            const long long nslot = slot + 1 == slots ? 0 : slot + 1;
            if (t == 0) {
                ring.actions[slot * N + n] = a;
                reinterpret_cast<float4*>(ring.observations)[nslot * N + n] = x;
                ring.rewards[nslot * N + n] = 1.0f;
                ring.terminated[nslot * N + n] = (uint8_t)(term ? 1 : 0);
                if (done) {
                    st_cnt += 1; st_len += fin_len; st_max = fin_len > st_max ? fin_len : st_max;
                    if (a_.episode_stats && a_.max_ep > 0) {
                        const int sl = atomicAdd(a_.episode_stats + 3, 1);
                        if (sl < a_.max_ep) a_.episodes[sl] = mi_episode_t{n, s, fin_ret, fin_len};
                    }
                }
            }
            slot = nslot;
            ctr += 1;
        }
        if (t == 0) {
            e.x[n] = s0; e.x_dot[n] = s1; e.theta[n] = s2; e.theta_dot[n] = s3;
            e.elapsed[n] = elapsed; e.ep_ret[n] = epret; e.ep_len[n] = eplen; e.episode[n] = episode; e.step_ctr[n] = ctr;
            reinterpret_cast<float4*>(a_.obs_cur)[n] = x;
        }
    }
    if (t == 0 && a_.episode_stats && st_cnt > 0) { atomicAdd(a_.episode_stats, st_cnt); atomicAdd(a_.episode_stats + 1, st_len); atomicMax(a_.episode_stats + 2, st_max); }
}

// The host side of mi_x_act_steps behind the library's own checks (its act struct, its schedule) and its epsilon table: the checks the four share, the statistics
// memset and the grid.  The library then picks FORCED and launches its kernel.
template <class RING>
static int rg_act_prelude(const mi_env* e, const RING* ring, const float* params, const float* obs_cur, int n_steps, int max_ep, const mi_episode_t* episodes,
                          int32_t* episode_stats, hipStream_t s, int& grid) {
    RG_CHECK_ARG(e != nullptr, "NULL pointer");
    RG_CHECK_ARG(params && obs_cur, "params or obs_cur is NULL");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs_cur), "params and obs_cur must be 16-byte aligned");
    const int rc = rg_check_ring(ring);
    if (rc != RG_OK) return rc;
    RG_CHECK_ARG(e->kind == MI_ENV_CARTPOLE_V1 && e->n > 0, "env is not a CartPole-v1 handle");
    RG_CHECK_ARG(e->n == ring->n_envs, "the ring's n_envs is not the handle's");
    RG_CHECK_ARG(n_steps > 0 && n_steps <= RG_MAX_STEPS, "n_steps must be in [1, 64]");
    RG_CHECK_ARG(max_ep >= 0 && (max_ep == 0 || (episodes && episode_stats)), "episodes / episode_stats buffer missing");
    if (episode_stats) RG_HIP(hipMemsetAsync(episode_stats, 0, 4 * sizeof(int32_t), s));
    grid = e->n < 1024 ? e->n : 1024;
    return RG_OK;
}

// ---- minibatch rows ---------------------------------------------------------------------------------
// the flat ring index of batch row b: drawn in the launch when upper > 0 (Philox stream 4, keyed by the update index; the thread with `store` set writes it to
// idx[b]), else read from idx[b].  A bad index reads a valid row, never past the ring.
__device__ __forceinline__ long long rg_row_index(uint64_t seed, uint64_t update, int64_t upper, int64_t* idx, int b, long long total, bool store) {
    long long i;
    if (upper > 0) {
        uint32_t r[4];
        mi_philox(seed, update, (uint64_t)b, RG_STREAM_SAMPLE, r);
        i = (long long)((((uint64_t)r[1] << 32) | r[0]) % (uint64_t)upper);
        if (store) idx[b] = i;
    } else {
        i = idx[b];
    }
    return i < 0 ? 0 : (i >= total ? total - 1 : i);
}

// ---- slab sum + Adam --------------------------------------------------------------------------------
struct rg_adam_consts { float w1, b2, w2, step_size, rbc2, eps; };
// the host-side coefficients exactly as libmirl's mi_adam forms them
static rg_adam_consts rg_adam_host(int64_t step, double lr, double beta1, double beta2, double eps) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    rg_adam_consts k;
    k.w1 = (float)(1.0 - beta1); k.b2 = (float)beta2; k.w2 = (float)(1.0 - beta2);
    k.step_size = (float)(lr / bc1); k.rbc2 = (float)(1.0 / sqrt(bc2)); k.eps = (float)eps;
    return k;
}

// The body of a library's reduce kernel, launched as <<<(NP + 1 + 31) / 32, 32 * RG_RED_GROUPS>>>.  32 elements x 16 slab groups per workgroup: thread (j, k) adds
// the slabs g = k, k + 16, ... of element j in ascending g on four interleaved accumulators, the 16 group sums are then added in ascending k.  Element NP is the sum
// of the row losses; STRIDE is the distance between two slabs.
#define RG_RED_GROUPS 16
template <int NP, int STRIDE>
__device__ __forceinline__ void rg_reduce(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads, float* __restrict__ loss,
                                          float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const rg_adam_consts& k, int adam) {
    __shared__ float part[RG_RED_GROUPS][32];
    const int j = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + j;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (i <= NP) {
        int g = grp;
        for (; g + 3 * RG_RED_GROUPS < n_slabs; g += 4 * RG_RED_GROUPS) {
            s0 += slabs[(size_t)(g + 0 * RG_RED_GROUPS) * STRIDE + i]; s1 += slabs[(size_t)(g + 1 * RG_RED_GROUPS) * STRIDE + i];
            s2 += slabs[(size_t)(g + 2 * RG_RED_GROUPS) * STRIDE + i]; s3 += slabs[(size_t)(g + 3 * RG_RED_GROUPS) * STRIDE + i];
        }
        if (g < n_slabs) s0 += slabs[(size_t)g * STRIDE + i];
        if (g + RG_RED_GROUPS < n_slabs) s1 += slabs[(size_t)(g + RG_RED_GROUPS) * STRIDE + i];
        if (g + 2 * RG_RED_GROUPS < n_slabs) s2 += slabs[(size_t)(g + 2 * RG_RED_GROUPS) * STRIDE + i];
    }
    part[grp][j] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (grp != 0 || i > NP) return;
    float sum = part[0][j];
#pragma unroll
    for (int q = 1; q < RG_RED_GROUPS; ++q) sum += part[q][j];
    if (i == NP) { loss[0] = sum * inv; return; }
    grads[i] = sum;
    if (adam) {
        float mi = m[i], vi = v[i];
        p[i] = mi_adam_elem(p[i], sum, mi, vi, k.w1, k.b2, k.w2, k.step_size, k.rbc2, k.eps);
        m[i] = mi; v[i] = vi;
    }
}

// ---- the gradient entry points (mi_x_grad / mi_x_update) ----------------------------------------------
// `own` is the library's part of "every buffer is there" (the members only its batch struct has), max_batch / batch_msg its bound on the batch
template <class RING, class BATCH, class OWN>
static int rg_check_batch(const RING* ring, const BATCH* b, int max_batch, const char* batch_msg, OWN own) {
    const int rc = rg_check_ring(ring);
    if (rc != RG_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->batch > 0 && b->batch <= max_batch, batch_msg);
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->next_actions && b->grads && b->loss && b->workspace && own(*b), "a batch buffer is NULL");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params) && rg_aligned(b->workspace), "params, target_params and workspace must be 16-byte aligned");
    RG_CHECK_ARG(b->sample_upper >= 0 && b->sample_upper <= ring->slots * (int64_t)ring->n_envs, "sample_upper outside [0, slots * n_envs]");
    return RG_OK;
}
template <class ADAM>
static int rg_check_opt(const ADAM* opt) {
    RG_CHECK_ARG(opt != nullptr, "opt is NULL");
    RG_CHECK_ARG(opt->exp_avg && opt->exp_avg_sq && opt->step >= 1, "an optimizer buffer is NULL or step < 1");
    return RG_OK;
}
// the gradient launch over `slabs` workgroups, the optional mid_event, the slab sum scaled by `inv`; with opt != NULL (checked) the sum's Adam step on b->params
using rg_reduce_fn = void (*)(const float*, int, float, float*, float*, float*, float*, float*, rg_adam_consts, int);
template <int NP, class RING, class BATCH, class ADAM>
static int rg_launch_grad(void (*grad)(RING, BATCH, float*), rg_reduce_fn reduce, const RING* ring, const BATCH* b, int slabs, float inv, const ADAM* opt, hipStream_t s) {
    grad<<<slabs, 256, 0, s>>>(*ring, *b, (float*)b->workspace);
    RG_HIP(hipGetLastError());
    if (b->mid_event) RG_HIP(hipEventRecord((hipEvent_t)b->mid_event, s));
    if (opt)
        reduce<<<(NP + 1 + 31) / 32, 32 * RG_RED_GROUPS, 0, s>>>((const float*)b->workspace, slabs, inv, b->grads, b->loss, (float*)b->params, opt->exp_avg, opt->exp_avg_sq,
                                                                 rg_adam_host(opt->step, opt->lr, opt->beta1, opt->beta2, opt->eps), 1);
    else
        reduce<<<(NP + 1 + 31) / 32, 32 * RG_RED_GROUPS, 0, s>>>((const float*)b->workspace, slabs, inv, b->grads, b->loss, nullptr, nullptr, nullptr, rg_adam_consts{}, 0);
    RG_HIP(hipGetLastError());
    return RG_OK;
}
