// grad_kernel and its LDS layout, compiled twice by mi_update.hip: GRAD_BX 0 = exact f32 on v_mfma_f32_16x16x4_f32 (GV(x) = x_f32, the default and the
// headline), GRAD_BX 1 = the three 64 x 64 contractions on the bf16 matrix pipe with both operands split into three bf16 parts (GV(x) = x_bx; experiment
// behind mi_ppo_set_contraction, see the split-bf16 block in mi_update.hip).  Everything outside the three contractions is the same source.
struct __attribute__((aligned(16))) GV(grad_weights) {
#if GRAD_BX
    bf16x8 W2g[4 * 2 * 3 * 64];           // [out tile mt][k-half s][part][lane]: 8 k-slots of c W2[16mt + (lane & 15)][unit(s, lane >> 4, e)]
    bf16x8 W2t[4 * 2 * 3 * 64];           // [in tile mt][k-half s][part][lane]: 8 k-slots of W2[unit(s, lane >> 4, e)][16mt + (lane & 15)]
#else
    float W2g[HID * HID];                 // see the header comment
    float W2t[HID * HID];
#endif
    float b1[HID], b2[HID];               // scaled by c
    float W3[2 * HID];
    float W1s[HID * OBS];                 // c W1[unit][k]: every wave picks its layer-1 A fragments from here after the staging barrier
    float b3s[4];
    // Wave-private staging, ONE contiguous block per wave (13 KB): every tile-loop access of a wave is `its base + an immediate offset`.
    // xs: the tile's observations TRANSPOSED, x[k][row]: written as 64 consecutive dwords (lane (j, g) -> g * 16 + j), read back for dW1 as four b128 per lane
    // = x[lane & 3][0..15] (4 distinct 16-byte addresses 64 B apart, broadcast over the lanes that share k: conflict-free) instead of sixteen b32 of a [row][k] image.
    struct {
#if GRAD_BX
        // transposed images for dW2 (layout: bx_store_image), read back as one b128 per lane = 8 rows of one unit.
        // imgH (h1) is dead once the dW2 MFMAs have read it; the [row][unit] f32 staging tile of dz1 (bufB) then reuses its bytes (LDS operations of
        // one wave execute in order).
        union { unsigned short imgH[BX_IMG]; float bufB[TROWS * W2S]; } hb;
        unsigned short imgZ[BX_IMG];
#else
        float bufA[TROWS * W2S];   // [row][unit] images for the transposed re-reads (row stride W2S: the 4 pad columns are unused)
        float bufB[TROWS * W2S];   // bufA: h1, bufB: dz1, bufC: dz2 — each written as soon as its tile exists, read phases later
        float bufC[TROWS * W2S];
#endif
        float xs[4 * TROWS];
    } __attribute__((aligned(16))) st[GRAD_WAVES];
};
static_assert(TROWS == 16, "xs is read back as four b128 per lane");
struct __attribute__((aligned(16))) GV(grad_smem) {
    union {
        GV(grad_weights) w;
        float red[GRAD_WAVES][RED_STRIDE];  // exit reduction (the weights are dead by then)
    };
    double nrm[4];
    double nparts[256];                   // block_grad_norm's S_t (only touched when the clip coefficient is recomputed from the whole gradient)
};

template <bool ACTOR>
__device__ __forceinline__ void GV(grad_body)(GV(grad_smem)& sm, const float* __restrict__ params, const grad_pending_t& pend,
                                          const float* __restrict__ observations,
                                          const int64_t* __restrict__ actions, const float* __restrict__ log_probs,
                                          const float* __restrict__ advantages, const float* __restrict__ returns,
                                          const float* __restrict__ values, const int32_t* __restrict__ idx, int mb,
                                          const double* __restrict__ adv_sums, float clip_coef, float ent_coef, float vf_coef,
                                          float invn, float* __restrict__ part, unsigned vb, grad_role_t rl) {
    constexpr int NOUT = ACTOR ? 2 : 1;
    constexpr int BASE = ACTOR ? 0 : C_BASE;
    // Categorical(logits) over TWO actions depends on the logits only through d = l0 - l1, and d loss / d l1 = - d loss / d l0 exactly (p0 + p1 = 1): the
    // actor tile evaluates ONE head, (W3[0] - W3[1]) . h2 — the form rollout_q4_kernel samples from — and one set of head gradients; dW3[1] = -dW3[0], db3[1] = -db3[0]
    // are written at exit.  -59 VALU instructions per actor tile (of ~425) and 16 fewer live registers; same function, another rounding (reference ppo.py:52-59,166-190).
    constexpr bool ANTI = ACTOR;
    constexpr int NHEAD = ANTI ? 1 : NOUT;   // head rows whose gradient is accumulated
    const int tid = threadIdx.x, lane = tid & 63;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction; said so, the tile loop's control and the wave's LDS base are scalar
    const int j = lane & 15, g = lane >> 4;
    const bool pending = pend.grads != nullptr;
    const float* p = (pending ? pend.p_in : params) + BASE;
    GV(grad_weights)& W = sm.w;
#ifdef GRAD_STAMPS
    unsigned long long rt_in, rt_ready, rt_loop;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_in) :: "memory");
#endif

#ifdef GRAD_STAMPS
    unsigned long long pro_t[6] = {0, 0, 0, 0, 0, 0};
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pro_t[0]) :: "memory");
#endif
    // ---- stage this net's weights (once per block), stepping them first when an optimizer step is owed ----
    // W2: thread (q, cg) < 256 owns the 4x4 block W2[4q..4q+3][4cg..4cg+3]: one float4 per row in, four float4 per image out.
    // Thin parameters (everything but W2): the net's flat vector outside W2 is two contiguous ranges, [0, N_W2) = W1 | b1 and [N_B2, N_W3 + NOUT HID) = b2 | W3
    // (320 + 64 + NOUT 64 = 512 / 448 elements): thread t owns ONE of them, coalesced; the NOUT values of b3 ride as a second element of threads 0 .. NOUT-1.
    // (Round 2 let every wave fetch its own W1 fragments and every thread nine thin elements: 36 scalar loads x 4 arrays per thread against 2 x 4 now; together with the
    // clip coefficient from grad_reduce_kernel's 144 block sums instead of all 9,155 gradients, the owed step's prologue issues 25 loads per thread instead of 61.)
    // ALL loads of the prologue are issued before the first one is waited for: one memory round trip.
    {
        const int q = (tid >> 4) & 15, cg = tid & 15;
        const bool writer = pending && rl.ri == 0;   // the first workgroup of each net writes the stepped state back
        const bool w2t = tid < 256;
        constexpr int NT_A = N_W2, NT_B = HID + NOUT * HID;
        const bool has0 = tid < NT_A + NT_B, has1 = tid < NOUT;
        const int f0 = !has0 ? 0 : (tid < NT_A ? tid : N_B2 + (tid - NT_A));
        const int f1 = N_W3 + NOUT * HID + (has1 ? tid : 0);
        f32x4 w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = w2t ? reinterpret_cast<const f32x4*>(p + N_W2)[(4 * q + e) * 16 + cg] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        float sp0 = p[f0], sp1 = p[f1];
        if (pending) {
            f32x4 gg[4], mm[4], vv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int at = w2t ? (4 * q + e) * 16 + cg : 0;
                gg[e] = reinterpret_cast<const f32x4*>(pend.grads + BASE + N_W2)[at];
                mm[e] = reinterpret_cast<const f32x4*>(pend.m_in + BASE + N_W2)[at];
                vv[e] = reinterpret_cast<const f32x4*>(pend.v_in + BASE + N_W2)[at];
            }
            const float sg0 = pend.grads[BASE + f0], sg1 = pend.grads[BASE + f1];
            float sm0 = pend.m_in[BASE + f0], sv0 = pend.v_in[BASE + f0], sm1 = pend.m_in[BASE + f1], sv1 = pend.v_in[BASE + f1];
            // fail-safe of the P2P carrier (mi_common.h): the exchange that produced pend.grads timed out -> the owed step is WITHHELD.  Through the step's scalar constants,
            // not through a branch round the vector code (a uniform `if (!hold)` round the three Adam blocks cost the plain headline 0.3 us per launch): with w1 = w2 = 0,
            // b2 = 1, step size 0 the element update is m + 0 (g - m), v 1 + 0 g^2, p - 0 (...) = the state as it was (the local share it reads is finite).
            // (pend.gate is NEVER null — without a P2P carrier it points at a word that is always zero — so that the load is unconditional: a guarded load is a basic
            // block of its own that ends in s_waitcnt vmcnt(0), i.e. a second memory latency in this prologue: +0.2 us per optimizer step when first written that way)
            const bool hold = __hip_atomic_load(pend.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            const float a_w1 = hold ? 0.0f : pend.w1, a_b2 = hold ? 1.0f : pend.b2, a_w2 = hold ? 0.0f : pend.w2, a_ss = hold ? 0.0f : pend.step_size;
#ifdef GRAD_STAMPS
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pro_t[1]) :: "memory");
#endif
            const float total = block_grad_norm(pend.grads, pend.norm_parts, NPARAMS, sm.nrm, sm.nparts);
#ifdef GRAD_STAMPS
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pro_t[2]) :: "memory");
#endif
            float coef = pend.max_norm / (total + 1e-6f);
            coef = coef > 1.0f ? 1.0f : coef;
            if (pend.grad_norm && vb == 0 && tid == 0) *pend.grad_norm = total;
            if (w2t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        float m_ = mm[e][x], v_ = vv[e][x];
                        w[e][x] = mi_adam_elem(w[e][x], gg[e][x] * coef, m_, v_, a_w1, a_b2, a_w2, a_ss, pend.rbc2, pend.eps);
                        mm[e][x] = m_; vv[e][x] = v_;
                    }
                    if (writer) {
                        reinterpret_cast<f32x4*>(pend.p_out + BASE + N_W2)[(4 * q + e) * 16 + cg] = w[e];
                        reinterpret_cast<f32x4*>(pend.m_out + BASE + N_W2)[(4 * q + e) * 16 + cg] = mm[e];
                        reinterpret_cast<f32x4*>(pend.v_out + BASE + N_W2)[(4 * q + e) * 16 + cg] = vv[e];
                    }
                }
            }
            sp0 = mi_adam_elem(sp0, sg0 * coef, sm0, sv0, a_w1, a_b2, a_w2, a_ss, pend.rbc2, pend.eps);
            sp1 = mi_adam_elem(sp1, sg1 * coef, sm1, sv1, a_w1, a_b2, a_w2, a_ss, pend.rbc2, pend.eps);
            if (writer && has0) { pend.p_out[BASE + f0] = sp0; pend.m_out[BASE + f0] = sm0; pend.v_out[BASE + f0] = sv0; }
            if (writer && has1) { pend.p_out[BASE + f1] = sp1; pend.m_out[BASE + f1] = sm1; pend.v_out[BASE + f1] = sv1; }
        }
#ifdef GRAD_STAMPS
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pro_t[3]) :: "memory");
#endif
        if (w2t) {
#if GRAD_BX
            // the thread's 4 x 4 block: rows o = 4q + e, columns i = 4cg + x.  Forward image: k-slots follow the INPUT unit i (s = cg >> 3, 4 slots from
            // 4 ((cg >> 2) & 1), lane group cg & 3), one 8-byte store per row and part; backward image: k-slots follow the OUTPUT unit o (s = q >> 3, ...).
            unsigned short* gimg = reinterpret_cast<unsigned short*>(W.W2g);
            unsigned short* timg = reinterpret_cast<unsigned short*>(W.W2t);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = 4 * q + e;
                unsigned h0, m0, l0, h1_, m1, l1;
                split3(w[e][0] * GRAD_PS, w[e][1] * GRAD_PS, h0, m0, l0); split3(w[e][2] * GRAD_PS, w[e][3] * GRAD_PS, h1_, m1, l1);
                const int lane_a = (o & 15) + 16 * (cg & 3), slot = 4 * ((cg >> 2) & 1);
                const int base = (((o >> 4) * 2 + (cg >> 3)) * 3) * 64 * 8 + lane_a * 8 + slot;
                *reinterpret_cast<uint2*>(gimg + base) = make_uint2(h0, h1_);
                *reinterpret_cast<uint2*>(gimg + base + 64 * 8) = make_uint2(m0, m1);
                *reinterpret_cast<uint2*>(gimg + base + 2 * 64 * 8) = make_uint2(l0, l1);
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int i = 4 * cg + x;
                unsigned h0, m0, l0, h1_, m1, l1;
                split3(w[0][x], w[1][x], h0, m0, l0); split3(w[2][x], w[3][x], h1_, m1, l1);
                const int lane_a = (i & 15) + 16 * (q & 3), slot = 4 * ((q >> 2) & 1);
                const int base = (((i >> 4) * 2 + (q >> 3)) * 3) * 64 * 8 + lane_a * 8 + slot;
                *reinterpret_cast<uint2*>(timg + base) = make_uint2(h0, h1_);
                *reinterpret_cast<uint2*>(timg + base + 64 * 8) = make_uint2(m0, m1);
                *reinterpret_cast<uint2*>(timg + base + 2 * 64 * 8) = make_uint2(l0, l1);
            }
#else
#pragma unroll
            for (int e = 0; e < 4; ++e) *reinterpret_cast<f32x4*>(&W.W2g[(cg * 64 + 4 * q + e) * 4]) = w[e] * GRAD_PS;
#pragma unroll
            for (int x = 0; x < 4; ++x) *reinterpret_cast<f32x4*>(&W.W2t[(q * 64 + 4 * cg + x) * 4]) = f32x4{w[0][x], w[1][x], w[2][x], w[3][x]};
#endif
        }
        // the thin image: W1s = c W1 (flat [unit][k]), b1 / b2 scaled by c, W3 and b3 as they are
        if (has0) {
            if (tid < N_B1) W.W1s[tid] = GRAD_PS * sp0;
            else if (tid < NT_A) W.b1[tid - N_B1] = GRAD_PS * sp0;
            else if (tid < NT_A + HID) W.b2[tid - NT_A] = GRAD_PS * sp0;
            else W.W3[tid - NT_A - HID] = sp0;
        }
        if (has1) W.b3s[tid] = sp1;
    }

    // advantage normalisation constants (ppo.py:169) from {sum, sum sq, count}
    float adv_mean = 0.0f, adv_rden = 1.0f;
    if constexpr (ACTOR) {
        const double s1 = adv_sums[0], s2 = adv_sums[1], cnt = adv_sums[2];
        const double mean = s1 / cnt;
        double var = (s2 - s1 * mean) / (cnt - 1.0);   // a one-row minibatch: 0 / 0 = NaN, as torch's unbiased std of one element — ppo.py:169 poisons that update, and so does this
        var = var < 0.0 ? 0.0 : var;                   // (rounding may leave a tiny negative variance; a NaN stays a NaN)
        adv_mean = (float)mean;
        adv_rden = 1.0f / ((float)sqrt(var) + 1e-8f);
    }

    const int n_tiles = (mb + TROWS - 1) / TROWS;
    // Tile assignment.  The SIMD arbitrates VALU issue between its two waves by priority, then AGE: the first-dispatched
    // workgroup of a CU (blockIdx < grid/2) wins every conflict and runs ~1.3x faster than the second one (measured with
    // s_memrealtime stamps: 60 vs 80 us for equal work).  So the older half of a role's waves takes GRAD_OLD_SHARE of every
    // 16 tile rounds and the younger half the rest; a fixed function of the indices, so results stay reproducible.
    // one workgroup per CU: its waves 0-3 are the older wave of their SIMD, waves 4-7 the younger one
    const int half = rl.nr * 4;                                   // older (or younger) waves of this role
    const bool split_ok = (gridDim.x % (2u << GRAD_ROLE_BIT)) == 0;
    const bool young = split_ok && wib >= 4;
    const int wi_half = rl.ri * 4 + (wib & 3);                    // index within its half
    int tile, stride, tile_end;
    if (split_ok) {
        const int rounds = (n_tiles + half - 1) / half;            // tile rounds over one half
        const int old_rounds = (rounds * GRAD_OLD_SHARE + 8) / 16; // rounds taken by the older half
        const int split = old_rounds * half < n_tiles ? old_rounds * half : n_tiles;
        const int wi = wi_half;
        stride = half;
        tile = young ? split + wi : wi;
        tile_end = young ? n_tiles : split;
    } else {  // small grids: plain striding
        stride = rl.nr * GRAD_WAVES;
        tile = rl.ri * GRAD_WAVES + wib;
        tile_end = n_tiles;
    }
    // Only the minibatch's LAST tile can be ragged (mb % TROWS rows); the wave that owns it runs it last and apart, with the guarded body.  Every tile below
    // `lim` is a full one of this wave: the main loop has no row guards.  (tile, stride, tile_end, lim are wave-uniform: scalar registers.)
    const int full_tiles = mb / TROWS;
    const int lim = tile_end < full_tiles ? tile_end : full_tiles;
    // ---- input prefetch pipeline: row index two tiles ahead, gathered row one tile ahead ----
    // The look-ahead past a wave's last full tile is clamped to the last full tile of the MINIBATCH by scalar arithmetic (never past idx[mb - 1]; what it
    // fetches is not used): the index load is `scalar tile base + 4 j`, no vector arithmetic at all.  The ragged tile fetches its own indices and rows (tile_rid).
    unsigned j4 = 4u * (unsigned)j;   // (used by full_rid alone: the asm statement there rewrites it in place)
    auto full_rid = [&](int t) {
        const int tc = t < full_tiles ? t : full_tiles - 1;
        gbl_bytes* base = (gbl_bytes*)(idx + (size_t)tc * TROWS);
        asm volatile("" : "+s"(base), "+v"(j4));   // keeps the scalar tile base and the 32-bit lane offset apart (folded together, and the offset widened outside
        return *(const __attribute__((address_space(1))) int*)(base + j4);   // the loop, they become a 64-bit vector add per tile)
    };
    auto tile_rid = [&](int t) { const int row = t * TROWS + j; return idx[row < mb ? row : mb - 1]; };
    int rid_next = 0;
    row_in cur = {0.0f, 0, 0.0f, 0.0f}, nxt = cur;
    if (tile < lim) {
        rid_next = full_rid(tile + stride);
        cur = gather_row<ACTOR>(full_rid(tile), g, observations, actions, log_probs, advantages, returns, values);
    }
    const bool only_ragged = tile >= lim && tile < tile_end;   // the ragged tile is this wave's only one: fetched here, under the weight staging, as any first tile
    if (only_ragged) cur = gather_row<ACTOR>(tile_rid(tile), g, observations, actions, log_probs, advantages, returns, values);
#ifdef GRAD_STAMPS
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pro_t[4]) :: "memory");
#endif
    __syncthreads();  // weights staged
    // layer-1 A fragments live in registers: lane (i = j, g), tile mt holds c W1[16mt + i][k = g]
    float w1f[4], b3[NOUT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) w1f[mt] = W.W1s[4 * (16 * mt + j) + g];
#pragma unroll
    for (int a = 0; a < NOUT; ++a) b3[a] = W.b3s[a];
    f32x4 w3d[4];   // ANTI: (W3[0] - W3[1])[16mt + 4g + r], resident for the whole launch (no head-weight LDS reads in the tile loop)
    if constexpr (ANTI) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float4 w0 = *reinterpret_cast<const float4*>(&W.W3[16 * mt + 4 * g]), w1 = *reinterpret_cast<const float4*>(&W.W3[HID + 16 * mt + 4 * g]);
            w3d[mt] = f32x4{w0.x - w1.x, w0.y - w1.y, w0.z - w1.z, w0.w - w1.w};
        }
    }
#ifdef GRAD_STAMPS
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pro_t[5]) :: "memory");
#endif

    // ---- accumulators that live across tiles ----
#if GRAD_BX
    f32x16 dW2x[2][2];   // 32 x 32 tiles (o tile, i tile): register q of lane l = dW2[32 ot + 8 (q >> 2) + 4 (l >> 5) + (q & 3)][32 it + (l & 31)]
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int it2 = 0; it2 < 2; ++it2)
#pragma unroll
            for (int q = 0; q < 16; ++q) dW2x[ot][it2][q] = 0.0f;
    f32x4 db2v[4];       // per-lane sums over this lane's rows of dz2[row][16mt + 4g + r], reduced over j at exit
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) db2v[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#else
    f32x4 dW2[4][4];
#pragma unroll
    for (int mo = 0; mo < 4; ++mo)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) dW2[mo][mi] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#endif
    f32x4 dW1a = {0.0f, 0.0f, 0.0f, 0.0f}, dW1b = dW1a;  // two chains: the 4x4x1 dependent latency exceeds its issue time
    f32x4 dW3v[NHEAD][4];   // per-lane partial sums over this lane's rows: dW3[a][16mt + 4g + r], reduced over j at exit
#pragma unroll
    for (int a = 0; a < NHEAD; ++a)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) dW3v[a][mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float db1 = 0.0f, db3[2] = {0.0f, 0.0f};
#if !GRAD_BX
    float db2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#endif
    float loss_a = 0.0f, loss_b = 0.0f;  // actor: sum pg, sum entropy; critic: sum max(vl1, vl2)

#if GRAD_BX
    unsigned short* imgH = W.st[wib].hb.imgH;
    unsigned short* imgZ = W.st[wib].imgZ;
    float* bufB = W.st[wib].hb.bufB;
#else
    float* bufA = W.st[wib].bufA;
    float* bufB = W.st[wib].bufB;
    float* bufC = W.st[wib].bufC;
#endif
    float* xs = W.st[wib].xs;
    // read bases of the tile loop's b32 re-reads (lds_read_base): dz1 rows 4k .. 4k + 3 at column `lane`; dz2 / h1 rows 4g .. 4g + 3 at columns j + 16m (252 dwords at most)
    const lds_f32* rdB[TROWS / 4];
#pragma unroll
    for (int k = 0; k < TROWS / 4; ++k) rdB[k] = lds_read_base(bufB + 4 * k * W2S + lane);
#if !GRAD_BX
    const lds_f32* rdA = lds_read_base(bufA + 4 * g * W2S + j);
    const lds_f32* rdC = lds_read_base(bufC + 4 * g * W2S + j);
#endif

#ifdef GRAD_STAMPS
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_ready) :: "memory");
    unsigned long long stamp_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, stamp_last, stamp_t0;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_last) :: "memory");
    stamp_t0 = stamp_last;
#endif
    [[maybe_unused]] int it = 0;   // tiles this wave processed (read by the GRAD_STAMPS build)
    // One tile.  RAGGED = false: all 16 rows are the minibatch's (no row guards); true: rows at and past mb are masked out of every sum, as ever.
    auto tile_body = [&](auto ragged, const int t, const row_in& cur) __attribute__((always_inline)) {
        constexpr bool RAGGED = decltype(ragged)::value;
        const bool valid = !RAGGED || t * TROWS + j < mb;
        xs[TROWS * g + j] = cur.x;
        STAMP(0);  // gathers issued

        // ---- layer 1: z1^T = W1 x^T + b1 (K = 4 = obs dim: one MFMA per 16-unit tile) ----
        f32x4 h1[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float4 b = *reinterpret_cast<const float4*>(&W.b1[16 * mt + 4 * g]);
            h1[mt] = mfma16(w1f[mt], cur.x, f32x4{b.x, b.y, b.z, b.w});
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) h1[mt][r] = GRAD_TANH(h1[mt][r]);
#if !GRAD_BX
        // h1's image for the dW2 re-read at the end of the tile, written while it is fresh (the previous tile's reads of these bytes precede in program order).
        // Round 3: the images used to be stored right in front of the dW2 MFMAs, whose operand reads then queued behind 8 ds_write_b128; stored here (and dz2's
        // below) the reads have nothing to wait for and the scheduler can start them under the dW1 MFMAs: 74.7 -> 73.2 us per launch, same bits.
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<float4*>(bufA + j * W2S + 16 * mt + 4 * g) = make_float4(h1[mt][0], h1[mt][1], h1[mt][2], h1[mt][3]);
#endif
        STAMP(1);  // layer 1 + tanh

        // ---- layer 2: z2^T = W2 h1^T + b2; k-steps 4c..4c+3 <-> units 16c + 4g + {0..3} ----
        f32x4 h2[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float4 b = *reinterpret_cast<const float4*>(&W.b2[16 * mt + 4 * g]);
            h2[mt] = f32x4{b.x, b.y, b.z, b.w};
        }
#if GRAD_BX
        wave_lds_fence();   // imgH shares its bytes with the previous tile's dz1 tile (typed float): keep the compiler from hoisting the stores over those reads
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) {
            const bx_parts bq = split8(h1[2 * sh], h1[2 * sh + 1]);
            bx_store_image(imgH, bq, sh, g, j);   // (the previous tile's dz1 tile in these bytes was consumed by its dW1 MFMAs)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                bf16x8 a[3];
#pragma unroll
                for (int pp = 0; pp < 3; ++pp) a[pp] = W.W2g[((mt * 2 + sh) * 3 + pp) * 64 + lane];
                h2[mt] = bx_mac(a, bq, h2[mt]);
            }
        }
#else
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            f32x4 a[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(&W.W2g[((4 * c + g) * 64 + 16 * mt + j) * 4]);
            // consecutive MFMAs go to different accumulators: the 16x16x4 dependent latency (40 clk) exceeds its issue (32)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) h2[mt] = mfma16(a[mt][r], h1[c][r], h2[mt]);
        }
#endif
        STAMP(2);  // layer 2 MFMAs issued
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) h2[mt][r] = GRAD_TANH(h2[mt][r]);
        STAMP(3);  // tanh h2 (includes waiting for the layer-2 accumulators)

        // ---- head: out[a] = W3[a] . h2 + b3[a]; the 4 lanes (g) of a row hold 16 units each ----
        float outp[NOUT];
        if constexpr (ANTI) {   // one head: d = l0 - l1; Categorical(logits = (d, 0)) is the same distribution
            float acc = 0.0f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                acc = __builtin_fmaf(w3d[mt][0], h2[mt][0], acc); acc = __builtin_fmaf(w3d[mt][1], h2[mt][1], acc);
                acc = __builtin_fmaf(w3d[mt][2], h2[mt][2], acc); acc = __builtin_fmaf(w3d[mt][3], h2[mt][3], acc);
            }
            outp[0] = groups_sum(acc) + (b3[0] - b3[NOUT - 1]);
            outp[NOUT - 1] = 0.0f;
        } else {
#pragma unroll
            for (int a = 0; a < NOUT; ++a) {
                float acc = 0.0f;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const float4 w = *reinterpret_cast<const float4*>(&W.W3[a * HID + 16 * mt + 4 * g]);
                    acc = __builtin_fmaf(w.x, h2[mt][0], acc); acc = __builtin_fmaf(w.y, h2[mt][1], acc);
                    acc = __builtin_fmaf(w.z, h2[mt][2], acc); acc = __builtin_fmaf(w.w, h2[mt][3], acc);
                }
                outp[a] = groups_sum(acc) + b3[a];
            }
        }

        // ---- loss and d loss / d out (ppo.py:166-187), identical in the 4 lanes of a row ----
        float dl[NOUT];
        const float count_me = (valid && g == 0) ? 1.0f : 0.0f;
        if constexpr (ACTOR) {
            float nl0, nl1, p0, p1, H;
            mi_categorical2_fast(outp[0], outp[NOUT - 1], nl0, nl1, p0, p1, H);
            const float A = (cur.f1 - adv_mean) * adv_rden;
            const float ratio = mi_fast_exp((cur.act ? nl1 : nl0) - cur.f0);
            const float lo = 1.0f - clip_coef, hi = 1.0f + clip_coef;
            const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
            const float pg1 = -A * ratio, pg2 = -A * rc;
            loss_a += count_me * (pg1 > pg2 ? pg1 : pg2);
            loss_b += count_me * H;
            const bool inrange = (ratio >= lo) && (ratio <= hi);
            float dpg;
            if (pg1 > pg2) dpg = -A;
            else if (pg1 < pg2) dpg = inrange ? -A : 0.0f;
            else dpg = -0.5f * A + (inrange ? -0.5f * A : 0.0f);
            const float g_lp = invn * dpg * ratio;
            const float ec = ent_coef * invn;
            dl[0] = g_lp * ((cur.act == 0 ? 1.0f : 0.0f) - p0) + ec * (p0 * (nl0 + H));
            dl[NOUT - 1] = 0.0f;   // = -dl[0]: never materialised
        } else {
            const float ret = cur.f0, v_old = cur.f1;
            const float v = outp[0];
            const float d1 = v - ret;
            const float vl1 = d1 * d1;
            const float dv = v - v_old;
            const float dvc = dv < -clip_coef ? -clip_coef : (dv > clip_coef ? clip_coef : dv);
            const float vc = v_old + dvc;
            const float d2 = vc - ret;
            const float vl2 = d2 * d2;
            loss_a += count_me * (vl1 > vl2 ? vl1 : vl2);
            const bool vin = (dv >= -clip_coef) && (dv <= clip_coef);
            float dmax;
            if (vl1 > vl2) dmax = 2.0f * d1;
            else if (vl1 < vl2) dmax = vin ? 2.0f * d2 : 0.0f;
            else dmax = d1 + (vin ? d2 : 0.0f);
            dl[0] = (vf_coef * 0.5f * invn) * dmax;
        }
#pragma unroll
        for (int a = 0; a < NHEAD; ++a) {
            dl[a] = valid ? dl[a] : 0.0f;
            db3[a] += (g == 0) ? dl[a] : 0.0f;
        }
        STAMP(4);  // head + loss

        // ---- dW3[a][unit] += dout[row][a] h2[row][unit]: this lane's row, this lane's 16 units (summed over rows at exit) ----
#pragma unroll
        for (int a = 0; a < NHEAD; ++a)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) dW3v[a][mt][r] = __builtin_fmaf(dl[a], h2[mt][r], dW3v[a][mt][r]);

        STAMP(5);  // dW3
        // ---- dz2 = (W3^T dout) * (1 - h2^2); h2 is dead afterwards ----
        f32x4 dz2[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (ANTI) {   // W3[0] dl0 + W3[1] (-dl0)
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = w3d[mt][r] * dl[0];
            } else {
#pragma unroll
                for (int a = 0; a < NOUT; ++a) {
                    const float4 w = *reinterpret_cast<const float4*>(&W.W3[a * HID + 16 * mt + 4 * g]);
                    d[0] = __builtin_fmaf(w.x, dl[a], d[0]); d[1] = __builtin_fmaf(w.y, dl[a], d[1]);
                    d[2] = __builtin_fmaf(w.z, dl[a], d[2]); d[3] = __builtin_fmaf(w.w, dl[a], d[3]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float t = h2[mt][r]; dz2[mt][r] = d[r] * __builtin_fmaf(-t, t, 1.0f); }
        }

#if !GRAD_BX
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<float4*>(bufC + j * W2S + 16 * mt + 4 * g) = make_float4(dz2[mt][0], dz2[mt][1], dz2[mt][2], dz2[mt][3]);
#endif
        STAMP(6);  // dz2
        // ---- dh1^T = W2^T dz2^T, dz1 = dh1 * (1 - h1^2); k-steps 4c..4c+3 <-> output units o = 16c + 4g + {0..3} ----
        f32x4 dz1[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) dz1[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#if GRAD_BX
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) {
            const bx_parts bq = split8(dz2[2 * sh], dz2[2 * sh + 1]);
            bx_store_image(imgZ, bq, sh, g, j);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                bf16x8 a[3];
#pragma unroll
                for (int pp = 0; pp < 3; ++pp) a[pp] = W.W2t[((mt * 2 + sh) * 3 + pp) * 64 + lane];
                dz1[mt] = bx_mac(a, bq, dz1[mt]);
            }
        }
        // ---- dW2[o][i] += sum_rows dz2[row][o] h1[row][i] over the tile's 16 rows = the K of one 32x32x16: A[o][k = row] from imgZ, B[k = row][i] from imgH ----
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) db2v[mt] += dz2[mt];
        wave_lds_fence();
        {
            const int at = (lane >> 5) * BX_HALF + (lane & 31) * 8;
#pragma unroll
            for (int it2 = 0; it2 < 2; ++it2) {
                bf16x8 hbv[3];
#pragma unroll
                for (int pp = 0; pp < 3; ++pp) hbv[pp] = *reinterpret_cast<const bf16x8*>(imgH + pp * BX_PART + 32 * it2 * 8 + at);
#pragma unroll
                for (int ot = 0; ot < 2; ++ot) {
                    bf16x8 za[3];
#pragma unroll
                    for (int pp = 0; pp < 3; ++pp) za[pp] = *reinterpret_cast<const bf16x8*>(imgZ + pp * BX_PART + 32 * ot * 8 + at);
                    dW2x[ot][it2] = bx_mac32(za, hbv, dW2x[ot][it2]);
                }
            }
        }
#else
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            f32x4 a[4];   // a[mt][r] = W2[16c + 4g + r][16mt + j]
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(&W.W2t[((4 * c + g) * 64 + 16 * mt + j) * 4]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) dz1[mt] = mfma16(a[mt][r], dz2[c][r], dz1[mt]);
        }
#endif
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float t = h1[mt][r]; dz1[mt][r] = dz1[mt][r] * __builtin_fmaf(-t, t, 1.0f); }

        STAMP(7);  // dh1 MFMAs + dz1
        // ---- dW1 += dz1^T x (4x4x1: A = dz1[row][4b+i], B = x[row][jj]) and db1; dz1 is dead afterwards ----
        wave_lds_fence();
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
            *reinterpret_cast<float4*>(bufB + j * W2S + 16 * mt + 4 * g) = make_float4(dz1[mt][0], dz1[mt][1], dz1[mt][2], dz1[mt][3]);
        wave_lds_fence();
        f32x4 xv[TROWS / 4];   // x[k = lane & 3][row 0..15]
#pragma unroll
        for (int q = 0; q < TROWS / 4; ++q) xv[q] = *reinterpret_cast<const f32x4*>(xs + TROWS * (lane & 3) + 4 * q);
#pragma unroll
        for (int rr = 0; rr < TROWS; rr += 2) {
            const float z0 = rdB[rr >> 2][(rr & 3) * W2S], z1v = rdB[(rr + 1) >> 2][((rr + 1) & 3) * W2S];   // dz1[rr][lane], dz1[rr + 1][lane]
            db1 += z0 + z1v;
            dW1a = mfma4(z0, xv[rr >> 2][rr & 3], dW1a);
            dW1b = mfma4(z1v, xv[(rr + 1) >> 2][(rr + 1) & 3], dW1b);
        }

        STAMP(8);  // stage dz1 + dW1
#if !GRAD_BX
        // ---- dW2[o][i] += sum_rows dz2[row][o] h1[row][i]: A[i=o][k=row], B[k=row][j=i], rows s + 4g per k-step ----
        wave_lds_fence();   // (both images were written phases ago: only reads are left here)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float a[4], b[4];   // dz2 / h1 [row s + 4g][16m + j]
#pragma unroll
            for (int m = 0; m < 4; ++m) { a[m] = rdC[s * W2S + 16 * m]; b[m] = rdA[s * W2S + 16 * m]; db2[m] += a[m]; }
#pragma unroll
            for (int mo = 0; mo < 4; ++mo)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) dW2[mo][mi] = mfma16(a[mo], b[mi], dW2[mo][mi]);
        }
#endif
        STAMP(9);  // dW2
    };
    // a full tile: issue the next tile's gathers into `n` and the index after that (they land while this tile computes), then compute on `c`
    auto full_step = [&](const row_in& c, row_in& n, const int t) __attribute__((always_inline)) {
        n = gather_row<ACTOR>(rid_next, g, observations, actions, log_probs, advantages, returns, values);
        rid_next = full_rid(t + 2 * stride);
        tile_body(grad_tag<false>{}, t, c);
        ++it;
    };
    // main loop over the full tiles, then the ragged one.  (Two tiles per trip with `cur` and `nxt` exchanging roles would save the hand-over's register copies,
    // 3 - 4 per tile; that form spilled — 1 VGPR here, 24 in the bf16x3 instantiation — and was dropped: docs/LEDGER.md.)
    for (; tile < lim; tile += stride) {
        full_step(cur, nxt, tile);
        cur = nxt;
    }
    if (tile < tile_end) {   // here tile == full_tiles
        if (!only_ragged) cur = gather_row<ACTOR>(tile_rid(tile), g, observations, actions, log_probs, advantages, returns, values);
        tile_body(grad_tag<true>{}, tile, cur);
        ++it;
    }
#ifdef GRAD_STAMPS
    if (lane == 0) {  // diagnostic build: the slabs behind GRAD_MAX_BLOCKS / 2 (unused by grids of <= 512 blocks) receive the stamps
        unsigned long long* dbg = STAMP_BASE(part) + 32 * wib;   // 32 words per wave: 0-10 phases, 11 loop cycles, 12 tiles, 13-16 realtime marks, 17 hw id, 20-25 prologue
        unsigned long long now;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now) :: "memory");
        for (int k = 0; k < 11; ++k) dbg[k] = stamp_acc[k];
        dbg[11] = now - stamp_t0;
        dbg[12] = (unsigned long long)it;   // tiles this wave processed
        for (int k = 0; k < 6; ++k) dbg[20 + k] = pro_t[k];
    }
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_loop) :: "memory");
#endif
    const f32x4 dW1 = dW1a + dW1b;

    // ---- deterministic cross-wave reduction, then one partial slab per block ----
    // every wave drops its partial sums into its own LDS slot (dW2 in accumulator-fragment order: 16 conflict-free b128 stores),
    // one barrier, then 256 threads add the four slots in wave order and write the slab.  The slab keeps dW2 in fragment
    // order (float4 F = (4mo + mi)*64 + lane, component r = dW2[16mo + 4g + r][16mi + j]); grad_reduce_kernel undoes it.
    __syncthreads();  // every wave is done with the weights and its staging tiles -> the LDS becomes the reduction buffer
    {
        float* slot = sm.red[wib];
#if GRAD_BX
        // same slab positions as the f32 fragments: dW2[o][i] sits in float4 (4 (o >> 4) + (i >> 4)) * 64 + (i & 15) + 16 ((o & 15) >> 2), component o & 3
#pragma unroll
        for (int ot = 0; ot < 2; ++ot)
#pragma unroll
            for (int it2 = 0; it2 < 2; ++it2)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) {
                    const int o = 32 * ot + 8 * qq + 4 * (lane >> 5), i = 32 * it2 + (lane & 31);
                    const f32x16& d = dW2x[ot][it2];
                    *reinterpret_cast<f32x4*>(&slot[((4 * (o >> 4) + (i >> 4)) * 64 + (i & 15) + 16 * ((o & 15) >> 2)) * 4]) =
                        f32x4{d[4 * qq], d[4 * qq + 1], d[4 * qq + 2], d[4 * qq + 3]};
                }
#else
#pragma unroll
        for (int mo = 0; mo < 4; ++mo)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) *reinterpret_cast<f32x4*>(&slot[((4 * mo + mi) * 64 + lane) * 4]) = dW2[mo][mi];
#endif
        float* sm_small = slot + HID * HID;
#pragma unroll
        for (int i = 0; i < 4; ++i) sm_small[(4 * (lane >> 2) + i) * 4 + (lane & 3)] = dW1[i];  // dW1[unit 4b+i][k=jj]
        sm_small[256 + lane] = db1;
#if GRAD_BX
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t = db2v[mt][r];
                t += dpp_xor1(t); t += dpp_xor2(t); t += dpp_half_mirror(t); t += dpp_mirror(t);
                if (j == 0) sm_small[320 + 16 * mt + 4 * g + r] = t;
            }
#else
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float t = groups_sum(db2[m]);
            if (g == 0) sm_small[320 + 16 * m + j] = t;
        }
#endif
#pragma unroll
        for (int a = 0; a < NHEAD; ++a)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = dW3v[a][mt][r];   // sum over the 16 rows (lanes j) of this lane group
                    t += dpp_xor1(t); t += dpp_xor2(t); t += dpp_half_mirror(t); t += dpp_mirror(t);
                    if (j == 0) {
                        sm_small[384 + a * HID + 16 * mt + 4 * g + r] = t;
                        if constexpr (ANTI) sm_small[384 + HID + 16 * mt + 4 * g + r] = -t;   // dW3[1] = -dW3[0]
                    }
                }
#pragma unroll
        for (int a = 0; a < NHEAD; ++a) {
            const float t = wave_sum(db3[a]);
            if (lane == 0) { sm_small[384 + NOUT * HID + a] = t; if constexpr (ANTI) sm_small[384 + NOUT * HID + 1] = -t; }
        }
        const float la = wave_sum(loss_a), lb = wave_sum(loss_b);
        if (lane == 0) { sm_small[520] = la; sm_small[521] = lb; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < HID * HID / 4 / (64 * GRAD_WAVES); ++k) {
        const int i = tid + 64 * GRAD_WAVES * k;
        const f32x4 a0 = reinterpret_cast<const f32x4*>(sm.red[0])[i], a1 = reinterpret_cast<const f32x4*>(sm.red[1])[i];
        const f32x4 a2 = reinterpret_cast<const f32x4*>(sm.red[2])[i], a3 = reinterpret_cast<const f32x4*>(sm.red[3])[i];
        const f32x4 a4 = reinterpret_cast<const f32x4*>(sm.red[4])[i], a5 = reinterpret_cast<const f32x4*>(sm.red[5])[i];
        const f32x4 a6 = reinterpret_cast<const f32x4*>(sm.red[6])[i], a7 = reinterpret_cast<const f32x4*>(sm.red[7])[i];
        reinterpret_cast<f32x4*>(part + N_W2)[i] = ((a0 + a2) + (a1 + a3)) + ((a4 + a6) + (a5 + a7));
    }
    constexpr int N_SMALL = 384 + NOUT * HID + NOUT;
    for (int i = tid; i < 522; i += 64 * GRAD_WAVES) {
        if (i >= N_SMALL && i < 520) continue;
        float t = (sm.red[0][HID * HID + i] + sm.red[1][HID * HID + i]) + (sm.red[2][HID * HID + i] + sm.red[3][HID * HID + i]);
        t += (sm.red[4][HID * HID + i] + sm.red[5][HID * HID + i]) + (sm.red[6][HID * HID + i] + sm.red[7][HID * HID + i]);
        int dst;
        if (i < 256) dst = N_W1 + i;
        else if (i < 320) dst = N_B1 + (i - 256);
        else if (i < 384) dst = N_B2 + (i - 320);
        else if (i < N_SMALL) dst = N_W3 + (i - 384);
        else dst = PART_LOSS + (i - 520);
        part[dst] = t;
    }
#ifdef GRAD_STAMPS
    if (lane == 0) {
        unsigned long long rt_out;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_out) :: "memory");
        unsigned long long* dbg = STAMP_BASE(part) + 32 * wib;
        dbg[13] = rt_in; dbg[14] = rt_ready; dbg[15] = rt_loop; dbg[16] = rt_out;
        const unsigned hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        dbg[17] = ((unsigned long long)xcc << 32) | hw_id;
    }
#endif
}

__global__ void __launch_bounds__(64 * GRAD_WAVES, GRAD_WPS)
GV(grad_kernel)(const float* __restrict__ params, grad_pending_t pend, const float* __restrict__ observations, const int64_t* __restrict__ actions,
            const float* __restrict__ log_probs, const float* __restrict__ advantages, const float* __restrict__ returns,
            const float* __restrict__ values, const int32_t* __restrict__ idx, int mb, const double* __restrict__ adv_sums,
            float clip_coef, float ent_coef, float vf_coef, float invn, float* __restrict__ workspace) {
    __shared__ GV(grad_smem) sm;
    MI_INSIDE_SCOPE(MI_PROF_GRAD);
    // Workgroups are dealt round-robin over the 8 XCDs (b % 8), so role = b & 1 would give each XCD ONE net and leave the
    // critic XCDs idle while the (heavier) actor ones finish.  Swap the two low bit fields instead: the slab index
    // `vb` keeps role = vb & 1 for the reduce kernel, while the physical block's role is bit GRAD_ROLE_BIT of blockIdx.
    const unsigned rb = GRAD_ROLE_BIT;
    const unsigned lowmask = (1u << rb) - 1u;
    const unsigned vb = (gridDim.x & ((2u << rb) - 1u)) ? blockIdx.x  // grid not a multiple of 2^(rb+1): identity
                                                        : ((blockIdx.x >> rb) & 1u) | (((blockIdx.x & lowmask) | ((blockIdx.x >> (rb + 1)) << rb)) << 1);
    float* part = workspace + (size_t)vb * PART_STRIDE;
    const grad_role_t rl = grad_role(vb, (int)gridDim.x);
    if (rl.role == 0)
        GV(grad_body)<true>(sm, params, pend, observations, actions, log_probs, advantages, returns, values, idx, mb, adv_sums, clip_coef,
                        ent_coef, vf_coef, invn, part, vb, rl);
    else
        GV(grad_body)<false>(sm, params, pend, observations, actions, log_probs, advantages, returns, values, idx, mb, adv_sums, clip_coef,
                         ent_coef, vf_coef, invn, part, vb, rl);
}
