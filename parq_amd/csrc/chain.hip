// Specialised small GEMMs of the per-iteration chain at one (or a few) scenes:  Y = act(pro(X) @ W^T + b) (+ R)
//
// Same arithmetic, same tiling idea and the same summation order as linear_f32_kernel (linear.hip) — 16-row tiles, 4 waves that
// split K round-robin in 16-wide chunks, exact fp32 v_mfma_f32_16x16x4_f32 with row-contiguous float4 operand loads — but every
// property the generic kernel tests at run time (K, the prologue, the addend, bias / ReLU / residual kind, GroupNorm moments,
// bounds) is a template parameter here.  Why: the chain is latency-bound and a load under a run-time branch costs a full memory
// round trip — hipcc cannot count outstanding loads across the join points and waits vmcnt(0) at each of them (the generic
// 256^3 kernel spends 3.0 us in its body where the bare tile of tools/bench_src/chain_seam.hip takes 1.3, profiles/
// r03_iter_timeline_stamped_before.txt).  Here a workgroup issues EVERY global load it will ever need — operands, prologue
// parameters, row statistics, scene moments, bias, residual — in straight-line code before the first wait, so a launch is one round
// trip + one MFMA chain + one LDS reduction + the stores.
//   * a workgroup owns 16 rows x (16 NT) columns: NT column sub-tiles share the A fragments (N = 768 / 528 launches fit the chip
//     with <= 256 .. 384 workgroups instead of 768 / 528);
//   * epilogue: wave t finishes sub-tile t with one float4 per lane (16 rows x 64 bytes per store instruction);
//   * GroupNorm moments of the output: one fp64 atomic pair per sub-tile wave (no workgroup reduction, no extra barrier).
// launch_linear (linear.hip) routes here when the shape qualifies (chain_linear_supported) and keeps the generic kernel for
// everything else (ragged shapes, ReLU masks of the backward, dropout, head-major output scatter, many scenes).
#include "common.hpp"
#include "sample_body.hpp"

namespace parq {

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

enum : int { kProNone = 0, kProLN = 1, kProGN = 2 };
enum : int { kResNone = 0, kResPlain = 1, kResLN = 2 };

template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT, bool LNP = false>
__device__ __forceinline__ void chain_tile(const LinearArgs& a, const int block_x, const int block_y) {
    if (block_x == 0 && block_y == 0) publish_progress(a);
    constexpr int NWV = 4;                            // waves of a workgroup: they split K
    static_assert(K % (16 * NWV) == 0 && NT >= 1 && NT <= 4, "tile shape");
    constexpr int NCH = K / (16 * NWV);               // 16-wide K chunks per wave
    constexpr int CS = 16 * NWV;                      // the workgroup's K step per chunk (wave w takes columns w*16 .. w*16+15 of it)
    __shared__ __attribute__((aligned(16))) float red[NWV * NT * 4 * 64];   // [wave][sub-tile][acc reg][lane]
    __shared__ float lnred[NWV * 16 * 2];

    const int g = block_y;
    const int ntn = a.N / (16 * NT);
    int n0, m0;
    if (a.tile_map == 0) {                            // column tiles fastest: XCD x (= block index % 8) reads all of X and 1/8 of W
        n0 = (int)(block_x % ntn) * 16 * NT;
        m0 = (int)(block_x / ntn) * 16;
    } else {                                          // a row block's column tiles on one XCD: XCD x reads 1/8 of X and all of W
        const int x = block_x & 7, loc = block_x >> 3;
        n0 = (loc % ntn) * 16 * NT;
        m0 = (x * (a.M / 128) + loc / ntn) * 16;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int kbase = wave * 16 + kq * 4;             // lane's float4 of its c-th chunk sits at kbase + CS c

    const float* xrow = a.X + g * a.gX + (int64_t)(m0 + li) * a.ldx + kbase;
    // W fragments: row-major rows (16 rows x 64 bytes per wave-wide load, row stride ldw: at ldw = 1024 floats the 16 segments of
    // a load sit 4 KB apart) or the tile-ordered copy (one contiguous KB per load); both are affine in (sub-tile, chunk)
    const float* wbase;
    int64_t wt_stride, wc_stride;
    if (a.Wp) {
        wbase = a.Wp + g * a.gW + ((int64_t)(n0 / 16) * (K / 16) + wave) * 256 + lane * 4;
        wt_stride = (int64_t)(K / 16) * 256;
        wc_stride = NWV * 256;
    } else {
        wbase = a.W + g * a.gW + (int64_t)(n0 + li) * a.ldw + kbase;
        wt_stride = 16 * a.ldw;
        wc_stride = CS;
    }

    // ---------------- every global load of the workgroup, before anything waits
    f32x4v av[NCH], bv[NT][NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) av[c] = *reinterpret_cast<const f32x4v*>(xrow + c * CS);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int c = 0; c < NCH; ++c) bv[t][c] = *reinterpret_cast<const f32x4v*>(wbase + t * wt_stride + c * wc_stride);
    f32x4v x2v[ADD2 ? NCH : 1];
    f32x4v b2v[ADD2 == 2 ? NT : 1][ADD2 == 2 ? NCH : 1];
    if constexpr (ADD2 != 0) {
        const float* x2row = a.X2 + (int64_t)(m0 + li) * a.ldx2 + kbase;
#pragma unroll
        for (int c = 0; c < NCH; ++c) x2v[c] = *reinterpret_cast<const f32x4v*>(x2row + c * CS);
    }
    if constexpr (ADD2 == 2) {                        // second weight matrix, same addressing as W
        const float* w2base = a.Wp ? a.W2p + (wbase - a.Wp) : a.W2 + (wbase - a.W);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int c = 0; c < NCH; ++c) b2v[t][c] = *reinterpret_cast<const f32x4v*>(w2base + t * wt_stride + c * wc_stride);
    }
    f32x4v pg[PRO != kProNone ? NCH : 1], pb[PRO != kProNone ? NCH : 1];
    float shift = 0.f;
    double gsm = 0.0, gsq = 0.0;
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    if constexpr (PRO == kProLN) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            pg[c] = *reinterpret_cast<const f32x4v*>(a.ln_gamma + kbase + c * CS);
            pb[c] = *reinterpret_cast<const f32x4v*>(a.ln_beta + kbase + c * CS);
        }
        shift = a.X[g * a.gX + (int64_t)(m0 + li) * a.ldx];
    }
    if constexpr (PRO == kProGN) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            pg[c] = *reinterpret_cast<const f32x4v*>(a.gn_gamma + g * a.gGamma + kbase + c * CS);
            pb[c] = *reinterpret_cast<const f32x4v*>(a.gn_beta + g * a.gGamma + kbase + c * CS);
        }
        const double* src = a.gn_sums + ((int64_t)((m0 / a.gn_rows_per_scene) * a.gn_ngroups + g) * a.gn_slots + lane) * 2;
        gn_lane_sums(src, a.gn_slots, gsm, gsq);
    }
    // epilogue operands: wave t finishes sub-tile t (waves >= NT request the operands of sub-tile wave % NT and drop them)
    const int et = wave % NT;
    const int erow = lane >> 2, ec = (lane & 3) * 4;
    const int om = m0 + erow, on = n0 + et * 16 + ec;
    f32x4v e_bias = {0.f, 0.f, 0.f, 0.f}, e_r = {0.f, 0.f, 0.f, 0.f}, e_rg = {1.f, 1.f, 1.f, 1.f}, e_rb = {0.f, 0.f, 0.f, 0.f};
    float rmean = 0.f, rrstd = 1.f;
    if constexpr (BIAS) e_bias = *reinterpret_cast<const f32x4v*>(a.bias + g * a.gBias + on);
    if constexpr (RES != kResNone) e_r = *reinterpret_cast<const f32x4v*>(a.R + (int64_t)om * a.ldr + on);
    if constexpr (RES == kResLN) {
        e_rg = *reinterpret_cast<const f32x4v*>(a.rln_gamma + on);
        e_rb = *reinterpret_cast<const f32x4v*>(a.rln_beta + on);
        rmean = a.rln_stats[(int64_t)om * 2 + 0];
        rrstd = a.rln_stats[(int64_t)om * 2 + 1];
    }
    // the machine scheduler otherwise sinks the loads next to their uses (4 in flight, the epilogue operands after the MFMAs =
    // a second round trip): nothing moves across this point
    __builtin_amdgcn_sched_barrier(0);

    // ---------------- prologue on A
    if constexpr (PRO == kProLN) {
        // row statistics over the full K: one pass over data shifted by the row's first element, reduced across the 4 kq lane
        // groups (shuffles) and the 4 K-slices (LDS) — the order linear_f32_kernel uses
        float sm = 0.f, sq = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = av[c][e] - shift;
                sm += d;
                sq += d * d;
            }
        sm += __shfl_xor(sm, 16); sq += __shfl_xor(sq, 16);
        sm += __shfl_xor(sm, 32); sq += __shfl_xor(sq, 32);
        if (kq == 0) { lnred[(wave * 16 + li) * 2 + 0] = sm; lnred[(wave * 16 + li) * 2 + 1] = sq; }
        lds_barrier();
        float Ssum = 0.f, Q2 = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) { Ssum += lnred[(w * 16 + li) * 2 + 0]; Q2 += lnred[(w * 16 + li) * 2 + 1]; }
        const float invK = 1.f / (float)K;
        const float dm = Ssum * invK;
        const float mean = shift + dm;
        const float var = fmaxf(Q2 * invK - dm * dm, 0.f);
        const float rstd = 1.f / sqrtf(var + a.norm_eps);
        if (a.ln_stats_out && n0 == 0 && wave == 0 && kq == 0) {
            a.ln_stats_out[(int64_t)(m0 + li) * 2 + 0] = mean;
            a.ln_stats_out[(int64_t)(m0 + li) * 2 + 1] = rstd;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) av[c][e] = (av[c][e] - mean) * rstd * pg[c][e] + pb[c][e];
    }
    if constexpr (ADD2 == 1) {
        if (n0 < a.x2_ncols) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) av[c] += x2v[c];
        }
    }
    if constexpr (PRO == kProGN) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { gsm += __shfl_xor(gsm, o); gsq += __shfl_xor(gsq, o); }
        float mean, rstd;
        gn_mean_rstd(gsm, gsq, 1.0 / ((double)a.gn_rows_per_scene * (double)K), a.norm_eps, mean, rstd);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = (av[c][e] - mean) * rstd * pg[c][e] + pb[c][e];
                av[c][e] = y > 0.f ? y : 0.f;
            }
    }

    // ---------------- MFMA chains (one per sub-tile), split-K partials to LDS
    f32x4v acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c][e], bv[t][c][e], acc[t], 0, 0, 0);
    if constexpr (ADD2 == 2) {
        if (n0 < a.x2_ncols) {                        // the second operand pair feeds the same accumulators
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x2v[c][e], b2v[t][c][e], acc[t], 0, 0, 0);
        }
    }
    // acc[t][r]: row 4 * (lane >> 4) + r, column lane & 15 of sub-tile t
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((wave * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
    lds_barrier();
    if (wave >= NT) return;

    // ---------------- epilogue of sub-tile `wave`: lane -> (row = lane >> 2, 4 consecutive columns)
    const int src = (wave * 4 + (erow & 3)) * 64 + (erow >> 2) * 16 + ec;
    f32x4v sum = *reinterpret_cast<const f32x4v*>(&red[src]);
#pragma unroll
    for (int w = 1; w < NWV; ++w) sum += *reinterpret_cast<const f32x4v*>(&red[src + w * NT * 256]);
    f32x4v y;
    double gs = 0.0, gq = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = sum[e] + e_bias[e];
        if constexpr (RELU) v = v > 0.f ? v : 0.f;
        if constexpr (RES == kResPlain) v += e_r[e];
        if constexpr (RES == kResLN) v += (e_r[e] - rmean) * rrstd * e_rg[e] + e_rb[e];
        y[e] = v;
        if constexpr (GNOUT || LNP) { gs += (double)v; gq += (double)v * (double)v; }
    }
    *reinterpret_cast<f32x4v*>(a.Y + g * a.gY + (int64_t)om * a.y_row + on) = y;
    if constexpr (LNP) {
        // partial sums of this workgroup's 16 NT columns for every row, for the LayerNorm a later launch finishes: the 4 lanes of a
        // row by shuffles, the NT sub-tile waves through LDS (NT == NWV: every wave is still here) -> ONE fp64 pair per (row, tile)
        static_assert(NT == NWV, "the partial sums of a tile are combined by all waves");
        __shared__ f64x2 lnpart[NWV * 16];
        double ps = gs, pq = gq;
        ps += __shfl_xor(ps, 1); pq += __shfl_xor(pq, 1);
        ps += __shfl_xor(ps, 2); pq += __shfl_xor(pq, 2);
        if ((lane & 3) == 0) lnpart[wave * 16 + erow] = f64x2{ps, pq};
        lds_barrier();
        if (wave == 0) {
            const int ntile = a.N / (16 * NT), tile = n0 / (16 * NT);
            if (lane < 16) {
                f64x2 t = lnpart[lane];
#pragma unroll
                for (int w = 1; w < NWV; ++w) t += lnpart[w * 16 + lane];
                if (a.lnp_flags) {
                    // consumers are workgroups of THIS launch: write-through (sc1) payload, drained, then the flag (relaxed, agent scope)
                    typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
                    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.lnp_out, 0, 0x7fffffff, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4s, t), rs, (int)((((int64_t)(m0 + lane)) * ntile + tile) * 16), 0, 16);
                } else {
                    reinterpret_cast<f64x2*>(a.lnp_out)[(int64_t)(m0 + lane) * ntile + tile] = t;
                }
            }
            if (a.lnp_flags) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0)
                    __hip_atomic_store(a.lnp_flags + (m0 >> 4) * ntile + tile, a.lnp_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if constexpr (GNOUT) {
        const int nt0 = n0 + wave * 16;                     // first column of this sub-tile
        if (nt0 < a.gn_out_ncols) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { gs += __shfl_xor(gs, o); gq += __shfl_xor(gq, o); }
            if (lane == 0) {
                const int grp = (nt0 + g * a.N) / a.gn_out_group_cols;
                // this sub-tile's own slot when the (scene, group) block has at most gn_slots sub-tiles (always, in batch-invariant mode): a plain store
                const int cbs = a.gn_out_group_cols >> 4;
                const int rb = (m0 % a.gn_out_rows_per_scene) >> 4, cb = ((nt0 + g * a.N) % a.gn_out_group_cols) >> 4;
                const bool own = (a.gn_out_rows_per_scene >> 4) * cbs <= a.gn_slots;
                const int slot = own ? rb * cbs + cb : gn_shared_slot((unsigned)(block_x * NT + wave), a.gn_slots);
                double* dst = a.gn_out_sums + (((int64_t)(m0 / a.gn_out_rows_per_scene) * a.gn_out_ngroups + grp) * a.gn_slots + slot) * 2;
                if (own) {
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2*>(dst) = f64x2{gs, gq};
                } else {
                    atomicAdd(dst, gs);
                    atomicAdd(dst + 1, gq);
                }
            }
        }
    }
}

template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
__global__ __launch_bounds__(256) void chain_linear_kernel(LinearArgs a) {
    PARQ_TL_KERNEL(kTlLinear);
    chain_tile<K, NT, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, (int)blockIdx.x, (int)blockIdx.y);
}

// ONE launch for the two independent stages at the head of an iteration (both depend only on the previous iteration's decode):
// workgroups [0, n_lin) are the tiles of the position MLP's first layer (384 -> C, ReLU; threads >= 256 leave at once),
// workgroups [n_lin, n_lin + B*Q) project and sample one (scene, query) each (sample_body.hpp).  Saves one dependent launch
// (1.9 us boundary + ramp) per iteration; the two bodies run side by side on different CUs.
struct SampleArgs {
    const void* tokens; const double* T_cl; const float* cam; const float* ref; ScaleBox sb; int V, h, w, C, Q;
    float* tgt; float* coord_pos; double* zero_f64; int zero_n; float* raw_count;
    const void* const* ind; int64_t coord_off;     // optional CallPtrs block of a captured forward: tokens = ind[0], coord_pos = ind[6] + coord_off
};
template <int NCH, int TT = kTokF32>
__global__ __launch_bounds__(1024) void pe1_sample_kernel(LinearArgs a, SampleArgs sa, int n_lin) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if ((int)blockIdx.x < n_lin) {
        PARQ_TL_KERNEL(kTlLinear);
        if (threadIdx.x >= 256) return;
        chain_tile<384, 1, kProNone, 0, true, true, kResNone, false>(a, (int)blockIdx.x, 0);
    } else {
        PARQ_TL_KERNEL(kTlProjectSample);
        if (sa.ind != nullptr) {
            sa.tokens = sa.ind[0];
            sa.coord_pos = reinterpret_cast<float*>(const_cast<void*>(sa.ind[6])) + sa.coord_off;
        }
        project_sample_body<NCH, double, TT>(sa.tokens, sa.T_cl, sa.cam, sa.ref, sa.sb, sa.V, sa.h, sa.w, sa.C, sa.Q, sa.tgt, sa.coord_pos,
                                         sa.zero_f64, sa.zero_n, sa.raw_count, (int)blockIdx.x - n_lin, (int)gridDim.x - n_lin, smem);
    }
}

// ONE launch for two stages that a LayerNorm separates (api.hip do_iterate).  A LayerNorm is affine in its input once the row statistics
// are known, so the linear map BEHIND it can be pushed in front of the statistics (SeamArgs, common.hpp): the consumer tiles contract
// operands that exist before the launch, with pack-time products of the weights (float64-accumulated, rounded once:
// build_derived_weights), and only their EPILOGUE needs (mean, rstd) — from the fp64 partial row sums that the tiles of x, workgroups
// of the same launch with smaller block indices, publish write-through + flag (chain_tile LNP; cdna_hip_programming.md Guideline 16,
// form R1: sc1 payload, drained, relaxed agent-scope flag; sc1 loads on the consumer).  The wait sits behind the consumer's own
// contraction, so it is normally over before it starts; it is bounded (a flag that never arrives raises SeamArgs::err and the
// outputs are NaN).  Producers never wait and have the smaller block indices: whatever the dispatch order, every workgroup a
// consumer waits for is resident or finished (the grid fits the chip twice over).
//   seam Q:  xa = tgt + sa Wo^T + bo (transformer_parq.py:375)  |  q = norm1(xa) Wq^T + pe_h (Wq W2)^T + b'  (:377)
// Where it pays: a hand-off through memory costs ~4 us on a busy chip (MI355X_MICROARCH.md "handoff-flag"), about what the launch
// boundary it replaces costs, so the consumer must have at least (producer tile + hand-off) of work of its own.  Seam Q does (three
// operand pairs, 7 us, against a 4.5 us xa tile): the stage takes 8.5 us where the two launches took 14.1.  The same construction
// at norm2 / FFN layer 1 was built and measured: f tiles 11 us median (6 us of own work + waiting), stage 14.0 against 14.6 us for the
// two launches — no gain, not kept (profiles/r05_iter_timeline_stamps_seams_q_and_f.txt).
__device__ __forceinline__ bool seam_wait(const unsigned* flag, unsigned epoch) {
    // bounded by the 100 MHz wall clock (~0.1 s; looked at every 64 polls): never reached unless a producer died.  The acquire fence
    // behind the successful poll orders the payload loads that follow after the flag load (program order alone does not)
    const unsigned long long t0 = (unsigned long long)wall_clock64();
    for (unsigned spin = 1;; ++spin) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            return true;
        }
        __builtin_amdgcn_s_sleep(1);
        if ((spin & 63u) == 0 && (unsigned long long)wall_clock64() - t0 > 10000000ull) return false;
    }
}

template <int K1, bool LN1, int K2, int K3, int NT, bool RELU, bool GNOUT>
__device__ __forceinline__ void seam_tile(const SeamArgs& a, const int block_x) {
    constexpr int NWV = 4, CS = 64;
    constexpr int NC1 = K1 / CS, NC2 = K2 / CS, NC3 = K3 > 0 ? K3 / CS : 1;
    constexpr bool HAS3 = K3 > 0;
    static_assert(K1 % CS == 0 && K2 % CS == 0 && K3 % CS == 0 && NT >= 1 && NT <= 4, "tile shape");
    static_assert(!LN1 || K1 > 0, "LayerNorm(X1) with given statistics");
    __shared__ __attribute__((aligned(16))) float red[(HAS3 ? 2 : 1) * NWV * NT * 4 * 64];   // [acc set][wave][sub-tile][acc reg][lane]
    typedef double f64x2 __attribute__((ext_vector_type(2)));

    const int ntn = a.N / (16 * NT);
    const int n0 = (block_x % ntn) * 16 * NT, m0 = (block_x / ntn) * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int kbase = wave * 16 + kq * 4;
    auto wptr = [&](const float* Wp, int K) { return Wp + ((int64_t)(n0 / 16) * (K / 16) + wave) * 256 + lane * 4; };

    // ---------------- every global load that does not depend on the producers, before anything waits
    f32x4v a1[NC1], a2[NC2], a3[NC3], w1[NT][NC1], w2[NT][NC2], w3[HAS3 ? NT : 1][NC3];
    {
        const float* x1 = a.X1 + (int64_t)(m0 + li) * a.ldx1 + kbase;
        const float* x2 = a.X2 + (int64_t)(m0 + li) * a.ldx2 + kbase;
#pragma unroll
        for (int c = 0; c < NC1; ++c) a1[c] = *reinterpret_cast<const f32x4v*>(x1 + c * CS);
#pragma unroll
        for (int c = 0; c < NC2; ++c) a2[c] = *reinterpret_cast<const f32x4v*>(x2 + c * CS);
        const float* p1 = wptr(a.W1p, K1);
        const float* p2 = wptr(a.W2p, K2);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int c = 0; c < NC1; ++c) w1[t][c] = *reinterpret_cast<const f32x4v*>(p1 + (int64_t)t * (K1 / 16) * 256 + c * NWV * 256);
#pragma unroll
            for (int c = 0; c < NC2; ++c) w2[t][c] = *reinterpret_cast<const f32x4v*>(p2 + (int64_t)t * (K2 / 16) * 256 + c * NWV * 256);
        }
        if constexpr (HAS3) {
            const float* x3 = a.X3 + (int64_t)(m0 + li) * a.ldx3 + kbase;
            const float* p3 = wptr(a.W3p, K3);
#pragma unroll
            for (int c = 0; c < NC3; ++c) a3[c] = *reinterpret_cast<const f32x4v*>(x3 + c * CS);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int c = 0; c < NC3; ++c) w3[t][c] = *reinterpret_cast<const f32x4v*>(p3 + (int64_t)t * (K3 / 16) * 256 + c * NWV * 256);
        }
    }
    f32x4v pg[LN1 ? NC1 : 1], pb[LN1 ? NC1 : 1];
    float st_mean = 0.f, st_rstd = 1.f;
    if constexpr (LN1) {
#pragma unroll
        for (int c = 0; c < NC1; ++c) {
            pg[c] = *reinterpret_cast<const f32x4v*>(a.ln1_g + kbase + c * CS);
            pb[c] = *reinterpret_cast<const f32x4v*>(a.ln1_b + kbase + c * CS);
        }
        st_mean = a.ln1_stats[(int64_t)(m0 + li) * 2 + 0];
        st_rstd = a.ln1_stats[(int64_t)(m0 + li) * 2 + 1];
    }
    const int et = wave % NT;
    const int erow = lane >> 2, ec = (lane & 3) * 4;
    const int om = m0 + erow, on = n0 + et * 16 + ec;
    const f32x4v e_b1 = *reinterpret_cast<const f32x4v*>(a.b1 + on), e_s = *reinterpret_cast<const f32x4v*>(a.srow + on);
    f32x4v e_b2 = {0.f, 0.f, 0.f, 0.f};
    if (a.b2) e_b2 = *reinterpret_cast<const f32x4v*>(a.b2 + on);
    __builtin_amdgcn_sched_barrier(0);

    if constexpr (LN1) {
#pragma unroll
        for (int c = 0; c < NC1; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) a1[c][e] = (a1[c][e] - st_mean) * st_rstd * pg[c][e] + pb[c][e];
    }
    // ---------------- MFMA chains, split-K partials to LDS
    f32x4v acc1[NT], acc2[HAS3 ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc1[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC1; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[c][e], w1[t][c][e], acc1[t], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NC2; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[c][e], w2[t][c][e], acc1[t], 0, 0, 0);
    if constexpr (HAS3) {
#pragma unroll
        for (int t = 0; t < NT; ++t) acc2[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC3; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[c][e], w3[t][c][e], acc2[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[((wave * NT + t) * 4 + r) * 64 + lane] = acc1[t][r];
            if constexpr (HAS3) red[NWV * NT * 256 + ((wave * NT + t) * 4 + r) * 64 + lane] = acc2[t][r];
        }
    lds_barrier();
    if (wave >= NT) return;

    // ---------------- epilogue of sub-tile `wave`: lane -> (row = lane >> 2, 4 consecutive columns)
    const int src = (wave * 4 + (erow & 3)) * 64 + (erow >> 2) * 16 + ec;
    f32x4v u = *reinterpret_cast<const f32x4v*>(&red[src]);
#pragma unroll
    for (int w = 1; w < NWV; ++w) u += *reinterpret_cast<const f32x4v*>(&red[src + w * NT * 256]);
    f32x4v v = e_b2;
    if constexpr (HAS3) {
#pragma unroll
        for (int w = 0; w < NWV; ++w) v += *reinterpret_cast<const f32x4v*>(&red[NWV * NT * 256 + src + w * NT * 256]);
    }
    // the row's statistics: lane (lane & 3) = j waits for tile j of this row block and reads its partial (sc1: past this CU's and
    // this XCD's caches), the four lanes of a row add up
    double S = 0.0, Q = 0.0;
    bool ok = true;
    {
        const int j = lane & 3;
        if (j < a.nparts) {
            ok = seam_wait(a.flags + (m0 >> 4) * a.nparts + j, a.epoch);
            typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
            __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.part, 0, 0x7fffffff, 0x00020000);
            const f64x2 pr = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(((int64_t)om * a.nparts + j) * 16), 0, 16));
            S = pr[0];
            Q = pr[1];
        }
    }
    S += __shfl_xor(S, 1); Q += __shfl_xor(Q, 1);
    S += __shfl_xor(S, 2); Q += __shfl_xor(Q, 2);
    if (!__all(ok)) {
        if (lane == 0 && a.err) atomicOr(a.err, 4);
        S = Q = __builtin_nan("");
    }
    const double inv = 1.0 / (double)a.width;
    const double mu = S * inv;
    double var = Q * inv - mu * mu;
    var = var > 0.0 ? var : 0.0;
    const float mean = (float)mu, vv = (float)var + a.eps;
    float rstd = __builtin_amdgcn_rsqf(vv);
    rstd = rstd * (1.5f - 0.5f * vv * rstd * rstd);
    if (S != S) rstd = __builtin_nanf("");
    if (a.ln_out && n0 == 0 && wave == 0 && (lane & 3) == 0) {
        a.ln_out[(int64_t)om * 2 + 0] = mean;
        a.ln_out[(int64_t)om * 2 + 1] = rstd;
    }
    f32x4v y;
    double gs = 0.0, gq = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = rstd * (u[e] + e_b1[e] - mean * e_s[e]) + v[e];
        if constexpr (RELU) t = t > 0.f ? t : 0.f;
        y[e] = t;
        if constexpr (GNOUT) { gs += (double)t; gq += (double)t * (double)t; }
    }
    *reinterpret_cast<f32x4v*>(a.Y + (int64_t)om * a.ldy + on) = y;
    if constexpr (GNOUT) {
        const int nt0 = n0 + wave * 16;
        if (nt0 < a.gn_out_ncols) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { gs += __shfl_xor(gs, o); gq += __shfl_xor(gq, o); }
            if (lane == 0) {
                const int grp = nt0 / a.gn_out_group_cols;
                const int cbs = a.gn_out_group_cols >> 4;
                const int rb = (m0 % a.gn_out_rows_per_scene) >> 4, cb = (nt0 % a.gn_out_group_cols) >> 4;
                const bool own = (a.gn_out_rows_per_scene >> 4) * cbs <= kGnSlots;
                const int slot = own ? rb * cbs + cb : (int)((block_x * NT + wave) % kGnSlots);
                double* dst = a.gn_out_sums + (((int64_t)(m0 / a.gn_out_rows_per_scene) * a.gn_out_ngroups + grp) * kGnSlots + slot) * 2;
                if (own) *reinterpret_cast<f64x2*>(dst) = f64x2{gs, gq};
                else { atomicAdd(dst, gs); atomicAdd(dst + 1, gq); }
            }
        }
    }
}

// seam Q: workgroups [0, nA) are the tiles of xa (K = 256, plain residual, partials published), the rest the tiles of q
template <int NTB>
__global__ __launch_bounds__(256) void seam_q_kernel(LinearArgs aA, SeamArgs sb, int nA) {
    PARQ_TL_KERNEL(kTlLinear);
    const int bx = (int)blockIdx.x;
    if (bx < nA) chain_tile<256, 4, kProNone, 0, true, false, kResPlain, false, true>(aA, bx, 0);
    else seam_tile<256, false, 256, 256, NTB, false, false>(sb, bx - nA);
}
// The same tile for LONG contractions (K = 1024: the reference's shipped decoder width, config/train.yaml:37-56): the A rows of
// the tile stay in registers for the whole contraction (K / 64 float4 per lane), the W rows are streamed in batches of 256
// contraction steps, double-buffered: batch b + 1 (with its prologue parameters) is requested before the MFMAs of batch b are
// issued.  Same prologues, epilogue and summation order as chain_linear_kernel.
template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
__global__ __launch_bounds__(256) void chain_linear_stream_kernel(LinearArgs a) {
    PARQ_TL_KERNEL(kTlLinear);
    publish_progress(a);
    static_assert(K % 256 == 0 && NT >= 1 && NT <= 4 && ADD2 != 2, "tile shape");
    constexpr int NCH = K / 64;                       // 16-wide K chunks per wave
    constexpr int BCH = 4;                            // chunks per streamed batch (256 contraction steps per workgroup)
    constexpr int NB = NCH / BCH;
    __shared__ __attribute__((aligned(16))) float red[4 * NT * 4 * 64];
    __shared__ float lnred[4 * 16 * 2];

    const int g = blockIdx.y;
    const int ntn = a.N / (16 * NT);
    const int n0 = (int)(blockIdx.x % ntn) * 16 * NT;
    const int m0 = (int)(blockIdx.x / ntn) * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int kbase = wave * 16 + kq * 4;
    const float* xrow = a.X + g * a.gX + (int64_t)(m0 + li) * a.ldx + kbase;
    const float* wbase;
    int64_t wt_stride, wc_stride;
    if (a.Wp) {
        wbase = a.Wp + g * a.gW + ((int64_t)(n0 / 16) * (K / 16) + wave) * 256 + lane * 4;
        wt_stride = (int64_t)(K / 16) * 256;
        wc_stride = 4 * 256;
    } else {
        wbase = a.W + g * a.gW + (int64_t)(n0 + li) * a.ldw + kbase;
        wt_stride = 16 * a.ldw;
        wc_stride = 64;
    }
    const float* x2row = ADD2 != 0 ? a.X2 + (int64_t)(m0 + li) * a.ldx2 + kbase : nullptr;
    const float* pgp = PRO == kProLN ? a.ln_gamma + kbase : (PRO == kProGN ? a.gn_gamma + g * a.gGamma + kbase : nullptr);
    const float* pbp = PRO == kProLN ? a.ln_beta + kbase : (PRO == kProGN ? a.gn_beta + g * a.gGamma + kbase : nullptr);

    struct Batch { f32x4v w[NT][BCH]; f32x4v pg[BCH], pb[BCH], x2[BCH]; };
    auto load_batch = [&](Batch& B, int b) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int c = 0; c < BCH; ++c) B.w[t][c] = *reinterpret_cast<const f32x4v*>(wbase + t * wt_stride + (b * BCH + c) * wc_stride);
        if constexpr (PRO != kProNone) {
#pragma unroll
            for (int c = 0; c < BCH; ++c) {
                B.pg[c] = *reinterpret_cast<const f32x4v*>(pgp + (b * BCH + c) * 64);
                B.pb[c] = *reinterpret_cast<const f32x4v*>(pbp + (b * BCH + c) * 64);
            }
        }
        if constexpr (ADD2) {
#pragma unroll
            for (int c = 0; c < BCH; ++c) B.x2[c] = *reinterpret_cast<const f32x4v*>(x2row + (b * BCH + c) * 64);
        }
    };

    f32x4v av[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) av[c] = *reinterpret_cast<const f32x4v*>(xrow + c * 64);
    Batch bt[2];
    load_batch(bt[0], 0);
    float shift = 0.f;
    double gsm = 0.0, gsq = 0.0;
    if constexpr (PRO == kProLN) shift = a.X[g * a.gX + (int64_t)(m0 + li) * a.ldx];
    if constexpr (PRO == kProGN) {
        const double* src = a.gn_sums + ((int64_t)((m0 / a.gn_rows_per_scene) * a.gn_ngroups + g) * a.gn_slots + lane) * 2;
        gn_lane_sums(src, a.gn_slots, gsm, gsq);
    }
    const int et = wave % NT;
    const int erow = lane >> 2, ec = (lane & 3) * 4;
    const int om = m0 + erow, on = n0 + et * 16 + ec;
    f32x4v e_bias = {0.f, 0.f, 0.f, 0.f}, e_r = {0.f, 0.f, 0.f, 0.f}, e_rg = {1.f, 1.f, 1.f, 1.f}, e_rb = {0.f, 0.f, 0.f, 0.f};
    float rmean = 0.f, rrstd = 1.f;
    if constexpr (BIAS) e_bias = *reinterpret_cast<const f32x4v*>(a.bias + g * a.gBias + on);
    if constexpr (RES != kResNone) e_r = *reinterpret_cast<const f32x4v*>(a.R + (int64_t)om * a.ldr + on);
    if constexpr (RES == kResLN) {
        e_rg = *reinterpret_cast<const f32x4v*>(a.rln_gamma + on);
        e_rb = *reinterpret_cast<const f32x4v*>(a.rln_beta + on);
        rmean = a.rln_stats[(int64_t)om * 2 + 0];
        rrstd = a.rln_stats[(int64_t)om * 2 + 1];
    }
    __builtin_amdgcn_sched_barrier(0);

    float mean = 0.f, rstd = 1.f;
    if constexpr (PRO == kProLN) {
        float sm = 0.f, sq = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = av[c][e] - shift;
                sm += d;
                sq += d * d;
            }
        sm += __shfl_xor(sm, 16); sq += __shfl_xor(sq, 16);
        sm += __shfl_xor(sm, 32); sq += __shfl_xor(sq, 32);
        if (kq == 0) { lnred[(wave * 16 + li) * 2 + 0] = sm; lnred[(wave * 16 + li) * 2 + 1] = sq; }
        lds_barrier();
        float Ssum = 0.f, Q2 = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { Ssum += lnred[(w * 16 + li) * 2 + 0]; Q2 += lnred[(w * 16 + li) * 2 + 1]; }
        const float invK = 1.f / (float)K;
        const float dm = Ssum * invK;
        mean = shift + dm;
        const float var = fmaxf(Q2 * invK - dm * dm, 0.f);
        rstd = 1.f / sqrtf(var + a.norm_eps);
        if (a.ln_stats_out && n0 == 0 && wave == 0 && kq == 0) {
            a.ln_stats_out[(int64_t)(m0 + li) * 2 + 0] = mean;
            a.ln_stats_out[(int64_t)(m0 + li) * 2 + 1] = rstd;
        }
    }
    if constexpr (PRO == kProGN) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { gsm += __shfl_xor(gsm, o); gsq += __shfl_xor(gsq, o); }
        gn_mean_rstd(gsm, gsq, 1.0 / ((double)a.gn_rows_per_scene * (double)K), a.norm_eps, mean, rstd);
    }
    const bool add2 = ADD2 != 0 && n0 < a.x2_ncols;

    f32x4v acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b + 1 < NB) load_batch(bt[(b + 1) & 1], b + 1);          // in flight behind this batch's arithmetic
        __builtin_amdgcn_sched_barrier(0);
        const Batch& B = bt[b & 1];
#pragma unroll
        for (int c = 0; c < BCH; ++c) {
            f32x4v x = av[b * BCH + c];
            if constexpr (PRO == kProLN) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = (x[e] - mean) * rstd * B.pg[c][e] + B.pb[c][e];
            }
            if constexpr (ADD2) {
                if (add2) x += B.x2[c];
            }
            if constexpr (PRO == kProGN) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float y = (x[e] - mean) * rstd * B.pg[c][e] + B.pb[c][e];
                    x[e] = y > 0.f ? y : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[e], B.w[t][c][e], acc[t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((wave * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
    lds_barrier();
    if (wave >= NT) return;
    const int src = (wave * 4 + (erow & 3)) * 64 + (erow >> 2) * 16 + ec;
    f32x4v sum = *reinterpret_cast<const f32x4v*>(&red[src]);
#pragma unroll
    for (int w = 1; w < 4; ++w) sum += *reinterpret_cast<const f32x4v*>(&red[src + w * NT * 256]);
    f32x4v y;
    double gs = 0.0, gq = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = sum[e] + e_bias[e];
        if constexpr (RELU) v = v > 0.f ? v : 0.f;
        if constexpr (RES == kResPlain) v += e_r[e];
        if constexpr (RES == kResLN) v += (e_r[e] - rmean) * rrstd * e_rg[e] + e_rb[e];
        y[e] = v;
        if constexpr (GNOUT) { gs += (double)v; gq += (double)v * (double)v; }
    }
    *reinterpret_cast<f32x4v*>(a.Y + g * a.gY + (int64_t)om * a.y_row + on) = y;
    if constexpr (GNOUT) {
        const int nt0 = n0 + wave * 16;
        if (nt0 < a.gn_out_ncols) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { gs += __shfl_xor(gs, o); gq += __shfl_xor(gq, o); }
            if (lane == 0) {
                const int grp = (nt0 + g * a.N) / a.gn_out_group_cols;
                // this sub-tile's own slot when the (scene, group) block has at most gn_slots sub-tiles (always, in batch-invariant mode): a plain store
                const int cbs = a.gn_out_group_cols >> 4;
                const int rb = (m0 % a.gn_out_rows_per_scene) >> 4, cb = ((nt0 + g * a.N) % a.gn_out_group_cols) >> 4;
                const bool own = (a.gn_out_rows_per_scene >> 4) * cbs <= a.gn_slots;
                const int slot = own ? rb * cbs + cb : gn_shared_slot((unsigned)(blockIdx.x * NT + wave), a.gn_slots);
                double* dst = a.gn_out_sums + (((int64_t)(m0 / a.gn_out_rows_per_scene) * a.gn_out_ngroups + grp) * a.gn_slots + slot) * 2;
                if (own) {
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2*>(dst) = f64x2{gs, gq};
                } else {
                    atomicAdd(dst, gs);
                    atomicAdd(dst + 1, gq);
                }
            }
        }
    }
}

// 32-row form of the streamed tile (round 6): 8 waves split K eight ways, every W fragment feeds TWO 16-row MFMAs (rows m0 .. m0 + 15
// and m0 + 16 .. m0 + 31), so a launch reads W M / 32 times instead of M / 16 — the K = 1024 launches with thousands of columns
// (self in-projection, head layers) are bound by that stream out of the L2s (profiles/NOTES_r06.md row 6).  A rows of both halves in
// registers (K / 128 float4 per lane and half), W in double-buffered batches of two 16-step chunks, partial sums folded 8 -> 4 -> 1
// through 32 KB of LDS.  Prologues / epilogue as in chain_linear_stream_kernel; the K split (and so the summation order) differs.
template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
__global__ __launch_bounds__(512) void chain_linear_stream32_kernel(LinearArgs a) {
    PARQ_TL_KERNEL(kTlLinear);
    publish_progress(a);
    static_assert(K % 256 == 0 && NT >= 1 && NT <= 4 && ADD2 != 2, "tile shape");
    constexpr int NWV = 8;
    constexpr int NCH = K / (16 * NWV);               // 16-wide K chunks per wave
    constexpr int BCH = 2;                            // chunks per streamed batch
    constexpr int NB = NCH / BCH;
    static_assert(NCH % BCH == 0, "batches");
    __shared__ __attribute__((aligned(16))) float red[4 * NT * 2 * 4 * 64];
    __shared__ float lnred[NWV * 32 * 2];

    const int g = blockIdx.y;
    const int ntn = a.N / (16 * NT);
    const int n0 = (int)(blockIdx.x % ntn) * 16 * NT;
    const int m0 = (int)(blockIdx.x / ntn) * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int kbase = wave * 16 + kq * 4;
    const float* xrow = a.X + g * a.gX + (int64_t)(m0 + li) * a.ldx + kbase;
    const int64_t xh = 16 * a.ldx;
    const float* wbase;
    int64_t wt_stride, wc_stride;
    if (a.Wp) {
        wbase = a.Wp + g * a.gW + ((int64_t)(n0 / 16) * (K / 16) + wave) * 256 + lane * 4;
        wt_stride = (int64_t)(K / 16) * 256;
        wc_stride = NWV * 256;
    } else {
        wbase = a.W + g * a.gW + (int64_t)(n0 + li) * a.ldw + kbase;
        wt_stride = 16 * a.ldw;
        wc_stride = NWV * 16;
    }
    const float* x2row = ADD2 != 0 ? a.X2 + (int64_t)(m0 + li) * a.ldx2 + kbase : nullptr;
    const int64_t x2h = ADD2 != 0 ? 16 * a.ldx2 : 0;
    const float* pgp = PRO == kProLN ? a.ln_gamma + kbase : (PRO == kProGN ? a.gn_gamma + g * a.gGamma + kbase : nullptr);
    const float* pbp = PRO == kProLN ? a.ln_beta + kbase : (PRO == kProGN ? a.gn_beta + g * a.gGamma + kbase : nullptr);

    struct Batch { f32x4v w[NT][BCH]; f32x4v pg[BCH], pb[BCH], x2[2][BCH]; };
    auto load_batch = [&](Batch& B, int b) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int c = 0; c < BCH; ++c) B.w[t][c] = *reinterpret_cast<const f32x4v*>(wbase + t * wt_stride + (b * BCH + c) * wc_stride);
        if constexpr (PRO != kProNone) {
#pragma unroll
            for (int c = 0; c < BCH; ++c) {
                B.pg[c] = *reinterpret_cast<const f32x4v*>(pgp + (b * BCH + c) * (NWV * 16));
                B.pb[c] = *reinterpret_cast<const f32x4v*>(pbp + (b * BCH + c) * (NWV * 16));
            }
        }
        if constexpr (ADD2) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < BCH; ++c) B.x2[h][c] = *reinterpret_cast<const f32x4v*>(x2row + h * x2h + (b * BCH + c) * (NWV * 16));
        }
    };

    f32x4v av[2][NCH];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < NCH; ++c) av[h][c] = *reinterpret_cast<const f32x4v*>(xrow + h * xh + c * (NWV * 16));
    Batch bt[2];
    load_batch(bt[0], 0);
    float shift[2] = {0.f, 0.f};
    double gsm = 0.0, gsq = 0.0;
    if constexpr (PRO == kProLN) {
        shift[0] = a.X[g * a.gX + (int64_t)(m0 + li) * a.ldx];
        shift[1] = a.X[g * a.gX + (int64_t)(m0 + 16 + li) * a.ldx];
    }
    if constexpr (PRO == kProGN) {
        const double* src = a.gn_sums + ((int64_t)((m0 / a.gn_rows_per_scene) * a.gn_ngroups + g) * a.gn_slots + lane) * 2;
        gn_lane_sums(src, a.gn_slots, gsm, gsq);
    }
    const int et = wave % NT, eh = wave / NT;         // the 16 x 16 sub-tile this wave finishes (waves >= 2 NT have none)
    const int erow = lane >> 2, ec = (lane & 3) * 4;
    const int om = m0 + eh * 16 + erow, on = n0 + et * 16 + ec;
    f32x4v e_bias = {0.f, 0.f, 0.f, 0.f}, e_r = {0.f, 0.f, 0.f, 0.f}, e_rg = {1.f, 1.f, 1.f, 1.f}, e_rb = {0.f, 0.f, 0.f, 0.f};
    float rmean = 0.f, rrstd = 1.f;
    if (wave < 2 * NT) {
        if constexpr (BIAS) e_bias = *reinterpret_cast<const f32x4v*>(a.bias + g * a.gBias + on);
        if constexpr (RES != kResNone) e_r = *reinterpret_cast<const f32x4v*>(a.R + (int64_t)om * a.ldr + on);
        if constexpr (RES == kResLN) {
            e_rg = *reinterpret_cast<const f32x4v*>(a.rln_gamma + on);
            e_rb = *reinterpret_cast<const f32x4v*>(a.rln_beta + on);
            rmean = a.rln_stats[(int64_t)om * 2 + 0];
            rrstd = a.rln_stats[(int64_t)om * 2 + 1];
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    float mean[2] = {0.f, 0.f}, rstd[2] = {1.f, 1.f};
    if constexpr (PRO == kProLN) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float sm = 0.f, sq = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = av[h][c][e] - shift[h];
                    sm += d;
                    sq += d * d;
                }
            sm += __shfl_xor(sm, 16); sq += __shfl_xor(sq, 16);
            sm += __shfl_xor(sm, 32); sq += __shfl_xor(sq, 32);
            if (kq == 0) { lnred[(wave * 32 + h * 16 + li) * 2 + 0] = sm; lnred[(wave * 32 + h * 16 + li) * 2 + 1] = sq; }
        }
        lds_barrier();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float Ssum = 0.f, Q2 = 0.f;
#pragma unroll
            for (int w = 0; w < NWV; ++w) { Ssum += lnred[(w * 32 + h * 16 + li) * 2 + 0]; Q2 += lnred[(w * 32 + h * 16 + li) * 2 + 1]; }
            const float invK = 1.f / (float)K;
            const float dm = Ssum * invK;
            mean[h] = shift[h] + dm;
            const float var = fmaxf(Q2 * invK - dm * dm, 0.f);
            rstd[h] = 1.f / sqrtf(var + a.norm_eps);
            if (a.ln_stats_out && n0 == 0 && wave == 0 && kq == 0) {
                a.ln_stats_out[(int64_t)(m0 + h * 16 + li) * 2 + 0] = mean[h];
                a.ln_stats_out[(int64_t)(m0 + h * 16 + li) * 2 + 1] = rstd[h];
            }
        }
    }
    if constexpr (PRO == kProGN) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { gsm += __shfl_xor(gsm, o); gsq += __shfl_xor(gsq, o); }
        gn_mean_rstd(gsm, gsq, 1.0 / ((double)a.gn_rows_per_scene * (double)K), a.norm_eps, mean[0], rstd[0]);
        mean[1] = mean[0];
        rstd[1] = rstd[0];
    }
    const bool add2 = ADD2 != 0 && n0 < a.x2_ncols;

    f32x4v acc[2][NT];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[h][t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b + 1 < NB) load_batch(bt[(b + 1) & 1], b + 1);          // in flight behind this batch's arithmetic
        __builtin_amdgcn_sched_barrier(0);
        const Batch& B = bt[b & 1];
#pragma unroll
        for (int c = 0; c < BCH; ++c) {
            f32x4v x[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                x[h] = av[h][b * BCH + c];
                if constexpr (PRO == kProLN) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[h][e] = (x[h][e] - mean[h]) * rstd[h] * B.pg[c][e] + B.pb[c][e];
                }
                if constexpr (ADD2) {
                    if (add2) x[h] += B.x2[h][c];
                }
                if constexpr (PRO == kProGN) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float y = (x[h][e] - mean[h]) * rstd[h] * B.pg[c][e] + B.pb[c][e];
                        x[h][e] = y > 0.f ? y : 0.f;
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int h = 0; h < 2; ++h) acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[h][e], B.w[t][c][e], acc[h][t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // 8 partial tiles -> 4 (waves 4..7 hand theirs to waves 0..3) -> 1 (the finishing wave of each sub-tile adds four)
    auto ridx = [&](int w4, int t, int h, int r) { return ((((w4 * NT + t) * 2 + h) * 4 + r) * 64); };
    if (wave >= 4) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[ridx(wave - 4, t, h, r) + lane] = acc[h][t][r];
    }
    lds_barrier();
    if (wave < 4) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[ridx(wave, t, h, r) + lane] += acc[h][t][r];
    }
    lds_barrier();
    if (wave >= 2 * NT) return;
    const int src = ridx(0, et, eh, erow & 3) + (erow >> 2) * 16 + ec;
    f32x4v sum = *reinterpret_cast<const f32x4v*>(&red[src]);
#pragma unroll
    for (int w = 1; w < 4; ++w) sum += *reinterpret_cast<const f32x4v*>(&red[src + w * NT * 2 * 256]);
    f32x4v y;
    double gs = 0.0, gq = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = sum[e] + e_bias[e];
        if constexpr (RELU) v = v > 0.f ? v : 0.f;
        if constexpr (RES == kResPlain) v += e_r[e];
        if constexpr (RES == kResLN) v += (e_r[e] - rmean) * rrstd * e_rg[e] + e_rb[e];
        y[e] = v;
        if constexpr (GNOUT) { gs += (double)v; gq += (double)v * (double)v; }
    }
    *reinterpret_cast<f32x4v*>(a.Y + g * a.gY + (int64_t)om * a.y_row + on) = y;
    if constexpr (GNOUT) {
        const int nt0 = n0 + et * 16, mt0 = m0 + eh * 16;
        if (nt0 < a.gn_out_ncols) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { gs += __shfl_xor(gs, o); gq += __shfl_xor(gq, o); }
            if (lane == 0) {
                const int grp = (nt0 + g * a.N) / a.gn_out_group_cols;
                const int cbs = a.gn_out_group_cols >> 4;
                const int rb = (mt0 % a.gn_out_rows_per_scene) >> 4, cb = ((nt0 + g * a.N) % a.gn_out_group_cols) >> 4;
                const bool own = (a.gn_out_rows_per_scene >> 4) * cbs <= a.gn_slots;
                const int slot = own ? rb * cbs + cb : gn_shared_slot((unsigned)((blockIdx.x * 2 + eh) * NT + et), a.gn_slots);
                double* dst = a.gn_out_sums + (((int64_t)(mt0 / a.gn_out_rows_per_scene) * a.gn_out_ngroups + grp) * a.gn_slots + slot) * 2;
                if (own) {
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2*>(dst) = f64x2{gs, gq};
                } else {
                    atomicAdd(dst, gs);
                    atomicAdd(dst + 1, gq);
                }
            }
        }
    }
}

// ---- fp16 x 3 form of the tile for LONG contractions (round 6; K = 1024 / 768: the shipped decoder width) -------------------------
// The fp32 MFMA (157 TF) bounds these launches: 0.54 GF per N = 1024 launch is 3.4 us at that peak with one tile per CU, 6.4 GF per
// iteration 41 us (profiles/r06_chain_k1024_forms_per_launch.txt).  Here every fp32 operand is carried as hi + lo (two fp16 values,
// 22 significant bits — the same arithmetic as the split-precision attention, flash_split.hip) and a product is
// a_hi w_hi + a_hi w_lo + a_lo w_hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation: 3 x 16 cycles per 32 contraction steps and
// sub-tile instead of 8 x 32.  Range is not a condition: the A rows are scaled by an exact power of two per row (row maximum -> [2^10,
// 2^11), found from the values the prologue produced) and the weight rows by one per output column at pack time
// (pack_w_half_kernel), and the epilogue multiplies both back — all exact — so any finite fp32 input gives the fp32-class result.
// Weights: LinearArgs::Wh, fragment-ordered (block (n / 16, k / 32) = 2 KB: plane hi then plane lo, lane (n % 16, (k % 32) / 8) holds
// 8 consecutive k as one 16-byte load), wh_scale[n] = the inverse column scale.  Prologues / epilogue / moments as in
// chain_linear_stream_kernel.  8 waves split K in 32-wide chunks and EVERY operand of the tile is requested before the first wait (with
// 16-cycle products a streamed W batch would expose its whole round trip: the 4-wave double-buffered form measured 8.8 us per N = 1024
// launch where the fp32 tile takes 10.8); RH = 2: 32-row tiles, every W fragment feeds two row halves.  The A rows (and the addend) come in as
// whole-kilobyte requests owned by one wave per row, which prepares them and leaves hi / lo halves in LDS for the fragment reads (see the
// kernel).  Measured and not kept (round 6,
// profiles/NOTES_r06.md): branch-free operand requests with counted waits (the waves then reach the barriers at different times: +1.1 %
// per forward), the other block -> XCD assignment (+5 %), touching the next launch's weights into the L2s from this launch (+0.6 %).
typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// LDS of the tile: the split A rows (hi plane, lo plane; row pitch K + 32 halfs so that the sixteen rows of a fragment read start 64 bytes
// apart modulo 256), the partial sums of the fold (after the planes — or ON them in the 32-row form, behind one more barrier: 160 KB per CU)
// and the inverse row scales.
template <int K, int NT, int RH>
struct H3Lds {
    static constexpr int pitch = K + 32;                                   // halfs
    static constexpr int plane_bytes = 16 * RH * pitch * 2;
    static constexpr int red_bytes = 4 * NT * RH * 4 * 64 * 4;
    static constexpr bool alias = RH == 2;
    static constexpr int red_off = alias ? 0 : 2 * plane_bytes;
    static constexpr int rinv_off = alias ? 2 * plane_bytes : 2 * plane_bytes + red_bytes;
    static constexpr int bytes = rinv_off + 16 * RH * 4;
};

template <int K, int NT, int RH, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT, int FOLD = 0>
__global__ __launch_bounds__(512) void chain_linear_h3_kernel(LinearArgs a) {
    PARQ_TL_KERNEL(kTlLinear);
    publish_progress(a);
    static_assert(K % 256 == 0 && NT >= 1 && NT <= 4 && (RH == 1 || RH == 2) && ADD2 != 2, "tile shape");
    // FOLD (LayerNorm prologues; pack_w_half_kernel): 1 = gamma sits in Wh and W beta in wh_bias — the prologue is (x - mean) rstd;
    // 2 = W beta in wh_bias only (an addend follows the LayerNorm: (x - mean) rstd gamma + x2)
    static_assert(FOLD == 0 || (PRO == kProLN && BIAS && (FOLD == 1) == (ADD2 == 0)), "fold");
    constexpr bool kGamma = PRO == kProGN || (PRO == kProLN && FOLD != 1), kBeta = PRO == kProGN || (PRO == kProLN && FOLD == 0);
    // register budget: with prologue parameters or an addend in flight the second half of the W fragments is requested only after the
    // prologue has consumed them (it lands behind the barrier and the fragment reads)
    constexpr bool kLateW = NT >= 2 && (ADD2 != 0 || kGamma);
    constexpr int NT0 = kLateW ? NT / 2 : NT;
    constexpr int NWV = 8;
    constexpr int NCH = K / (32 * NWV);               // 32-wide K chunks per wave in the products (4 at K = 1024)
    constexpr int ROWS = 16 * RH;
    constexpr int RPW = ROWS / NWV;                   // rows a wave brings in and prepares (2 or 4)
    constexpr int KQ = K / 256;                       // whole-kilobyte requests per row
    typedef H3Lds<K, NT, RH> Lds;
    extern __shared__ __attribute__((aligned(16))) unsigned char h3_lds[];
    _Float16* const plane_hi = reinterpret_cast<_Float16*>(h3_lds);
    _Float16* const plane_lo = reinterpret_cast<_Float16*>(h3_lds + Lds::plane_bytes);
    float* const red = reinterpret_cast<float*>(h3_lds + Lds::red_off);
    float* const rinv = reinterpret_cast<float*>(h3_lds + Lds::rinv_off);

    const int g = blockIdx.y;
    const int ntn = (a.N / 16 + NT - 1) / NT;         // the last column tile may hold fewer than NT sub-tiles (head layer 1: 129 = 32 x 4 + 1)
    // the row tiles of a column tile share an XCD (block index mod 8) and with it one L2 copy of their W columns — also when the column
    // tile count is no multiple of 8 (head layer 1: 43): XCD x takes column tiles x, x + 8, ..., the grid is padded to 8 ceil(ntn / 8) per
    // row tile and the workgroups past the last column tile leave at once (27.6 -> 23.0 us at one scene, 80.8 -> 66.0 at four)
    const int ntn8 = (ntn + 7) >> 3;
    const int ct = (int)(blockIdx.x & 7u) + 8 * (int)((blockIdx.x >> 3) % ntn8);
    if (ct >= ntn) return;
    const int n0 = ct * 16 * NT;
    const int ntv = a.N / 16 - ct * NT < NT ? a.N / 16 - ct * NT : NT;      // sub-tiles of this column tile (the others re-read sub-tile 0 and are dropped)
    const int m0 = (int)((blockIdx.x >> 3) / ntn8) * ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const bool add2 = ADD2 != 0 && n0 < a.x2_ncols;

    // ---- operands.  A (and the addend) arrive as WHOLE-KILOBYTE requests — wave w owns rows w RPW .. w RPW + RPW - 1 of the tile, a request
    // is 1 KB of one row — not in the MFMA operand pattern (16 rows x 64 bytes per request), which costs several times more per byte
    // (tools/bench_src/row_stride_loads.hip: 64 KB per workgroup over 768 workgroups 3.7 us against 0.17 us above the launch floor); the
    // owner wave applies the prologue, finds the row maximum, splits, and the products read their fragments from LDS.
    const float* xr = a.X + g * a.gX + (int64_t)(m0 + wave * RPW) * a.ldx + lane * 4;
    f32x4v av[RPW][KQ];
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
        for (int c = 0; c < KQ; ++c) av[j][c] = *reinterpret_cast<const f32x4v*>(xr + (int64_t)j * a.ldx + c * 256);
    f32x4v pg[KQ], pb[KQ], x2[RPW][KQ];
    if constexpr (kGamma) {
        const float* pgp = (PRO == kProLN ? a.ln_gamma : a.gn_gamma + g * a.gGamma) + lane * 4;
#pragma unroll
        for (int c = 0; c < KQ; ++c) pg[c] = *reinterpret_cast<const f32x4v*>(pgp + c * 256);
    }
    if constexpr (kBeta) {
        const float* pbp = (PRO == kProLN ? a.ln_beta : a.gn_beta + g * a.gGamma) + lane * 4;
#pragma unroll
        for (int c = 0; c < KQ; ++c) pb[c] = *reinterpret_cast<const f32x4v*>(pbp + c * 256);
    }
    if constexpr (ADD2) {
        if (add2) {
            const float* x2r = a.X2 + (int64_t)(m0 + wave * RPW) * a.ldx2 + lane * 4;
#pragma unroll
            for (int j = 0; j < RPW; ++j)
#pragma unroll
                for (int c = 0; c < KQ; ++c) x2[j][c] = *reinterpret_cast<const f32x4v*>(x2r + (int64_t)j * a.ldx2 + c * 256);
        }
    }
    const f32x4v* wbase = reinterpret_cast<const f32x4v*>(a.Wh + g * a.gW) + ((int64_t)(n0 / 16) * (K / 32) + wave) * 128 + lane;
    constexpr int64_t wt_stride = (int64_t)(K / 32) * 128, wc_stride = NWV * 128;      // float4 units
    f32x4v wh[NT][NCH], wl[NT][NCH];
#pragma unroll
    for (int t = 0; t < NT0; ++t)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            wh[t][c] = wbase[(t < ntv ? t : 0) * wt_stride + c * wc_stride];
            wl[t][c] = wbase[(t < ntv ? t : 0) * wt_stride + c * wc_stride + 64];
        }
    double gsm = 0.0, gsq = 0.0;
    if constexpr (PRO == kProGN) {
        const double* src = a.gn_sums + ((int64_t)((m0 / a.gn_rows_per_scene) * a.gn_ngroups + g) * a.gn_slots + lane) * 2;
        gn_lane_sums(src, a.gn_slots, gsm, gsq);
    }
    const int et = wave % NT, eh = wave / NT;         // the 16 x 16 sub-tile this wave finishes (waves >= NT RH have none)
    const int erow = lane >> 2, ec = (lane & 3) * 4;
    const int om = m0 + eh * 16 + erow, on = n0 + et * 16 + ec;
    f32x4v e_bias = {0.f, 0.f, 0.f, 0.f}, e_r = {0.f, 0.f, 0.f, 0.f}, e_rg = {1.f, 1.f, 1.f, 1.f}, e_rb = {0.f, 0.f, 0.f, 0.f};
    f32x4v e_ws = {1.f, 1.f, 1.f, 1.f};
    float rmean = 0.f, rrstd = 1.f;
    if (wave < NT * RH && et < ntv) {
        e_ws = *reinterpret_cast<const f32x4v*>(a.wh_scale + g * (a.gW >> 8) + on);
        if constexpr (BIAS) e_bias = *reinterpret_cast<const f32x4v*>((FOLD != 0 ? a.wh_bias : a.bias + g * a.gBias) + on);
        if constexpr (RES != kResNone) e_r = *reinterpret_cast<const f32x4v*>(a.R + (int64_t)om * a.ldr + on);
        if constexpr (RES == kResLN) {
            e_rg = *reinterpret_cast<const f32x4v*>(a.rln_gamma + on);
            e_rb = *reinterpret_cast<const f32x4v*>(a.rln_beta + on);
            rmean = a.rln_stats[(int64_t)om * 2 + 0];
            rrstd = a.rln_stats[(int64_t)om * 2 + 1];
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- the owner wave prepares its rows: statistics from its own registers (a whole row per wave: no workgroup reduction), prologue in
    // fp32, exact power of two that takes the row maximum into [2^10, 2^11) (1 for an all-zero, tiny or non-finite row: those go through as
    // they are), hi / lo halves into the LDS planes
    float gmean = 0.f, grstd = 1.f;
    if constexpr (PRO == kProGN) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { gsm += __shfl_xor(gsm, o); gsq += __shfl_xor(gsq, o); }
        gn_mean_rstd(gsm, gsq, 1.0 / ((double)a.gn_rows_per_scene * (double)K), a.norm_eps, gmean, grstd);
    }
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int row = wave * RPW + j;
        float mean = gmean, rstd = grstd;
        if constexpr (PRO == kProLN) {
            const float shift = __shfl(av[j][0][0], 0);                   // X[row][0]
            float sm = 0.f, sq = 0.f;
#pragma unroll
            for (int c = 0; c < KQ; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = av[j][c][e] - shift;
                    sm += d;
                    sq += d * d;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o); sq += __shfl_xor(sq, o); }
            const float invK = 1.f / (float)K;
            const float dm = sm * invK;
            mean = shift + dm;
            const float var = fmaxf(sq * invK - dm * dm, 0.f);
            rstd = 1.f / sqrtf(var + a.norm_eps);
            if (a.ln_stats_out && n0 == 0 && lane == 0) {
                a.ln_stats_out[(int64_t)(m0 + row) * 2 + 0] = mean;
                a.ln_stats_out[(int64_t)(m0 + row) * 2 + 1] = rstd;
            }
        }
        float amax = 0.f;
#pragma unroll
        for (int c = 0; c < KQ; ++c) {
            f32x4v x = av[j][c];
            if constexpr (PRO != kProNone) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    x[e] = (x[e] - mean) * rstd;
                    if constexpr (kGamma) x[e] *= pg[c][e];
                    if constexpr (kBeta) x[e] += pb[c][e];
                    if constexpr (PRO == kProGN) x[e] = x[e] > 0.f ? x[e] : 0.f;
                }
            }
            if constexpr (ADD2) {
                if (add2) x += x2[j][c];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(x[e]));
            av[j][c] = x;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        const int ex = (int)((__float_as_uint(amax) >> 23) & 255u);
        const bool plain = ex < 16 || ex == 255;
        const float sc = plain ? 1.f : __uint_as_float((unsigned)(127 + 10 + 127 - ex) << 23);
        if (lane == 0) rinv[row] = plain ? 1.f : __uint_as_float((unsigned)(ex - 10) << 23);
#pragma unroll
        for (int c = 0; c < KQ; ++c) {
            const f32x4v x = av[j][c] * sc;
            const f16x2v h0 = __builtin_convertvector(f32x2v{x[0], x[1]}, f16x2v), h1 = __builtin_convertvector(f32x2v{x[2], x[3]}, f16x2v);
            const f16x2v l0 = __builtin_convertvector(f32x2v{x[0] - (float)h0[0], x[1] - (float)h0[1]}, f16x2v);
            const f16x2v l1 = __builtin_convertvector(f32x2v{x[2] - (float)h1[0], x[3] - (float)h1[1]}, f16x2v);
            typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
            *reinterpret_cast<f16x4v*>(plane_hi + row * Lds::pitch + c * 256 + lane * 4) = f16x4v{h0[0], h0[1], h1[0], h1[1]};
            *reinterpret_cast<f16x4v*>(plane_lo + row * Lds::pitch + c * 256 + lane * 4) = f16x4v{l0[0], l0[1], l1[0], l1[1]};
        }
    }
    PARQ_TL_MARK();                                   // 1: A (and everything else this CU asked for) arrived, rows prepared
    if constexpr (kLateW) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = NT0; t < NT; ++t)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                wh[t][c] = wbase[(t < ntv ? t : 0) * wt_stride + c * wc_stride];
                wl[t][c] = wbase[(t < ntv ? t : 0) * wt_stride + c * wc_stride + 64];
            }
        __builtin_amdgcn_sched_barrier(0);
    }
    lds_barrier();
    // ---- fragments of the products: lane (row li, k group kq) holds 8 consecutive k of its c-th chunk, k = (8 c + wave) 32 + 8 kq
    f16x8v ah[RH][NCH], al[RH][NCH];
#pragma unroll
    for (int h = 0; h < RH; ++h)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int off = (h * 16 + li) * Lds::pitch + (c * NWV + wave) * 32 + kq * 8;
            ah[h][c] = *reinterpret_cast<const f16x8v*>(plane_hi + off);
            al[h][c] = *reinterpret_cast<const f16x8v*>(plane_lo + off);
        }
    PARQ_TL_MARK();                                   // 2: barrier passed, fragments read

    f32x4v acc[RH][NT];
#pragma unroll
    for (int h = 0; h < RH; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[h][t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const f16x8v bh = __builtin_bit_cast(f16x8v, wh[t][c]), bl = __builtin_bit_cast(f16x8v, wl[t][c]);
#pragma unroll
            for (int h = 0; h < RH; ++h) {
                acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[h][c], bh, acc[h][t], 0, 0, 0);
                acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[h][c], bl, acc[h][t], 0, 0, 0);
                acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[h][c], bh, acc[h][t], 0, 0, 0);
            }
        }
    PARQ_TL_MARK();                                   // 3: products issued
    if constexpr (Lds::alias) lds_barrier();          // every wave has read its fragments: the partial sums may overwrite the planes
    // 8 partial tiles -> 4 (waves 4..7 hand theirs to waves 0..3) -> 1 (the finishing wave of each sub-tile adds four)
    auto ridx = [&](int w4, int t, int h, int r) { return ((((w4 * NT + t) * RH + h) * 4 + r) * 64); };
    if (wave >= 4) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < RH; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[ridx(wave - 4, t, h, r) + lane] = acc[h][t][r];
    }
    lds_barrier();
    if (wave < 4) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < RH; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[ridx(wave, t, h, r) + lane] += acc[h][t][r];
    }
    lds_barrier();
    PARQ_TL_MARK();                                   // 4: partial sums folded
    if (wave >= NT * RH || et >= ntv) return;
    const int src = ridx(0, et, eh, erow & 3) + (erow >> 2) * 16 + ec;
    f32x4v sum = *reinterpret_cast<const f32x4v*>(&red[src]);
#pragma unroll
    for (int w = 1; w < 4; ++w) sum += *reinterpret_cast<const f32x4v*>(&red[src + w * NT * RH * 256]);
    const float rs = rinv[eh * 16 + erow];
    f32x4v y;
    double gs = 0.0, gq = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = sum[e] * (rs * e_ws[e]) + e_bias[e];
        if constexpr (RELU) v = v > 0.f ? v : 0.f;
        if constexpr (RES == kResPlain) v += e_r[e];
        if constexpr (RES == kResLN) v += (e_r[e] - rmean) * rrstd * e_rg[e] + e_rb[e];
        y[e] = v;
        if constexpr (GNOUT) { gs += (double)v; gq += (double)v * (double)v; }
    }
    *reinterpret_cast<f32x4v*>(a.Y + g * a.gY + (int64_t)om * a.y_row + on) = y;
    if constexpr (GNOUT) {
        const int nt0 = n0 + et * 16, mt0 = m0 + eh * 16;
        if (nt0 < a.gn_out_ncols) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { gs += __shfl_xor(gs, o); gq += __shfl_xor(gq, o); }
            if (lane == 0) {
                const int grp = (nt0 + g * a.N) / a.gn_out_group_cols;
                const int cbs = a.gn_out_group_cols >> 4;
                const int rb = (mt0 % a.gn_out_rows_per_scene) >> 4, cb = ((nt0 + g * a.N) % a.gn_out_group_cols) >> 4;
                const bool own = (a.gn_out_rows_per_scene >> 4) * cbs <= a.gn_slots;
                const int slot = own ? rb * cbs + cb : gn_shared_slot((unsigned)((blockIdx.x * RH + eh) * NT + et), a.gn_slots);
                double* dst = a.gn_out_sums + (((int64_t)(mt0 / a.gn_out_rows_per_scene) * a.gn_out_ngroups + grp) * a.gn_slots + slot) * 2;
                if (own) {
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2*>(dst) = f64x2{gs, gq};
                } else {
                    atomicAdd(dst, gs);
                    atomicAdd(dst + 1, gq);
                }
            }
        }
    }
}

// Wh / wh_scale of a row-major [N][K] matrix: one workgroup per 16 output columns.  Column scale 2^f takes the row's largest |w| into
// [2^10, 2^11); hi = fp16(w 2^f), lo = fp16(w 2^f - hi) (round to nearest); scales[n] = 2^-f.  LayerNorm folds of the consumer's
// prologue: gamma != nullptr packs W diag(gamma) (rounded to fp32 once); beta != nullptr writes bias_out[n] = bias[n] + sum_k W[n][k]
// beta[k] (float64 sum, rounded once) — LN(x) W^T + b = ((x - mean) rstd) (W diag gamma)^T + (b + W beta).
__global__ __launch_bounds__(256) void pack_w_half_kernel(const float* __restrict__ W, int64_t ldw, int N, int K, float* __restrict__ dst,
                                                          float* __restrict__ scales, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ bias,
                                                          float* __restrict__ bias_out) {
    __shared__ float mx[16][17];
    __shared__ double bs[16][17];
    __shared__ float sc[16];
    const int nt = blockIdx.x, tid = threadIdx.x;
    {
        const int r = tid >> 4, p = tid & 15;
        const float* wr = W + (int64_t)(nt * 16 + r) * ldw;
        float m = 0.f;
        double bsum = 0.0;
        for (int k = p; k < K; k += 16) {
            const float w = wr[k];
            m = fmaxf(m, fabsf(gamma ? w * gamma[k] : w));
            if (beta) bsum += (double)w * (double)beta[k];
        }
        mx[r][p] = m;
        bs[r][p] = bsum;
    }
    __syncthreads();
    if (tid < 16) {
        float m = 0.f;
        double bsum = 0.0;
        for (int p = 0; p < 16; ++p) { m = fmaxf(m, mx[tid][p]); bsum += bs[tid][p]; }
        const int ex = (int)((__float_as_uint(m) >> 23) & 255u);
        const bool plain = ex < 16 || ex == 255;
        sc[tid] = plain ? 1.f : __uint_as_float((unsigned)(127 + 10 + 127 - ex) << 23);
        scales[nt * 16 + tid] = plain ? 1.f : __uint_as_float((unsigned)(ex - 10) << 23);
        if (beta) bias_out[nt * 16 + tid] = (float)((bias ? (double)bias[nt * 16 + tid] : 0.0) + bsum);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const float s = sc[li];
    const float* wr = W + (int64_t)(nt * 16 + li) * ldw + kq * 8;
    f32x4v* out = reinterpret_cast<f32x4v*>(dst) + (int64_t)nt * (K / 32) * 128 + lane;
    for (int kc = wave; kc < K / 32; kc += 4) {
        f16x8v hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float w = wr[kc * 32 + j];
            if (gamma) w *= gamma[kc * 32 + kq * 8 + j];
            w *= s;
            const _Float16 h = (_Float16)w;
            hi[j] = h;
            lo[j] = (_Float16)(w - (float)h);
        }
        out[(int64_t)kc * 128] = __builtin_bit_cast(f32x4v, hi);
        out[(int64_t)kc * 128 + 64] = __builtin_bit_cast(f32x4v, lo);
    }
}

// tile-ordered copy of a row-major weight matrix (LinearArgs::Wp): thread = one float4 of the destination
__global__ void pack_w_tiles_kernel(const float* __restrict__ W, int64_t ldw, int N, int K, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // float4 index in dst
    if (i >= (int64_t)N * K / 4) return;
    const int lane = (int)(i & 63);
    const int64_t blk = i >> 6;
    const int kc = (int)(blk % (K / 16)), nt = (int)(blk / (K / 16));
    const int li = lane & 15, kq = lane >> 4;
    *reinterpret_cast<f32x4v*>(dst + i * 4) = *reinterpret_cast<const f32x4v*>(W + (int64_t)(nt * 16 + li) * ldw + kc * 16 + kq * 4);
}

// pack-time fold of the position MLP's last layer into a consumer: thread = one element of out_w (float64 accumulation)
__global__ void fold_pos_weights_kernel(const float* __restrict__ Wa, const float* __restrict__ ba, const float* __restrict__ W2,
                                        const float* __restrict__ b2, int R, int C, float* __restrict__ out_w, float* __restrict__ out_b) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)R * C) return;
    const int r = (int)(i / C), k = (int)(i - (int64_t)r * C);
    double acc = 0.0;
    for (int j = 0; j < C; ++j) acc += (double)Wa[(int64_t)r * C + j] * (double)W2[(int64_t)j * C + k];
    out_w[i] = (float)acc;
    if (k == 0) {
        double b = (double)ba[r];
        for (int j = 0; j < C; ++j) b += (double)Wa[(int64_t)r * C + j] * (double)b2[j];
        out_b[r] = (float)b;
    }
}

// pack time, LayerNorm pushed through a linear map (see seam_tile / SeamArgs): thread = one row r of W [R][C]
//   Wg[r][k] = W[r][k] gamma[k],   s[r] = sum_k Wg[r][k],   bb[r] = b[r] + sum_k W[r][k] beta[k]        (float64 sums)
__global__ void ln_fold_kernel(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ gamma,
                               const float* __restrict__ beta, int R, int C, float* __restrict__ Wg, float* __restrict__ srow, float* __restrict__ bb) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double ss = 0.0, sb = (double)b[r];
    for (int k = 0; k < C; ++k) {
        const float wg = W[(int64_t)r * C + k] * gamma[k];
        Wg[(int64_t)r * C + k] = wg;
        ss += (double)wg;
        sb += (double)W[(int64_t)r * C + k] * (double)beta[k];
    }
    srow[r] = (float)ss;
    bb[r] = (float)sb;
}
// out[r][j] = sum_k A[r][k] Bm[k][j],  ob[r] = sum_k A[r][k] bv[k]   (A [R][C], Bm [C][C]; float64 accumulation): thread = one element
__global__ void matmul_fold_kernel(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ bv, int R, int C,
                                   float* __restrict__ out, float* __restrict__ ob) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)R * C) return;
    const int r = (int)(i / C), j = (int)(i - (int64_t)r * C);
    double acc = 0.0;
    for (int k = 0; k < C; ++k) acc += (double)A[(int64_t)r * C + k] * (double)Bm[(int64_t)k * C + j];
    out[i] = (float)acc;
    if (j == 0) {
        double b = 0.0;
        for (int k = 0; k < C; ++k) b += (double)A[(int64_t)r * C + k] * (double)bv[k];
        ob[r] = (float)b;
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// feature signature of a launch (what the template parameters must match)
struct Sig { int K, pro; int add2; bool bias, relu; int res; bool gnout; };

Sig sig_of(const LinearArgs& a) {
    Sig s;
    s.K = a.K;
    s.pro = a.ln_gamma ? kProLN : (a.gn_sums ? kProGN : kProNone);
    s.add2 = a.X2 == nullptr ? 0 : (a.W2 != nullptr ? 2 : 1);
    s.bias = a.bias != nullptr;
    s.relu = a.relu != 0;
    s.res = a.R ? (a.rln_stats ? kResLN : kResPlain) : kResNone;
    s.gnout = a.gn_out_sums != nullptr;
    return s;
}

thread_local bool g_dry_run = false;      // chain_linear_supported: match the launch against the instantiations without launching

template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
hipError_t go(const LinearArgs& a0, int groups, hipStream_t s) {
    if (g_dry_run) return hipSuccess;
    static const int map_env = [] { const char* e = dev_env("PARQ_CHAIN_MAP"); return e ? atoi(e) : 0; }();
    LinearArgs a = a0;
    a.tile_map = (map_env == 1 && a.M % 128 == 0) ? 1 : 0;
    const dim3 grid((unsigned)((a.N / (16 * NT)) * (a.M / 16)), groups, 1);
    hipLaunchKernelGGL((chain_linear_kernel<K, NT, PRO, ADD2, BIAS, RELU, RES, GNOUT>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
hipError_t go_stream(const LinearArgs& a0, int groups, hipStream_t s) {
    if (g_dry_run) return hipSuccess;
    LinearArgs a = a0;
    a.tile_map = 0;
    const dim3 grid((unsigned)((a.N / (16 * NT)) * (a.M / 16)), groups, 1);
    hipLaunchKernelGGL((chain_linear_stream_kernel<K, NT, PRO, ADD2, BIAS, RELU, RES, GNOUT>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
hipError_t go_stream32(const LinearArgs& a0, int groups, hipStream_t s) {
    if (g_dry_run) return hipSuccess;
    LinearArgs a = a0;
    a.tile_map = 0;
    const dim3 grid((unsigned)((a.N / (16 * NT)) * (a.M / 32)), groups, 1);
    hipLaunchKernelGGL((chain_linear_stream32_kernel<K, NT, PRO, ADD2, BIAS, RELU, RES, GNOUT>), grid, dim3(512), 0, s, a);
    return hipGetLastError();
}

template <int K, int NT, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
hipError_t go_h3(const LinearArgs& a0, int groups, hipStream_t s) {
    // LayerNorm prologues exist in the folded forms only (pack_w_half_kernel: gamma in Wh unless an addend follows, W beta in wh_bias)
    constexpr int FOLD = PRO == kProLN ? (ADD2 ? 2 : 1) : 0;
    if (FOLD != 0 && (a0.wh_fold != FOLD || !a0.wh_bias || !al16(a0.wh_bias) || groups != 1)) return hipErrorNotSupported;
    if (g_dry_run) return hipSuccess;
    LinearArgs a = a0;
    a.tile_map = 0;
    // 32-row tiles (every W fragment feeds two row halves) while their grid still has a workgroup per CU
    constexpr int min_wg32 = 256;
    const int gm = a.geom_M > 0 ? a.geom_M : a.M;      // batch-invariant inference: ONE scene's rows decide, so that the scene meets the
    // same row-tile form alone and in a batch
    const int64_t wg32 = (int64_t)((a.N / 16 + NT - 1) / NT) * (gm / 32) * groups;
    // measured per launch at the shipped width (profiles/r06_chain_fp16x3_rows32_threshold.txt): 32-row tiles win wherever their grid has a
    // workgroup per CU, except the launch with a plain addend (self in-projection: A and the addend for two row halves) below two full rounds
    constexpr int64_t need32 = (PRO == kProNone && ADD2 != 0) ? 2 * min_wg32 : min_wg32;
    const bool rows32 = gm % 32 == 0 && a.M % 32 == 0 && wg32 >= need32 && (!a.gn_sums || a.gn_rows_per_scene % 32 == 0) &&
                        (!a.gn_out_sums || a.gn_out_rows_per_scene % 32 == 0);
    if (rows32) {
        static DynLdsOnce once;
        if (hipError_t e = once.ensure(reinterpret_cast<const void*>(&chain_linear_h3_kernel<K, NT, 2, PRO, ADD2, BIAS, RELU, RES, GNOUT, FOLD>), (size_t)H3Lds<K, NT, 2>::bytes); e != hipSuccess) return e;
        const dim3 grid((unsigned)((((a.N / 16 + NT - 1) / NT + 7) / 8 * 8) * (a.M / 32)), groups, 1);
        constexpr int lds = H3Lds<K, NT, 2>::bytes;
        hipLaunchKernelGGL((chain_linear_h3_kernel<K, NT, 2, PRO, ADD2, BIAS, RELU, RES, GNOUT, FOLD>), grid, dim3(512), lds, s, a);
    } else {
        static DynLdsOnce once;
        if (hipError_t e = once.ensure(reinterpret_cast<const void*>(&chain_linear_h3_kernel<K, NT, 1, PRO, ADD2, BIAS, RELU, RES, GNOUT, FOLD>), (size_t)H3Lds<K, NT, 1>::bytes); e != hipSuccess) return e;
        const dim3 grid((unsigned)((((a.N / 16 + NT - 1) / NT + 7) / 8 * 8) * (a.M / 16)), groups, 1);
        constexpr int lds = H3Lds<K, NT, 1>::bytes;
        hipLaunchKernelGGL((chain_linear_h3_kernel<K, NT, 1, PRO, ADD2, BIAS, RELU, RES, GNOUT, FOLD>), grid, dim3(512), lds, s, a);
    }
    return hipGetLastError();
}

// column sub-tiles per workgroup for an N-wide launch: the widest of {1, 2, 3, 4} that divides N / 16 (and the addend / moment
// boundaries) while the grid still has at least ~3/4 of a workgroup per CU at one scene
int pick_nt(const LinearArgs& a, int want) {
    const int nt16 = a.N / 16;
    for (int nt = want; nt > 1; --nt) {
        if (nt16 % nt != 0) continue;
        if (a.X2 && a.x2_ncols % (16 * nt) != 0 && a.x2_ncols < a.N) continue;
        return nt;
    }
    return 1;
}

// the fp32 tile with pick_nt(a, WANT) sub-tiles.  pick_nt walks WANT, WANT - 1, .. 2 and falls back to 1, so it returns a value in
// [1, WANT] and every one of them for some N / 16 (N / 16 = 5: 1): exactly the forms up to WANT are instantiated
template <int WANT, int K, int PRO, int ADD2, bool BIAS, bool RELU, int RES, bool GNOUT>
hipError_t go_nt(const LinearArgs& a, int groups, hipStream_t s) {
    static_assert(WANT >= 2 && WANT <= 4, "sub-tiles per workgroup");
    const int nt = pick_nt(a, WANT);
    if constexpr (WANT >= 4) if (nt == 4) return go<K, 4, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);
    if constexpr (WANT >= 3) if (nt == 3) return go<K, 3, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);
    if (nt == 2) return go<K, 2, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);
    return go<K, 1, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);
}

}  // namespace

// The instantiations are the launches of one decoder iteration (api.hip do_iterate) at the reference's widths:
//   pe1 (384 -> C, ReLU) | pe2 | self in-proj (+pos on the q, k columns) | self out-proj (+tgt) | cross q-proj (LN1, +pos) |
//   cross out-proj (+LN1(xa)) | FFN1 (LN2, ReLU) | FFN2 (K = F, +LN2(xb)) | heads layer 1 (LN3, moments) | heads layer 2 (GN, moments)
// returns hipErrorNotSupported when no instantiation matches (the caller then launches the generic kernel).
hipError_t launch_chain_linear(const LinearArgs& a_in, int groups, hipStream_t s) {
    // the latency-bound regime (one or a few scenes); above it the generic kernel's 32 x 32 tiles fill the chip
    static const int chain_max_m = [] { const char* e = dev_env("PARQ_CHAIN_MAX_M"); return e ? atoi(e) : 4096; }();   // 0: generic kernel only (measured at 8 scenes, M = 2048: 1.64 -> 1.37 ms of linears)
    // batch-invariant inference (LinearArgs::geom_M): every choice below — this kernel family or the generic one, sub-tiles per
    // workgroup, 16- or 32-row tiles — is made from ONE scene's rows; the batch only multiplies the grid
    const int gm = a_in.geom_M > 0 ? a_in.geom_M : a_in.M;
    if (gm > chain_max_m) return hipErrorNotSupported;
    LinearArgs a = a_in;
    if (a.gn_slots <= 0) a.gn_slots = kGnSlots;
    if (a.gn_slots % 64 != 0) return hipErrorInvalidValue;
    if (a.Wp && (!al16(a.Wp) || a.ldw != a.K)) a.Wp = nullptr;     // the tile-ordered copy mirrors a dense [N][K] matrix
    // shape / layout conditions of the specialised kernel
    if (gm % 16 != 0 || a.M % 16 != 0 || a.N % 16 != 0) return hipErrorNotSupported;
    if (a.relu_mask || a.drop_p > 0.f || a.rows_per_batch != a.M || a.col_blk != a.N) return hipErrorNotSupported;
    if ((a.ldx | a.ldw | a.y_row) % 4 != 0 || !al16(a.X) || !al16(a.W) || !al16(a.Y)) return hipErrorNotSupported;
    if ((a.gX | a.gW | a.gY | a.gBias | a.gGamma) % 4 != 0) return hipErrorNotSupported;
    if (a.bias && !al16(a.bias)) return hipErrorNotSupported;
    if (a.X2 && (a.ldx2 % 4 != 0 || !al16(a.X2) || a.x2_ncols % 16 != 0)) return hipErrorNotSupported;
    if (a.R && (a.ldr % 4 != 0 || !al16(a.R))) return hipErrorNotSupported;
    if (a.W2 && (!a.X2 || !al16(a.W2) || (a.Wp && !a.W2p))) return hipErrorNotSupported;
    if (a.rln_stats && (!al16(a.rln_gamma) || !al16(a.rln_beta))) return hipErrorNotSupported;
    if (a.ln_gamma && (a.gn_sums || !al16(a.ln_gamma) || !al16(a.ln_beta) || groups != 1)) return hipErrorNotSupported;
    if (a.gn_sums && (a.gn_rows_per_scene % 16 != 0 || !al16(a.gn_gamma) || !al16(a.gn_beta))) return hipErrorNotSupported;
    if (a.gn_out_sums && (a.gn_out_rows_per_scene % 16 != 0 || a.gn_out_ncols % 16 != 0 || a.gn_out_group_cols % 16 != 0))
        return hipErrorNotSupported;
    const Sig g = sig_of(a);
    auto is = [&](int K, int pro, int add2, bool bias, bool relu, int res, bool gnout) {
        return g.K == K && g.pro == pro && g.add2 == add2 && g.bias == bias && g.relu == relu && g.res == res && g.gnout == gnout;
    };
    // ---- K = 1024 / 768 with the fp16 hi / lo mirror (LinearArgs::Wh): fp16 x 3 tile
    if (a.Wh && a.wh_scale && al16(a.Wh) && al16(a.wh_scale) && a.ldw == a.K && (a.gW % 256) == 0) {
        // pick_nt(a, 4) returns any of 4 .. 1 (N / 16 = 129 at head layer 1: 3): all four forms stay
#define PARQ_H3(KK, PRO, ADD2, BIAS, RELU, RES, GNOUT)                                                          \
    {                                                                                                           \
        int nt = pick_nt(a, 4);                                                                                 \
        /* a ragged sub-tile count (head layer 1: 129) takes full-width tiles with a partial last one instead of narrower tiles */ \
        /* where the grid is four rounds and more (head layer 1 at one / two / four / eight scenes: 23.0 | 24.2, 35.4 | 36.8, 66.0 | 60.5 us, -0.75 % per forward at eight) */ \
        if (nt < 4 && a.N >= 1024 && (!a.X2 || a.x2_ncols >= a.N) &&                                            \
            (int64_t)((a.N / 16 + 3) / 4) * (gm / 32) * groups >= 1024) nt = 4;                                 \
        const hipError_t e = nt == 4   ? go_h3<KK, 4, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s)          \
                             : nt == 3 ? go_h3<KK, 3, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s)          \
                             : nt == 2 ? go_h3<KK, 2, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s)          \
                                       : go_h3<KK, 1, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);         \
        if (e != hipErrorNotSupported) return e;        /* (a LayerNorm launch whose mirror lacks the fold: fp32 tiles) */ \
    }
        if (is(1024, kProNone, false, true, false, kResNone, false)) PARQ_H3(1024, kProNone, false, true, false, kResNone, false)     // pe2
        if (is(1024, kProNone, true, true, false, kResNone, false)) PARQ_H3(1024, kProNone, true, true, false, kResNone, false)       // self in-proj
        if (is(1024, kProNone, false, true, false, kResPlain, false)) PARQ_H3(1024, kProNone, false, true, false, kResPlain, false)   // self out-proj
        if (is(1024, kProLN, true, true, false, kResNone, false)) PARQ_H3(1024, kProLN, true, true, false, kResNone, false)           // cross q-proj
        if (is(1024, kProNone, false, true, false, kResLN, false)) PARQ_H3(1024, kProNone, false, true, false, kResLN, false)         // cross out-proj
        if (is(1024, kProLN, false, true, true, kResNone, false)) PARQ_H3(1024, kProLN, false, true, true, kResNone, false)           // FFN1
        if (is(1024, kProLN, false, true, false, kResNone, true)) PARQ_H3(1024, kProLN, false, true, false, kResNone, true)           // heads layer 1
        if (is(1024, kProGN, false, false, false, kResNone, true)) PARQ_H3(1024, kProGN, false, false, false, kResNone, true)         // heads layer 2
        if (is(768, kProNone, false, true, false, kResLN, false) && a.N >= 512) PARQ_H3(768, kProNone, false, true, false, kResLN, false)   // FFN2 at the shipped width
        if (is(768, kProNone, false, true, false, kResNone, false) && a.N >= 512) PARQ_H3(768, kProNone, false, true, false, kResNone, false)   // (kernel-level entry parq_k_linear_half)
#undef PARQ_H3
    }
    // sub-tiles wanted per launch (go_nt<WANT, ...>): 4 at the self in-projection, 3 at the N = 768 / 528 launches, 2 at head layer 2.
    // pick_nt(a, WANT) returns the largest nt in WANT .. 2 that divides N / 16 (and the addend boundary), else 1: never more than
    // WANT, so go_nt<3> has no NT = 4 form and go_nt<2> no NT = 4 / 3 form; every nt <= WANT occurs for some N and stays
    if (is(384, kProNone, false, true, true, kResNone, false)) return go<384, 1, kProNone, false, true, true, kResNone, false>(a, groups, s);      // pe1
    if (is(256, kProNone, false, true, false, kResNone, false)) return go<256, 1, kProNone, false, true, false, kResNone, false>(a, groups, s);    // pe2
    if (is(256, kProNone, true, true, false, kResNone, false)) {                                                                                   // self in-proj
        return go_nt<4, 256, kProNone, true, true, false, kResNone, false>(a, groups, s);
    }
    if (is(256, kProNone, 2, true, false, kResNone, false)) {                                                                                      // self in-proj, folded pos MLP
        return go_nt<4, 256, kProNone, 2, true, false, kResNone, false>(a, groups, s);
    }
    if (is(256, kProLN, 2, true, false, kResNone, false)) return go<256, 1, kProLN, 2, true, false, kResNone, false>(a, groups, s);                 // cross q-proj, folded pos MLP
    if (is(256, kProNone, false, true, false, kResPlain, false)) return go<256, 1, kProNone, false, true, false, kResPlain, false>(a, groups, s);  // self out-proj
    if (is(256, kProLN, true, true, false, kResNone, false)) return go<256, 1, kProLN, true, true, false, kResNone, false>(a, groups, s);          // cross q-proj
    if (is(256, kProNone, false, true, false, kResLN, false)) return go<256, 1, kProNone, false, true, false, kResLN, false>(a, groups, s);        // cross out-proj
    if (is(256, kProLN, false, true, true, kResNone, false)) {                                                                                     // FFN1
        return go_nt<3, 256, kProLN, false, true, true, kResNone, false>(a, groups, s);
    }
    if (is(768, kProNone, false, true, false, kResLN, false)) return go<768, 1, kProNone, false, true, false, kResLN, false>(a, groups, s);        // FFN2
    if (is(256, kProLN, false, true, false, kResNone, true)) {                                                                                     // heads layer 1
        return go_nt<3, 256, kProLN, false, true, false, kResNone, true>(a, groups, s);
    }
    if (is(256, kProGN, false, false, false, kResNone, true)) {                                                                                    // heads layer 2
        return go_nt<2, 256, kProGN, false, false, false, kResNone, true>(a, groups, s);
    }
    // ---- K = 1024 (the reference's shipped DEC_DIM): streamed-W kernel.  Sub-tiles: 4 (64 columns per workgroup: at one scene
    // N = 1024 gives 256 workgroups) where the addend / moment boundaries allow it
    // (W double-buffered in 256-step batches, 4 waves: measured 1.55 ms of linears per shipped-size forward, against 1.66 ms with
    // 8 waves splitting K and everything in flight at once)
    // 32-row form (chain_linear_stream32_kernel) for launches whose 32-row grid still has a workgroup per CU (512 lanes and ~200
    // registers: one per CU is all that fits).  Shipped geometry, per launch, 16-row -> 32-row (profiles/r06_ab_chain_rows32.txt):
    // one scene: head layer 1 34.9 -> 32.5 us, head layer 2 23.3 -> 18.5, self in-projection 30.8 -> 31.6, the N = 1024 launches
    // (128 workgroups: below the threshold) 10.8 -> 20; forward 2.380 -> 2.333 ms at one scene, 7.51 -> 6.82 ms at four
    constexpr int min_wg32 = 256;
    const bool rows32_ok = gm % 32 == 0 && a.M % 32 == 0 && (!a.gn_sums || a.gn_rows_per_scene % 32 == 0) &&
                           (!a.gn_out_sums || a.gn_out_rows_per_scene % 32 == 0);
    // Both tables below ask pick_nt(a, 4), which returns any of 4, 3, 2, 1 (N / 16 = 64: 4; 129 at head layer 1: 3; 2: 2; 1: 1), so
    // go_stream keeps all four forms.  The 32-row kernel was never instantiated with one sub-tile: nt == 1 goes to go_stream
#define PARQ_STREAM(PRO, ADD2, BIAS, RELU, RES, GNOUT)                                                          \
    {                                                                                                           \
        if (rows32_ok) {                                                                                        \
            const int nt = pick_nt(a, 4);                                                                       \
            if ((int64_t)(a.N / (16 * nt)) * (gm / 32) * groups >= min_wg32) {                                 \
                if (nt == 4) return go_stream32<1024, 4, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);      \
                if (nt == 3) return go_stream32<1024, 3, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);      \
                if (nt == 2) return go_stream32<1024, 2, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);      \
            }                                                                                                   \
        }                                                                                                       \
        const int nt = pick_nt(a, 4);                                                                           \
        if (nt == 4) return go_stream<1024, 4, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);                \
        if (nt == 3) return go_stream<1024, 3, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);                \
        if (nt == 2) return go_stream<1024, 2, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);                \
        return go_stream<1024, 1, PRO, ADD2, BIAS, RELU, RES, GNOUT>(a, groups, s);                             \
    }
    if (is(1024, kProNone, false, true, false, kResNone, false)) PARQ_STREAM(kProNone, false, true, false, kResNone, false)     // pe2
    if (is(1024, kProNone, true, true, false, kResNone, false)) PARQ_STREAM(kProNone, true, true, false, kResNone, false)       // self in-proj
    if (is(1024, kProNone, false, true, false, kResPlain, false)) PARQ_STREAM(kProNone, false, true, false, kResPlain, false)   // self out-proj
    if (is(1024, kProLN, true, true, false, kResNone, false)) PARQ_STREAM(kProLN, true, true, false, kResNone, false)           // cross q-proj
    if (is(1024, kProNone, false, true, false, kResLN, false)) PARQ_STREAM(kProNone, false, true, false, kResLN, false)         // cross out-proj
    if (is(1024, kProLN, false, true, true, kResNone, false)) PARQ_STREAM(kProLN, false, true, true, kResNone, false)           // FFN1
    if (is(1024, kProLN, false, true, false, kResNone, true)) PARQ_STREAM(kProLN, false, true, false, kResNone, true)           // heads layer 1
    if (is(1024, kProGN, false, false, false, kResNone, true)) PARQ_STREAM(kProGN, false, false, false, kResNone, true)         // heads layer 2
#undef PARQ_STREAM
    return hipErrorNotSupported;
}

hipError_t launch_pack_w_half(const float* W, int64_t ldw, int N, int K, float* dst, float* scales, hipStream_t s, const float* gamma,
                              const float* beta, const float* bias, float* bias_out) {
    if (N % 16 != 0 || K % 32 != 0 || (beta && !bias_out)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_w_half_kernel, dim3((unsigned)(N / 16)), dim3(256), 0, s, W, ldw, N, K, dst, scales, gamma, beta, bias, bias_out);
    return hipGetLastError();
}

hipError_t launch_pack_w_tiles(const float* W, int64_t ldw, int N, int K, float* dst, hipStream_t s) {
    if (N % 16 != 0 || K % 16 != 0 || ldw % 4 != 0) return hipErrorInvalidValue;
    const int64_t n4 = (int64_t)N * K / 4;
    hipLaunchKernelGGL(pack_w_tiles_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, W, ldw, N, K, dst);
    return hipGetLastError();
}

hipError_t launch_fold_pos_weights(const float* Wa, const float* ba, const float* W2, const float* b2, int R, int C, float* out_w, float* out_b,
                                   hipStream_t s) {
    const int64_t n = (int64_t)R * C;
    hipLaunchKernelGGL(fold_pos_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Wa, ba, W2, b2, R, C, out_w, out_b);
    return hipGetLastError();
}

// fused first launch of an iteration: pe1 (args `a`: K = 384, ReLU, bias) + project/sample.  hipErrorNotSupported when the shapes
// do not fit (the caller then launches the two stages separately).
template <int TT>
static void launch_pe1_sample_t(int nch, dim3 grid, dim3 block, size_t smem, hipStream_t s, const LinearArgs& a, const SampleArgs& sa, int n_lin) {
    switch (nch) {
        case 1: hipLaunchKernelGGL((pe1_sample_kernel<1, TT>), grid, block, smem, s, a, sa, n_lin); break;
        case 2: hipLaunchKernelGGL((pe1_sample_kernel<2, TT>), grid, block, smem, s, a, sa, n_lin); break;
        case 3: hipLaunchKernelGGL((pe1_sample_kernel<3, TT>), grid, block, smem, s, a, sa, n_lin); break;
        default: hipLaunchKernelGGL((pe1_sample_kernel<4, TT>), grid, block, smem, s, a, sa, n_lin); break;
    }
}

hipError_t launch_pe1_sample(const LinearArgs& a_in, const void* tokens, const double* T_cl, const float* cam, const float* ref, ScaleBox sb,
                             int B, int V, int h, int w, int C, int Q, float* tgt, float* coord_pos, double* zero_f64, int zero_n,
                             float* raw_count, hipStream_t s, const void* const* ind, int64_t coord_off, int tok_type) {
    if (tok_type != kTokF32 && tok_type != kTokF16 && tok_type != kTokBF16) return hipErrorInvalidValue;
    if (!chain_linear_supported(a_in, 1)) return hipErrorNotSupported;
    const Sig g = sig_of(a_in);
    if (!(g.K == 384 && g.pro == kProNone && g.add2 == 0 && g.bias && g.relu && g.res == kResNone && !g.gnout)) return hipErrorNotSupported;
    if (C % 4 != 0 || C > 1024 || V <= 0 || V > 16) return hipErrorNotSupported;
    LinearArgs a = a_in;
    if (a.Wp && (!al16(a.Wp) || a.ldw != a.K)) a.Wp = nullptr;
    a.tile_map = 0;
    const int n_lin = (a.N / 16) * (a.M / 16);
    const int nwv = V < 4 ? 4 : V;                                   // >= 4 waves: the linear tiles need 256 threads
    const size_t smem = (size_t)nwv * C * sizeof(float) + (size_t)nwv * sizeof(int) + (size_t)V * 32 + 16;
    SampleArgs sa{tokens, T_cl, cam, ref, sb, V, h, w, C, Q, tgt, coord_pos, zero_f64, zero_n, raw_count, ind, coord_off};
    const dim3 grid((unsigned)(n_lin + B * Q)), block(nwv * 64);
    const int nch = (C / 4 + 63) / 64;
    if (tok_type == kTokF16) launch_pe1_sample_t<kTokF16>(nch, grid, block, smem, s, a, sa, n_lin);
    else if (tok_type == kTokBF16) launch_pe1_sample_t<kTokBF16>(nch, grid, block, smem, s, a, sa, n_lin);
    else launch_pe1_sample_t<kTokF32>(nch, grid, block, smem, s, a, sa, n_lin);
    return hipGetLastError();
}

static bool fused_tile_ok(const LinearArgs& a) {
    return a.M % 16 == 0 && a.N == 256 && a.K == 256 && (a.ldx | a.ldw | a.y_row) % 4 == 0 && al16(a.X) && al16(a.W) && al16(a.Y) &&
           a.bias && al16(a.bias) && a.rows_per_batch == a.M && a.col_blk == a.N && !a.relu && !a.relu_mask && a.drop_p == 0.f && !a.X2 &&
           a.R && a.ldr % 4 == 0 && al16(a.R) && a.Wp && al16(a.Wp) && a.ldw == a.K && a.lnp_out && a.lnp_flags;
}
static bool seam_ok(const SeamArgs& b, int M, int nt) {
    return b.M == M && b.N % (16 * nt) == 0 && b.nparts == 4 && b.width == 256 && al16(b.X1) && al16(b.X2) && al16(b.W1p) && al16(b.W2p) &&
           (b.ldx1 | b.ldx2 | b.ldy) % 4 == 0 && al16(b.b1) && al16(b.srow) && (!b.b2 || al16(b.b2)) && al16(b.Y) && b.part && b.flags;
}

// xa tiles (+ published partial row sums) | q tiles: see seam_tile
hipError_t launch_seam_q(const LinearArgs& xa, const SeamArgs& q, hipStream_t s) {
    if (!fused_tile_ok(xa) || xa.rln_stats || !seam_ok(q, xa.M, 4) || !q.X3 || !al16(q.X3) || !al16(q.W3p) || q.ldx3 % 4 != 0) return hipErrorNotSupported;
    LinearArgs a = xa;
    a.tile_map = 0;
    // two column sub-tiles per query workgroup (against one and four: profiles/r05_ab_seam_query_tile_width.txt)
    const int nA = (a.N / 64) * (a.M / 16), nB = (q.N / 32) * (q.M / 16);
    hipLaunchKernelGGL((seam_q_kernel<2>), dim3((unsigned)(nA + nB)), dim3(256), 0, s, a, q, nA);
    return hipGetLastError();
}

hipError_t launch_ln_fold(const float* W, const float* b, const float* gamma, const float* beta, int R, int C, float* Wg, float* srow, float* bb, hipStream_t s) {
    hipLaunchKernelGGL(ln_fold_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, s, W, b, gamma, beta, R, C, Wg, srow, bb);
    return hipGetLastError();
}
hipError_t launch_matmul_fold(const float* A, const float* Bm, const float* bv, int R, int C, float* out, float* ob, hipStream_t s) {
    const int64_t n = (int64_t)R * C;
    hipLaunchKernelGGL(matmul_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, Bm, bv, R, C, out, ob);
    return hipGetLastError();
}

bool chain_linear_supported(const LinearArgs& a, int groups) {
    g_dry_run = true;
    const hipError_t e = launch_chain_linear(a, groups, nullptr);
    g_dry_run = false;
    return e == hipSuccess;
}

PARQ_TL_DEFINE_SETTER(tl_set_chain)

}  // namespace parq
