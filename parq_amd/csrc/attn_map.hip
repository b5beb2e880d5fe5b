// Cross-attention maps for gfx950: the probabilities the flash kernels only ever hold as MFMA fragments, written out on request
// (include/parq_hip.h parq_attention_map).  The reference forms them in every decoder layer and drops them
// (nn.MultiheadAttention with need_weights=True, model/transformer_parq.py:377-380).
//
//     P[b,h,q,n] = softmax_n( q_h[b,q] . k_h[b,n] / sqrt(dh) )          map = mean_h P
//
// q is the projected query the last iteration left in the workspace ("cross_q"), k is what that forward's K cache holds for the head.
// Nothing of the forward is reused beyond those two: the kernels compute their own row maxima and sums.
//
//   phase 0  attn_map_qfrag_kernel   the selected query rows, split hi + lo fp16, in MFMA fragment order (once per call)
//   phase 1  attn_map_stats_kernel   S^T = K Q^T per 32-key block (keys on the accumulator rows: a lane keeps ONE running maximum and
//                                    sum for its query), one (m, l) partial per query row and key split of kKeysPerSplit keys;
//            attn_map_merge_kernel   the partials in split order -> (m, 1 / l) per row
//   phase 2  attn_map_kernel         S = Q K^T recomputed per 32 x 32 tile (keys on the lanes), exp2(s - m) / l, the heads summed in
//                                    registers, one store per tile row: 32 lanes write 128 consecutive bytes along n.
//                                    The view mass (what = 2) sums the same tiles over a view's keys instead of storing them: fixed
//                                    segments of kViewSegKeys keys per view, summed in segment order by attn_map_view_kernel.
//
// Scores: the fp16 x 3 product of flash_split.hip (q_hi k_hi + q_hi k_lo + q_lo k_hi, v_mfma_f32_32x32x16_f16, fp32 accumulation).
// K fragments come straight from global memory: in the cache layouts a lane's 8 contraction elements are one 16-byte chunk of the
// block (kv_layout.hpp), so there is no LDS stage and no barrier; the contraction order over d is the cache's (kv_dmap), and
// phase 0 orders q the same way.  Per layout (a head of "split8" with tiers is read in the layout ITS region has):
//   fp32 K (mode 0, head dims without a cache)   split in registers, d in natural order
//   split cache                                  hi, lo as stored
//   single fp16 cache                            the value, no lo term
//   single bf16 cache                            the value widened and split (exact within the fp16 range)
//   mode-4 stages                                hi16 as stored, lo = the e4m3 residual decoded and scaled by 2^-10 (exact in fp16)
// The key partition of both phases depends on N only, never on the selection: a row's numbers are the same bits whichever rows are
// computed beside it, and two calls give the same bits (no atomics anywhere).
#include "common.hpp"

namespace parq {

namespace {

constexpr int kKeysPerSplit = 512;                  // keys of one statistics partial
constexpr int kSplitBlks = kKeysPerSplit / 32;
constexpr int kViewSegKeys = 256;                   // keys of one view-mass segment
// Phase 2 takes ONE 32-key block per wave and pass.  Measured at BASELINE cfg 3 (full map, ms) with 1 / 2 / 4 blocks per pass: 0.605 /
// 0.618 / 0.770 — more blocks reuse the q fragments but cost registers (three waves per SIMD at 1), and the kernel lives on waves in
// flight, not on reuse

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

struct KHead { const char* p; int lay; };

// where K of (scene b, head h, 64-dim group g of the head) starts, and in which layout
__device__ __forceinline__ KHead k_head(const AttnMapArgs& a, int b, int h, int g) {
    KHead r;
    r.lay = (a.klayout == kMapStage8 && ((a.safe_mask >> h) & 1u)) ? kMapSplit3 : a.klayout;
    if (a.klayout == kMapF32) r.p = reinterpret_cast<const char*>(a.kbase) + ((int64_t)b * 2 * a.N * a.C + (int64_t)h * a.N * a.dh) * 4;
    else r.p = reinterpret_cast<const char*>(a.kbase) + ((int64_t)b * (a.C / 64) + (int64_t)h * (a.dh / 64) + g) * a.head_bytes;
    return r;
}

// the fragment of contraction step s (16 dims; fp32 layout: step of the whole head, cache layouts: step 0..3 of the 64-dim group) of
// key `key` of block `blk` for lane half kh: 8 elements as hi + lo fp16
// LAY is a template parameter: the kernels are instantiated per layout (a runtime switch at each of the unrolled call sites made the
// kernels several times larger than the instruction cache)
template <int LAY>
__device__ __forceinline__ void load_kfrag(const KHead& k, const AttnMapArgs& a, int blk, int key, int kh, int s, half8& hi, half8& lo) {
    const int pos = kv_kswz(key, 4 * kh + s) * 8 + key * 64;      // 16-bit units inside a K plane of the cache layouts
    if constexpr (LAY == kMapF32) {
        int64_t n = (int64_t)blk * 32 + key;
        n = n < a.N ? n : a.N - 1;
        const float* p = reinterpret_cast<const float*>(k.p) + n * a.dh + 16 * s + 8 * kh;
        const f32x4 u = *reinterpret_cast<const f32x4*>(p), v = *reinterpret_cast<const f32x4*>(p + 4);
        const float x[8] = {u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
        split8(x, hi, lo);
    } else if constexpr (LAY == kMapSplit3) {
        const _Float16* p = reinterpret_cast<const _Float16*>(k.p + (int64_t)blk * KvBlk<3>::bytes);
        hi = *reinterpret_cast<const half8*>(p + pos);
        lo = *reinterpret_cast<const half8*>(p + KvBlk<3>::k_lo + pos);
    } else if constexpr (LAY == kMapF16) {
        const _Float16* p = reinterpret_cast<const _Float16*>(k.p + (int64_t)blk * KvBlk<1>::bytes);
        hi = *reinterpret_cast<const half8*>(p + pos);
        lo = half8{0, 0, 0, 0, 0, 0, 0, 0};
    } else if constexpr (LAY == kMapBF16) {
        const _Float16* p = reinterpret_cast<const _Float16*>(k.p + (int64_t)blk * KvBlk<1>::bytes);
        const u32x4 raw = *reinterpret_cast<const u32x4*>(p + pos);
        float x[8];
        widen8<kTokBF16>(raw, x);
        split8(x, hi, lo);
    } else {        // kMapStage8: a 64-key stage holds two blocks
        const char* st = k.p + (int64_t)(blk >> 1) * kStage8Bytes;
        const int b2 = blk & 1;
        hi = *reinterpret_cast<const half8*>(st + kS8Kh16 + b2 * kS8Blk16Bytes + pos * 2);
        // piece (b2, c = s & 1, kh) of the key, bytes 8 (s >> 1) .. + 7: d = kv_dmap(kh, s, e)
        const int piece = kv_piece8(b2, s & 1, kh, key);
        const uint2 w = *reinterpret_cast<const uint2*>(st + kS8K8lo + piece * kS8PieceBytes + 8 * (s >> 1));
        const auto f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
        const auto f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
        constexpr float inv = 1.f / kLo8Scale;      // e4m3 x 2^-10: at most 4 significant bits, >= 2^-19 — exact in fp16
        lo = half8{(_Float16)(f0[0] * inv), (_Float16)(f0[1] * inv), (_Float16)(f1[0] * inv), (_Float16)(f1[1] * inv),
                   (_Float16)(f2[0] * inv), (_Float16)(f2[1] * inv), (_Float16)(f3[0] * inv), (_Float16)(f3[1] * inv)};
    }
}

__device__ __forceinline__ const half8* qfrag_ptr(const AttnMapArgs& a, int b, int h, int tile, int s, int lane) {
    return a.qfrag + ((((int64_t)(b * a.H + h) * a.qtiles + tile) * (a.dh / 16) + s) * 2) * 64 + lane;
}

__device__ __forceinline__ f32x16 mfma_h(half8 x, half8 y, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0); }

__device__ __forceinline__ void store_p(void* out, int out_f16, int64_t idx, float v) {
    if (out_f16) reinterpret_cast<unsigned short*>(out)[idx] = (unsigned short)(round2_tok16<kTokF16>(v, 0.f) & 0xffffu);
    else reinterpret_cast<float*>(out)[idx] = v;
}

// ---- phase 0: selected query rows -> hi / lo fragments.  grid (query tiles, H, B), one wave.
__global__ __launch_bounds__(64) void attn_map_qfrag_kernel(AttnMapArgs a, const float* __restrict__ qc, const int* __restrict__ sel, int Q,
                                                            half8* __restrict__ dst) {
    const int lane = threadIdx.x, row = lane & 31, kh = lane >> 5;
    const int tile = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int qi = tile * 32 + row;
    int src = -1;
    if (qi < a.nsel) {
        src = sel ? sel[qi] : qi;
        src = src < 0 ? 0 : (src >= Q ? Q - 1 : src);          // (the caller checks its indices; this only keeps the read inside cross_q)
    }
    const float* qp = qc + ((int64_t)b * Q + (src < 0 ? 0 : src)) * a.C + h * a.dh;
    const int nsteps = a.dh / 16;
    for (int s = 0; s < nsteps; ++s) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = a.klayout == kMapF32 ? 16 * s + 8 * kh + e : 64 * (s >> 2) + kv_dmap(kh, s & 3, e);
            x[e] = src < 0 ? 0.f : qp[d];
        }
        half8 hi, lo;
        split8(x, hi, lo);
        half8* o = dst + ((((int64_t)(b * a.H + h) * a.qtiles + tile) * nsteps + s) * 2) * 64 + lane;
        o[0] = hi;
        o[64] = lo;
    }
}

// ---- phase 1: one (m, l) per query row and key split (log2 domain).  grid (nsplit, ceil(query tiles / 4), B * H); the four waves of a
// workgroup take four query tiles of the SAME keys, so that a K chunk is fetched from L2 once per workgroup and found in the CU's
// vector cache by the other three.
template <int NSTEPS, int LAY>
__device__ __forceinline__ void stats_body(const AttnMapArgs& a, int lane, int split, int tile, int bh) {
    const int col = lane & 31, kh = lane >> 5;
    const int b = bh / a.H, h = bh - b * a.H;
    constexpr int NG = (NSTEPS + 3) / 4;
    half8 qh[NSTEPS], ql[NSTEPS];
#pragma unroll
    for (int s = 0; s < NSTEPS; ++s) {
        const half8* p = qfrag_ptr(a, b, h, tile, s, lane);
        qh[s] = p[0];
        ql[s] = p[64];
    }
    KHead kd[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) kd[g] = k_head(a, b, h, g);
    const int nblk = (a.N + 31) / 32;
    const int blk_end = (split + 1) * kSplitBlks < nblk ? (split + 1) * kSplitBlks : nblk;
    float m = -INFINITY, l = 0.f;
    for (int blk = split * kSplitBlks; blk < blk_end; ++blk) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            half8 khi, klo;
            load_kfrag<LAY>(kd[s >> 2], a, blk, col, kh, LAY == kMapF32 ? s : (s & 3), khi, klo);
            if (LAY != kMapF16) acc = mfma_h(klo, qh[s], acc);
            acc = mfma_h(khi, ql[s], acc);
            acc = mfma_h(khi, qh[s], acc);
        }
        float t[16], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            t[r] = n < a.N ? acc[r] * a.scale_log2 : -INFINITY;
            mx = fmaxf(mx, t[r]);
        }
        if (mx > m) { l *= fexp2(m - mx); m = mx; }
        if (m > -INFINITY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) l += fexp2(t[r] - m);
        }
    }
    // the two lane halves hold the two halves of every block's keys
    const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32);
    const float M = fmaxf(m, mo);
    float L = 0.f;
    if (M > -INFINITY) {
        const float x = m > -INFINITY ? l * fexp2(m - M) : 0.f, y = mo > -INFINITY ? lo * fexp2(mo - M) : 0.f;
        L = x + y;
    }
    if (kh == 0) {
        const int64_t o = ((int64_t)bh * a.nsplit + split) * a.nsel_pad + tile * 32 + col;
        a.part_m[o] = M;
        a.part_l[o] = L;
    }
}

template <int NSTEPS, int LAY>
__global__ __launch_bounds__(256) void attn_map_stats_kernel(AttnMapArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int split = blockIdx.x;
    const int tile = blockIdx.y * 4 + wave, bh = blockIdx.z;
    if (tile >= a.qtiles) return;
    if constexpr (LAY == kMapStage8) {          // per-head tiers: this head's region may be in the split layout
        if ((a.safe_mask >> (bh % a.H)) & 1u) { stats_body<NSTEPS, kMapSplit3>(a, lane, split, tile, bh); return; }
    }
    stats_body<NSTEPS, LAY>(a, lane, split, tile, bh);
}

// partials in split order -> row maximum and reciprocal row sum.  One thread per (b * H + h, padded row).
__global__ void attn_map_merge_kernel(AttnMapArgs a, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const int64_t bh = i / a.nsel_pad, q = i - bh * a.nsel_pad;
    const float* pm = a.part_m + bh * a.nsplit * a.nsel_pad + q;
    const float* pl = a.part_l + bh * a.nsplit * a.nsel_pad + q;
    float M = -INFINITY;
    for (int s = 0; s < a.nsplit; ++s) M = fmaxf(M, pm[(int64_t)s * a.nsel_pad]);
    float L = 0.f;
    for (int s = 0; s < a.nsplit; ++s) {
        const float ms = pm[(int64_t)s * a.nsel_pad];
        if (ms > -INFINITY) L += pl[(int64_t)s * a.nsel_pad] * fexp2(ms - M);
    }
    a.stat_m[i] = M;
    a.stat_il[i] = 1.f / L;
}

// ---- phase 2.  WHAT 0 / 1: grid (32-key blocks, ceil(query tiles / 4), B).
//               WHAT 2: grid (V * nseg, ceil(query tiles / 4), B): (view, segment), one block per pass over the segment.
// The four waves of a workgroup take four query tiles of the same keys (see phase 1).
// the score tile of head h for block blk
template <int LAY>
__device__ __forceinline__ void head_scores(const AttnMapArgs& a, int b, int h, int tile, int lane, int blk, f32x16& sacc) {
    const int col = lane & 31, kh = lane >> 5;
    const int ngroups = (a.dh + 63) / 64, nsteps = a.dh / 16;
    for (int g = 0; g < ngroups; ++g) {
        const KHead kd = k_head(a, b, h, g);
        const int ns = nsteps - 4 * g < 4 ? nsteps - 4 * g : 4;
        half8 qh[4], ql[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < ns) {
                const half8* p = qfrag_ptr(a, b, h, tile, 4 * g + s, lane);
                qh[s] = p[0];
                ql[s] = p[64];
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < ns) {
                half8 khi, klo;
                load_kfrag<LAY>(kd, a, blk, col, kh, LAY == kMapF32 ? 4 * g + s : s, khi, klo);
                if (LAY != kMapF16) sacc = mfma_h(qh[s], klo, sacc);
                sacc = mfma_h(ql[s], khi, sacc);
                sacc = mfma_h(qh[s], khi, sacc);
            }
        }
    }
}

template <int WHAT, int LAY>
__global__ __launch_bounds__(256) void attn_map_kernel(AttnMapArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, kh = lane >> 5;
    const int tile = blockIdx.y * 4 + wave, b = blockIdx.z;
    const int unit = blockIdx.x;
    if (tile >= a.qtiles) return;
    int64_t lo, hi;
    if (WHAT == 2) {
        const int v = unit / a.nseg, seg = unit - v * a.nseg;
        lo = (int64_t)v * a.hw + (int64_t)seg * kViewSegKeys;
        hi = lo + kViewSegKeys < (int64_t)(v + 1) * a.hw ? lo + kViewSegKeys : (int64_t)(v + 1) * a.hw;
    } else {
        lo = (int64_t)unit * 32;
        if (lo >= a.N) return;
        hi = lo + 32 < a.N ? lo + 32 : a.N;
    }
    const float invH = 1.f / (float)a.H;
    f32x16 vacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) vacc[r] = 0.f;
    // (lo < hi <= N: every block of the loop starts inside the keys)
    for (int blk = (int)(lo >> 5); (int64_t)blk * 32 < hi; ++blk) {
        const int64_t n = (int64_t)blk * 32 + col;
        const bool in = n >= lo && n < hi;
        f32x16 pacc, sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) pacc[r] = 0.f;
        for (int h = 0; h < a.H; ++h) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
            if (LAY == kMapStage8 && ((a.safe_mask >> h) & 1u)) head_scores<kMapSplit3>(a, b, h, tile, lane, blk, sacc);   // per-head tiers
            else head_scores<LAY>(a, b, h, tile, lane, blk, sacc);
            // this lane's 16 rows: (r & 3) + 8 (r >> 2) + 4 kh
            const int64_t so = (int64_t)(b * a.H + h) * a.nsel_pad + tile * 32 + 4 * kh;
            f32x4 m4[4], l4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m4[j] = *reinterpret_cast<const f32x4*>(a.stat_m + so + 8 * j);
                l4[j] = *reinterpret_cast<const f32x4*>(a.stat_il + so + 8 * j);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = in ? fexp2(sacc[r] * a.scale_log2 - m4[r >> 2][r & 3]) * l4[r >> 2][r & 3] : 0.f;
                if (WHAT == 1) {
                    const int q = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (in && q < a.nsel) store_p(a.out, a.out_f16, (((int64_t)b * a.H + h) * a.nsel + q) * a.N + n, p);
                } else {
                    pacc[r] += p;
                }
            }
        }
        if (WHAT == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (n < hi && q < a.nsel) store_p(a.out, a.out_f16, ((int64_t)b * a.nsel + q) * a.N + n, pacc[r] * invH);
            }
        }
        if (WHAT == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) vacc[r] += pacc[r];
        }
    }
    if (WHAT == 2) {
        const int v = unit / a.nseg, seg = unit - v * a.nseg;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float x = vacc[r];
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) x += __shfl_xor(x, d);       // over the 32 keys of the lane half, fixed order
            const int q = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (col == 0) a.vpart[(((int64_t)b * a.nsel_pad + q) * a.V + v) * a.nseg + seg] = x;
        }
    }
}

// view mass: a view's segments in order, the head mean.  One thread per (b, selected row, view).
__global__ void attn_map_view_kernel(AttnMapArgs a, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int v = (int)(i % a.V);
    const int64_t bq = i / a.V;
    const int q = (int)(bq % a.nsel);
    const int64_t b = bq / a.nsel;
    const float* p = a.vpart + ((b * a.nsel_pad + q) * a.V + v) * a.nseg;
    float s = 0.f;
    for (int k = 0; k < a.nseg; ++k) s += p[k];
    store_p(a.out, a.out_f16, i, s * (1.f / (float)a.H));
}

inline int64_t up64(int64_t x) { return (x + 63) / 64 * 64; }

struct Carve { int64_t qfrag, part_m, part_l, stat_m, stat_il, vpart, total; int qtiles, nsel_pad, nsplit, nseg; };

Carve carve(int B, int H, int dh, int N, int V, int hw, int nsel) {
    Carve c;
    c.qtiles = (nsel + 31) / 32;
    c.nsel_pad = c.qtiles * 32;
    c.nsplit = (N + kKeysPerSplit - 1) / kKeysPerSplit;
    c.nseg = (hw + kViewSegKeys - 1) / kViewSegKeys;
    int64_t off = 0;                                     // in floats
    auto take = [&](int64_t n) { const int64_t o = off; off += up64(n); return o; };
    c.qfrag = take((int64_t)B * H * c.nsel_pad * dh);    // hi + lo fp16 of every element
    c.part_m = take((int64_t)B * H * c.nsplit * c.nsel_pad);
    c.part_l = take((int64_t)B * H * c.nsplit * c.nsel_pad);
    c.stat_m = take((int64_t)B * H * c.nsel_pad);
    c.stat_il = take((int64_t)B * H * c.nsel_pad);
    c.vpart = take((int64_t)B * c.nsel_pad * V * c.nseg);
    c.total = off;
    return c;
}

}  // namespace

size_t attn_map_scratch_bytes(int B, int H, int dh, int N, int V, int hw, int nsel) {
    return (size_t)carve(B, H, dh, N, V, hw, nsel).total * sizeof(float);
}

// `a`: kbase, klayout, safe_mask, head_bytes, B, H, dh, C, N, V, hw, nsel, what, out, out_f16 set by the caller
hipError_t launch_attn_map(AttnMapArgs a, const float* cross_q, const int* query_index, int Q, void* scratch, hipStream_t s) {
    if (a.dh != 32 && a.dh != 64 && a.dh != 128 && a.dh != 256) return hipErrorNotSupported;
    if (a.klayout != kMapF32 && a.dh != 64 && a.dh != 256) return hipErrorNotSupported;      // the cache layouts exist for these two only
    const Carve c = carve(a.B, a.H, a.dh, a.N, a.V, a.hw, a.nsel);
    if (c.qtiles > 65535 || (int64_t)a.B * a.H > 65535) return hipErrorInvalidValue;
    float* sp = reinterpret_cast<float*>(scratch);
    a.qtiles = c.qtiles; a.nsel_pad = c.nsel_pad; a.nsplit = c.nsplit; a.nseg = c.nseg;
    a.qfrag = reinterpret_cast<const half8*>(sp + c.qfrag);
    a.part_m = sp + c.part_m; a.part_l = sp + c.part_l; a.stat_m = sp + c.stat_m; a.stat_il = sp + c.stat_il; a.vpart = sp + c.vpart;
    a.scale_log2 = 1.4426950408889634f / sqrtf((float)a.dh);
    hipLaunchKernelGGL(attn_map_qfrag_kernel, dim3(c.qtiles, a.H, a.B), dim3(64), 0, s, a, cross_q, query_index, Q,
                       reinterpret_cast<half8*>(sp + c.qfrag));
    const dim3 gs(c.nsplit, (c.qtiles + 3) / 4, a.B * a.H);
#define PARQ_MAP_STATS(NS, L) hipLaunchKernelGGL((attn_map_stats_kernel<NS, L>), gs, dim3(256), 0, s, a)
#define PARQ_MAP_STATS_CACHE(L)                                 \
    do {                                                        \
        if (a.dh == 64) PARQ_MAP_STATS(4, L);                   \
        else if (a.dh == 256) PARQ_MAP_STATS(16, L);            \
        else return hipErrorNotSupported;                       \
    } while (0)
    switch (a.klayout) {
    case kMapF32:
        if (a.dh == 32) PARQ_MAP_STATS(2, kMapF32);
        else if (a.dh == 64) PARQ_MAP_STATS(4, kMapF32);
        else if (a.dh == 128) PARQ_MAP_STATS(8, kMapF32);
        else PARQ_MAP_STATS(16, kMapF32);
        break;
    case kMapSplit3: PARQ_MAP_STATS_CACHE(kMapSplit3); break;
    case kMapF16: PARQ_MAP_STATS_CACHE(kMapF16); break;
    case kMapBF16: PARQ_MAP_STATS_CACHE(kMapBF16); break;
    case kMapStage8: PARQ_MAP_STATS(4, kMapStage8); break;
    default: return hipErrorInvalidValue;
    }
    const int64_t rows = (int64_t)a.B * a.H * c.nsel_pad;
    hipLaunchKernelGGL(attn_map_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, a, rows);
#define PARQ_MAP_LAUNCH(W, G)                                                                                               \
    switch (a.klayout) {                                                                                                    \
    case kMapF32: hipLaunchKernelGGL((attn_map_kernel<W, kMapF32>), G, dim3(256), 0, s, a); break;                          \
    case kMapSplit3: hipLaunchKernelGGL((attn_map_kernel<W, kMapSplit3>), G, dim3(256), 0, s, a); break;                    \
    case kMapF16: hipLaunchKernelGGL((attn_map_kernel<W, kMapF16>), G, dim3(256), 0, s, a); break;                          \
    case kMapBF16: hipLaunchKernelGGL((attn_map_kernel<W, kMapBF16>), G, dim3(256), 0, s, a); break;                        \
    default: hipLaunchKernelGGL((attn_map_kernel<W, kMapStage8>), G, dim3(256), 0, s, a); break;                            \
    }
    if (a.what == 2) {
        const dim3 gv(a.V * c.nseg, (c.qtiles + 3) / 4, a.B);
        PARQ_MAP_LAUNCH(2, gv);
        const int64_t total = (int64_t)a.B * a.nsel * a.V;
        hipLaunchKernelGGL(attn_map_view_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, total);
    } else {
        const dim3 gm((a.N + 31) / 32, (c.qtiles + 3) / 4, a.B);
        if (a.what == 1) { PARQ_MAP_LAUNCH(1, gm); }
        else { PARQ_MAP_LAUNCH(0, gm); }
    }
#undef PARQ_MAP_LAUNCH
#undef PARQ_MAP_STATS_CACHE
#undef PARQ_MAP_STATS
    return hipGetLastError();
}

}  // namespace parq
