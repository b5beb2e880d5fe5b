// Average precision per (IoU threshold, class) on the device from the evaluator's two track stores (include/parq_hip.h:
// parq_average_precision, where the rule is stated in full; its NumPy statement is tests/average_precision_cases.py ap_statement).
// The reference's evaluator has no AP: the oracle is that statement and an independent sequential formulation.
//
// Launch 1, ap_target_kernel: a workgroup of kApWaves wavefronts per (scene, block of kApRows prediction rows).  A wavefront owns a
//   prediction at a time: its lanes stride the scene's ground truth, skip boxes of another class before the clip, run obb_pair.hpp's
//   routine with the ground truth as the first box (f1_counts.hip with the sides swapped: the two see one IoU matrix), keep the
//   maximum with the first index that reaches it, and a butterfly takes the wave-wide (maximum, lowest index).  The workgroup also
//   writes the 64-bit sort key of each of its store positions, class | ~score key | slot * capacity + position, all ones for a
//   position that is not ranked, and its share of the all-ones padding; block 0 of a scene counts the labels of both sides.
// Launch 2, ap_counts_kernel: one workgroup sums the per-scene label counts into counts / invalid and lays the classes out one after
//   another (class_start).
// Launch 3, ap_flags_kernel: one workgroup per scene, the scene's keys, maxima and targets in LDS.  A prediction is a true positive at
//   threshold t when its maximum passes and no prediction of the scene with the same target and a smaller key passes too: T bits.
// Launches 4.., the sort: a bitonic network over the padded keys, every stride below the tile inside LDS (ap_sort_tile_kernel,
//   ap_sort_merge_kernel), the others one compare-exchange per lane in global memory (ap_sort_step_kernel).  Keys are unique.
// Last launch, ap_curve_kernel: one workgroup per (class, threshold) walks its segment of the sorted keys in chunks of 256: the
//   cumulative true positives left to right, then right to left the precision, its running maximum, and the sum, which wavefront 0
//   takes one true-positive rank at a time in DESCENDING rank (the order is part of the rule).  Column K of the grid fills the tail.
// No atomics, no scratch, nothing allocated; the number and geometry of the launches depend on the arguments alone.  Every count,
// class_start and key read back from device memory is checked before it indexes anything.  Contraction off, as everywhere the IoU runs.
#include "obb_pair.hpp"

#include <algorithm>

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kApWaves = 2, kApRows = 16;        // 2 x 24 KB of polygon buffers per workgroup; 8 predictions per wavefront, in turn
static_assert(kApWaves == 2, "block 0 counts the labels of the two sides with a wavefront each");
constexpr int kApThreads = 256;                  // flags, sort and curve kernels
constexpr int kApTile = 2048;                    // keys of a sort tile: 16 KB of LDS
constexpr int kApSide = 2048;                    // the largest capacity of a store
constexpr uint64_t kApNoKey = ~0ull;
constexpr uint32_t kApIndexMask = (uint32_t)kApMaxPositions - 1;

__device__ __forceinline__ const int32_t* ap_slot(const int32_t* store, int slot, int mt) { return store + (int64_t)slot * (2 + 26 * (int64_t)mt); }

__device__ __forceinline__ int ap_count(const int32_t* slot, int mt) {
    const int32_t n = slot[0];
    return (n >= 0 && n <= mt) ? n : 0;
}

__device__ __forceinline__ const float* ap_corners(const int32_t* slot, int mt, int t) {
    return reinterpret_cast<const float*>(slot + 2 + 2 * (int64_t)mt) + (int64_t)t * 24;
}

// ranked: label in [0, K) and a score that is not NaN (the score as its 32 bits)
__device__ __forceinline__ bool ap_ranked(int32_t cls, uint32_t bits, int K) { return cls >= 0 && cls < K && (bits & 0x7fffffffu) <= 0x7f800000u; }

struct ApLayout {
    size_t keys, best, target, flags, partial, cstart, cum, total;
};

__host__ __device__ inline size_t ap_up16(size_t x) { return (x + 15) & ~(size_t)15; }

inline int64_t ap_padded(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

inline ApLayout ap_layout(int S, int pred_mt, int T, int K) {
    const size_t N = (size_t)S * (size_t)pred_mt;
    ApLayout l;
    size_t off = 0;
    l.keys = off;    off += ap_up16((size_t)ap_padded((int64_t)N) * 8);
    l.best = off;    off += ap_up16(N * 8);
    l.target = off;  off += ap_up16(N * 4);
    l.flags = off;   off += ap_up16(N);
    l.partial = off; off += ap_up16((size_t)S * 2 * (size_t)(K + 1) * 4);
    l.cstart = off;  off += ap_up16((size_t)(K + 1) * 4);
    l.cum = off;     off += ap_up16((size_t)T * N * 4);
    l.total = off;
    return l;
}

__global__ __launch_bounds__(kApWaves* kWave) void ap_target_kernel(const int32_t* __restrict__ pred_store, int pred_mt,
                                                                    const int32_t* __restrict__ gt_store, int gt_mt, int K, int64_t N,
                                                                    int64_t Npad, uint64_t* __restrict__ keys, double* __restrict__ best_out,
                                                                    int32_t* __restrict__ target_out, int32_t* __restrict__ partial) {
    __shared__ ObbPolyLds lds[kApWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int scene = blockIdx.y, blk = blockIdx.x;
    const int32_t* gs = ap_slot(gt_store, scene, gt_mt);
    const int32_t* ps = ap_slot(pred_store, scene, pred_mt);
    const int ng = ap_count(gs, gt_mt), np = ap_count(ps, pred_mt);
    const int row0 = blk * kApRows;
    // the keys of this workgroup's store positions, ranked or not
    for (int j = row0 + tid; j < min(pred_mt, row0 + kApRows); j += kApWaves * kWave) {
        uint64_t key = kApNoKey;
        if (j < np) {
            const int32_t cls = ps[2 + j];
            const uint32_t b = (uint32_t)ps[2 + pred_mt + j];
            if (ap_ranked(cls, b, K)) {
                const uint32_t skey = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
                key = ((uint64_t)cls << 52) | ((uint64_t)(uint32_t)~skey << 20) | (uint64_t)((int64_t)scene * pred_mt + j);
            }
        }
        keys[(int64_t)scene * pred_mt + j] = key;
    }
    {   // the padding behind the last position, shared out among all workgroups
        const int64_t lin = (int64_t)scene * gridDim.x + blk, all = (int64_t)gridDim.x * gridDim.y * (kApWaves * kWave);
        for (int64_t i = N + lin * (kApWaves * kWave) + tid; i < Npad; i += all) keys[i] = kApNoKey;
    }
    const int row_end = min(np, row0 + kApRows);
    for (int j = row0 + wave; j < row_end; j += kApWaves) {
        const int32_t cls = ps[2 + j];
        double m = -1.0;                                                    // nothing seen
        int idx = -1;
        if (ap_ranked(cls, (uint32_t)ps[2 + pred_mt + j], K)) {             // wave-uniform
            Corners cp;
            const bool bad_p = load_canonical(ap_corners(ps, pred_mt, j), cp);
            for (int i0 = 0; i0 < ng; i0 += kWave) {
                const int i = i0 + lane;
                if (i < ng && gs[2 + i] == cls) {
                    Corners cg;
                    const bool bad_g = load_canonical(ap_corners(gs, gt_mt, i), cg);
                    double r3, r2;
                    obb_pair_iou(cg, bad_g, cp, bad_p, lds[wave], lane, r3, r2);
                    if (r3 > m) {                                           // strict: the first index that reaches it; a NaN never does
                        m = r3;
                        idx = i;
                    }
                }
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const double om = __shfl_xor(m, off, kWave);
                const int oi = __shfl_xor(idx, off, kWave);
                if (om > m || (om == m && (unsigned)oi < (unsigned)idx)) {
                    m = om;
                    idx = oi;
                }
            }
        }
        if (lane == 0) {
            best_out[(int64_t)scene * pred_mt + j] = idx >= 0 ? m : 0.0;
            target_out[(int64_t)scene * pred_mt + j] = idx;
        }
    }
    if (blk == 0) {
        // the labels of both sides: wave 0 the ground truth, wave 1 the predictions; lane c keeps class c, element K the rest
        const int32_t* side = wave == 0 ? gs : ps;
        const int n = wave == 0 ? ng : np;
        int mine = 0, bad = 0;
        for (int j0 = 0; j0 < n; j0 += kWave) {
            const int j = j0 + lane;
            const int32_t cls = j < n ? side[2 + j] : -1;
            const bool in = j < n && (wave == 0 ? (cls >= 0 && cls < K) : ap_ranked(cls, (uint32_t)side[2 + pred_mt + j], K));
            bad += __popcll(__ballot(j < n && !in));
            for (int c = 0; c < K; ++c) {
                const int hits = __popcll(__ballot(in && cls == c));
                if (lane == c) mine += hits;
            }
        }
        int32_t* out = partial + ((int64_t)scene * 2 + wave) * (K + 1);
        if (lane < K) out[lane] = mine;
        if (lane == K) out[K] = bad;
    }
}

// counts (2, K), invalid (2) and class_start (K + 1) from the per-scene label counts; one workgroup, a wavefront per element in turn
__global__ __launch_bounds__(kApThreads) void ap_counts_kernel(const int32_t* __restrict__ partial, int S, int K, int64_t* __restrict__ counts,
                                                               int64_t* __restrict__ invalid, int32_t* __restrict__ cstart,
                                                               int32_t* __restrict__ cstart_out) {
    __shared__ long long ranked[kF1MaxClasses];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int e = wave; e < 2 * (K + 1); e += kApThreads / kWave) {
        const int side = e / (K + 1), c = e - side * (K + 1);
        long long sum = 0;
        for (int s = lane; s < S; s += kWave) sum += partial[((int64_t)s * 2 + side) * (K + 1) + c];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
        if (lane == 0) {
            if (c < K) {
                counts[side * K + c] = sum;
                if (side == 1) ranked[c] = sum;
            } else {
                invalid[side] = sum;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        long long at = 0;
        for (int c = 0; c <= K; ++c) {
            cstart[c] = (int32_t)at;
            if (cstart_out) cstart_out[c] = (int32_t)at;
            if (c < K) at += ranked[c];
        }
    }
}

// T flag bits per prediction: bit t set = a true positive at threshold t
__global__ __launch_bounds__(kApThreads) void ap_flags_kernel(const int32_t* __restrict__ pred_store, int pred_mt, F1Thresholds thr, int T,
                                                              const uint64_t* __restrict__ keys, const double* __restrict__ best,
                                                              const int32_t* __restrict__ target, unsigned char* __restrict__ flags) {
    __shared__ uint64_t s_key[kApSide];
    __shared__ int32_t s_tgt[kApSide];
    __shared__ unsigned char s_pass[kApSide];
    const int tid = threadIdx.x, scene = blockIdx.x;
    const int np = ap_count(ap_slot(pred_store, scene, pred_mt), pred_mt);
    const int64_t base = (int64_t)scene * pred_mt;
    for (int p = tid; p < np; p += kApThreads) {
        const int32_t tg = target[base + p];
        const double b = best[base + p];
        unsigned pass = 0;
        if (tg >= 0) {
#pragma unroll
            for (int t = 0; t < kF1MaxThresholds; ++t)
                if (t < T && b > thr.thr[t]) pass |= 1u << t;               // float64, strict
        }
        s_key[p] = keys[base + p];
        s_tgt[p] = tg;
        s_pass[p] = (unsigned char)pass;
    }
    __syncthreads();
    for (int p = tid; p < np; p += kApThreads) {
        const int32_t tg = s_tgt[p];
        const uint64_t key = s_key[p];
        unsigned pass = s_pass[p], blocked = 0;
        if (pass) {
            for (int q = 0; q < np; ++q)
                if (s_tgt[q] == tg && s_key[q] < key) blocked |= s_pass[q];   // an earlier claimant of the same box
        }
        flags[base + p] = (unsigned char)(pass & ~blocked);
    }
}

__device__ __forceinline__ void ap_cmpx(uint64_t& a, uint64_t& b, bool up) {
    if (up ? a > b : a < b) {
        const uint64_t t = a;
        a = b;
        b = t;
    }
}

// the network's steps (k, j) with j < tile inside LDS: k_only = 0 runs every k up to the tile, else the strides below the tile of that k
__global__ __launch_bounds__(kApThreads) void ap_sort_tile_kernel(uint64_t* __restrict__ keys, int tile, int64_t k_only) {
    __shared__ uint64_t s[kApTile];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * tile;
    for (int i = tid; i < tile; i += kApThreads) s[i] = keys[base + i];
    for (int64_t k = k_only ? k_only : 2; k <= (k_only ? k_only : (int64_t)tile); k <<= 1) {
        for (int j = k > (int64_t)tile ? tile >> 1 : (int)(k >> 1); j > 0; j >>= 1) {
            __syncthreads();
            for (int p = tid; p < tile / 2; p += kApThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                ap_cmpx(s[i], s[l], ((base + i) & k) == 0);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < tile; i += kApThreads) keys[base + i] = s[i];
}

// one step (k, j) with j >= tile: a compare-exchange per lane
__global__ __launch_bounds__(kApThreads) void ap_sort_step_kernel(uint64_t* __restrict__ keys, int64_t half, int64_t k, int64_t j) {
    const int64_t p = (int64_t)blockIdx.x * kApThreads + threadIdx.x;
    if (p >= half) return;
    const int64_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
    uint64_t a = keys[i], b = keys[l];
    const uint64_t a0 = a;
    ap_cmpx(a, b, (i & k) == 0);
    if (a != a0) {
        keys[i] = a;
        keys[l] = b;
    }
}

// one workgroup per (class c = blockIdx.x, threshold t = blockIdx.y); c == K: the tail behind the last class
__global__ __launch_bounds__(kApThreads) void ap_curve_kernel(const uint64_t* __restrict__ keys, const unsigned char* __restrict__ flags,
                                                              const int32_t* __restrict__ cstart, const int64_t* __restrict__ counts, int K,
                                                              int64_t N, int32_t* __restrict__ cum, int fill_tail, double* __restrict__ ap,
                                                              int32_t* __restrict__ order) {
    __shared__ int32_t s_wsum[kApThreads / kWave];
    __shared__ double s_wmax[kApThreads / kWave];
    __shared__ double s_pmax[kApThreads];
    __shared__ unsigned char s_f[kApThreads];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int c = blockIdx.x, t = blockIdx.y;
    int32_t* cum_t = cum + (int64_t)t * N;
    if (c == K) {
        int64_t from = cstart[K];
        if (from < 0 || from > N) from = N;
        for (int64_t r = from + tid; r < N; r += kApThreads) {
            if (order && t == 0) order[r] = -1;
            if (fill_tail) cum_t[r] = 0;
        }
        return;
    }
    int64_t cs = cstart[c], ce = cstart[c + 1];
    if (!(cs >= 0 && cs <= ce && ce <= N)) cs = ce = 0;
    const int64_t n = ce - cs;
    // left to right: the cumulative true positives
    int32_t carry = 0;
    for (int64_t base = 0; base < n; base += kApThreads) {
        const int64_t r = base + tid;
        int f = 0;
        if (r < n) {
            const uint32_t idx = (uint32_t)(keys[cs + r] & kApIndexMask);
            const bool ok = (int64_t)idx < N;
            if (ok) f = (flags[idx] >> t) & 1;
            if (order && t == 0) order[cs + r] = ok ? (int32_t)idx : -1;
        }
        int v = f;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int o = __shfl_up(v, off, kWave);
            if (lane >= off) v += o;
        }
        if (lane == kWave - 1) s_wsum[wave] = v;
        __syncthreads();
        int before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < kApThreads / kWave; ++w) {
            if (w < wave) before += s_wsum[w];
            total += s_wsum[w];
        }
        if (r < n) cum_t[cs + r] = before + v;                              // read back below by the thread that wrote it
        carry += total;
        __syncthreads();
    }
    // right to left: precision, its running maximum, and the sum over the true-positive ranks in descending rank
    double acc = 0.0, right_max = 0.0;
    for (int64_t base = (n + kApThreads - 1) / kApThreads * kApThreads - kApThreads; base >= 0; base -= kApThreads) {
        const int64_t r = base + tid;
        int f = 0;
        double prec = 0.0;
        if (r < n) {
            const uint32_t idx = (uint32_t)(keys[cs + r] & kApIndexMask);
            if ((int64_t)idx < N) f = (flags[idx] >> t) & 1;
            prec = (double)cum_t[cs + r] / (double)(r + 1);
        }
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const double o = __shfl_down(prec, off, kWave);
            if (lane + off < kWave && o > prec) prec = o;
        }
        if (lane == 0) s_wmax[wave] = prec;
        __syncthreads();
        double right = right_max, all = right_max;
#pragma unroll
        for (int w = 0; w < kApThreads / kWave; ++w) {
            const double x = s_wmax[w];
            if (w > wave && x > right) right = x;
            if (x > all) all = x;
        }
        s_pmax[tid] = right > prec ? right : prec;
        s_f[tid] = (unsigned char)f;
        right_max = all;
        __syncthreads();
        if (wave == 0) {
            for (int g = kApThreads / kWave - 1; g >= 0; --g) {
                unsigned long long mask = __ballot(s_f[g * kWave + lane] != 0);
                while (mask) {
                    const int hi = 63 - __clzll((long long)mask);
                    acc = acc + s_pmax[g * kWave + hi];
                    mask &= ~(1ull << hi);
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t npos = counts[c];
        ap[t * K + c] = (npos > 0 && n > 0) ? acc / (double)npos : 0.0;
    }
}

}  // namespace

size_t average_precision_workspace_bytes(int S, int pred_max_tracks, int T, int K) { return ap_layout(S, pred_max_tracks, T, K).total; }

hipError_t launch_average_precision(const int32_t* pred_store, int pred_max_tracks, const int32_t* gt_store, int gt_max_tracks, int S,
                                    const F1Thresholds& thr, int T, int K, void* ws, double* ap, int64_t* counts, int64_t* invalid,
                                    int32_t* order, int32_t* class_start, int32_t* cum_tp, double* pred_best, int32_t* pred_target,
                                    hipStream_t s) {
    if (S < 1 || S > 65535 || T < 1 || T > kF1MaxThresholds || K < 1 || K > kF1MaxClasses || pred_max_tracks < 1 || pred_max_tracks > kApSide ||
        gt_max_tracks < 1 || gt_max_tracks > kApSide || (int64_t)S * pred_max_tracks > kApMaxPositions)
        return hipErrorInvalidValue;
    const ApLayout l = ap_layout(S, pred_max_tracks, T, K);
    char* w = static_cast<char*>(ws);
    const int64_t N = (int64_t)S * pred_max_tracks, Npad = ap_padded(N);
    uint64_t* keys = reinterpret_cast<uint64_t*>(w + l.keys);
    double* best = pred_best ? pred_best : reinterpret_cast<double*>(w + l.best);
    int32_t* target = pred_target ? pred_target : reinterpret_cast<int32_t*>(w + l.target);
    unsigned char* flags = reinterpret_cast<unsigned char*>(w + l.flags);
    int32_t* partial = reinterpret_cast<int32_t*>(w + l.partial);
    int32_t* cstart = reinterpret_cast<int32_t*>(w + l.cstart);
    int32_t* cum = cum_tp ? cum_tp : reinterpret_cast<int32_t*>(w + l.cum);
    const int blocks = (pred_max_tracks + kApRows - 1) / kApRows;
    hipLaunchKernelGGL(ap_target_kernel, dim3((unsigned)blocks, (unsigned)S), dim3(kApWaves * kWave), 0, s, pred_store, pred_max_tracks, gt_store,
                       gt_max_tracks, K, N, Npad, keys, best, target, partial);
    hipLaunchKernelGGL(ap_counts_kernel, dim3(1), dim3(kApThreads), 0, s, partial, S, K, counts, invalid, cstart, class_start);
    hipLaunchKernelGGL(ap_flags_kernel, dim3((unsigned)S), dim3(kApThreads), 0, s, pred_store, pred_max_tracks, thr, T, keys, best, target, flags);
    const int tile = (int)std::min<int64_t>(Npad, kApTile);
    const unsigned tiles = (unsigned)(Npad / tile);
    hipLaunchKernelGGL(ap_sort_tile_kernel, dim3(tiles), dim3(kApThreads), 0, s, keys, tile, (int64_t)0);
    for (int64_t k = 2 * (int64_t)tile; k <= Npad; k <<= 1) {
        for (int64_t j = k >> 1; j >= tile; j >>= 1)
            hipLaunchKernelGGL(ap_sort_step_kernel, dim3((unsigned)((Npad / 2 + kApThreads - 1) / kApThreads)), dim3(kApThreads), 0, s, keys,
                               Npad / 2, k, j);
        hipLaunchKernelGGL(ap_sort_tile_kernel, dim3(tiles), dim3(kApThreads), 0, s, keys, tile, k);
    }
    hipLaunchKernelGGL(ap_curve_kernel, dim3((unsigned)(K + 1), (unsigned)T), dim3(kApThreads), 0, s, keys, flags, cstart, counts, K, N, cum,
                       cum_tp ? 1 : 0, ap, order);
    return hipGetLastError();
}

}  // namespace parq
