// The evaluator's end-of-epoch counts on the device (include/parq_hip.h: parq_f1_counts; parq_amd/f1_eval.py count_matches summed
// over scenes): per care class the ground-truth tracks, the prediction tracks and, per IoU threshold, the ground-truth tracks whose
// best same-class prediction lies above it.  Both sides are track stores of tracks.hip with the same slot numbering.
//
// count_matches does not consume a prediction at its first match, so a ground-truth track counts exactly when SOME same-class
// prediction overlaps it by more than the threshold: best[i] = max_j IoU(i, j) decides for every threshold, and one IoU pass serves
// them all.  The maximum of float64 values does not depend on the order it is taken in, so lanes may stride the predictions.
//
// Launch 1: a workgroup of kF1Waves wavefronts per (scene, block of kF1Rows ground-truth rows).  A wavefront owns a row at a time:
// its lanes stride the scene's predictions, skip those of another class before the clip, run obb_pair.hpp's routine (the polygon
// buffers of the wave's 64 lanes are its own ObbPolyLds), and a butterfly takes the wave-wide maximum.  The workgroup's counts are
// int32 in LDS, a table per wave, added up and written to its column of the partials; block 0 of a scene also counts the labels of
// both sides.  Launch 2: one wavefront per output element sums that element's column.  No atomics, no scratch; every loop bound is
// a count checked against its capacity (a count outside [0, capacity] reads as 0).  Contraction off, as everywhere the IoU runs.
#include "obb_pair.hpp"

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kF1Waves = 2, kF1Rows = 16;        // 2 x 24 KB of polygon buffers per workgroup; 8 rows per wavefront, in turn
static_assert(kF1Waves == 2, "block 0 counts the labels of the two sides with a wavefront each");
constexpr int kF1Elems =(2 + kF1MaxThresholds) * kF1MaxClasses + 2;

__device__ __forceinline__ const int32_t* f1_slot(const int32_t* store, int slot, int mt) { return store + (int64_t)slot * (2 + 26 * (int64_t)mt); }

__device__ __forceinline__ int f1_count(const int32_t* slot, int mt) {
    const int32_t n = slot[0];
    return (n >= 0 && n <= mt) ? n : 0;
}

__device__ __forceinline__ const float* f1_corners(const int32_t* slot, int mt, int t) {
    return reinterpret_cast<const float*>(slot + 2 + 2 * (int64_t)mt) + (int64_t)t * 24;
}

__host__ __device__ inline int f1_blocks(int gt_mt) { return (gt_mt + kF1Rows - 1) / kF1Rows; }

// elements of the partials, in the order of the outputs: counts (2 + T, K) row-major, then invalid[2]
__global__ __launch_bounds__(kF1Waves* kWave) void f1_best_kernel(const int32_t* __restrict__ pred_store, int pred_mt,
                                                                  const int32_t* __restrict__ gt_store, int gt_mt, F1Thresholds thr, int T, int K,
                                                                  int32_t* __restrict__ partials, int64_t columns, double* __restrict__ best_iou) {
    __shared__ ObbPolyLds lds[kF1Waves];
    __shared__ int32_t tally[kF1Waves][kF1Elems];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int scene = blockIdx.y, blk = blockIdx.x;
    const int E = (2 + T) * K + 2;
    const int32_t* gs = f1_slot(gt_store, scene, gt_mt);
    const int32_t* ps = f1_slot(pred_store, scene, pred_mt);
    const int ng = f1_count(gs, gt_mt), np = f1_count(ps, pred_mt);
    for (int e = lane; e < E; e += kWave) tally[wave][e] = 0;
    __syncthreads();
    const int row_end = min(ng, (blk + 1) * kF1Rows);
    for (int i = blk * kF1Rows + wave; i < row_end; i += kF1Waves) {
        const int32_t cls = gs[2 + i];
        Corners cg;
        const bool bad_g = load_canonical(f1_corners(gs, gt_mt, i), cg);
        double best = 0.0;
        for (int j0 = 0; j0 < np; j0 += kWave) {
            const int j = j0 + lane;
            if (j < np && ps[2 + j] == cls) {
                Corners cp;
                const bool bad_p = load_canonical(f1_corners(ps, pred_mt, j), cp);
                double r3, r2;
                obb_pair_iou(cg, bad_g, cp, bad_p, lds[wave], lane, r3, r2);
                if (r3 > best) best = r3;                                   // a NaN never counts
            }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const double other = __shfl_xor(best, off, kWave);
            if (other > best) best = other;
        }
        if (lane == 0) {
            if (best_iou) best_iou[(int64_t)scene * gt_mt + i] = best;
            if (cls >= 0 && cls < K) {
#pragma unroll
                for (int t = 0; t < kF1MaxThresholds; ++t)
                    if (t < T && best > thr.thr[t]) tally[wave][(2 + t) * K + cls] += 1;      // float64, strict
            }
        }
    }
    if (blk == 0) {
        // the labels of both sides: wave 0 the ground truth (row 0 of counts, invalid[0]), wave 1 the predictions (row 1, invalid[1])
        const int32_t* side = wave == 0 ? gs : ps;
        const int n = wave == 0 ? ng : np;
        int bad = 0;
        for (int j0 = 0; j0 < n; j0 += kWave) {
            const int j = j0 + lane;
            const int32_t cls = j < n ? side[2 + j] : 0;
            const bool in = j < n && cls >= 0 && cls < K;
            bad += __popcll(__ballot(j < n && !in));
            for (int c = 0; c < K; ++c) {
                const int hits = __popcll(__ballot(in && cls == c));
                if (lane == 0) tally[wave][wave * K + c] += hits;
            }
        }
        if (lane == 0) tally[wave][(2 + T) * K + wave] = bad;
    }
    __syncthreads();
    const int64_t col = (int64_t)scene * gridDim.x + blk;
    for (int e = tid; e < E; e += kF1Waves * kWave) {
        int32_t sum = 0;
#pragma unroll
        for (int w = 0; w < kF1Waves; ++w) sum += tally[w][e];
        partials[(int64_t)e * columns + col] = sum;
    }
}

// element e of the outputs = the sum of its `columns` partials; one wavefront per element, lanes striding the columns
__global__ __launch_bounds__(kWave) void f1_sum_kernel(const int32_t* __restrict__ partials, int64_t columns, int n_counts,
                                                       int64_t* __restrict__ counts, int64_t* __restrict__ invalid) {
    const int e = blockIdx.x, lane = threadIdx.x;
    long long sum = 0;
    for (int64_t c = lane; c < columns; c += kWave) sum += partials[(int64_t)e * columns + c];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
    if (lane == 0) {
        if (e < n_counts) counts[e] = sum;
        else invalid[e - n_counts] = sum;
    }
}

}  // namespace

size_t f1_counts_workspace_bytes(int S, int gt_max_tracks, int T, int K) {
    return (((size_t)((2 + T) * K + 2) * (size_t)S * (size_t)f1_blocks(gt_max_tracks)) * 4 + 15) & ~(size_t)15;
}

hipError_t launch_f1_counts(const int32_t* pred_store, int pred_max_tracks, const int32_t* gt_store, int gt_max_tracks, int S,
                            const F1Thresholds& thr, int T, int K, void* ws, int64_t* counts, int64_t* invalid, double* best_iou,
                            hipStream_t s) {
    if (S < 1 || S > 65535 || T < 1 || T > kF1MaxThresholds || K < 1 || K > kF1MaxClasses || pred_max_tracks < 1 || pred_max_tracks > 2048 ||
        gt_max_tracks < 1 || gt_max_tracks > 2048)
        return hipErrorInvalidValue;
    const int blocks = f1_blocks(gt_max_tracks);
    const int64_t columns = (int64_t)S * blocks;
    hipLaunchKernelGGL(f1_best_kernel, dim3((unsigned)blocks, (unsigned)S), dim3(kF1Waves * kWave), 0, s, pred_store, pred_max_tracks, gt_store,
                       gt_max_tracks, thr, T, K, static_cast<int32_t*>(ws), columns, best_iou);
    const int E = (2 + T) * K + 2;
    hipLaunchKernelGGL(f1_sum_kernel, dim3((unsigned)E), dim3(kWave), 0, s, static_cast<const int32_t*>(ws), columns, E - 2, counts, invalid);
    return hipGetLastError();
}

}  // namespace parq
