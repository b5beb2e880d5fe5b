// The matcher of the set loss on the device (utils/matcher.py:31-115; host mirror: parq_amd/loss.py HungarianMatcherModified and the
// loop of decoder_loss_batched): for all S = I * B (iteration, scene) problems of a training step in ONE enqueue of four launches,
// with nothing read back to the host (include/parq_hip.h: parq_set_match; NumPy statement: tests/set_match_cases.py).
//
//   cost    one lane per row (k, b, q): float32 softmax of the row's logits, L1 distance of its reference point to every box centre of
//           the scene, m = -(cost_bbox * l1 - cost_class * prob[label]) packed row-major (Q x n) per segment, the segment table of
//           the assignment written from t_count, and the "near" bytes (l1 < ratio), stored box-major so that both sides are coalesced.
//   assign  launch_assign_max (tracks.hip): one wavefront per segment, exact, pinned to scipy.
//   pairs   one workgroup per segment: per box the neighbours, capped to the max_padding smallest (key, q) of a counter-based hash;
//           one box per prediction (the assigned column, else the lowest box that chose it); the punish mask of the LAST box; the
//           dense pairs [4][S * Q] that parq_set_loss_flags consumes, the segment's pair count and punish / sum(punish).
//   finish  one workgroup per segment: valid_bs = segments with a pair (every workgroup counts them itself: no atomics, no
//           cross-workgroup order), pair_coef and row_weight in the float32 operations of loss.py _device_set_loss.
//
// No atomics, no allocation, no host synchronisation.  Every number read from device memory (box counts, labels, assigned columns) is
// checked before it indexes anything; every loop is bounded by a shape argument.  The rank loop of an over-full box costs Q LDS reads
// per neighbour (Q <= 2048), which is what bounds a workgroup's time at the limits.  Floating-point contraction is off: the
// statement's roundings are the kernel's.
#include "common.hpp"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchMaxSide = 2048;

struct SetMatchArgs {
    const float *logits, *coord;                       // (I, B, Q, ncls | 3)
    const float* t_center;                             // (B, nmax, 3)
    const int32_t *t_label, *t_count;                  // (B, nmax), (B)
    int I, B, Q, ncls, nmax, max_padding;
    float cost_class, cost_bbox, ratio;
    uint32_t seed_lo, seed_hi, step;
    int64_t* seg;                                      // workspace: (S, 4) segment table of the assignment
    float* m;                                          // workspace: S regions of Q * nmax floats, segment s packed (Q x n)
    unsigned char* near;                               // workspace: (S, nmax, Q) bytes
    int32_t *row_to_col, *pairs, *stats;               // (S * Q), [4][S * Q], (S + 1)
    float *coef, *row_weight;                          // (S * Q) each
    float* cost_out;                                   // (I, B, Q, nmax) or null
    unsigned char* near_out;                           // (I, B, Q, nmax) or null
};

// boxes of scene b; a count outside [0, nmax] describes no boxes
__device__ __forceinline__ int box_count(const SetMatchArgs& a, int b) {
    const int n = a.t_count[b];
    return (n < 0 || n > a.nmax) ? 0 : n;
}

// one word into the key: common.hpp hash_absorb, the text the ground-truth jitter shares (tracks.hip)
__device__ __forceinline__ uint32_t absorb(uint32_t h, uint32_t w) { return hash_absorb(h, w); }

__global__ __launch_bounds__(kMatchThreads) void setmatch_cost_kernel(SetMatchArgs a) {
    const int64_t row = (int64_t)blockIdx.x * kMatchThreads + threadIdx.x;
    if (row >= (int64_t)a.I * a.B * a.Q) return;
    const int q = (int)(row % a.Q);
    const int64_t s = row / a.Q;
    const int b = (int)(s % a.B);
    const int n = box_count(a, b);
    const int64_t m_off = s * a.Q * a.nmax;
    if (q == 0) {
        a.seg[s * 4 + 0] = m_off;
        a.seg[s * 4 + 1] = a.Q;
        a.seg[s * 4 + 2] = n;
        a.seg[s * 4 + 3] = s * a.Q;
    }
    const float* lg = a.logits + row * a.ncls;
    float mx = lg[0];
    for (int c = 1; c < a.ncls; ++c) mx = lg[c] > mx ? lg[c] : mx;
    float sum = 0.f;
    for (int c = 0; c < a.ncls; ++c) sum = sum + expf(lg[c] - mx);
    const float x = a.coord[row * 3 + 0], y = a.coord[row * 3 + 1], z = a.coord[row * 3 + 2];
    for (int j = 0; j < n; ++j) {
        const int64_t tb = (int64_t)b * a.nmax + j;
        const int lab = a.t_label[tb];
        const float prob = (lab >= 0 && lab < a.ncls) ? expf(lg[lab] - mx) / sum : 0.f;
        const float l1 = (fabsf(x - a.t_center[tb * 3 + 0]) + fabsf(y - a.t_center[tb * 3 + 1])) + fabsf(z - a.t_center[tb * 3 + 2]);
        const float c = a.cost_bbox * l1 - a.cost_class * prob;
        float mv = -c;
        if (!__builtin_isfinite(mv)) mv = -3.0e38f;       // the outputs of a forward the range policy will re-run
        const unsigned char nr = l1 < a.ratio ? 1 : 0;
        a.m[m_off + (int64_t)q * n + j] = mv;
        a.near[(s * a.nmax + j) * a.Q + q] = nr;
        if (a.cost_out) a.cost_out[row * a.nmax + j] = mv;
        if (a.near_out) a.near_out[row * a.nmax + j] = nr;
    }
}

// sum of v over the workgroup (4 waves), the same in every thread
__device__ __forceinline__ int block_count(int v, int* sh) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    const int r = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kMatchThreads) void setmatch_pairs_kernel(SetMatchArgs a) {
    __shared__ uint32_t key[kMatchMaxSide];
    __shared__ int16_t extra[kMatchMaxSide];            // lowest box that chose q, or -1
    __shared__ unsigned char nr[kMatchMaxSide], punish[kMatchMaxSide];
    __shared__ int sh[kMatchThreads / kWave];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int b = (int)(s % a.B), k = (int)(s / a.B);
    const int n = box_count(a, b), Q = a.Q;
    for (int q = tid; q < Q; q += kMatchThreads) {
        extra[q] = -1;
        punish[q] = 1;
    }
    __syncthreads();
    const uint32_t h_kb = absorb(absorb(absorb(absorb(absorb(0x9e3779b9u, a.seed_lo), a.seed_hi), a.step), (uint32_t)k), (uint32_t)b);
    for (int j = 0; j < n; ++j) {
        const unsigned char* near_j = a.near + (s * a.nmax + j) * Q;
        const uint32_t h_j = absorb(h_kb, (uint32_t)j);
        int c = 0;
        for (int q = tid; q < Q; q += kMatchThreads) {
            const unsigned char f = near_j[q] != 0 ? 1 : 0;
            nr[q] = f;
            key[q] = absorb(h_j, (uint32_t)q);
            c += f;
        }
        c = block_count(c, sh);                          // (its barriers also publish nr / key)
        const bool over = c > a.max_padding;
        for (int q = tid; q < Q; q += kMatchThreads) {
            bool chosen = nr[q] != 0;
            if (chosen && over) {                        // the max_padding neighbours of smallest (key, q)
                const uint32_t kq = key[q];
                int rank = 0;
                for (int p = 0; p < Q; ++p) rank += (nr[p] != 0 && (key[p] < kq || (key[p] == kq && p < q))) ? 1 : 0;
                chosen = rank < a.max_padding;
            }
            if (chosen && extra[q] < 0) extra[q] = (int16_t)j;
            if (j == n - 1) punish[q] = (nr[q] == 0 || chosen) ? 1 : 0;
        }
        __syncthreads();
    }
    const int64_t P = (int64_t)a.I * a.B * Q;
    int cnt = 0, ps = 0;
    for (int q = tid; q < Q; q += kMatchThreads) {
        const int64_t row = s * Q + q;
        const int r = a.row_to_col[row];
        const int g = (r >= 0 && r < n) ? r : (int)extra[q];
        a.pairs[row] = k;
        a.pairs[P + row] = b;
        a.pairs[2 * P + row] = q;
        a.pairs[3 * P + row] = g;
        cnt += g >= 0 ? 1 : 0;
        ps += punish[q];
    }
    cnt = block_count(cnt, sh);
    ps = block_count(ps, sh);
    for (int q = tid; q < Q; q += kMatchThreads) a.row_weight[s * Q + q] = ps > 0 ? (float)punish[q] / (float)ps : 0.f;
    if (tid == 0) a.stats[s] = cnt;
}

__global__ __launch_bounds__(kMatchThreads) void setmatch_finish_kernel(SetMatchArgs a) {
    __shared__ int sh[kMatchThreads / kWave];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x, S = (int64_t)a.I * a.B;
    int vb = 0;
    for (int64_t t = tid; t < S; t += kMatchThreads) vb += a.stats[t] > 0 ? 1 : 0;
    vb = block_count(vb, sh);
    const int cnt = a.stats[s];
    const float valid = cnt > 0 ? 1.f : 0.f;
    const float cf = (cnt > 0 && vb > 0) ? 1.0f / ((float)cnt * (float)vb) : 0.f;
    for (int q = tid; q < a.Q; q += kMatchThreads) {
        const int64_t row = s * a.Q + q;
        a.coef[row] = cf;
        a.row_weight[row] = vb > 0 ? (a.row_weight[row] * valid) / (float)vb : 0.f;
    }
    if (s == 0 && tid == 0) a.stats[S] = vb;             // (no workgroup reads this word)
}

size_t duals_bytes(int64_t S, int Q, int nmax) { return (size_t)S * ((size_t)Q + (size_t)nmax) * 8; }

}  // namespace

// [duals of the assignment: S * (Q + nmax) float64 | segment table: S * 4 int64 | m: S * Q * nmax float32 | near: S * nmax * Q bytes]
size_t set_match_workspace_bytes(int I, int B, int Q, int nmax) {
    const size_t S = (size_t)I * (size_t)B, cells = S * (size_t)Q * (size_t)nmax;
    return (duals_bytes((int64_t)S, Q, nmax) + S * 32 + cells * 4 + cells + 15) & ~(size_t)15;
}

hipError_t launch_set_match(const float* logits, const float* coord, int I, int B, int Q, int ncls, const float* t_center,
                            const int32_t* t_label, const int32_t* t_count, int nmax, float cost_class, float cost_bbox, float ratio,
                            int max_padding, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void* ws, int32_t* row_to_col,
                            int32_t* pairs, float* coef, float* row_weight, int32_t* stats, float* cost_out, unsigned char* near_out,
                            hipStream_t st) {
    const int64_t S = (int64_t)I * B;
    if (S < 1 || S > INT32_MAX || Q < 1 || Q > kMatchMaxSide || nmax < 1 || nmax > kMatchMaxSide || ncls < 2) return hipErrorInvalidValue;
    char* base = static_cast<char*>(ws);
    SetMatchArgs a;
    a.logits = logits; a.coord = coord; a.t_center = t_center; a.t_label = t_label; a.t_count = t_count;
    a.I = I; a.B = B; a.Q = Q; a.ncls = ncls; a.nmax = nmax; a.max_padding = max_padding;
    a.cost_class = cost_class; a.cost_bbox = cost_bbox; a.ratio = ratio;
    a.seed_lo = seed_lo; a.seed_hi = seed_hi; a.step = step;
    double* duals = reinterpret_cast<double*>(base);
    a.seg = reinterpret_cast<int64_t*>(base + duals_bytes(S, Q, nmax));
    a.m = reinterpret_cast<float*>(base + duals_bytes(S, Q, nmax) + (size_t)S * 32);
    a.near = reinterpret_cast<unsigned char*>(a.m + S * Q * nmax);
    a.row_to_col = row_to_col; a.pairs = pairs; a.stats = stats; a.coef = coef; a.row_weight = row_weight;
    a.cost_out = cost_out; a.near_out = near_out;
    const int64_t rows = S * Q;
    hipLaunchKernelGGL(setmatch_cost_kernel, dim3((unsigned)((rows + kMatchThreads - 1) / kMatchThreads)), dim3(kMatchThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_assign_max(a.m, S * Q * nmax, a.seg, (int)S, Q, nmax, duals, row_to_col, rows, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(setmatch_pairs_kernel, dim3((unsigned)S), dim3(kMatchThreads), 0, st, a);
    hipLaunchKernelGGL(setmatch_finish_kernel, dim3((unsigned)S), dim3(kMatchThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace parq
