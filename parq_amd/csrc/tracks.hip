// A device-resident track store for the scene-level tracker (parq_amd/scene_tracks.py; the reference's utils/f1_eval.py:293-352
// matching_pred), and the rectangular assignment solver it needs (include/parq_hip.h: parq_assign_max, parq_tracks_update).
//
// Assignment: shortest augmenting paths with float64 duals on cost = -(double)m, rows in index order, on the transpose (by index)
// when there are more rows than columns.  ONE wavefront per problem: lanes stride the columns, the column minimum is a butterfly
// reduction over the wave, and every piece of state (duals u / v, path costs, path, the two assignment maps, the scanned flags)
// lives in LDS: 31 bytes per index, 62 KB at the limit of 2048, so there are two instantiations (512 and 2048 indices) and a
// small problem does not hold a large allocation.  The maps are 16-bit (indices < 2048).  Tie rule, the one of
// tests/scene_tracks_cases.py assign_statement: among equal minima an unassigned column before an assigned one, then the lower
// index; the reduction compares (cost, assigned << 16 | index) lexicographically, so its result does not depend on its order.
// No atomics.  The workgroup is one wave, so __syncthreads() is a compiler / LDS ordering point, not a hardware barrier between
// waves.  Compiled with floating-point contraction off (obb_pair.hpp), as the IoU is.
// The evaluator's ground-truth store (parq_gt_tracks_update) is the same store and the same launches 2 and 3 behind a select
// kernel of its own (gt_tracks_select_kernel).
#include "obb_pair.hpp"

#include <climits>

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kCapSmall = 512, kCapLarge = 2048;
// the ground-truth jitter per hash unit: sqrt(3) * 1e-3 / 2^16 (the division by a power of two is exact)
constexpr double kGtJitterUnit = 1.7320508075688772e-3 / 65536.0;

template <int CAP>
struct AssignLds {
    double u[CAP], v[CAP], sp[CAP];                 // row duals, column duals, shortest path cost to each column
    int16_t path[CAP], row4col[CAP], col4row[CAP];
    unsigned char scanned[CAP];
};

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// Solves max sum m[i][c] over the (nr x nc) row-major float32 matrix m (nr, nc <= CAP) and leaves the result in L: with n = min(nr,
// nc) problem rows and k = max(nr, nc) problem columns, col4row[0..n) / row4col[0..k) (problem row = matrix column when nr > nc).
template <int CAP>
__device__ void assign_max_wave(const float* __restrict__ m, int nr, int nc, AssignLds<CAP>& L, int lane) {
    const bool tr = nr > nc;
    const int n = tr ? nc : nr, k = tr ? nr : nc;
    for (int j = lane; j < k; j += kWave) {
        L.v[j] = 0.0;
        L.row4col[j] = -1;
    }
    for (int i = lane; i < n; i += kWave) {
        L.u[i] = 0.0;
        L.col4row[i] = -1;
    }
    __syncthreads();
    for (int cur = 0; cur < n; ++cur) {
        for (int j = lane; j < k; j += kWave) {
            L.sp[j] = pos_inf();
            L.path[j] = -1;
            L.scanned[j] = 0;
        }
        __syncthreads();
        double min_val = 0.0;
        int i = cur, sink = -1;
        // every step scans one more column and at most `cur` < k columns are assigned: a sink is met within k steps
        for (int step = 0; step < k && sink < 0; ++step) {
            const double ui = L.u[i];
            double best = pos_inf();
            int best_key = INT_MAX;
            for (int j = lane; j < k; j += kWave) {
                if (L.scanned[j]) continue;
                const double c = -(double)(tr ? m[(int64_t)j * nc + i] : m[(int64_t)i * nc + j]);
                const double r = ((min_val + c) - ui) - L.v[j];
                double s = L.sp[j];
                if (r < s) {
                    s = r;
                    L.sp[j] = r;
                    L.path[j] = (int16_t)i;
                }
                const int key = (L.row4col[j] >= 0 ? 1 << 16 : 0) | j;
                if (s < best || (s == best && key < best_key)) {
                    best = s;
                    best_key = key;
                }
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, kWave);
                const int ok = __shfl_xor(best_key, off, kWave);
                if (ob < best || (ob == best && ok < best_key)) {
                    best = ob;
                    best_key = ok;
                }
            }
            if (best_key == INT_MAX) break;                       // no unscanned column left: cannot happen for n <= k
            const int j = best_key & 0xffff;
            min_val = best;
            const int r4 = L.row4col[j];
            if (lane == 0) L.scanned[j] = 1;
            if (r4 < 0) sink = j; else i = r4;
            __syncthreads();
        }
        if (sink < 0) continue;
        // duals: the scanned rows are `cur` and the rows assigned to the scanned columns
        for (int j = lane; j < k; j += kWave) {
            if (!L.scanned[j]) continue;
            const double d = min_val - L.sp[j];
            const int r = L.row4col[j];
            if (r >= 0) L.u[r] = L.u[r] + d;
            L.v[j] = L.v[j] - d;
        }
        __syncthreads();
        if (lane == 0) {
            L.u[cur] = L.u[cur] + min_val;
            int j = sink;
            for (int g = 0; g <= n; ++g) {                          // a path visits each row at most once
                const int r = L.path[j];
                if (r < 0 || j < 0) break;
                L.row4col[j] = (int16_t)r;
                const int next = L.col4row[r];
                L.col4row[r] = (int16_t)j;
                j = next;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
}

// the column matrix row `row` got (-1: none), after assign_max_wave on an (nr x nc) matrix
template <int CAP>
__device__ __forceinline__ int assigned_col(const AssignLds<CAP>& L, int nr, int nc, int row) {
    return nr > nc ? (int)L.row4col[row] : (int)L.col4row[row];
}

template <int CAP>
__global__ __launch_bounds__(kWave) void assign_max_kernel(const float* __restrict__ m, int64_t m_total, const int64_t* __restrict__ seg,
                                                           int max_rows, int max_cols, double* __restrict__ duals,
                                                           int32_t* __restrict__ row_to_col, int64_t out_total) {
    __shared__ AssignLds<CAP> L;
    const int lane = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t m_off = seg[s * 4], nr64 = seg[s * 4 + 1], nc64 = seg[s * 4 + 2], o_off = seg[s * 4 + 3];
    // a table row that does not describe the arrays it came with writes nothing rather than reaching outside them
    if (nr64 < 0 || nc64 < 0 || nr64 > max_rows || nc64 > max_cols || m_off < 0 || o_off < 0 || m_off > m_total ||
        nr64 * nc64 > m_total - m_off || o_off > out_total || nr64 > out_total - o_off)
        return;
    const int nr = (int)nr64, nc = (int)nc64;
    assign_max_wave<CAP>(m + m_off, nr, nc, L, lane);
    for (int r = lane; r < nr; r += kWave) row_to_col[o_off + r] = assigned_col(L, nr, nc, r);
    // the duals of cost = -m in the matrix's own orientation: u_row + v_col <= -m[row][col], equal on the assigned pairs
    double* du = duals + s * ((int64_t)max_rows + max_cols);
    const bool tr = nr > nc;
    for (int r = lane; r < nr; r += kWave) du[r] = tr ? L.v[r] : L.u[r];
    for (int c = lane; c < nc; c += kWave) du[max_rows + c] = tr ? L.u[c] : L.v[c];
}

// ------------------------------------------------------------------ the track store
struct SlotChunk {
    int32_t slot[kTrackChunk];
};

__device__ __forceinline__ int32_t* slot_base(int32_t* store, int slot, int mt) { return store + (int64_t)slot * (2 + 26 * (int64_t)mt); }

struct SceneWs {
    int32_t* hdr;        // [detections D, tracks n (-1: the slot's count is outside [0, max_tracks])]
    int32_t* det_q;      // [Q] query of detection d
    int32_t* det_label;  // [Q]
    float* det_score;    // [Q]
    float* iou;          // [D x n], row-major
};

__device__ __host__ inline int64_t scene_ws_words(int Q, int mt) { return (4 + 3 * (int64_t)Q + (int64_t)Q * mt + 3) & ~(int64_t)3; }

__device__ __forceinline__ SceneWs scene_ws(void* ws, int b, int Q, int mt) {
    int32_t* p = static_cast<int32_t*>(ws) + (int64_t)b * scene_ws_words(Q, mt);
    SceneWs w;
    w.hdr = p;
    w.det_q = p + 4;
    w.det_label = p + 4 + Q;
    w.det_score = reinterpret_cast<float*>(p + 4 + 2 * (int64_t)Q);
    w.iou = reinterpret_cast<float*>(p + 4 + 3 * (int64_t)Q);
    return w;
}

// launch 1: the detections of each scene, compacted in query order; track_id = -1 everywhere
__global__ __launch_bounds__(kWave) void tracks_select_kernel(SlotChunk slots, int b0, int32_t* __restrict__ store, int mt,
                                                              const float* __restrict__ prob, const unsigned char* __restrict__ mask,
                                                              int Q, int K, float conf, void* __restrict__ ws,
                                                              int32_t* __restrict__ track_id) {
    const int lane = threadIdx.x, b = b0 + blockIdx.x;
    const int32_t cnt = slot_base(store, slots.slot[blockIdx.x], mt)[0];
    const int n = (cnt >= 0 && cnt <= mt) ? cnt : -1;
    const SceneWs w = scene_ws(ws, b, Q, mt);
    int D = 0;
    for (int q0 = 0; q0 < Q; q0 += kWave) {
        const int q = q0 + lane;
        bool det = false;
        int arg = 0;
        float best = 0.f;
        if (q < Q) {
            const float* p = prob + ((int64_t)b * Q + q) * K;
            best = p[0];
            bool nan = best != best;
            for (int c = 1; c < K; ++c) {
                const float x = p[c];
                nan |= x != x;
                if (x > best) {
                    best = x;
                    arg = c;
                }
            }
            det = n >= 0 && !nan && arg != K - 1 && best > conf && mask[(int64_t)b * Q + q] != 0;
            track_id[(int64_t)b * Q + q] = -1;
        }
        const unsigned long long votes = __ballot(det);
        if (det) {
            const int pos = D + __popcll(votes & ((1ull << lane) - 1ull));
            w.det_q[pos] = q;
            w.det_label[pos] = arg;
            w.det_score[pos] = best;
        }
        D += __popcll(votes);
    }
    if (lane == 0) {
        w.hdr[0] = D;
        w.hdr[1] = n;
    }
}

// launch 1 of the ground-truth store (parq_gt_tracks_update): the valid rows of each scene, compacted in row order, with label
// labels[row] and score 1; their corners, each box moved by its hashed jitter (include/parq_hip.h: the rule in full), go to
// `jittered` (B,P,8,3), which stands in for corners_world in launches 2 and 3.  `visits`: updates the scene's slot has had before.
__global__ __launch_bounds__(kWave) void gt_tracks_select_kernel(SlotChunk slots, SlotChunk visits, int b0, int32_t* __restrict__ store, int mt,
                                                                 const float* __restrict__ corners_world, const int32_t* __restrict__ labels,
                                                                 const unsigned char* __restrict__ valid, int P, uint32_t seed_lo,
                                                                 uint32_t seed_hi, void* __restrict__ ws, float* __restrict__ jittered) {
    const int lane = threadIdx.x, b = b0 + blockIdx.x;
    const int32_t slot = slots.slot[blockIdx.x];
    const int32_t cnt = slot_base(store, slot, mt)[0];
    const int n = (cnt >= 0 && cnt <= mt) ? cnt : -1;
    const SceneWs w = scene_ws(ws, b, P, mt);
    const uint32_t h_scene = hash_absorb(hash_absorb(hash_absorb(hash_absorb(0x9e3779b9u, seed_lo), seed_hi), (uint32_t)slot),
                                         (uint32_t)visits.slot[blockIdx.x]);
    int D = 0;
    for (int q0 = 0; q0 < P; q0 += kWave) {
        const int q = q0 + lane;
        const bool det = q < P && n >= 0 && valid[(int64_t)b * P + q] != 0;
        const unsigned long long votes = __ballot(det);
        if (det) {
            const int pos = D + __popcll(votes & ((1ull << lane) - 1ull));
            w.det_q[pos] = q;
            w.det_label[pos] = labels[(int64_t)b * P + q];
            w.det_score[pos] = 1.0f;
            const uint32_t h = hash_absorb(h_scene, (uint32_t)pos);
            const uint32_t w0 = hash_absorb(h, 0u), w1 = hash_absorb(h, 1u);
            const int u = (int)((w0 & 0xffffu) + (w0 >> 16) + (w1 & 0xffffu) + (w1 >> 16)) - 131070;
            const double jitter = (double)u * kGtJitterUnit;
            const float* src = corners_world + ((int64_t)b * P + q) * 24;
            float* dst = jittered + ((int64_t)b * P + q) * 24;
#pragma unroll
            for (int i = 0; i < 24; ++i) dst[i] = (float)((double)src[i] + jitter);
        }
        D += __popcll(votes);
    }
    if (lane == 0) {
        w.hdr[0] = D;
        w.hdr[1] = n;
    }
}

// launch 2: IoU of every (detection, track) pair, one lane per pair
__global__ __launch_bounds__(kWave) void tracks_iou_kernel(SlotChunk slots, int b0, int32_t* __restrict__ store, int mt,
                                                           const float* __restrict__ corners_world, int Q, void* __restrict__ ws,
                                                           float* __restrict__ iou_out) {
    __shared__ ObbPolyLds lds;
    const int lane = threadIdx.x, b = b0 + blockIdx.y;
    const SceneWs w = scene_ws(ws, b, Q, mt);
    const int D = w.hdr[0], n = w.hdr[1];
    if (D < 1 || D > Q || n < 1 || n > mt) return;
    const int64_t p = (int64_t)blockIdx.x * kWave + lane;
    if (p >= (int64_t)D * n) return;
    const int d = (int)(p / n), t = (int)(p % n);
    const int q = w.det_q[d];
    if (q < 0 || q >= Q) return;
    const float* trk = reinterpret_cast<const float*>(slot_base(store, slots.slot[blockIdx.y], mt) + 2 + 2 * (int64_t)mt) + (int64_t)t * 24;
    Corners c1, c2;
    const bool bad1 = load_canonical(corners_world + ((int64_t)b * Q + q) * 24, c1), bad2 = load_canonical(trk, c2);
    double r3, r2;
    obb_pair_iou(c1, bad1, c2, bad2, lds, lane, r3, r2);
    w.iou[p] = (float)r3;
    if (iou_out) iou_out[((int64_t)b * Q + d) * mt + t] = (float)r3;
}

__device__ __forceinline__ void put_track(int32_t* base, int mt, int t, int label, float score, const float* corners) {
    base[2 + t] = label;
    reinterpret_cast<float*>(base + 2 + mt)[t] = score;
    float* dst = reinterpret_cast<float*>(base + 2 + 2 * (int64_t)mt) + (int64_t)t * 24;
#pragma unroll
    for (int i = 0; i < 24; ++i) dst[i] = corners[i];
}

// launch 3: the assignment, then matches and births
template <int CAP>
__global__ __launch_bounds__(kWave) void tracks_assign_update_kernel(SlotChunk slots, int b0, int32_t* __restrict__ store, int mt,
                                                                     const float* __restrict__ corners_world, int Q, float iou_thresh,
                                                                     void* __restrict__ ws, int32_t* __restrict__ track_id) {
    __shared__ AssignLds<CAP> L;
    const int lane = threadIdx.x, b = b0 + blockIdx.x;
    const SceneWs w = scene_ws(ws, b, Q, mt);
    const int D = w.hdr[0], n = w.hdr[1];
    if (D < 1 || D > Q || n < 0 || n > mt) return;
    int32_t* base = slot_base(store, slots.slot[blockIdx.x], mt);
    if (n > 0) assign_max_wave<CAP>(w.iou, D, n, L, lane);
    const float* scores = reinterpret_cast<const float*>(base + 2 + mt);
    int births = 0;
    for (int d0 = 0; d0 < D; d0 += kWave) {
        const int d = d0 + lane;
        bool birth = false;
        int q = -1;
        if (d < D) {
            q = w.det_q[d];
            if (q >= 0 && q < Q) {
                const int c = n > 0 ? assigned_col(L, D, n, d) : -1;
                const bool matched = c >= 0 && c < n && !(w.iou[(int64_t)d * n + c] < iou_thresh);
                if (matched) {
                    track_id[(int64_t)b * Q + q] = c;
                    if (scores[c] < w.det_score[d]) put_track(base, mt, c, w.det_label[d], w.det_score[d], corners_world + ((int64_t)b * Q + q) * 24);
                } else {
                    birth = true;
                }
            }
        }
        const unsigned long long votes = __ballot(birth);
        if (birth) {
            const int pos = n + births + __popcll(votes & ((1ull << lane) - 1ull));
            if (pos < mt) put_track(base, mt, pos, w.det_label[d], w.det_score[d], corners_world + ((int64_t)b * Q + q) * 24);
            track_id[(int64_t)b * Q + q] = pos < mt ? pos : -2;
        }
        births += __popcll(votes);
    }
    if (lane == 0) {
        const int total = n + births;
        base[0] = total < mt ? total : mt;
        if (total > mt) base[1] = base[1] + (total - mt);
    }
}

}  // namespace

size_t tracks_update_workspace_bytes(int B, int Q, int max_tracks) { return (size_t)B * (size_t)scene_ws_words(Q, max_tracks) * 4; }

hipError_t launch_assign_max(const float* m, int64_t m_total, const int64_t* seg, int S, int max_rows, int max_cols, double* duals,
                             int32_t* row_to_col, int64_t out_total, hipStream_t s) {
    if (S < 1 || max_rows > kCapLarge || max_cols > kCapLarge) return hipErrorInvalidValue;
    if (max_rows <= kCapSmall && max_cols <= kCapSmall)
        hipLaunchKernelGGL(assign_max_kernel<kCapSmall>, dim3((unsigned)S), dim3(kWave), 0, s, m, m_total, seg, max_rows, max_cols, duals,
                           row_to_col, out_total);
    else
        hipLaunchKernelGGL(assign_max_kernel<kCapLarge>, dim3((unsigned)S), dim3(kWave), 0, s, m, m_total, seg, max_rows, max_cols, duals,
                           row_to_col, out_total);
    return hipGetLastError();
}

hipError_t launch_tracks_update(int32_t* store, int max_tracks, const int32_t* slots_host, int b0, int nb, const float* corners_world,
                                const float* prob, const unsigned char* mask, int Q, int K, float conf, float iou_thresh, void* ws,
                                int32_t* track_id, float* iou_out, hipStream_t s) {
    if (nb < 1 || nb > kTrackChunk || Q < 1 || Q > kCapLarge || max_tracks < 1 || max_tracks > kCapLarge) return hipErrorInvalidValue;
    SlotChunk slots;
    for (int i = 0; i < kTrackChunk; ++i) slots.slot[i] = i < nb ? slots_host[b0 + i] : 0;
    hipLaunchKernelGGL(tracks_select_kernel, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, max_tracks, prob, mask, Q, K, conf, ws,
                       track_id);
    const unsigned pair_blocks = (unsigned)(((int64_t)Q * max_tracks + kWave - 1) / kWave);
    hipLaunchKernelGGL(tracks_iou_kernel, dim3(pair_blocks, (unsigned)nb), dim3(kWave), 0, s, slots, b0, store, max_tracks, corners_world, Q,
                       ws, iou_out);
    if (Q <= kCapSmall && max_tracks <= kCapSmall)
        hipLaunchKernelGGL(tracks_assign_update_kernel<kCapSmall>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, max_tracks,
                           corners_world, Q, iou_thresh, ws, track_id);
    else
        hipLaunchKernelGGL(tracks_assign_update_kernel<kCapLarge>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, max_tracks,
                           corners_world, Q, iou_thresh, ws, track_id);
    return hipGetLastError();
}

// workspace of the ground-truth update: the B scene regions of launch_tracks_update, a (B,P) track_id nobody reads, the jittered corners
static size_t gt_ws_id_words(int B, int P) { return ((size_t)B * (size_t)P + 3) & ~(size_t)3; }

size_t gt_tracks_update_workspace_bytes(int B, int P, int max_tracks) {
    return ((size_t)B * (size_t)scene_ws_words(P, max_tracks) + gt_ws_id_words(B, P) + (size_t)B * (size_t)P * 24) * 4;
}

hipError_t launch_gt_tracks_update(int32_t* store, int max_tracks, const int32_t* slots_host, const int32_t* visits_host, int b0, int nb, int B,
                                   const float* corners_world, const int32_t* labels, const unsigned char* valid, int P, float iou_thresh,
                                   uint32_t seed_lo, uint32_t seed_hi, void* ws, float* iou_out, hipStream_t s) {
    if (nb < 1 || nb > kTrackChunk || b0 < 0 || b0 + nb > B || P < 1 || P > kCapLarge || max_tracks < 1 || max_tracks > kCapLarge)
        return hipErrorInvalidValue;
    SlotChunk slots, visits;
    for (int i = 0; i < kTrackChunk; ++i) {
        slots.slot[i] = i < nb ? slots_host[b0 + i] : 0;
        visits.slot[i] = i < nb ? visits_host[b0 + i] : 0;
    }
    int32_t* track_id = static_cast<int32_t*>(ws) + (size_t)B * (size_t)scene_ws_words(P, max_tracks);
    float* jittered = reinterpret_cast<float*>(track_id + gt_ws_id_words(B, P));
    hipLaunchKernelGGL(gt_tracks_select_kernel, dim3((unsigned)nb), dim3(kWave), 0, s, slots, visits, b0, store, max_tracks, corners_world,
                       labels, valid, P, seed_lo, seed_hi, ws, jittered);
    const unsigned pair_blocks = (unsigned)(((int64_t)P * max_tracks + kWave - 1) / kWave);
    hipLaunchKernelGGL(tracks_iou_kernel, dim3(pair_blocks, (unsigned)nb), dim3(kWave), 0, s, slots, b0, store, max_tracks,
                       (const float*)jittered, P, ws, iou_out);
    if (P <= kCapSmall && max_tracks <= kCapSmall)
        hipLaunchKernelGGL(tracks_assign_update_kernel<kCapSmall>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, max_tracks,
                           (const float*)jittered, P, iou_thresh, ws, track_id);
    else
        hipLaunchKernelGGL(tracks_assign_update_kernel<kCapLarge>, dim3((unsigned)nb), dim3(kWave), 0, s, slots, b0, store, max_tracks,
                           (const float*)jittered, P, iou_thresh, ws, track_id);
    return hipGetLastError();
}

}  // namespace parq
