// A snippet's training targets from depth and poses (parq_snippet_targets; the reference's offline pass
// scripts/scannet_preprocessing/generate_scannet_anno_snippet.py:189-256,317-329 over processing_utils.py:132-154,206-263,304-336,
// there an (N, P, 3) float64 broadcast per frame).  The rule is written out in include/parq_hip.h and, in NumPy, in
// tests/snippet_cases.py; the operations and their order ARE the rule, so contraction is off for the whole file.
//
// snippet_count_kernel: a workgroup of 256 threads per tile of kTileWords aligned 8-byte words (4 depth pixels each) of one frame.
//   1. thread n < N builds box n's camera-frame record in LDS — origin (corner 4), the edges to corners 5, 0 and 7 and their squared
//      lengths, 15 doubles = 120 B — from the row (or the given world corners) and the general affine inverse of the frame's pose.  A
//      padding row gets squared lengths of -1: no point is ever inside it;
//   2. every lane loads its words (a word that is not wholly inside the depth buffer is put together from 2-byte loads of its inside
//      pixels; pixels of the word outside the frame are masked), forms its four float32 points once and tests them against every box in
//      float64; per box the four ballots' population counts go into the wave's own LDS counter row (one lane adds: no atomics);
//   3. thread n < N adds the four waves' counters and writes the tile's int32 partial.
// snippet_finalize_kernel: a workgroup of 4 x 128 threads per scene, thread (g, n) = group g, box n.  Per frame the four groups add
// the tiles' partials (every fourth tile each, eight loads in flight; integer sums, so the tile-order sum whatever the order) and
// group 0 projects the 8 camera-frame corners for the truncation ratio; then the maxima over the frames, the level and the valid
// flag; a prefix sum over the flags (two wave ballots) places every valid row, and the workgroup pads the rest with -1.
// No atomics, no dependence on the order in which workgroups run, nothing allocated, no synchronisation.
#include "../../include/parq_hip.h"
#include "common.hpp"

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kCountThreads = 256;
constexpr int kWaves = kCountThreads / 64;
constexpr int kIters = 2;                                  // words per lane
constexpr int kTileWords = kCountThreads * kIters;         // 512 words = 2048 pixels per workgroup
constexpr int kMaxBoxes = 128;
constexpr int kMaxFrames = 64;
constexpr int kMaxSide = 8192;
constexpr int kMaxLevels = 8;
constexpr int kRec = 15;                                   // doubles of a box record
constexpr int kFinGroups = 4;                              // thread groups of the finalising workgroup that share a frame's tiles
constexpr int kFinThreads = kFinGroups * kMaxBoxes;

struct Levels { int32_t count[kMaxLevels]; float ratio[kMaxLevels]; int32_t n; int32_t max_level; };

struct Inverse { double r[9]; double t[3]; };

// the general affine inverse of [R | t; 0 0 0 1] (pose: R row-major then t): the 3 x 3 block by cofactors, never the transpose
__device__ inline Inverse affine_inverse(const double* __restrict__ p) {
    const double a00 = p[0], a01 = p[1], a02 = p[2], a10 = p[3], a11 = p[4], a12 = p[5], a20 = p[6], a21 = p[7], a22 = p[8];
    const double c00 = a11 * a22 - a12 * a21, c01 = a10 * a22 - a12 * a20, c02 = a10 * a21 - a11 * a20;
    const double det = (a00 * c00 - a01 * c01) + a02 * c02;
    Inverse v;
    v.r[0] = c00 / det;
    v.r[1] = (a02 * a21 - a01 * a22) / det;
    v.r[2] = (a01 * a12 - a02 * a11) / det;
    v.r[3] = (a12 * a20 - a10 * a22) / det;
    v.r[4] = (a00 * a22 - a02 * a20) / det;
    v.r[5] = (a02 * a10 - a00 * a12) / det;
    v.r[6] = c02 / det;
    v.r[7] = (a01 * a20 - a00 * a21) / det;
    v.r[8] = (a00 * a11 - a01 * a10) / det;
    const double t0 = p[9], t1 = p[10], t2 = p[11];
    v.t[0] = -((v.r[0] * t0 + v.r[1] * t1) + v.r[2] * t2);
    v.t[1] = -((v.r[3] * t0 + v.r[4] * t1) + v.r[5] * t2);
    v.t[2] = -((v.r[6] * t0 + v.r[7] * t1) + v.r[8] * t2);
    return v;
}

__device__ inline bool row_is_padding(const float* __restrict__ row) {
    bool pad = true;
#pragma unroll
    for (int i = 0; i < 19; ++i) pad = pad && row[i] == -1.0f;
    return pad;
}

// corner k (the order of Obb3D.bb3corners_object) of a box in the world frame: the given corner, or the row's in float64
template <int k>
__device__ inline void corner_world(const float* __restrict__ row, const double* __restrict__ given, double* w) {
    if (given) {
        w[0] = given[k * 3 + 0];
        w[1] = given[k * 3 + 1];
        w[2] = given[k * 3 + 2];
        return;
    }
    constexpr int sx = ((k + 1) >> 1) & 1, sy = (k >> 1) & 1, sz = k >> 2;
    const double x = (double)row[sx], y = (double)row[2 + sy], z = (double)row[4 + sz];
    w[0] = (((double)row[6] * x + (double)row[7] * y) + (double)row[8] * z) + (double)row[15];
    w[1] = (((double)row[9] * x + (double)row[10] * y) + (double)row[11] * z) + (double)row[16];
    w[2] = (((double)row[12] * x + (double)row[13] * y) + (double)row[14] * z) + (double)row[17];
}

template <int k>
__device__ inline void corner_camera(const float* __restrict__ row, const double* __restrict__ given, const Inverse& v, double* c) {
    double w[3];
    corner_world<k>(row, given, w);
    c[0] = ((v.r[0] * w[0] + v.r[1] * w[1]) + v.r[2] * w[2]) + v.t[0];
    c[1] = ((v.r[3] * w[0] + v.r[4] * w[1]) + v.r[5] * w[2]) + v.t[1];
    c[2] = ((v.r[6] * w[0] + v.r[7] * w[1]) + v.r[8] * w[2]) + v.t[2];
}

__global__ __launch_bounds__(kCountThreads) void snippet_count_kernel(
    const uint16_t* __restrict__ depth, int64_t total_px, int T, int Hd, int Wd, const float* __restrict__ kinv, const double* __restrict__ poses,
    const float* __restrict__ obbs, const double* __restrict__ corners, int N, float depth_scale, int tiles, int32_t* __restrict__ partials) {
    __shared__ double rec[kMaxBoxes * kRec];
    __shared__ int32_t cnt[kWaves][kMaxBoxes];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, f = blockIdx.y, b = f / T;
    const int64_t HW = (int64_t)Hd * Wd;

    if (tid < N) {
        const float* row = obbs + ((size_t)b * N + tid) * 19;
        const double* given = corners ? corners + ((size_t)b * N + tid) * 24 : nullptr;
        const Inverse v = affine_inverse(poses + (size_t)f * 12);
        double o[3], c5[3], c0[3], c7[3];
        corner_camera<4>(row, given, v, o);
        corner_camera<5>(row, given, v, c5);
        corner_camera<0>(row, given, v, c0);
        corner_camera<7>(row, given, v, c7);
        double* r = rec + tid * kRec;
        const bool pad = row_is_padding(row);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            r[i] = o[i];
            r[3 + i] = c5[i] - o[i];
            r[6 + i] = c0[i] - o[i];
            r[9 + i] = c7[i] - o[i];
        }
        r[12] = pad ? -1.0 : (r[3] * r[3] + r[4] * r[4]) + r[5] * r[5];
        r[13] = pad ? -1.0 : (r[6] * r[6] + r[7] * r[7]) + r[8] * r[8];
        r[14] = pad ? -1.0 : (r[9] * r[9] + r[10] * r[10]) + r[11] * r[11];
    }
    for (int i = tid; i < kWaves * kMaxBoxes; i += kCountThreads) (&cnt[0][0])[i] = 0;
    __syncthreads();

    const float* ki = kinv + (size_t)b * 16;
    const float k00 = ki[0], k01 = ki[1], k02 = ki[2], k03 = ki[3], k10 = ki[4], k11 = ki[5], k12 = ki[6], k13 = ki[7];
    const float k20 = ki[8], k21 = ki[9], k22 = ki[10], k23 = ki[11];
    const uintptr_t buf_lo = reinterpret_cast<uintptr_t>(depth), buf_hi = buf_lo + (uintptr_t)total_px * 2;
    const uintptr_t frame_lo = buf_lo + (uintptr_t)((int64_t)f * HW) * 2;
    const uintptr_t word0 = (frame_lo & ~(uintptr_t)7) + (uintptr_t)tile * kTileWords * 8;

    for (int it = 0; it < kIters; ++it) {
        const uintptr_t a = word0 + (uintptr_t)(it * kCountThreads + tid) * 8;
        // pixel index within the frame of the word's first pixel: negative in the frame's first word when it starts inside one
        const int64_t p_first = ((int64_t)a - (int64_t)frame_lo) / 2;       // both even, the difference at least -6
        uint32_t lo = 0, hi = 0;
        if (p_first + 4 > 0 && p_first < HW) {
            if (a >= buf_lo && a + 8 <= buf_hi) {
                const uint2 v = *reinterpret_cast<const uint2*>(a);
                lo = v.x;
                hi = v.y;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uintptr_t e = a + 2 * j;
                    if (e >= buf_lo && e + 2 <= buf_hi) {
                        const uint32_t u = *reinterpret_cast<const uint16_t*>(e);
                        if (j < 2) lo |= u << (16 * j);
                        else hi |= u << (16 * (j - 2));
                    }
                }
            }
        }
        float px[4], py[4], pz[4];
        bool ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t p = p_first + j;
            const bool in_frame = p >= 0 && p < HW;
            const uint32_t u = ((j < 2 ? lo : hi) >> (16 * (j & 1))) & 0xFFFFu;
            const int pi = in_frame ? (int)p : 0;
            const int y = pi / Wd, x = pi - y * Wd;
            const float d = __fdiv_rn((float)u, depth_scale);
            const float v0 = (float)x * d, v1 = (float)y * d;
            px[j] = ((k00 * v0 + k01 * v1) + k02 * d) + k03;
            py[j] = ((k10 * v0 + k11 * v1) + k12 * d) + k13;
            pz[j] = ((k20 * v0 + k21 * v1) + k22 * d) + k23;
            ok[j] = in_frame && pz[j] > 0.0f;
        }
        if (__ballot(ok[0] || ok[1] || ok[2] || ok[3]) == 0) continue;       // uniform: nothing of this wave's 256 pixels counts
        for (int n = 0; n < N; ++n) {
            const double* r = rec + n * kRec;
            const double ox = r[0], oy = r[1], oz = r[2];
            const double ax = r[3], ay = r[4], az = r[5], bx = r[6], by = r[7], bz = r[8], cx = r[9], cy = r[10], cz = r[11];
            const double va = r[12], vb = r[13], vc = r[14];
            int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double qx = (double)px[j] - ox, qy = (double)py[j] - oy, qz = (double)pz[j] - oz;
                const double m0 = (qx * ax + qy * ay) + qz * az;
                const double m1 = (qx * bx + qy * by) + qz * bz;
                const double m2 = (qx * cx + qy * cy) + qz * cz;
                const bool in = ok[j] && 0.0 < m0 && m0 < va && 0.0 < m1 && m1 < vb && 0.0 < m2 && m2 < vc;
                c += __popcll(__ballot(in));
            }
            if (lane == 0 && c) cnt[wave][n] += c;
        }
    }
    __syncthreads();
    if (tid < N) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += cnt[w][tid];
        partials[((size_t)f * tiles + tile) * N + tid] = s;
    }
}

__device__ inline float clipf(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

// one projected corner folded into the running extents
__device__ inline void fold_corner(const double* c, const float* __restrict__ kc, bool first, float& xmin, float& xmax, float& ymin, float& ymax) {
    const float x = (float)c[0], y = (float)c[1], z = (float)c[2];
    const float p0 = ((kc[0] * x + kc[1] * y) + kc[2] * z) + kc[3];
    const float p1 = ((kc[4] * x + kc[5] * y) + kc[6] * z) + kc[7];
    const float p2 = ((kc[8] * x + kc[9] * y) + kc[10] * z) + kc[11];
    const float zc = p2 > 1.0f ? p2 : 1.0f;
    const float u = __fdiv_rn(p0, zc), v = __fdiv_rn(p1, zc);
    if (first) {
        xmin = xmax = u;
        ymin = ymax = v;
    } else {
        xmin = u < xmin ? u : xmin;
        xmax = u > xmax ? u : xmax;
        ymin = v < ymin ? v : ymin;
        ymax = v > ymax ? v : ymax;
    }
}

__global__ __launch_bounds__(kFinThreads) void snippet_finalize_kernel(
    const int32_t* __restrict__ partials, int tiles, int T, const float* __restrict__ kcolor, int color_h, int color_w,
    const double* __restrict__ poses, const float* __restrict__ obbs, const double* __restrict__ corners, const uint32_t* __restrict__ sym,
    uint32_t sym_pad, int S, int N, int max_box, Levels lv, float* __restrict__ obbs_out, uint32_t* __restrict__ sym_out,
    int32_t* __restrict__ num_valid, int32_t* __restrict__ frame_points, float* __restrict__ frame_trunc, int32_t* __restrict__ points,
    float* __restrict__ trunc, int32_t* __restrict__ difficulty, int32_t* __restrict__ valid_out) {
    __shared__ int32_t part[kFinGroups][kMaxBoxes];
    __shared__ int wave_total[2];
    // thread = (group g, box n): the groups share a frame's tiles (integer sums: any order gives the tile-order sum), group 0 goes on
    const int tid = threadIdx.x, n = tid & (kMaxBoxes - 1), g = tid >> 7, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool owner = g == 0 && n < N;
    const float* row = obbs + ((size_t)b * N + (n < N ? n : 0)) * 19;
    const double* given = corners ? corners + ((size_t)b * N + (n < N ? n : 0)) * 24 : nullptr;
    const float* kc = kcolor + (size_t)b * 16;
    const bool pad = owner ? row_is_padding(row) : true;
    const float wmax = (float)(color_w - 1), hmax = (float)(color_h - 1);
    int best_count = 0;
    float best_ratio = 0.0f;
    for (int t = 0; t < T; ++t) {
        const size_t f = (size_t)b * T + t;
        int s = 0;
        if (n < N) {
            const int32_t* p = partials + f * tiles * N + n;
#pragma unroll 8
            for (int k = g; k < tiles; k += kFinGroups) s += p[(size_t)k * N];
        }
        part[g][n] = s;
        __syncthreads();
        if (owner) {
            int count = 0;
#pragma unroll
            for (int i = 0; i < kFinGroups; ++i) count += part[i][n];
            float ratio = 0.0f;
            if (!pad) {
                const Inverse v = affine_inverse(poses + f * 12);
                float xmin, xmax, ymin, ymax;
                double c[3];
                corner_camera<0>(row, given, v, c);
                fold_corner(c, kc, true, xmin, xmax, ymin, ymax);
                corner_camera<1>(row, given, v, c);
                fold_corner(c, kc, false, xmin, xmax, ymin, ymax);
                corner_camera<2>(row, given, v, c);
                fold_corner(c, kc, false, xmin, xmax, ymin, ymax);
                corner_camera<3>(row, given, v, c);
                fold_corner(c, kc, false, xmin, xmax, ymin, ymax);
                corner_camera<4>(row, given, v, c);
                fold_corner(c, kc, false, xmin, xmax, ymin, ymax);
                corner_camera<5>(row, given, v, c);
                fold_corner(c, kc, false, xmin, xmax, ymin, ymax);
                corner_camera<6>(row, given, v, c);
                fold_corner(c, kc, false, xmin, xmax, ymin, ymax);
                corner_camera<7>(row, given, v, c);
                fold_corner(c, kc, false, xmin, xmax, ymin, ymax);
                const float area = (xmax - xmin) * (ymax - ymin);
                const float cx0 = clipf(xmin, wmax), cx1 = clipf(xmax, wmax), cy0 = clipf(ymin, hmax), cy1 = clipf(ymax, hmax);
                const float inside = (cx1 - cx0) * (cy1 - cy0);
                ratio = __fdiv_rn(inside, area > 1.0f ? area : 1.0f);
            }
            frame_points[f * N + n] = count;
            frame_trunc[f * N + n] = ratio;
            if (t == 0 || count > best_count) best_count = count;
            if (t == 0 || ratio > best_ratio) best_ratio = ratio;
        }
        __syncthreads();
    }
    bool valid = false;
    if (owner) {
        int level = lv.n;
        for (int i = lv.n - 1; i >= 0; --i)
            if (best_count > lv.count[i] && best_ratio > lv.ratio[i]) level = i;      // the first match wins
        valid = !pad && level < lv.max_level;
        points[(size_t)b * N + n] = best_count;
        trunc[(size_t)b * N + n] = best_ratio;
        difficulty[(size_t)b * N + n] = level;
        valid_out[(size_t)b * N + n] = valid ? 1 : 0;
    }
    const unsigned long long mask = __ballot(valid);
    if (lane == 0 && wave < 2) wave_total[wave] = __popcll(mask);                     // group 0 is waves 0 and 1
    __syncthreads();
    const int slot = __popcll(mask & ((1ull << lane) - 1ull)) + (wave ? wave_total[0] : 0);
    const int total = wave_total[0] + wave_total[1];
    const int kept = total < max_box ? total : max_box;
    if (valid && slot < max_box) {
        float* dst = obbs_out + ((size_t)b * max_box + slot) * 19;
#pragma unroll
        for (int i = 0; i < 19; ++i) dst[i] = row[i];
    }
    if (valid && slot < S) sym_out[(size_t)b * S + slot] = n < S ? sym[(size_t)b * S + n] : sym_pad;
    for (int i = kept * 19 + tid; i < max_box * 19; i += kFinThreads) obbs_out[(size_t)b * max_box * 19 + i] = -1.0f;
    for (int i = (total < S ? total : S) + tid; i < S; i += kFinThreads) sym_out[(size_t)b * S + i] = sym_pad;
    if (tid == 0) num_valid[b] = kept;
}

}  // namespace

bool snippet_sizes_ok(int B, int T, int Hd, int Wd, int N) {
    return B >= 1 && B <= 65535 / kMaxFrames && T >= 1 && T <= kMaxFrames && Hd >= 1 && Wd >= 1 && Hd <= kMaxSide && Wd <= kMaxSide && N >= 1 &&
           N <= kMaxBoxes;
}

// tiles of one frame: a frame that starts inside a word spans up to (H W + 3) / 4 rounded up words
int snippet_tiles(int Hd, int Wd) {
    const int64_t words = ((int64_t)Hd * Wd + 3 + 3) / 4;
    return (int)((words + kTileWords - 1) / kTileWords);
}

size_t snippet_workspace_bytes(int B, int T, int Hd, int Wd, int N) {
    return ((size_t)B * T * snippet_tiles(Hd, Wd) * N * 4 + 15) / 16 * 16;
}

hipError_t launch_snippet_targets(const uint16_t* depth, int B, int T, int Hd, int Wd, const float* kinv, const float* kcolor, int color_h,
                                  int color_w, const double* poses, const float* obbs, const double* corners, const void* sym, int sym_is_int,
                                  int S, int N, int max_box, const int32_t* level_counts, const float* level_ratios, int n_levels,
                                  int max_level, float depth_scale, void* ws, float* obbs_out, void* sym_out, int32_t* num_valid,
                                  int32_t* frame_points, float* frame_trunc, int32_t* points, float* trunc, int32_t* difficulty,
                                  int32_t* valid, hipStream_t s) {
    const int tiles = snippet_tiles(Hd, Wd);
    int32_t* partials = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(snippet_count_kernel, dim3((unsigned)tiles, (unsigned)(B * T)), dim3(kCountThreads), 0, s, depth,
                       (int64_t)B * T * Hd * Wd, T, Hd, Wd, kinv, poses, obbs, corners, N, depth_scale, tiles, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    Levels lv{};
    for (int i = 0; i < n_levels; ++i) {
        lv.count[i] = level_counts[i];
        lv.ratio[i] = level_ratios[i];
    }
    lv.n = n_levels;
    lv.max_level = max_level;
    const uint32_t sym_pad = sym_is_int ? 0xFFFFFFFFu : 0xBF800000u;      // -1 as int32, -1.0f
    hipLaunchKernelGGL(snippet_finalize_kernel, dim3((unsigned)B), dim3(kFinThreads), 0, s, partials, tiles, T, kcolor, color_h, color_w, poses,
                       obbs, corners, static_cast<const uint32_t*>(sym), sym_pad, S, N, max_box, lv, obbs_out, static_cast<uint32_t*>(sym_out),
                       num_valid, frame_points, frame_trunc, points, trunc, difficulty, valid);
    return hipGetLastError();
}

}  // namespace parq
