// Predicted / ground-truth boxes drawn into the input views on the device (parq_draw_boxes; the reference's draw_detections,
// utils/parq_utils.py:141-211, is a host loop over views x boxes through cv2).  Three launches, no atomics, no dependence on the
// order in which workgroups run:
//   1. draw_minmax_kernel   per-view min / max of the 3*H*W values in kParts contiguous parts, NaN propagating, into the workspace;
//   2. draw_project_kernel  one thread per (scene, view, box): the 8 world corners through T_world_pseudoCam^-1, T_camera_pseudoCam
//                           and the pinhole camera in float64 (contraction off: the NumPy statement of the rule performs the same
//                           correctly rounded operations in the same order), truncated, into 12 fixed slots of four int16 per box
//                           (x0, y0, x1, y1; x0 = kSentinel: nothing to draw).  Fixed slots keep the draw order without a prefix pass;
//   3. draw_raster_kernel   gather: one thread per output pixel (three channels), a workgroup per kTileW x kTileH tile.  The view's
//                           slots are walked from the last chunk of kChunk slots to the first; the slots of a chunk whose bounding
//                           box grown by 1 px meets the tile — and whose line passes within the capsule's width of it, which spares
//                           the pixels the long diagonals — are compacted in order into LDS (ballot + popcount), every pixel scans
//                           that list from the back and stops at its first hit — the last segment drawn over it.
// Coverage of a pixel by a segment is an integer capsule test (thickness 2 = half-width 1 around the integer segment).
#include "common.hpp"

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kParts = 64;                   // parts of a view in the min / max reduction (one workgroup each)
constexpr int kMinMaxThreads = 256;
constexpr int kTileW = 64, kTileH = 16;      // a wave owns one 64-pixel row of the tile: whole 256-byte rows per store
constexpr int kRasterThreads = kTileW * kTileH;
constexpr int kChunk = kRasterThreads;       // slots examined, and at most kept in LDS, per round: one per thread
constexpr int kGroup = 3;                    // chunks whose slots are loaded together (one load latency for the group); 256 boxes are
                                             // 3 chunks, and a fourth would pass 64 VGPRs, i.e. cost the second workgroup per CU
constexpr int kWaves = kRasterThreads / 64;
constexpr int kSentinel = -32768;
constexpr int kMaxCoord = 8191;              // endpoints are inside [0, kMaxCoord]: every product of the capsule test fits an int32

__device__ inline float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

struct MinMax {
    float mn, mx;
    bool nan;
    __device__ inline void take(float v) {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        nan |= v != v;
    }
};

// grid (kParts, B*T): part p of view v reduces the floats [p * per, min(n, (p + 1) * per)) of the view; 16-byte loads where the
// address allows, scalar loads for the ragged head and tail
__global__ __launch_bounds__(kMinMaxThreads) void draw_minmax_kernel(const float* __restrict__ images, int64_t n, int64_t per,
                                                                     float2* __restrict__ parts) {
    __shared__ float s_mn[kMinMaxThreads / 64], s_mx[kMinMaxThreads / 64];
    __shared__ int s_nan[kMinMaxThreads / 64];
    const int tid = threadIdx.x, view = blockIdx.y, part = blockIdx.x;
    const float* src = images + (int64_t)view * n;
    int64_t g0 = (int64_t)part * per, g1 = g0 + per;
    if (g1 > n) g1 = n;
    MinMax r{__builtin_inff(), -__builtin_inff(), false};
    if (g0 < g1) {
        // first index >= g0 whose address is a multiple of 16 bytes
        const int64_t mis = (int64_t)(((uintptr_t)(src + g0) >> 2) & 3);
        int64_t a = g0 + ((4 - mis) & 3);
        if (a > g1) a = g1;
        const int64_t nvec = (g1 - a) >> 2, tail = a + nvec * 4;
        if (tid < a - g0) r.take(src[g0 + tid]);
        const float4* v4 = reinterpret_cast<const float4*>(src + a);
        for (int64_t i = tid; i < nvec; i += kMinMaxThreads) {
            const float4 v = v4[i];
            r.take(v.x); r.take(v.y); r.take(v.z); r.take(v.w);
        }
        if (tid < g1 - tail) r.take(src[tail + tid]);
    }
    const float mn = wave_min(r.mn), mx = wave_max(r.mx);
    const bool nan = __ballot(r.nan) != 0ull;
    if ((tid & 63) == 0) {
        s_mn[tid >> 6] = mn; s_mx[tid >> 6] = mx; s_nan[tid >> 6] = nan;
    }
    __syncthreads();
    if (tid == 0) {
        MinMax t{s_mn[0], s_mx[0], s_nan[0] != 0};
#pragma unroll
        for (int w = 1; w < kMinMaxThreads / 64; ++w) {
            t.mn = s_mn[w] < t.mn ? s_mn[w] : t.mn;
            t.mx = s_mx[w] > t.mx ? s_mx[w] : t.mx;
            t.nan |= s_nan[w] != 0;
        }
        const float q = __builtin_nanf("");
        parts[(int64_t)view * kParts + part] = t.nan ? make_float2(q, q) : make_float2(t.mn, t.mx);
    }
}

// one thread per (scene, view, box); slots (B, T, M, 12) of packed (x0 | y0 << 16, x1 | y1 << 16)
__global__ __launch_bounds__(64) void draw_project_kernel(const float* __restrict__ camera, const float* __restrict__ T_cp,
                                                          const float* __restrict__ T_wp, const float* __restrict__ corners,
                                                          const int32_t* __restrict__ labels, const unsigned char* __restrict__ keep,
                                                          const int32_t* __restrict__ count, int num_classes, int T, int M, int64_t total,
                                                          int2* __restrict__ slots) {
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= total) return;
    const int m = (int)(idx % M);
    const int64_t view = idx / M, box = (view / T) * M + m;
    const int lab = labels[box];
    bool draw = lab >= 0 && lab < num_classes - 1;                   // the background class num_classes - 1 and foreign labels: nothing
    if (keep && keep[box] == 0) draw = false;
    if (count && m >= count[view / T]) draw = false;
    int px[8], py[8];
    unsigned valid = 0u;
    if (draw) {
        double Rw[9], tw[3], Rc[9], tc[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) { Rw[i] = (double)T_wp[view * 12 + i]; Rc[i] = (double)T_cp[view * 12 + i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) { tw[i] = (double)T_wp[view * 12 + 9 + i]; tc[i] = (double)T_cp[view * 12 + 9 + i]; }
        const float* cam = camera + view * 6;
        const double w1 = (double)cam[0] - 1.0, h1 = (double)cam[1] - 1.0, fx = (double)cam[2], fy = (double)cam[3], cx = (double)cam[4],
                     cy = (double)cam[5];
        const float* cw = corners + box * 24;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double d0 = (double)cw[3 * k] - tw[0], d1 = (double)cw[3 * k + 1] - tw[1], d2 = (double)cw[3 * k + 2] - tw[2];
            const double p0 = (Rw[0] * d0 + Rw[3] * d1) + Rw[6] * d2;        // R_wp^T (p_w - t_wp)
            const double p1 = (Rw[1] * d0 + Rw[4] * d1) + Rw[7] * d2;
            const double p2 = (Rw[2] * d0 + Rw[5] * d1) + Rw[8] * d2;
            const double x = ((Rc[0] * p0 + Rc[1] * p1) + Rc[2] * p2) + tc[0];
            const double y = ((Rc[3] * p0 + Rc[4] * p1) + Rc[5] * p2) + tc[1];
            const double z = ((Rc[6] * p0 + Rc[7] * p1) + Rc[8] * p2) + tc[2];
            const bool front = z > 1e-3;
            const double zc = z > 1e-3 ? z : 1e-3;
            const double u = (x / zc) * fx + cx, v = (y / zc) * fy + cy;
            // a NaN fails every comparison; the kMaxCoord guard only matters for a camera larger than the largest image
            const bool ok = front && u >= 0.0 && u <= w1 && v >= 0.0 && v <= h1 && u <= (double)kMaxCoord && v <= (double)kMaxCoord;
            px[k] = ok ? (int)u : 0;
            py[k] = ok ? (int)v : 0;
            valid |= ok ? (1u << k) : 0u;
        }
    }
    constexpr int ea[12] = {0, 1, 2, 0, 0, 1, 2, 3, 4, 5, 6, 4}, eb[12] = {1, 2, 3, 3, 4, 5, 6, 7, 5, 6, 7, 7};
    int2* dst = slots + idx * 12;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const bool ok = ((valid >> ea[e]) & (valid >> eb[e]) & 1u) != 0u;
        int2 s;
        s.x = ok ? (px[ea[e]] | (py[ea[e]] << 16)) : (kSentinel & 0xffff);
        s.y = ok ? (px[eb[e]] | (py[eb[e]] << 16)) : 0;
        dst[e] = s;
    }
}

// floor(sqrt(n)), 0 <= n < 2^31: for integers, cross^2 <= L2 is |cross| <= isqrt(L2), which keeps the per-pixel test in 32 bits
__device__ inline int isqrt(int n) {
    int r = (int)__builtin_sqrt((double)n);
    while ((int64_t)r * r > (int64_t)n) --r;
    while ((int64_t)(r + 1) * (r + 1) <= (int64_t)n) ++r;
    return r;
}

// a kept segment as the pixels read it: a = (x0, y0, dx, dy), b = (L2, isqrt(L2), class, -)
__device__ inline bool capsule_covers(int x, int y, const int4 a, const int4 b) {
    const int qx = x - a.x, qy = y - a.y;
    const int u = qx * a.z + qy * a.w;
    if (b.x == 0 || u <= 0) return qx * qx + qy * qy <= 1;
    if (u >= b.x) {
        const int rx = qx - a.z, ry = qy - a.w;
        return rx * rx + ry * ry <= 1;
    }
    const int cr = a.z * qy - a.w * qx;
    return (cr < 0 ? -cr : cr) <= b.y;
}

// grid (ceil(W / kTileW), ceil(H / kTileH), B*T); out (B, 3, T*H, W) float32 or uint8
template <bool kU8>
__global__ __launch_bounds__(kRasterThreads) void draw_raster_kernel(const float* __restrict__ images, const float2* __restrict__ parts,
                                                                     const int2* __restrict__ slots, const int32_t* __restrict__ labels,
                                                                     const float* __restrict__ colors, int T, int H, int W, int M,
                                                                     void* __restrict__ out) {
    __shared__ int4 s_a[kChunk], s_b[kChunk];
    __shared__ int s_wave[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int view = blockIdx.z, b = view / T, t = view - b * T;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const int x = tx0 + lane, y = ty0 + wave;
    const bool inside = x < W && y < H;

    // the view's min / max from its kParts parts (every wave for itself: no barrier)
    static_assert(kParts == 64, "one part per lane");
    const float2 pm = parts[(int64_t)view * kParts + lane];
    const bool nan = __ballot(pm.x != pm.x || pm.y != pm.y) != 0ull;
    float mn = wave_min(pm.x), mx = wave_max(pm.y);
    if (nan) mn = mx = __builtin_nanf("");

    // the pixel's three values are requested before the slots are walked: the walk hides their latency
    const int64_t hw = (int64_t)H * W;
    float px[3] = {0.f, 0.f, 0.f};
    if (inside) {
        const float* src = images + (int64_t)view * 3 * hw + (int64_t)y * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = src[c * hw];
    }

    int hit = -1;
    const int S = M * 12;
    const int2* vs = slots + (int64_t)view * S;
    // chunks from the last to the first, kGroup at a time: the slots of a group are requested together, one load latency per group
    for (int cg = (S + kChunk - 1) / kChunk; cg > 0; cg -= kGroup) {
        int2 e[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            const int s = (cg - 1 - j) * kChunk + tid;
            e[j] = (cg - 1 - j >= 0 && s < S) ? vs[s] : make_int2(kSentinel & 0xffff, 0);
        }
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (cg - 1 - j < 0) break;                    // the same in every thread
            const int s = (cg - 1 - j) * kChunk + tid;
            const int x0 = (short)(e[j].x & 0xffff), y0 = e[j].x >> 16, x1 = (short)(e[j].y & 0xffff), y1 = e[j].y >> 16;
            const int lo_x = (x0 < x1 ? x0 : x1) - 1, hi_x = (x0 < x1 ? x1 : x0) + 1;
            const int lo_y = (y0 < y1 ? y0 : y1) - 1, hi_y = (y0 < y1 ? y1 : y0) + 1;
            bool keep = x0 != kSentinel && lo_x <= tx0 + kTileW - 1 && hi_x >= tx0 && lo_y <= ty0 + kTileH - 1 && hi_y >= ty0;
            int4 ea = make_int4(0, 0, 0, 0), eb = make_int4(0, 0, 0, 0);
            if (keep) {
                // a second, equally conservative cut: every covered pixel has |cross| <= isqrt(L2) (the end caps too: there |cross| is
                // |dx| or |dy|), and cross is linear, so a tile whose four corners lie beyond that on one side holds no covered pixel
                const int dx = x1 - x0, dy = y1 - y0, L2 = dx * dx + dy * dy, r = isqrt(L2);
                const int ax = tx0 - x0, bx = ax + kTileW - 1, ay = ty0 - y0, by = ay + kTileH - 1;
                const int c0 = dx * ay - dy * ax, c1 = dx * ay - dy * bx, c2 = dx * by - dy * ax, c3 = dx * by - dy * bx;
                const int cmin = min(min(c0, c1), min(c2, c3)), cmax = max(max(c0, c1), max(c2, c3));
                keep = cmin <= r && cmax >= -r;
                ea = make_int4(x0, y0, dx, dy);
                eb = make_int4(L2, r, 0, 0);
            }
            const unsigned long long bal = __ballot(keep);
            if (lane == 0) s_wave[wave] = __popcll(bal);
            __syncthreads();                              // (also: every wave is done scanning the previous chunk's list)
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const int c = s_wave[w];
                before += w < wave ? c : 0;
                total += c;
            }
            if (keep) {
                const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
                eb.z = labels[(int64_t)b * M + s / 12];
                s_a[pos] = ea;
                s_b[pos] = eb;
            }
            __syncthreads();                              // (also: every wave has read s_wave before the next chunk rewrites it)
            if (inside && hit < 0) {
                for (int k = total - 1; k >= 0; --k) {
                    const int4 gb = s_b[k];
                    if (capsule_covers(x, y, s_a[k], gb)) {
                        hit = gb.z;
                        break;
                    }
                }
            }
        }
    }
    if (!inside) return;
    const int64_t o = ((int64_t)b * 3 * T * H + (int64_t)t * H + y) * W + x, ostride = (int64_t)T * hw;
    const float den = mx - mn;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v;
        if (hit >= 0) v = colors[hit * 3 + c];
        else v = (px[c] - mn) / den;
        if (kU8) {
            const float s255 = v * 255.0f;                // truncation toward zero; NaN -> 0
            static_cast<unsigned char*>(out)[o + c * ostride] = s255 == s255 ? (unsigned char)(int)s255 : (unsigned char)0;
        } else {
            static_cast<float*>(out)[o + c * ostride] = v;
        }
    }
}

}  // namespace

size_t draw_minmax_bytes(int B, int T) { return (size_t)B * T * kParts * sizeof(float2); }

hipError_t launch_draw_minmax(const float* images, int B, int T, int H, int W, void* parts, hipStream_t s) {
    const int64_t n = (int64_t)3 * H * W;
    const int64_t per = (n + kParts - 1) / kParts;
    hipLaunchKernelGGL(draw_minmax_kernel, dim3(kParts, (unsigned)(B * T)), dim3(kMinMaxThreads), 0, s, images, n, per,
                       static_cast<float2*>(parts));
    return hipGetLastError();
}

hipError_t launch_draw_project(const float* camera, const float* T_cp, const float* T_wp, const float* corners, const int32_t* labels,
                               const unsigned char* keep, const int32_t* count, int num_classes, int B, int T, int M, void* slots,
                               hipStream_t s) {
    const int64_t total = (int64_t)B * T * M, blocks = (total + 63) / 64;
    if (total < 1 || blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_project_kernel, dim3((unsigned)blocks), dim3(64), 0, s, camera, T_cp, T_wp, corners, labels, keep, count,
                       num_classes, T, M, total, static_cast<int2*>(slots));
    return hipGetLastError();
}

hipError_t launch_draw_raster(const float* images, const void* parts, const void* slots, const int32_t* labels, const float* colors, int B,
                              int T, int H, int W, int M, void* out, int out_uint8, hipStream_t s) {
    const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)(B * T));
    if (out_uint8)
        hipLaunchKernelGGL(draw_raster_kernel<true>, grid, dim3(kRasterThreads), 0, s, images, static_cast<const float2*>(parts),
                           static_cast<const int2*>(slots), labels, colors, T, H, W, M, out);
    else
        hipLaunchKernelGGL(draw_raster_kernel<false>, grid, dim3(kRasterThreads), 0, s, images, static_cast<const float2*>(parts),
                           static_cast<const int2*>(slots), labels, colors, T, H, W, M, out);
    return hipGetLastError();
}

}  // namespace parq
