// Raw camera frames resized on the device (parq_frames_resize; the reference's ResizeImage + ToTensor + Normalize,
// datasets/transforms.py:77-100,118-132,177-188, resize every frame with Pillow on one host core).  The rule is Pillow's 8-bit
// bilinear resample restated in integers (include/parq_hip.h): a per-axis plan of 22-bit fixed-point coefficients made on the host in
// float64 (parq_frame_plan, below: contraction off, the operations and their order are the rule), a horizontal pass rounded to
// 8 bits and a vertical pass over that.  One launch, no atomics, no dependence on the order in which workgroups run.
//
// frames_resize_kernel: a workgroup of 256 threads per kTileW x kTileH output tile of one frame.
//   1. the tile's part of both plans goes into LDS, every tap range cut down to the taps that fall on real (not padded) pixels: a
//      padded pixel is 0 and adds nothing to a sum, so the border is never read, in memory or in LDS;
//   2. the real input rows the tile's vertical taps span are staged into LDS in chunks of `chunk_rows` rows, as the aligned dwords
//      that cover the bytes the tile's horizontal taps span.  Rows of 3 * W_in bytes start at any address modulo 4: the row's first
//      needed byte sits at (address & 3) of its first dword.  A dword that is not wholly inside the N frames (the first of an
//      unaligned buffer, the last of a buffer whose size is no multiple of 4) is put together from byte loads of its inside bytes;
//   3. the horizontal pass reads the chunk and writes the 8-bit intermediate rows (LDS), one thread per (row, output column), three
//      channels each; the vertical pass reads those and writes the output, consecutive lanes on consecutive output columns.
// A plan is device memory this code cannot trust: every xmin / n read from it is clamped so that no LDS or global index leaves what
// the launch sized (a wrong plan gives wrong pixels, never a wild access).
#include "../../include/parq_hip.h"
#include "common.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kTileW = 32, kTileH = 8;       // output pixels per workgroup; at 4.05x the 8 rows redo about a fifth of the horizontal work
constexpr int kThreads = 256;
constexpr int kMaxSide = 8192;               // every side: input, padded input, output
constexpr int kMaxDown = 8;                  // padded input side <= kMaxDown * output side: at most 2 * 8 + 1 = 17 taps
constexpr int kMaxTaps = 2 * kMaxDown + 1;
constexpr int kBits = 22;                    // fractional bits of a coefficient
constexpr int kStageBytes = 32 * 1024;       // LDS for one chunk of staged input rows
constexpr int kTmpStride = kTileW * 3;       // bytes of an intermediate row

int plan_ksize(int in, int out) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(fs) * 2 + 1;
}

bool plan_sizes_ok(int in, int out) {
    return in >= 1 && out >= 1 && in <= kMaxSide && out <= kMaxSide && (int64_t)in <= (int64_t)kMaxDown * out;
}

// the largest number of input pixels the taps of `tile` consecutive outputs span: the first tap of output i is above
// (i + 0.5) scale - support - 0.5 and the last below (i + 0.5) scale + support + 0.5
int span_bound(int in, int out, int tile) {
    const double scale = (double)in / (double)out;
    const double support = scale < 1.0 ? 1.0 : scale;
    const int b = (int)std::ceil((tile - 1) * scale + 2.0 * support) + 2;
    return b < in ? b : in;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

template <bool kU8>
__global__ __launch_bounds__(kThreads) void frames_resize_kernel(
    const unsigned char* __restrict__ frames, int64_t total_bytes, int H_in, int W_in, int left, int top,
    const int32_t* __restrict__ plan_x, const int32_t* __restrict__ plan_y, int kx, int ky, int H_out, int W_out, void* __restrict__ out,
    int cols_max, int rows_max, int row_dwords, int chunk_rows) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* stage = smem;                                              // chunk_rows x row_dwords
    int* cxs = reinterpret_cast<int*>(stage + (size_t)chunk_rows * row_dwords);   // kTileW x kx coefficients
    int* cys = cxs + kTileW * kx;                                        // kTileH x ky
    int* xk0 = cys + kTileH * ky;                                        // first / one-past-last tap on a real column, per output column
    int* xk1 = xk0 + kTileW;
    int* xsrc = xk1 + kTileW;                                            // byte offset of tap 0's pixel from the first staged byte of a row
    int* yk0 = xsrc + kTileW;
    int* yk1 = yk0 + kTileH;
    int* ysrc = yk1 + kTileH;                                            // intermediate row of tap 0
    unsigned char* tmp = reinterpret_cast<unsigned char*>(ysrc + kTileH);   // rows_max x kTmpStride

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int tw = min(kTileW, W_out - x0), th = min(kTileH, H_out - y0);
    const int ex = 2 + kx, ey = 2 + ky;
    const int32_t* px = plan_x + 1 + (size_t)x0 * ex;
    const int32_t* py = plan_y + 1 + (size_t)y0 * ey;
    const unsigned char* frame = frames + (size_t)blockIdx.z * H_in * W_in * 3;

    // the real columns and rows the tile reads (uniform: every thread computes the same)
    int cx0 = clampi(clampi(px[0], 0, 2 * kMaxSide) - left, 0, W_in);
    const int32_t* pxl = px + (size_t)(tw - 1) * ex;
    int cx1 = clampi(clampi(pxl[0], 0, 2 * kMaxSide) + clampi(pxl[1], 0, kx) - left, cx0, W_in);
    cx1 = min(cx1, cx0 + cols_max);
    int ry0 = clampi(clampi(py[0], 0, 2 * kMaxSide) - top, 0, H_in);
    const int32_t* pyl = py + (size_t)(th - 1) * ey;
    int ry1 = clampi(clampi(pyl[0], 0, 2 * kMaxSide) + clampi(pyl[1], 0, ky) - top, ry0, H_in);
    ry1 = min(ry1, ry0 + rows_max);

    for (int i = tid; i < tw * kx; i += kThreads) {
        const int xx = i / kx, k = i - xx * kx;
        cxs[i] = px[(size_t)xx * ex + 2 + k];
    }
    for (int i = tid; i < th * ky; i += kThreads) {
        const int yy = i / ky, k = i - yy * ky;
        cys[i] = py[(size_t)yy * ey + 2 + k];
    }
    if (tid < tw) {
        const int32_t* p = px + (size_t)tid * ex;
        const int s = clampi(p[0], 0, 2 * kMaxSide) - left;              // real column of tap 0 (negative: in the left border)
        const int n = clampi(p[1], 0, kx);
        const int k0 = clampi(cx0 - s, 0, n);
        xk0[tid] = k0;
        xk1[tid] = clampi(cx1 - s, k0, n);
        xsrc[tid] = (s - cx0) * 3;
    } else if (tid >= 64 && tid < 64 + th) {
        const int yy = tid - 64;
        const int32_t* p = py + (size_t)yy * ey;
        const int s = clampi(p[0], 0, 2 * kMaxSide) - top;
        const int n = clampi(p[1], 0, ky);
        const int k0 = clampi(ry0 - s, 0, n);
        yk0[yy] = k0;
        yk1[yy] = clampi(ry1 - s, k0, n);
        ysrc[yy] = s - ry0;
    }
    __syncthreads();

    const int nbytes = (cx1 - cx0) * 3;
    const int ndw = (nbytes + 6) / 4;                                    // dwords that cover nbytes bytes from any of the 4 alignments
    const uintptr_t buf_lo = reinterpret_cast<uintptr_t>(frames), buf_hi = buf_lo + (uintptr_t)total_bytes;
    for (int c0 = ry0; c0 < ry1; c0 += chunk_rows) {
        const int nr = min(chunk_rows, ry1 - c0);
        if (nbytes > 0) {
            for (int i = tid; i < nr * ndw; i += kThreads) {
                const int r = i / ndw, d = i - r * ndw;
                const uintptr_t g = reinterpret_cast<uintptr_t>(frame) + ((size_t)(c0 + r) * W_in + cx0) * 3;
                const uintptr_t a = (g & ~(uintptr_t)3) + (uintptr_t)d * 4;
                uint32_t v = 0;
                if (a < g + (uintptr_t)nbytes) {                         // (the last of the ndw dwords is past the row's bytes at some alignments)
                    if (a >= buf_lo && a + 4 <= buf_hi) {
                        v = *reinterpret_cast<const uint32_t*>(a);
                    } else {
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (a + b >= buf_lo && a + b < buf_hi) v |= (uint32_t)(*reinterpret_cast<const unsigned char*>(a + b)) << (8 * b);
                    }
                }
                stage[(size_t)r * row_dwords + d] = v;
            }
        }
        __syncthreads();
        for (int i = tid; i < nr * tw; i += kThreads) {
            const int r = i / tw, xx = i - r * tw;
            const uint32_t shift = ((uint32_t)reinterpret_cast<uintptr_t>(frame) + ((uint32_t)(c0 + r) * (uint32_t)W_in + (uint32_t)cx0) * 3u) & 3u;
            const unsigned char* row = reinterpret_cast<const unsigned char*>(stage + (size_t)r * row_dwords) + shift + xsrc[xx];
            const int* cf = cxs + xx * kx;
            int a0 = 1 << (kBits - 1), a1 = a0, a2 = a0;
            const int k1 = xk1[xx];
            for (int k = xk0[xx]; k < k1; ++k) {
                const int c = cf[k];
                const unsigned char* p = row + k * 3;
                a0 += c * (int)p[0];
                a1 += c * (int)p[1];
                a2 += c * (int)p[2];
            }
            unsigned char* t = tmp + (size_t)(c0 - ry0 + r) * kTmpStride + xx * 3;
            t[0] = (unsigned char)min(a0 >> kBits, 255);                 // the weights are never negative: no clamp at 0
            t[1] = (unsigned char)min(a1 >> kBits, 255);
            t[2] = (unsigned char)min(a2 >> kBits, 255);
        }
        __syncthreads();
    }

    const size_t plane = (size_t)H_out * W_out;
    for (int i = tid; i < 3 * th * tw; i += kThreads) {
        const int c = i / (th * tw), rem = i - c * (th * tw);
        const int yy = rem / tw, xx = rem - yy * tw;
        const int* cf = cys + yy * ky;
        const unsigned char* col = tmp + (ptrdiff_t)ysrc[yy] * kTmpStride + xx * 3 + c;
        int acc = 1 << (kBits - 1);
        const int k1 = yk1[yy];
        for (int k = yk0[yy]; k < k1; ++k) acc += cf[k] * (int)col[(ptrdiff_t)k * kTmpStride];
        const int res = min(acc >> kBits, 255);
        const size_t o = ((size_t)blockIdx.z * 3 + c) * plane + (size_t)(y0 + yy) * W_out + (x0 + xx);
        if (kU8) static_cast<unsigned char*>(out)[o] = (unsigned char)res;
        else static_cast<float*>(out)[o] = __fdiv_rn((float)res, 255.0f);    // one correctly rounded division, as NumPy's / torch's
    }
}

}  // namespace

bool frames_sizes_ok(int N, int H_in, int W_in, int pl, int pt, int pr, int pb, int H_out, int W_out) {
    if (N < 1 || H_in < 1 || W_in < 1 || H_out < 1 || W_out < 1 || pl < 0 || pt < 0 || pr < 0 || pb < 0) return false;
    if (H_in > kMaxSide || W_in > kMaxSide || pl > kMaxSide || pt > kMaxSide || pr > kMaxSide || pb > kMaxSide) return false;
    return N <= 65535 && plan_sizes_ok(W_in + pl + pr, W_out) && plan_sizes_ok(H_in + pt + pb, H_out);
}

hipError_t launch_frames_resize(const unsigned char* frames, int N, int H_in, int W_in, int pl, int pt, int pr, int pb, const int32_t* plan_x,
                                const int32_t* plan_y, int H_out, int W_out, void* out, int out_uint8, hipStream_t s) {
    const int Wp = W_in + pl + pr, Hp = H_in + pt + pb;
    const int kx = plan_ksize(Wp, W_out), ky = plan_ksize(Hp, H_out);
    const int cols_max = std::min(W_in, span_bound(Wp, W_out, kTileW)), rows_max = std::min(H_in, span_bound(Hp, H_out, kTileH));
    const int row_dwords = ((cols_max * 3 + 6) / 4) | 1;                 // odd: consecutive rows start on different banks
    const int chunk_rows = std::max(1, std::min(rows_max, kStageBytes / (row_dwords * 4)));
    const size_t lds = ((size_t)chunk_rows * row_dwords + (size_t)kTileW * kx + (size_t)kTileH * ky + 3 * kTileW + 3 * kTileH) * 4 +
                       ((size_t)rows_max * kTmpStride + 3) / 4 * 4;
    const dim3 grid((unsigned)((W_out + kTileW - 1) / kTileW), (unsigned)((H_out + kTileH - 1) / kTileH), (unsigned)N);
    const int64_t total = (int64_t)N * H_in * W_in * 3;
    if (out_uint8)
        hipLaunchKernelGGL(frames_resize_kernel<true>, grid, dim3(kThreads), lds, s, frames, total, H_in, W_in, pl, pt, plan_x, plan_y, kx, ky,
                           H_out, W_out, out, cols_max, rows_max, row_dwords, chunk_rows);
    else
        hipLaunchKernelGGL(frames_resize_kernel<false>, grid, dim3(kThreads), lds, s, frames, total, H_in, W_in, pl, pt, plan_x, plan_y, kx, ky,
                           H_out, W_out, out, cols_max, rows_max, row_dwords, chunk_rows);
    return hipGetLastError();
}

}  // namespace parq

// ---- the per-axis plan: pure host functions (no GPU, no allocation, no environment) ---------------------------------------------
extern "C" size_t parq_frame_plan_ints(int32_t in_size, int32_t out_size) {
    if (!parq::plan_sizes_ok(in_size, out_size)) return 0;
    return 1 + (size_t)out_size * (2 + (size_t)parq::plan_ksize(in_size, out_size));
}

extern "C" int parq_frame_plan(int32_t in_size, int32_t out_size, int32_t* plan_host) {
    if (!plan_host || !parq::plan_sizes_ok(in_size, out_size)) return PARQ_ERR_ARG;
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    plan_host[0] = ksize;
    double w[parq::kMaxTaps];
    for (int xx = 0; xx < out_size; ++xx) {
        int32_t* e = plan_host + 1 + (size_t)xx * (2 + ksize);
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        int n = xmax - xmin;
        if (n > ksize) n = ksize;                                        // (never: n <= 2 * support + 1 <= ksize)
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        e[0] = xmin;
        e[1] = n;
        for (int x = 0; x < ksize; ++x) e[2 + x] = 0;
        for (int x = 0; x < n; ++x) {
            const double k = ww != 0.0 ? w[x] / ww : w[x];
            e[2 + x] = (int32_t)(0.5 + k * 4194304.0);
        }
    }
    return PARQ_OK;
}
