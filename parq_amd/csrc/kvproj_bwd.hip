// Weight / bias gradient of the hoisted K/V projection (training backward):
//
//     dW_kv[n][k] += sum_m g[m][n] * tokens[m][k]          db_kv[n] += sum_m g[m][n]
//
// with m running over ALL tokens of the scene batch (768 000 rows at BASELINE cfg 4 per GPU), n over the 2C = 512 K|V columns and
// k over the C = 256 token channels: 201 GFLOP whose output is 0.5 MB.  The generic row-split fp32 kernel (gemm_tn_kernel,
// backward.hip: one 4-byte load per lane per MFMA operand) runs it at 45 TFLOP/s; here the same contraction goes through the
// fp16 matrix pipe with the hi/lo split used by the forward projection (three 32x32x16 MFMAs per product, fp32 accumulation,
// fp32-class result) and every token / gradient element is fetched and converted once per workgroup.
//
// Both operands are row-major [m][col] and the contraction runs over m, so both MFMA fragments (8 consecutive m for one column)
// are transposes of the memory layout.  The transpose happens in the staging pass: thread = one column, it loads 32 consecutive
// rows of its column (the 64 lanes of a wave read 256 contiguous bytes of each row), splits them and writes the LDS image
// [column][32 m] as 8-byte pieces; fragments are then plain 16-byte reads.
//
//   workgroup = 512 threads = 256 columns of g (one of the two n-slabs) + the 256 token channels, 32 rows per step,
//               double-buffered LDS (2 x 64 KB), one barrier per step, the next step's rows in flight in registers;
//   wave (wn, wk) of the 4 x 2 wave grid owns the 64 x 128 block of the slab's 256 x 256 outputs: 2 x 4 accumulators;
//   grid      = 2 slabs x S row ranges (S = CUs / 2); partial results are added to the gradient arena with float atomics
//               (as the row-split generic kernel does); the bias gradient falls out of the staging pass (column sums of g).
//
// g is multiplied by a power of two read from `scale` (max |g| -> ~2^10, measured by the attention backward's epilogue) so that
// the low halves of small gradient values stay clear of the fp16 subnormals; the result is multiplied back.
//
// Token type TT (training on 16-bit tokens, parq_set_train_token_type): the x operand is read as fp32, fp16 or bf16 elements.  A
// 16-bit token thread owns TWO adjacent channels and 16 of the step's 32 rows, so a wave still reads 256 contiguous bytes of a row
// with one 4-byte load per lane, and it writes whole 16-byte pieces (8 rows of one channel) of the same LDS image.  bf16 values are
// widened in registers and split exactly as their fp32 copies would be (same hi / lo bits).  An fp16 value IS its hi half and its lo
// half is zero: no B_lo image is built (2 x 48 KB of LDS) and the a_hi x b_lo product is not issued — two MFMAs per product; what is
// left out adds exact zeros, so the accumulators equal those of the fp32 instantiation on the widened tokens.
#include "common.hpp"

namespace parq {

namespace {

constexpr int kTM = 32;                          // rows per step
constexpr int kCols = 256;                       // columns of each operand per workgroup
constexpr int kImgHalfs = kCols * kTM;           // one operand image (hi or lo), 16 KB
template <int TT> constexpr int buf_halfs() { return (TT == kTokF16 ? 3 : 4) * kImgHalfs; }   // A_hi | A_lo | B_hi | B_lo (no B_lo: fp16 x)

struct KvBwdArgs {
    const float* g; int64_t ldg;                 // [M][2C] gradient of K | V (token-major)
    const void* x; int64_t ldx;                  // [M][C] tokens, elements of the kernel's token type (ldx in elements)
    float* dW; int64_t ldw;                      // [2C][C], +=
    float* db;                                   // [2C], +=
    const float* scale;                          // power of two applied to g
    int M, nsplit;
    float* part;                                 // deterministic mode: [nsplit][512][256] partials of this launch's dW block, then
                                                 // [nsplit][512] of db — plain stores, summed in row-range order; null = atomics
};

// position (in 16-bit units) of rows [8 q, 8 q + 8) of column c inside an operand image: 64 bytes per column, the 16-byte chunk
// index q is XOR-ed with bits 2..3 of the column so that the 16 lanes a ds_read_b128 serves per cycle hit 16 different slots
__device__ __forceinline__ int img_off(int c, int q) { return c * kTM + ((q ^ ((c >> 2) & 3)) << 3); }

template <int TT>
__global__ __launch_bounds__(512, 1) void kvproj_bwd_split_kernel(KvBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];          // [2 buffers][A_hi | A_lo | B_hi | B_lo]
    constexpr int kBufHalfs = buf_halfs<TT>();
    constexpr bool T16 = TT != kTokF32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int slab = blockIdx.x & 1, split = blockIdx.x >> 1;
    const float sc = *a.scale, inv_sc = 1.f / sc;

    // rows of this workgroup: a contiguous range, multiple of 32 except for the last one
    const int steps_total = (a.M + kTM - 1) / kTM;
    const int s_begin = (int)((int64_t)split * steps_total / a.nsplit);
    const int s_end = (int)((int64_t)(split + 1) * steps_total / a.nsplit);

    // staging: thread -> one column (threads 0..255: g column slab*256 + tid, threads 256..511: token channel tid - 256)
    const bool isA = tid < kCols;
    const int col = isA ? tid : tid - kCols;
    const float* src = isA ? a.g + slab * kCols + col : reinterpret_cast<const float*>(a.x) + col;
    const int64_t ld = isA ? a.ldg : a.ldx;
    const float mul = isA ? sc : 1.f;
    // 16-bit tokens: token thread -> channels 2 cp, 2 cp + 1 (one 4-byte word per row) and rows [16 rh, 16 rh + 16) of the step
    const int cp = col & 127, rh = col >> 7;
    const unsigned int* src16 = reinterpret_cast<const unsigned int*>(a.x) + cp;       // row stride ldx / 2 words
    float stg[kTM];                              // (16-bit token threads: 16 raw words)
    float csum = 0.f;
    auto fetch = [&](int step) {
        const int m0 = step * kTM;
        if (T16 && !isA) {
            const int r0 = m0 + rh * 16;
            const int64_t ldw = a.ldx >> 1;
            if (m0 + kTM <= a.M) {
#pragma unroll
                for (int r = 0; r < 16; ++r) stg[r] = __builtin_bit_cast(float, src16[(int64_t)(r0 + r) * ldw]);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) stg[r] = r0 + r < a.M ? __builtin_bit_cast(float, src16[(int64_t)(r0 + r) * ldw]) : 0.f;
            }
            return;
        }
        if (m0 + kTM <= a.M) {
#pragma unroll
            for (int r = 0; r < kTM; ++r) stg[r] = src[(int64_t)(m0 + r) * ld];
        } else {
#pragma unroll
            for (int r = 0; r < kTM; ++r) stg[r] = m0 + r < a.M ? src[(int64_t)(m0 + r) * ld] : 0.f;
        }
    };
    auto stage = [&](int buf) {
        _Float16* hi = lds + buf * kBufHalfs + (isA ? 0 : 2 * kImgHalfs);
        _Float16* lo = hi + kImgHalfs;
        typedef _Float16 half4v __attribute__((ext_vector_type(4)));
        if constexpr (T16) {
            if (!isA) {
                // one 16-byte piece = rows [8 q, 8 q + 8) of one channel.  Odd channel pairs write their odd channel first: the 8 lanes
                // a ds_write_b128 serves per cycle then cover both 64-byte halves x 4 swizzled chunks = the 8 slots of the 128-byte
                // bank row (the same channel from all 8 lanes would use 4 of them twice)
                const bool odd = cp & 1;
#pragma unroll
                for (int qq = 0; qq < 2; ++qq) {
                    u32x4 H[2], L[2];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned int u0 = __builtin_bit_cast(unsigned int, stg[8 * qq + 2 * j]);
                        const unsigned int u1 = __builtin_bit_cast(unsigned int, stg[8 * qq + 2 * j + 1]);
                        if constexpr (TT == kTokF16) {
                            H[0][j] = (u0 & 0xffffu) | (u1 << 16);
                            H[1][j] = (u0 >> 16) | (u1 & 0xffff0000u);
                        } else {
                            half2v h, l;
                            split_pair(bf16_bits_to_f32(u0 & 0xffffu), bf16_bits_to_f32(u1 & 0xffffu), h, l);
                            H[0][j] = __builtin_bit_cast(unsigned int, h);
                            L[0][j] = __builtin_bit_cast(unsigned int, l);
                            split_pair(bf16_bits_to_f32(u0 >> 16), bf16_bits_to_f32(u1 >> 16), h, l);
                            H[1][j] = __builtin_bit_cast(unsigned int, h);
                            L[1][j] = __builtin_bit_cast(unsigned int, l);
                        }
                    }
                    const int q = 2 * rh + qq;
                    const int off0 = img_off(2 * cp + (odd ? 1 : 0), q), off1 = img_off(2 * cp + (odd ? 0 : 1), q);
                    *reinterpret_cast<u32x4*>(hi + off0) = odd ? H[1] : H[0];
                    *reinterpret_cast<u32x4*>(hi + off1) = odd ? H[0] : H[1];
                    if constexpr (TT == kTokBF16) {
                        *reinterpret_cast<u32x4*>(lo + off0) = odd ? L[1] : L[0];
                        *reinterpret_cast<u32x4*>(lo + off1) = odd ? L[0] : L[1];
                    }
                }
                return;
            }
        }
#pragma unroll
        for (int p = 0; p < kTM / 4; ++p) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                csum += stg[4 * p + e];
                v[e] = stg[4 * p + e] * mul;
            }
            half2v h0, l0, h1, l1;
            split_pair(v[0], v[1], h0, l0);
            split_pair(v[2], v[3], h1, l1);
            const int off = img_off(col, p >> 1) + (p & 1) * 4;
            *reinterpret_cast<half4v*>(hi + off) = half4v{h0[0], h0[1], h1[0], h1[1]};
            *reinterpret_cast<half4v*>(lo + off) = half4v{l0[0], l0[1], l1[0], l1[1]};
        }
    };

    const int wn = wave >> 1, wk = wave & 1;
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (s_begin < s_end) {
        fetch(s_begin);
        stage(0);
    }
    __syncthreads();
    for (int step = s_begin; step < s_end; ++step) {
        const int buf = (step - s_begin) & 1;
        const bool more = step + 1 < s_end;
        if (more) fetch(step + 1);
        const _Float16* Ah = lds + buf * kBufHalfs;
        const _Float16* Al = Ah + kImgHalfs;
        const _Float16* Bh = Ah + 2 * kImgHalfs;
        const _Float16* Bl = Ah + 3 * kImgHalfs;       // (fp16 tokens: not built, not read)
#pragma unroll
        for (int s = 0; s < 2; ++s) {              // two 16-row MFMA steps
            const int q = 2 * s + kh;
            half8 ah[2], al[2], bh[4], bl[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = wn * 64 + i * 32 + li;
                ah[i] = *reinterpret_cast<const half8*>(Ah + img_off(c, q));
                al[i] = *reinterpret_cast<const half8*>(Al + img_off(c, q));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = wk * 128 + j * 32 + li;
                bh[j] = *reinterpret_cast<const half8*>(Bh + img_off(c, q));
                if constexpr (TT != kTokF16) bl[j] = *reinterpret_cast<const half8*>(Bl + img_off(c, q));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                    if constexpr (TT != kTokF16) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
        if (more) stage(buf ^ 1);                  // the other buffer was last read in step - 1, closed by that step's barrier
        __syncthreads();
    }

    // outputs: accumulator register r of lane (li, kh) is row n = mfma32_row(r, lane), column k = li of its 32 x 32 block
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (a.part) {
                float* o = a.part + ((int64_t)split * 2 * kCols + slab * kCols + wn * 64 + i * 32) * kCols + wk * 128 + j * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) o[(int64_t)mfma32_row(r, lane) * kCols] = acc[i][j][r] * inv_sc;
                continue;
            }
            float* o = a.dW + (int64_t)(slab * kCols + wn * 64 + i * 32) * a.ldw + wk * 128 + j * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) atomicAdd(o + (int64_t)mfma32_row(r, lane) * a.ldw, acc[i][j][r] * inv_sc);
        }
    if (isA && a.db) {
        if (a.part) a.part[(int64_t)a.nsplit * 2 * kCols * kCols + (int64_t)split * 2 * kCols + slab * kCols + col] = csum;
        else atomicAdd(a.db + slab * kCols + col, csum);
    }
}

// scale[0] = 2^(10 - exponent(max)) from the float bit pattern in bits[0] (1 when the maximum is 0 or not finite)
__global__ void pow2_scale_kernel(const unsigned int* __restrict__ bits, float* __restrict__ scale) {
    const float mx = __uint_as_float(bits[0]);
    int ex = 0;
    if (mx > 0.f && mx < 3.0e38f) frexpf(mx, &ex);
    scale[0] = ldexpf(1.f, 10 - ex);
}

// the row-split launch: in deterministic mode (common.hpp DetScratch) every row range writes its partial block and db slice, summed
// into dW / db in range order behind it (one launch more; the partials of all ranges are 512 x 256 floats each)
template <int TT>
hipError_t launch_split_rows_t(KvBwdArgs a, int64_t M, hipStream_t s) {
    static DynLdsOnce once;
    const size_t ldsb = (size_t)2 * buf_halfs<TT>() * sizeof(_Float16);     // 128 KB (fp16 tokens: 96 KB)
    if (hipError_t e = once.ensure(reinterpret_cast<const void*>(&kvproj_bwd_split_kernel<TT>), ldsb); e != hipSuccess) return e;
    const int steps = (int)((M + kTM - 1) / kTM);
    int nsplit = device_num_cus() / 2;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > steps) nsplit = steps;
    const DetScratch* det = det_scratch();
    const int64_t per = (int64_t)2 * kCols * kCols + 2 * kCols;
    a.part = nullptr;
    if (det) {
        if (det->floats / per < nsplit) nsplit = (int)(det->floats / per);
        if (nsplit < 1) return hipErrorInvalidValue;
        a.part = det->base;
    }
    a.nsplit = nsplit;
    hipLaunchKernelGGL(kvproj_bwd_split_kernel<TT>, dim3(2 * nsplit), dim3(512), ldsb, s, a);
    if (!det) return hipGetLastError();
    hipError_t e = launch_slab_reduce(a.part, nsplit, (int64_t)2 * kCols * kCols, 2 * kCols, kCols, a.dW, a.ldw, 1, s);
    if (e != hipSuccess || !a.db) return e;
    return launch_slab_reduce(a.part + (int64_t)nsplit * 2 * kCols * kCols, nsplit, 2 * kCols, 1, 2 * kCols, a.db, 0, 1, s);
}

// x_type: element type of a.x.  16-bit rows are read as 4-byte words of two channels: base and row stride must allow that
hipError_t launch_split_rows(KvBwdArgs a, int64_t M, int x_type, const unsigned int* absmax_bits, float* scale_scratch, hipStream_t s) {
    if (x_type != kTokF32 && x_type != kTokF16 && x_type != kTokBF16) return hipErrorInvalidValue;
    if (x_type != kTokF32 && ((reinterpret_cast<uintptr_t>(a.x) & 3) != 0 || (a.ldx & 1) != 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pow2_scale_kernel, dim3(1), dim3(1), 0, s, absmax_bits, scale_scratch);
    if (x_type == kTokF16) return launch_split_rows_t<kTokF16>(a, M, s);
    if (x_type == kTokBF16) return launch_split_rows_t<kTokBF16>(a, M, s);
    return launch_split_rows_t<kTokF32>(a, M, s);
}

}  // namespace

bool kvproj_bwd_split_supported(int C) { return C == kCols; }
int64_t det_kvbwd_floats() {
    const int n = device_num_cus() / 2;
    return (int64_t)(n < 1 ? 1 : n) * (2 * kCols * kCols + 2 * kCols);
}

// g [M][2C], tokens [M][C] -> dW [2C][C] (+=), db [2C] (+=).  absmax_bits: device word holding the bit pattern of max |g|
// (non-negative floats order like unsigned integers); scale_scratch: one device float.
// The same contraction for any [M][512-column slice] operand: out[n][k] += sum_m g[m][n] x[m][k], n < 512, k < 256; g rows ldg apart
// (the head-dim-256 attention backward forms dQ^T slices this way: g = dS^T, x = K).  db may be null.  x_type: element type of x
// (kTokF32 / kTokF16 / kTokBF16; ldx in elements).
hipError_t launch_tn_split_512x256(const float* g, int64_t ldg, const void* x, int64_t ldx, int64_t M, float* out, int64_t ldo,
                                   float* db, const unsigned int* absmax_bits, float* scale_scratch, hipStream_t s, int x_type) {
    if (M < 1 || M > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    KvBwdArgs a;
    a.g = g; a.ldg = ldg; a.x = x; a.ldx = ldx; a.dW = out; a.ldw = ldo; a.db = db; a.scale = scale_scratch; a.M = (int)M;
    return launch_split_rows(a, M, x_type, absmax_bits, scale_scratch, s);
}

hipError_t launch_kvproj_bwd_split(const float* g, const void* tokens, int64_t M, int C, float* dW, float* db,
                                   const unsigned int* absmax_bits, float* scale_scratch, hipStream_t s, int tok_type) {
    if (C != kCols || M < 1 || M > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    KvBwdArgs a;
    a.g = g; a.ldg = 2 * C; a.x = tokens; a.ldx = C; a.dW = dW; a.ldw = C; a.db = db; a.scale = scale_scratch; a.M = (int)M;
    return launch_split_rows(a, M, tok_type, absmax_bits, scale_scratch, s);
}

}  // namespace parq
