// Shared declarations of the gfx950 kernel chain behind libparq_hip.so.
// Everything here targets CDNA4 (wave64; v_mfma_f32_32x32x16_f16 split products and fp32 MFMA) directly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "kv_layout.hpp"      // mfma32_row and the K/V cache layouts: block / stage geometry, index maps, swizzles

namespace parq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Development knobs (A/B switches, kernels with ingredients removed) are read from the environment ONLY in the development build
// (-DPARQ_DEV_PROBES -> parq_amd/_C/libparq_hip_dev.so, loaded by tools/ through PARQ_HIP_LIB).  The product library never calls
// getenv: every knob takes its default and the probe instantiations (wrong results by construction) are not compiled in.
#ifdef PARQ_DEV_PROBES
inline const char* dev_env(const char* name) { return getenv(name); }
#else
inline const char* dev_env(const char*) { return nullptr; }
#endif

// ---- in-kernel time stamps (development build only): where a launch spends its time between two kernel boundaries.
// Wave 0 of every workgroup of an instrumented kernel appends {kernel id | grid size | XCD, linear block index, start, end} to a
// device buffer (parq_dev_timeline); stamps are s_memrealtime (100 MHz, chip-wide), `end` is taken after the wave's own stores
// have been acknowledged.  tools/iter_timeline_stamps.py turns the records into a per-launch table (first / last workgroup start,
// last end, gap to the previous launch's last end = the dependent-dispatch boundary).
enum : int { kTlLinear = 1, kTlProjectSample = 2, kTlSelfAttn = 3, kTlFlashSplit = 4, kTlFlashMerge = 5, kTlBoxDecode = 6, kTlPosemb = 7,
             kTlKvProj = 8, kTlChain = 9 };
#ifdef PARQ_DEV_PROBES
static __device__ unsigned long long* parq_tl_buf = nullptr;      // one copy per translation unit (no relocatable device code)
static __device__ unsigned int parq_tl_cap = 0;
struct TlStamp {
    unsigned long long t0, idx; int id;
    unsigned long long ph = 0ull; int nph = 0;        // up to four phase marks inside the kernel: 11-bit offsets from t0 in 10 ns ticks
    __device__ __forceinline__ void mark() {
        if (threadIdx.x == 0 && parq_tl_buf) {
            __builtin_amdgcn_sched_barrier(0);
            unsigned long long d = wall_clock64() - t0;
            d = d > 2047ull ? 2047ull : d;
            ph |= d << (11 * nph);
            ++nph;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the record slot is claimed at the START (the atomic's round trip overlaps the kernel); the end costs one wait for the wave's
    // own stores and four fire-and-forget stores
    __device__ __forceinline__ TlStamp(int id_) : id(id_) {
        t0 = 0ull; idx = ~0ull;
        if (threadIdx.x == 0 && parq_tl_buf) { t0 = wall_clock64(); idx = atomicAdd(parq_tl_buf, 1ull); }
    }
    __device__ __forceinline__ ~TlStamp() {
        if (threadIdx.x == 0 && parq_tl_buf) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned long long t1 = wall_clock64();
            if (idx < parq_tl_cap) {
                unsigned long long* r = parq_tl_buf + 4 + idx * 4;
                const unsigned long long nblk = (unsigned long long)gridDim.x * gridDim.y * gridDim.z;
                const unsigned long long xcc = __builtin_amdgcn_s_getreg(6164) & 15u;     // HW_REG_XCC_ID
                r[0] = (unsigned long long)id | (nblk << 8) | (xcc << 40);
                r[1] = (blockIdx.x + (unsigned long long)gridDim.x * (blockIdx.y + (unsigned long long)gridDim.y * blockIdx.z)) | (ph << 20);   // (block index < 2^20 wherever marks are used)
                r[2] = t0; r[3] = t1;
            }
        }
    }
};
#define PARQ_TL_KERNEL(id) ::parq::TlStamp parq_tl_stamp_(id)
// phase marks cost a pointer load and a branch each even with the timeline off: only in builds that ask for them
// (PARQ_DEV_EXTRA_FLAGS=-DPARQ_TL_MARKS python -c 'import __graft_entry__ as g; g.build_dev()'; tools/r06_h3_phases.py)
#ifdef PARQ_TL_MARKS
#define PARQ_TL_MARK() parq_tl_stamp_.mark()
#else
#define PARQ_TL_MARK() do { } while (0)
#endif
// each instrumented translation unit defines its setter with this macro; api.hip calls them all from parq_dev_timeline()
#define PARQ_TL_DEFINE_SETTER(fn)                                                                              \
    hipError_t fn(unsigned long long* buf, unsigned int cap) {                                                 \
        hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(parq_tl_buf), &buf, sizeof(buf));                          \
        if (e != hipSuccess) return e;                                                                         \
        return hipMemcpyToSymbol(HIP_SYMBOL(parq_tl_cap), &cap, sizeof(cap));                                  \
    }
hipError_t tl_set_linear(unsigned long long*, unsigned int);
hipError_t tl_set_elementwise(unsigned long long*, unsigned int);
hipError_t tl_set_flash(unsigned long long*, unsigned int);
hipError_t tl_set_flash_split(unsigned long long*, unsigned int);
hipError_t tl_set_flash_split8(unsigned long long*, unsigned int);
hipError_t tl_set_kvproj_split(unsigned long long*, unsigned int);
hipError_t tl_set_chain(unsigned long long*, unsigned int);
#else
#define PARQ_TL_KERNEL(id) do { } while (0)
#define PARQ_TL_MARK() do { } while (0)
#define PARQ_TL_DEFINE_SETTER(fn)
#endif

constexpr int kWave = 64;
// GroupNorm moment slots per (scene, group).  Producers either OWN a slot (chain.hip: sub-tile (row block, column block) of a
// 256-query x 256-channel block -> slot 16 rb + cb, a plain store: no atomic round trip at the end of the launch, and a summation
// order that does not depend on arrival) or add into slot (tile % kGnSlots) with fp64 atomics (generic kernel; slots zeroed by the
// iteration's first kernel).  Consumers sum all slots: 4 per lane and one shuffle tree.
constexpr int kGnSlots = 256;
// a consumer lane's share of the slots of one (scene, group): slots lane, lane + 64, ... in that order (src points at slot `lane`).
// Batch-invariant inference sizes the slots per launch (LinearArgs::gn_slots); the default count keeps its unrolled form.
__device__ __forceinline__ void gn_lane_sums(const double* __restrict__ src, int slots, double& sm, double& sq) {
    if (slots == kGnSlots) {
#pragma unroll
        for (int i = 0; i < kGnSlots / 64; ++i) { sm += src[i * 128]; sq += src[i * 128 + 1]; }
    } else {
        // four slots' loads in flight at a time; the additions keep the slot order
        const int n = slots / 64;
        int i = 0;
        for (; i + 4 <= n; i += 4) {
            double m[4], q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { m[j] = src[(i + j) * 128]; q[j] = src[(i + j) * 128 + 1]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) { sm += m[j]; sq += q[j]; }
        }
        for (; i < n; ++i) { sm += src[i * 128]; sq += src[i * 128 + 1]; }
    }
}
// the shared slot of a producer without a slot of its own (default geometry only): index mod slots, the default count as a constant
__device__ __forceinline__ int gn_shared_slot(unsigned idx, int slots) {
    return slots == kGnSlots ? (int)(idx % (unsigned)kGnSlots) : (int)(idx % (unsigned)slots);
}

// LDS-DMA (global_load_lds, 16 bytes per lane, wave-uniform LDS base + lane * 16) issued through inline asm.  hipcc knows that the
// builtin writes LDS asynchronously and answers with s_waitcnt vmcnt(0) in front of later C++ reads of LDS it cannot prove
// disjoint — which turns a prefetch into a blocking load.  Through asm the compiler does not see it: the caller waits with a
// counted s_waitcnt vmcnt(N) + a barrier before anybody reads the destination.
// M0 (the LDS base of the instruction) is saved and restored inside the statement: hipcc does not honour an "m0" clobber, and it may
// keep its own value there (indexed register access, its own LDS-DMA builtins).
__device__ __forceinline__ void lds_dma16(const void* gsrc, unsigned lds_base) {
    const unsigned base = __builtin_amdgcn_readfirstlane(lds_base);
    unsigned saved;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(saved)
                 : "s"(base), "v"(gsrc)
                 : "memory");
}
// workgroup barrier that only orders LDS traffic: __syncthreads() is a release / acquire fence and makes hipcc wait for every
// outstanding global store and load (s_waitcnt vmcnt(0)) first
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Cross-half reductions of the attention kernels (a query's 32 scores of a block sit in lanes l and l + 32).
// v_permlane32_swap exchanges lanes 32..63 of its first operand with lanes 0..31 of its second: fed the same value twice, the first
// comes back as the low half broadcast to both halves and the second as the high half.  Written as inline asm: with hipcc of
// ROCm 7.2 the SECOND result of __builtin_amdgcn_permlane32_swap is mis-assigned to the first result's register ("r[0] + r[1]"
// compiled to v0 + v0 even for unrelated inputs: the row sums came out doubled).  s_nop: VALU write -> permlane read hazard.
__device__ __forceinline__ void xhalf_swap(float v, float& lo_bcast, float& hi_bcast) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    lo_bcast = a;
    hi_bcast = b;
}
__device__ __forceinline__ float xhalf_max(float v) {       // max over the two 32-lane halves, result in every lane
    float a, b, o;
    xhalf_swap(v, a, b);
    asm("v_max_f32 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b));
    return o;
}
__device__ __forceinline__ float xhalf_sum(float v) {
    float a, b;
    xhalf_swap(v, a, b);
    return a + b;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: a process that drives several GPUs must set
// it on each of them.  One static instance per kernel; bit d of `done` = already set on device ordinal d.
struct DynLdsOnce {
    unsigned long long done = 0;
    hipError_t ensure(const void* fn, size_t bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const bool track = dev >= 0 && dev < 64;
        if (track && ((done >> dev) & 1ull)) return hipSuccess;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess && track) done |= 1ull << dev;
        return e;
    }
};

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ fp32 -> (hi, lo) fp16 split
// x ~= hi + lo with hi = fp16(x) and lo = fp16(x - hi).  `hi` MUST be the value the residual is
// taken against: hipcc is free to materialise `(_Float16)x` twice (v_cvt_f16_f32 for the residual,
// v_cvt_pk_f16_f32 for the packed MFMA operand) and on gfx950 the two disagree on exact ties, which
// silently costs a full fp16 ulp (2^-11 relative).  Going through the packed round-toward-zero
// builtin pins one conversion; the residual is derived from ITS result.
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_pair(float x0, float x1, half2v& hi, half2v& lo) {
    const auto h = __builtin_amdgcn_cvt_pkrtz(x0, x1);
    hi = __builtin_bit_cast(half2v, h);
    // x - hi as v_fma_mix_f32(hi (fp16 half of the packed register), -1.0, x): one instruction per element instead of cvt + sub
    // (hipcc only forms the mixed fma when a multiply feeds the subtraction); the difference is exact either way
    float d0, d1;
    const unsigned int hp = __builtin_bit_cast(unsigned int, h);
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(hp), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d1) : "v"(hp), "v"(x1));
    lo = __builtin_bit_cast(half2v, __builtin_amdgcn_cvt_pkrtz(d0, d1));
}

__device__ __forceinline__ void split8(const float* x, half8& hi, half8& lo) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        half2v h, l;
        split_pair(x[e], x[e + 1], h, l);
        hi[e] = h[0]; hi[e + 1] = h[1];
        lo[e] = l[0]; lo[e + 1] = l[1];
    }
}

// ---- fp8 (OCP e4m3) operand forms of the MX cross terms (flash_split8.hip, the K/V projection's mode-4 epilogue)
template <bool CLAMP = true>
__device__ __forceinline__ float clamp_e4m3(float x) { return CLAMP ? __builtin_amdgcn_fmed3f(x, -448.f, 448.f) : x; }
// e4m3 of four floats, byte i = x[i]; values past +-448 saturate (v_cvt_pk_fp8_f32 itself returns NaN beyond its rounding range).
// CLAMP = false is for callers that know all four inside +-448 (the K/V projection decides that once per block): the same bytes
template <bool CLAMP = true>
__device__ __forceinline__ int pack4_e4m3(float a, float b, float c, float d) {
    const int w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_e4m3<CLAMP>(a), clamp_e4m3<CLAMP>(b), 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(clamp_e4m3<CLAMP>(c), clamp_e4m3<CLAMP>(d), w, true);
}
// x0, x1 -> packed hi16 (round toward zero: the value split_pair takes its residual against) and the fp32 residuals x - hi (exact)
__device__ __forceinline__ void split_rtz(float x0, float x1, unsigned& hi, float& d0, float& d1) {
    hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x0, x1));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(hi), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d1) : "v"(hi), "v"(x1));
}
constexpr float kLo8Scale = 1024.f;          // lo parts of K, V, Q enter e4m3 as lo * 2^10 (|lo| < 2^-10 |x|); E8M0 scale 117 undoes it
typedef int i32x4 __attribute__((ext_vector_type(4)));
// 16 floats -> 16 bytes e4m3(x) and 16 bytes e4m3((x - hi16(x)) * 2^10), byte i = x[i].  (|x - hi16(x)| 2^10 < max(2^floor(log2 |x|), 2^-14)
// — hi16 rounds toward zero — so CLAMP = false needs |x| <= 448 only)
template <bool CLAMP = true>
__device__ __forceinline__ void pieces_e4m3(const float* x, i32x4& hi8, i32x4& lo8) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        unsigned h0, h1;
        float d[4];
        split_rtz(x[4 * w], x[4 * w + 1], h0, d[0], d[1]);
        split_rtz(x[4 * w + 2], x[4 * w + 3], h1, d[2], d[3]);
        hi8[w] = pack4_e4m3<CLAMP>(x[4 * w], x[4 * w + 1], x[4 * w + 2], x[4 * w + 3]);
        lo8[w] = pack4_e4m3<CLAMP>(d[0] * kLo8Scale, d[1] * kLo8Scale, d[2] * kLo8Scale, d[3] * kLo8Scale);
    }
}

// ---- dropout (training): counter-based keep decision, identical in forward and backward.  Element (row, col) of stream `seed`
// is kept when a 24-bit hash is >= p * 2^24; kept values are scaled by 1 / (1 - p) (torch.nn.Dropout semantics).
__host__ __device__ constexpr uint32_t rng_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// The chained hash of the matcher's keys (setmatch.hip) and of the ground-truth jitter (tracks.hip): h = 0x9e3779b9, then one
// hash_absorb per 32-bit word.  tests/set_match_cases.py mix32 is rng_mix.
__host__ __device__ constexpr uint32_t hash_absorb(uint32_t h, uint32_t w) { return rng_mix((h ^ w) + 0x9e3779b9U); }
__host__ __device__ inline uint32_t rng_stream(uint32_t base, uint32_t stream) { return rng_mix(base ^ rng_mix(stream * 0x9e3779b9U + 0x85ebca6bU)); }
// The index space of a dropout site is 2-D, (row, col): activations (m, n); attention probabilities (bh * Lq + q, key).  The row
// part of the hash is computed once per row (per lane in the forward attention kernels, per query tile in the backward ones),
// the column part once per column where a kernel can share it (below).
__host__ __device__ inline uint32_t drop_rowhash(uint32_t seed, uint32_t row) { return rng_mix(seed ^ (row * 0x9e3779b1U)); }
// keep(row, col) = mix(rowhash(seed, row) ^ colhash(col)) >= ceil(p * 2^24) * 256: the column part does not depend on the seed, so
// the attention kernels hash a key ONCE (per stage in the forward, per lane in the backward, where a lane owns a key) and spend
// xor + 24-bit multiply + shift-xor + 24-bit multiply + compare per element.  The final mix matters: comparing the bare xor against a threshold makes the
// dropped set of a row the preimage of `rowhash ^ [0, thr)`, whose large dyadic sub-blocks depend only on the top bits of the
// row hash — 1/16 of all row pairs then share >60 % of their dropped columns at p = 0.1 (a 4-wise xor dependence that uniformity
// and pairwise independence do not show).  multiply / shift-xor / multiply after the xor breaks that linearity: over all pairs of
// 512 rows the worst shared-drop fraction is 0.171 - 0.176 at p = 0.1 (a full 32-bit finaliser gives 0.178; one multiply + shift-xor
// still leaves 0.20-0.23 against the 6-sigma bound 0.196).  tests/test_host_cpu.py simulates the hash in NumPy,
// tests/test_gpu_kernels.py::test_dropout_masks_of_row_pairs_overlap_like_independent_draws checks the masks the kernels use.
// Column hash = hash of the 32-column block ^ one of 16 constants chosen by bits 0, 1, 3, 4 of the column ^ a constant where bit 2
// is set.  In the attention kernels a lane's 16 accumulator registers of a 32-key block are the columns (r & 3) + 8 (r >> 2) + 4 kh
// (kh = lane >> 5): the block part is wave-uniform (scalar unit), the kh part folds into the lane's row hash once, and the register
// part is a literal operand of the xor in drop_keep_h — no per-key hashing, no table in LDS, no registers (the forward kernel
// used to hash 32 keys per block, park them in LDS and read 16 back: two dependent LDS round trips at the head of every step,
// +32 % on the training forward).  The fixed xor offsets between the columns of a block are decorrelated by the two multiplies
// of drop_keep_h like the row offsets: co-drop frequency of every in-block column pair within 1.7 % of p^2 over 6 M samples.
__host__ __device__ constexpr uint32_t drop_blockhash(uint32_t blk) { return rng_mix(blk * 0x85ebca77U + 0x6a09e667U); }
__host__ __device__ constexpr uint32_t drop_regpart(uint32_t r) { return rng_mix(0x3c6ef372U + r); }       // r = 0 .. 15
constexpr uint32_t kDropBit2Part = rng_mix(0xa54ff53aU);
__host__ __device__ constexpr uint32_t drop_colhash(uint32_t col) {
    const uint32_t k = col & 31u;
    return drop_blockhash(col >> 5) ^ drop_regpart((k & 3u) | ((k >> 3) << 2)) ^ ((k & 4u) ? kDropBit2Part : 0u);
}
// threshold in the scale of the full 32-bit hash: (h >> 8) >= ceil(p 2^24)  <=>  h >= ceil(p 2^24) * 256 (saturated: p ~ 1 keeps nothing
// but h = 2^32 - 1)
__host__ __device__ inline uint32_t drop_threshold(float p) {
    const float t = ceilf(p * 16777216.0f);
    return t >= 16777216.0f ? 0xffffffffU : ((uint32_t)t << 8);
}
// Both multiplies are 24 x 24-bit (v_mul_u32_u24, full rate; the 32-bit v_mul_lo_u32 is a quarter-rate instruction and two of them per
// probability were ~2/3 of the mask's issue time in the attention kernels): the low 24 bits of the xor of two full 32-bit hashes,
// times a 24-bit odd constant, shift-xor, low 24 bits times a second constant; the compared top bits depend on every one of the 24
// bits.  Same statistics as the 32-bit form in the simulation of tests/test_host_cpu.py (worst shared-drop fraction over all pairs of
// 512 rows 0.171 - 0.176 for three seeds, 32-bit form 0.175).
__host__ __device__ inline bool drop_keep_h(uint32_t rowhash, uint32_t colhash, uint32_t thr) {
    uint32_t h = ((rowhash ^ colhash) & 0xffffffU) * 0x9E3779U;
    h ^= h >> 16;
    h = (h & 0xffffffU) * 0x85EBCBU;
    return h >= thr;
}
__host__ __device__ inline bool drop_keep(uint32_t rowhash, uint32_t col, float p) {
    return drop_keep_h(rowhash, drop_colhash(col), drop_threshold(p));
}

// 16-bit operand kinds of the matrix pipe.  A half8 is used as the raw 8 x 16-bit container for both.
enum : int { kF16 = 0, kBF16 = 1 };
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// round-to-nearest conversion of 8 floats (the single-term "half" attention modes)
template <int KIND>
__device__ __forceinline__ half8 cvt8_rn(const float* x) {
    if constexpr (KIND == kF16) {
        half8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (_Float16)x[e];
        return h;
    } else {
        bf16x8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (__bf16)x[e];
        return __builtin_bit_cast(half8, h);
    }
}

// ---- element type of the memory tokens (parq_set_token_type): fp32, or 16-bit rows widened to fp32 in registers.  Both 16-bit
// formats are subsets of fp32, so the widening is exact (NaN and infinities included) and everything after it is the fp32-token
// kernel's arithmetic unchanged.
enum : int { kTokF32 = 0, kTokF16 = 1, kTokBF16 = 2 };
template <int TT> struct TokElem { typedef float type; };
template <> struct TokElem<kTokF16> { typedef _Float16 type; };
template <> struct TokElem<kTokBF16> { typedef unsigned short type; };       // raw bf16 bits
template <int TT> constexpr int tok_bytes() { return TT == kTokF32 ? 4 : 2; }

__device__ __forceinline__ float bf16_bits_to_f32(unsigned int b) { return __builtin_bit_cast(float, b << 16); }

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// two fp32 -> two 16-bit tokens of type TT (kTokF16 / kTokBF16) packed low | high, each rounded to nearest even as torch.Tensor.to
// does, NaN stays NaN: the packed conversions v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32.  fp16 goes through inline asm because a lone
// (_Float16) cast compiles to v_cvt_f16_f32, which on gfx950 rounds some exact ties the other way (see split_pair above).
template <int TT>
__device__ __forceinline__ unsigned int round2_tok16(float y0, float y1) {
    static_assert(TT != kTokF32, "16-bit token types only");
    if constexpr (TT == kTokF16) {
        unsigned int r;
        asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(y0), "v"(y1));
        return r;
    } else {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 v = {(__bf16)y0, (__bf16)y1};
        return __builtin_bit_cast(unsigned int, v);
    }
}
// 8 consecutive 16-bit tokens (one 16-byte piece) -> fp32
template <int TT>
__device__ __forceinline__ void widen8(u32x4 raw, float* x) {
    static_assert(TT != kTokF32, "16-bit token types only");
    const unsigned int w[4] = {raw[0], raw[1], raw[2], raw[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (TT == kTokF16) {
            const half2v h = __builtin_bit_cast(half2v, w[i]);
            x[2 * i] = (float)h[0];
            x[2 * i + 1] = (float)h[1];
        } else {
            x[2 * i] = bf16_bits_to_f32(w[i] & 0xffffu);
            x[2 * i + 1] = bf16_bits_to_f32(w[i] >> 16);
        }
    }
}

// 4 consecutive tokens at element offset 4 * c4 of `row` -> fp32 (one 16-byte or 8-byte load)
template <int TT>
__device__ __forceinline__ f32x4 load_tok4(const void* row, int c4) {
    if constexpr (TT == kTokF32) {
        return reinterpret_cast<const f32x4*>(row)[c4];
    } else {
        const uint2 r = reinterpret_cast<const uint2*>(row)[c4];
        if constexpr (TT == kTokF16) {
            const half2v a = __builtin_bit_cast(half2v, r.x), b = __builtin_bit_cast(half2v, r.y);
            return f32x4{(float)a[0], (float)a[1], (float)b[0], (float)b[1]};
        } else {
            return f32x4{bf16_bits_to_f32(r.x & 0xffffu), bf16_bits_to_f32(r.x >> 16), bf16_bits_to_f32(r.y & 0xffffu),
                         bf16_bits_to_f32(r.y >> 16)};
        }
    }
}

// one token at element index i of `base` -> fp32
template <int TT>
__device__ __forceinline__ float load_tok(const void* base, int64_t i) {
    if constexpr (TT == kTokF32) return reinterpret_cast<const float*>(base)[i];
    else if constexpr (TT == kTokF16) return (float)reinterpret_cast<const _Float16*>(base)[i];
    else return bf16_bits_to_f32(reinterpret_cast<const unsigned short*>(base)[i]);
}

template <int KIND>
__device__ __forceinline__ f32x16 mfma16(half8 a, half8 b, f32x16 c) {
    if constexpr (KIND == kF16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ------------------------------------------------------------------ linear (small GEMM)
struct LinearArgs {
    const float* X;  int64_t ldx;       // A operand, row-major [M][K] with row stride ldx
    const float* X2; int64_t ldx2;      // optional addend on A (e.g. + pos_feat) ...
    int x2_ncols;                       // ... applied only to output columns < x2_ncols (tile granular)
    const float* W;  int64_t ldw;       // [N][K] row-major (torch Linear / Conv1d(k=1) weight)
    const float* bias;                  // [N] or nullptr
    const float* R;  int64_t ldr;       // residual [M][N] or nullptr
    float* Y;
    int M, N, K;
    int relu;
    const float* relu_mask; int64_t ldmask;   // backward of a ReLU: y = relu_mask[m][n] > 0 ? y * mask_scale : 0 (applied after bias)
    float mask_scale;                         // 0 is read as 1
    // training dropout on the output, after bias / ReLU and before the residual: element (m, n) of stream drop_seed
    float drop_p; uint32_t drop_seed;
    // output address: Y + (m / rows_per_batch) * y_batch + (m % rows_per_batch) * y_row
    //                   + (n / col_blk) * y_blk + (n % col_blk)
    int rows_per_batch; int64_t y_batch; int64_t y_row; int col_blk; int64_t y_blk;
    float norm_eps;                     // eps of the fused LayerNorm / GroupNorm
    // LayerNorm applied to the rows of A on load (statistics over the full K computed by the tile):
    //   a' = (a - mean_m) * rstd_m * ln_gamma[k] + ln_beta[k]   (then + X2 if given)
    // ln_stats_out[m] = (mean, rstd) is published by the first column tile for later residual use.
    const float* ln_gamma; const float* ln_beta; float* ln_stats_out;
    // residual taken as LayerNorm(R) recomputed from published row statistics:
    //   r' = (R[m][n] - mean_m) * rstd_m * rln_gamma[n] + rln_beta[n]
    const float* rln_stats; const float* rln_gamma; const float* rln_beta;
    // GroupNorm(1 group over rows_per_scene x K) + ReLU applied to A on load, from the scene-wide
    // moments (sum, sum of squares; fp64) the producer accumulated:
    //   a' = relu((a - mean) * rstd * gamma[k] + beta[k]),  (S, Q) = gn_sums[scene][group]
    const double* gn_sums; const float* gn_gamma; const float* gn_beta;
    int gn_rows_per_scene; int gn_ngroups;
    // moments of the OUTPUT (columns < gn_out_ncols) accumulated with fp64 atomics into
    // gn_out_sums[scene][(n + g*N) / gn_out_group_cols][gn_slots][2] (zeroed by an earlier kernel)
    double* gn_out_sums; int gn_out_ncols; int gn_out_group_cols; int gn_out_rows_per_scene; int gn_out_ngroups;
    // grouped launch: blockIdx.y = g adds these element offsets
    int64_t gX, gW, gBias, gY, gGamma;
    // chain.hip only: a SECOND operand pair accumulated into the same output, Y += X2 @ W2^T, for output columns < x2_ncols (the
    // position MLP's last layer folded into its consumers: (x + h W2^T + b2) W^T = x W^T + h (W W2)^T + W b2).  X2 / ldx2 above is then
    // the second A operand (K columns) instead of an addend; W2 is [N][K] row-major with row stride ldw, W2p its tile-ordered copy.
    const float* W2; const float* W2p;
    // chain.hip only: the same matrix in tile order (launch_pack_w_tiles): block (n / 16, k / 16) = 1 KB holding element (n % 16,
    // k % 16) at float ((k % 16) / 4 * 16 + n % 16) * 4 + k % 4, i.e. one wave-wide float4 load = one contiguous KB.  nullptr: read W.
    const float* Wp;
    // chain.hip only: the same matrix as fp16 hi / lo pairs in MFMA-fragment order with one power-of-two scale per output column
    // (pack_w_half_kernel; element offsets as W's) and wh_scale[n] = the inverse scale.  nullptr: the fp32 kernels.
    const float* Wh; const float* wh_scale;
    // LayerNorm folds of that mirror (pack_w_half_kernel): wh_fold 1 = gamma inside Wh and W beta inside wh_bias, 2 = W beta inside wh_bias only
    const float* wh_bias; int wh_fold;
    int tile_map;                       // chain.hip only: 1 = the workgroups of a row block run on one XCD (set by launch_chain_linear)
    // chain.hip only — LayerNorm seams inside one launch (seam_tile): a launch that produces rows x which a LayerNorm normalises
    // publishes, per (row, workgroup tile of 64 columns), the fp64 partial sums (sum x, sum x^2): lnp_out[row][N / 64][2]
    double* lnp_out;
    // IN-LAUNCH publication of lnp_out (chain.hip seam kernels): the partials are stored write-through (sc1) and flag
    // lnp_flags[row block][tile] = lnp_epoch follows once they are acknowledged; consumers are workgroups of the SAME launch with
    // larger block indices (seam_tile)
    unsigned* lnp_flags; unsigned lnp_epoch;
    // Early completion signal of a forward (api.hip: set on the first launch behind the LAST iteration's cross-attention merge — no
    // kernel of the forward can raise a flag after it): thread 0 of workgroup (0, 0) copies what the forward has raised into the caller's
    // host-visible mirror word (the bits of BoxDecodeArgs::poison_mirror) and then stores this call's epoch (left in the workspace by the
    // call's prologue launch) into the host-visible progress word, so that a host that only needs to know WHETHER the forward has to
    // be re-run can stop waiting one chain tail (~36 us at BASELINE cfg 3) before the forward ends.  nullptr: nothing to publish.
    const int* pub_flags; int* pub_mirror; int* pub_word; const int* pub_epoch; int pub_mask; int pub_peaky;
    // Batch-invariant inference (parq_set_batch_invariant): the launchers choose kernel, tile shape and sub-tile count from geom_M rows
    // — ONE scene's — instead of M (0: from M), so that a scene's rows meet the same kernel whatever shares the call.
    int geom_M;
    // slots per (scene, group) of gn_sums / gn_out_sums (a multiple of 64; launch_linear reads 0 as kGnSlots).  The mode sizes them so
    // that every 16 x 16 sub-tile of a (scene, group) block owns one: plain stores, summed by the consumers in slot order.
    int gn_slots;
    // generic kernel (linear.hip) only: 1 = a tile stores its moments into the slot of its own coordinates inside the scene's block
    // instead of adding into slot (tile index % slots) with atomics (the caller sized gn_slots for it and the tiles lie inside scenes)
    int gn_own;
};
__device__ __forceinline__ void publish_progress(const LinearArgs& a) {
    if (a.pub_word != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        const int f0 = a.pub_flags[0] & a.pub_mask, pk = a.pub_peaky ? a.pub_flags[1] : 0;
        const int bits = ((f0 & ~4) ? 1 : 0) | (f0 & 4) | (pk != 0 ? (2 | (pk << 8)) : 0);
        if (bits != 0 && a.pub_mirror != nullptr) __hip_atomic_fetch_or(a.pub_mirror, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.pub_word, *a.pub_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // behind the mirror bits
    }
}
// A consumer tile of a LayerNorm seam inside ONE launch (chain.hip seam_tile).  The LayerNorm is pushed through the linear map behind it,
//   LN(x) W^T + b = rstd (x Wg^T - mean s) + b',   Wg = W diag(gamma), s = row sums of Wg, b' = b + W beta,
// and x Wg^T is computed from the operands x itself is made of (x = r + y Wo^T + bo  ->  x Wg^T = r Wg^T + y (Wg Wo)^T + Wg bo), so
// the tile's contraction does not wait for x; only its epilogue needs (mean, rstd), which it takes from the fp64 partial row sums the
// x tiles of the same launch publish.  out = act(rstd (acc1 + b1 - mean s) + acc2 + b2):
//   acc1 = X1' W1^T + X2 W2^T   (X1' = X1, or LayerNorm(X1) with GIVEN statistics ln1_stats and gamma / beta ln1_g / ln1_b)
//   acc2 = X3 W3^T              (optional: a part the LayerNorm does not scale)
struct SeamArgs {
    const float* X1; int64_t ldx1; const float* W1p;          // tile-ordered weights (launch_pack_w_tiles), [N][K1]
    const float* X2; int64_t ldx2; const float* W2p;          // [N][K2]
    const float* X3; int64_t ldx3; const float* W3p;          // [N][K3] or nullptr
    const float* ln1_stats; const float* ln1_g; const float* ln1_b;
    const float* b1; const float* srow; const float* b2;      // [N] each (b2 may be nullptr)
    float* Y; int64_t ldy; int M, N;
    const double* part; const unsigned* flags; unsigned epoch; int nparts; int width;   // the producer's partials / flags (nparts <= 4 per row)
    float eps;
    float* ln_out;                                             // optional [M][2]: (mean, rstd) of x published for later launches
    double* gn_out_sums; int gn_out_ncols; int gn_out_group_cols; int gn_out_rows_per_scene; int gn_out_ngroups;   // as LinearArgs
    int* err;                                                  // raised (bit 2) if a flag never arrives: outputs are then NaN
};
hipError_t launch_linear(const LinearArgs& a, int groups, hipStream_t s);
// chain.hip: compile-time specialised kernels for the launches of one decoder iteration; hipErrorNotSupported = no instantiation
// matches this launch (launch_linear then uses the generic kernel)
hipError_t launch_chain_linear(const LinearArgs& a, int groups, hipStream_t s);
bool chain_linear_supported(const LinearArgs& a, int groups);      // would launch_chain_linear take this launch?
// chain.hip: two stages that a LayerNorm separates as ONE launch (SeamArgs below; seam_tile); hipErrorNotSupported = shapes do not fit
hipError_t launch_seam_q(const LinearArgs& xa, const SeamArgs& q, hipStream_t s);
// pack time: Wg = W diag(gamma), srow = row sums of Wg, bb = b + W beta | out = A Bm, ob = A bv  (float64 accumulation)
hipError_t launch_ln_fold(const float* W, const float* b, const float* gamma, const float* beta, int R, int C, float* Wg, float* srow, float* bb, hipStream_t s);
hipError_t launch_matmul_fold(const float* A, const float* Bm, const float* bv, int R, int C, float* out, float* ob, hipStream_t s);
hipError_t launch_pack_w_half(const float* W, int64_t ldw, int N, int K, float* dst, float* scales, hipStream_t s, const float* gamma = nullptr,
                              const float* beta = nullptr, const float* bias = nullptr, float* bias_out = nullptr);
hipError_t launch_pack_w_tiles(const float* W, int64_t ldw, int N, int K, float* dst, hipStream_t s);   // N % 16 == K % 16 == 0
// pack time: out_w[r][k] = sum_j Wa[r][j] W2[j][k], out_b[r] = ba[r] + sum_j Wa[r][j] b2[j]  (float64 accumulation), r < R; Wa [R][C], W2 [C][C]
hipError_t launch_fold_pos_weights(const float* Wa, const float* ba, const float* W2, const float* b2, int R, int C, float* out_w, float* out_b, hipStream_t s);

// ------------------------------------------------------------------ attention
struct FlashArgs {
    const float* q; int64_t q_batch, q_head, q_row;     // element strides
    const float* k; int64_t k_batch, k_head, k_row;
    const float* v; int64_t v_batch, v_head, v_row;
    int B, H, Lq, Lk, dh;
    int nsplit;                 // key splits (each writes one partial)
    float* o_part;              // [B*H][nsplit][dh][Lq_pad]
    float* m_part;              // [B*H][nsplit][Lq_pad]   (log2 domain running max)
    float* l_part;              // [B*H][nsplit][Lq_pad]
    float* out; int64_t out_batch, out_row;              // merged (b, q, h*dh + d)
    float defer_log2;           // split kernel: running max moves only past this margin (0 = always)
    float* lse;                 // optional [B*H][Lq_pad]: log2-domain log-sum-exp of every query row (training)
    float drop_p; uint32_t drop_seed;   // training: dropout on the attention probabilities, element (row bh * Lq + q, col key)
    int flags;                  // bit 0: raise the priority of the younger half of the workgroup (pipelined split kernel)
    // attention mode 4: its error grows as a row concentrates on few keys (flash_split8.hip).  The merge kernel knows every row's
    // sum l of probabilities relative to the row's reference maximum — roughly the number of keys that carry the row — and
    // raises bit h of *peaky (and of *peaky_it, this iteration's own word, if given) when some row of head h has l under peaky_l
    // (nullptr / 0: no check); *peaky_min (optional) keeps the smallest l seen as 0x7fffffff - its bits (atomicMax; 0 = none)
    int* peaky; float peaky_l;
    int* peaky_it; int* peaky_min;
    int* head_min;              // optional [H]: the smallest l of every head of this launch, same code (what a head on the fp16 x 3 tier would
                                // look like to the guard: PARQDecoder.tier_return_after)
    // a launch over SOME of the heads (attention mode 4 with per-head tiers: the heads whose rows rest on few keys run the fp16 x 3
    // kernel, the others the mode-4 kernel, each class with its own launch, key-split count and partial buffers).  nh = 0: all H heads.
    // nh > 0: grid index z = b * nh + i covers head (hmap >> 4 i) & 15; partials are indexed by z, everything else by b * H + head.
    int nh; unsigned long long hmap;
    int64_t cache_head_bytes;   // bytes between the cache regions of two (scene, head) pairs; 0 = the kernel's own packed layout
    int geom_B;                 // batch-invariant inference: the scene count the launchers choose waves / merge width from (0: B)
};
struct FlashHead { int b, h, bh; };
// grid index z of a partial-producing / merging launch -> (scene, head, b * H + head)
__device__ __forceinline__ FlashHead flash_head(const FlashArgs& a, int z) {
    FlashHead r;
    if (a.nh > 0) { r.b = z / a.nh; r.h = (int)((a.hmap >> (4 * (z - r.b * a.nh))) & 15ull); }
    else { r.b = z / a.H; r.h = z - r.b * a.H; }
    r.bh = r.b * a.H + r.h;
    return r;
}
inline int flash_launch_heads(const FlashArgs& a) { return a.nh > 0 ? a.nh : a.H; }
int flash_key_tile(int dh);                    // keys per LDS tile
int flash_lq_pad(int Lq);
int flash_pick_nw(int B, int H, int Lq, int Lk, int dh, int num_cus);   // waves per workgroup
int flash_pick_splits(int B, int H, int Lq, int Lk, int dh, int num_cus);
int device_num_cus();                          // cached CU count of the current device
size_t flash_scratch_bytes(int B, int H, int Lq, int dh, int nsplit);
hipError_t launch_flash(const FlashArgs& a, hipStream_t s);       // partials
hipError_t launch_flash_merge(const FlashArgs& a, hipStream_t s); // partials -> out

// split-precision (fp16 hi/lo, 3-term products) cross-attention, head dim 64 (flash_split.hip).
// `terms` = 3: split precision (fp32-class accuracy); 1: single fp16 / bf16 products (`kind` = kF16 / kBF16),
// cache blocks hold only [K | V] (8 KB instead of 16 KB).
size_t kvsplit_cache_bytes(int B, int H, int N, int terms = 3);
int flash_split_pick_splits(int B, int H, int Lq, int Lk, int num_cus);
// kvproj_big.hip: the K/V projection for C > 256 (pre-split tokens, LDS-DMA operands); scratch = kvproj_big_scratch_floats floats
size_t kvproj_big_scratch_floats(int B, int N, int C);
hipError_t launch_kvproj_big(const void* tokens, const void* Whi, const void* Wlo, const float* bias, int B, int N, int C,
                             void* cache, int* overflow, float* scratch, hipStream_t s, int terms = 3, int kind = kF16,
                             int tok_type = kTokF32,       // tok_type: element type of `tokens` (kTokF32 / kTokF16 / kTokBF16)
                             int row0 = 0, int row_end = -1);   // token rows [row0, row_end) of every scene (row_end < 0: all); multiples of 32 or N
// flash_split256.hip: the same for head dim 256 (a head = 4 virtual heads of 64 in the cache; wave pairs split the head dim)
int flash_split256_pick_splits(int B, int H, int Lq, int Lk, int num_cus);
hipError_t launch_flash_split256(const FlashArgs& a, const void* cache, hipStream_t s, int terms = 3, int kind = kF16);
hipError_t launch_kvsplit_convert(const float* K, const float* V, int64_t k_batch, int64_t k_head, int64_t k_row,
                                  int64_t v_batch, int64_t v_head, int64_t v_row, int B, int H, int N, void* cache,
                                  int* overflow_flag, hipStream_t s, int terms = 3, int kind = kF16);
// split cache (terms = 3) -> fp32 head-major K / V ([n][64] rows per (b, h))
hipError_t launch_kvsplit_to_f32(const void* cache, int B, int H, int N, float* K, float* V, int64_t k_batch, int64_t k_head,
                                 int64_t v_batch, int64_t v_head, hipStream_t s, int chunks = 1,   // H cache heads = model heads x chunks
                                 int terms = 3, int kind = kF16);                                   // terms = 1: the single 16-bit cache
hipError_t launch_flash_split(const FlashArgs& a, const void* cache, hipStream_t s, int terms = 3,
                              int kind = kF16);   // partials; merge as usual
// flash_split8.hip: attention mode 4 — the scores with their two cross terms on the MX-scaled fp8 matrix instruction, P V in fp16 with a
// self-consistent normaliser (head dim 64, whole 64-key stages only: flash_split8_supported).  Cache = Lk / 64 stages of 24 KB per
// (scene, head) — within the size kvsplit_cache_bytes(.., 3) gives for such Lk.
bool flash_split8_supported(int dh, int Lk);
hipError_t launch_kvsplit8_convert(const float* K, const float* V, int64_t k_batch, int64_t k_head, int64_t k_row, int64_t v_batch,
                                   int64_t v_head, int64_t v_row, int B, int H, int N, void* cache, hipStream_t s);
hipError_t launch_flash_split8(const FlashArgs& a, const void* cache, hipStream_t s);
// attention modes 2 / 3 on whole 64-key stages of the single-product cache (flash_split8.hip); flash_split8_supported(dh, Lk) says where
hipError_t launch_flash_single_stage(const FlashArgs& a, const void* cache, hipStream_t s, int kind);
// attn_map.hip: the cross-attention probabilities of a finished iteration, recomputed from its projected queries and the K cache
// (parq_attention_map).  klayout says how K of a head is stored; kMapStage8 with safe_mask: head h is in the split layout where bit h is set.
enum : int { kMapF32 = 0, kMapSplit3 = 1, kMapF16 = 2, kMapBF16 = 3, kMapStage8 = 4 };
struct AttnMapArgs {
    const void* kbase;          // fp32 head-major K/V of the layer ([b][K heads | V heads][N][dh]) or the layer's cache
    int klayout; unsigned safe_mask;
    int64_t head_bytes;         // cache layouts: bytes between the regions of two (scene, 64-dim cache head) pairs
    int B, H, dh, C, N, V, hw;  // hw = keys per view (N = V * hw)
    int nsel;                   // selected query rows
    int what, out_f16;          // 0 head mean (B, nsel, N) | 1 per head (B, H, nsel, N) | 2 view mass (B, nsel, V); element type of out
    void* out;
    // filled by launch_attn_map from the scratch
    int qtiles, nsel_pad, nsplit, nseg;
    float scale_log2;
    const half8* qfrag;
    float* part_m; float* part_l; float* stat_m; float* stat_il; float* vpart;
};
size_t attn_map_scratch_bytes(int B, int H, int dh, int N, int V, int hw, int nsel);
hipError_t launch_attn_map(AttnMapArgs a, const float* cross_q, const int* query_index, int Q, void* scratch, hipStream_t s);
// kvproj_split.hip: tokens -> split cache directly (W pre-split with launch_split_f32)
hipError_t launch_split_f32(const float* src, void* hi, void* lo, int64_t n, hipStream_t s);
// elementwise.hip: up to kGatherMax device-to-device float copies in ONE launch (the weight pack: ~50 tensors per training step)
constexpr int kGatherMax = 64;
struct GatherArgs { const float* src[kGatherMax]; float* dst[kGatherMax]; int64_t n[kGatherMax]; int count; };
hipError_t launch_gather_copy(const GatherArgs& g, hipStream_t s);
// setloss.hip: loss terms + d term / d output for a given matching (three launches)
hipError_t launch_set_loss(const float* logits, const float* center, const float* size, const float* o6, int I, int B, int Q, int ncls,
                           const float* t_center, const float* t_size, const float* t_rot, const int32_t* t_label, const int32_t* t_sym,
                           int nmax, const int32_t* pairs, const float* coef, int P, const float* row_weight, const float* class_weight,
                           const float* w4, int background, float* terms, float* g_logits, float* g_center, float* g_size, float* g_o6,
                           int32_t* cls, hipStream_t s, float* det_part = nullptr);   // det_part: setloss_part_floats(P, I*B*Q) floats
inline int64_t setloss_part_floats(int64_t P, int64_t rows) { return 3 * ((P + 255) / 256) + (rows + 255) / 256; }
// terms = 11: attention mode 4 with per-head tiers — head h as mode-4 stages, or in the split layout where bit h of safe_mask is set;
// every (scene, head) region of the cache then spans ceil(N / 32) * 16 KB (the split layout's size)
hipError_t launch_kvproj_split(const void* tokens, const void* Whi, const void* Wlo, const float* bias, int B, int N,
                               int C, int H, void* cache, int* overflow, hipStream_t s, int terms = 3, int kind = kF16, unsigned safe_mask = 0,
                               int tok_type = kTokF32, int row0 = 0, int row_end = -1);      // rows [row0, row_end) of every scene (row_end < 0: all)
int kvproj_split_granule(int C);      // what row0 / row_end of launch_kvproj_split are multiples of (row_end may also be N)
// fp32 -> 16-bit (round to nearest) weights of the single-term modes
hipError_t launch_cvt16(const float* src, void* dst, int64_t n, int kind, hipStream_t s);
// 16-bit tokens (tok_type kTokF16 / kTokBF16) -> fp32, exact: the fp32 K/V projection of attention mode 0 reads the widened copy
hipError_t launch_widen_tokens(const void* src, float* dst, int64_t n, int tok_type, hipStream_t s);
// 16-bit tokens -> `kind` (kF16 / kBF16) rounded to nearest from their exact fp32 value: what launch_cvt16 makes of the widened tokens
hipError_t launch_cvt16_tokens(const void* src, void* dst, int64_t n, int kind, int tok_type, hipStream_t s);

// raype.hip: ray-point positional encoding + tokenisation
// The four FPN levels of a pyramid (parq_fpn_levels): level l is (B*V, cl, h[l], w[l]) fp32, resized bilinearly (torch's
// align_corners=False formula) to the size of level `layer` and read as channels l*cl .. l*cl + cl - 1 of the feature maps.
// launch_raype_fused / launch_gemm_split take one in place of `feat` (the one-pass kernel at C = 256, the generic epilogue).
struct FpnDev {
    const float* lv[4];
    int h[4], w[4];
    int layer, cl;
};
hipError_t launch_raype_points(const float* cam, const float* T_cp, const float* T_wp, const float* T_wl,
                               const float* scale6, float min_depth, float max_depth, int B, int V, int h, int w, int S,
                               float* P, hipStream_t s);
hipError_t launch_raype_fused(const float* cam, const float* T_cp, const float* T_wp, const float* T_wl, const float* scale6,
                              float min_depth, float max_depth, int B, int V, int h, int w, const void* W1hi, const void* W1lo,
                              const float* b1, const void* W2hi, const void* W2lo, const float* b2, const float* feat,
                              float* hidden, double* Tl, double* depth, float* out, int nchw_out, hipStream_t s,
                              void* W2f, int w2f_cached = 0,      // W2f: 256 KB for W2 in fragment order; cached: it holds this W2 already
                              int out16 = kTokF32,       // out16: kTokF16 / kTokBF16 token rows (one-pass kernel, no hidden, channels-last)
                              const FpnDev* fpn = nullptr);   // features gathered from a pyramid (feat == nullptr)
// d level_l (B*V, cl, h[l], w[l]) for all four levels from d tokens (B*V*h*w, 4*cl): the adjoint of the bilinear gather in gather
// form (a fixed summation order per texel, no atomics)
hipError_t launch_fpn_backward(const float* d_tokens, int BV, const FpnDev& fpn, float* const* d_level, hipStream_t s);
// GroupNorm(1, C) statistics from the float64 moments (sum, sum of squares) of a group, all in float64 (the variance is a difference
// of two nearly equal numbers) with one reciprocal of the element count.  Used by the forward consumers and by the backward that
// re-normalises from the same moments.  (An fp32 reciprocal square root was measured: the consumers' times did not move — the
// statistics hide behind the operand fetch — so the float64 form stays.)
__device__ __forceinline__ void gn_mean_rstd(double S, double Q, double inv_cnt, float eps, float& mean, float& rstd) {
    const double mu = S * inv_cnt;
    double var = Q * inv_cnt - mu * mu;
    var = var < 0.0 ? 0.0 : var;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}
struct ScaleBox { float lo[3]; float hi[3]; };
// ---- deterministic mode (parq_set_deterministic, PARQ_RAYPE_BWD_DETERMINISTIC).  While a DetScope is alive on the enqueuing host
// thread, the backward launchers take their fixed-order forms: row-split reductions write one fp32 partial per row range into this
// scratch (plain stores) and a second launch sums the partials in index order; the token-gradient scatter becomes a gather per
// destination token.  Nothing changes while no scope is alive (the default path).
struct DetScratch {
    float* base = nullptr;            // device scratch, 16-byte aligned
    int64_t floats = 0;
};
const DetScratch* det_scratch();      // nullptr outside a DetScope
struct DetScope {
    DetScratch saved;
    DetScope(float* base, int64_t floats);
    ~DetScope();
};
// scratch floats the fixed-order forms need for one call: the row-split slabs, plus `sample_rows` gather records (B*Q*V of the
// project + sample backward) and `dq_floats` dQ partials of the short-key attention backward (det_attn_dq_floats)
int64_t det_scratch_floats(int64_t sample_rows, int64_t dq_floats);
int64_t det_attn_dq_floats(int B, int H, int Lq, int Lk);
int64_t det_kvbwd_floats();            // row-range partials of kvproj_bwd_split_kernel (launch_kvproj_bwd_split, launch_tn_split_512x256)
// out[r][c] (+)= sum over s of part[s * stride + r * cols + c], in s order
hipError_t launch_slab_reduce(const float* part, int S, int64_t stride, int R, int cols, float* out, int64_t ldo, int accumulate,
                              hipStream_t s);
// sums[(scene * ngroups + g) * kGnSlots + slot][2] = the moments of rows slot, slot + kGnSlots, ... of x's (scene, group) block, fixed order
hipError_t launch_gn_moments_det(const float* x, int64_t ldx, int C, int ngroups, int rows_per_scene, int B, double* sums, hipStream_t s);
// ---- backward (backward.hip, attn_bwd.hip)
hipError_t launch_transpose(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int R, int Cc, hipStream_t s);
hipError_t launch_gemm_tn(const float* A, int64_t lda, const void* B, int64_t ldb, float* out, int64_t ldo, int M, int N, int K,
                          int accumulate, hipStream_t s, float* bias = nullptr, int bias_from = 0,    // bias[n] (+)= column sums of A, n >= bias_from
                          int b_type = kTokF32);      // element type of B (16-bit memory tokens are widened as they are loaded; ldb in elements)
hipError_t launch_colsum(const float* X, int64_t ldx, int M, int N, float* out, int accumulate, hipStream_t s);
hipError_t launch_add(const float* a, const float* b, float* y, int64_t n, hipStream_t s);
hipError_t launch_axpy_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int M, int N, int accumulate, hipStream_t s);
hipError_t launch_ln_bwd(const float* gy, const float* x, const float* stats, const float* gamma, float* gx, int M, int C,
                         int accumulate, float* dgamma, float* dbeta, hipStream_t s);
hipError_t launch_gn_apply(const float* x, int64_t ldx, const double* sums, const float* gamma, const float* beta, int M, int C,
                           int ngroups, int rows_per_scene, float eps, float* y, int64_t ldy, hipStream_t s);
hipError_t launch_gn_bwd(const float* x, int64_t ldx, const double* sums, const float* gamma, const float* beta, int M, int C,
                         int ngroups, int rows_per_scene, float eps, const float* gy, int64_t ldgy, float* gz, double* bsums,
                         float* gx, int64_t ldgx, float* dgamma, float* dbeta, hipStream_t s);
hipError_t launch_decode_bwd(const float* g_logits, const float* g_center, const float* g_size, const float* g_rot,
                             const float* center, const float* size, const float* ref, ScaleBox sb, int M, int ncls, int NH1, int C,
                             float* g_h3, float* g_h1, float* g_ref, hipStream_t s);
hipError_t launch_head3_bwd(const float* g_h3, const float* w3, float* g_act, int M, int C, hipStream_t s);
hipError_t launch_posemb_bwd(const float* g_emb, const float* ref, const float* dim_t, int M, float* g_ref, hipStream_t s);
hipError_t launch_refpoint_bwd(const float* g_ref, const float* ref0, int B, int Q, float* g_w, hipStream_t s);
hipError_t launch_sample_bwd(const void* tokens, const double* T_cl, const float* cam, const float* ref, ScaleBox sb, int B, int V,
                             int h, int w, int C, int Q, const float* g_tgt, float* g_tokens, float* g_ref, hipStream_t s,
                             int tok_type = kTokF32);     // element type of `tokens` (read for g_ref only)
hipError_t launch_attn_bwd(const float* q, int64_t q_batch, int64_t q_head, int64_t q_row, const float* k, int64_t k_batch,
                           int64_t k_head, int64_t k_row, const float* v, int64_t v_batch, int64_t v_head, int64_t v_row,
                           const float* dO, int64_t do_batch, int64_t do_head, int64_t do_row, const float* lse, const float* D,
                           float* gq, int64_t gq_batch, int64_t gq_head, int64_t gq_row, float* gk, int64_t gk_batch,
                           int64_t gk_head, int64_t gk_row, float* gv, int64_t gv_batch, int64_t gv_head, int64_t gv_row, int B, int H,
                           int Lq, int Lk, int dh, int accumulate_kv, hipStream_t s, float* gq_part = nullptr, float drop_p = 0.f,
                           uint32_t drop_seed = 0, unsigned int* absmax = nullptr,    // absmax: 8-byte device scratch -> split-precision kernel
                           float* mat_scratch = nullptr);   // attn_bwd_mat_scratch_floats(...) floats: head dims other than 32 / 64
size_t attn_bwd_mat_scratch_floats(int Lq, int Lk, int dh);
// all recurrent iterations that share K / V in one launch (split-precision kernel; see attn_bwd.hip)
hipError_t launch_attn_bwd_batched(const float* q, const int64_t* q_off, int64_t q_batch, int64_t q_head, int64_t q_row, const float* k,
                                   int64_t k_batch, int64_t k_head, int64_t k_row, const float* v, int64_t v_batch, int64_t v_head,
                                   int64_t v_row, const float* dO, int64_t do_it, int64_t do_batch, int64_t do_head, int64_t do_row,
                                   const float* lse, const int64_t* lse_off, const float* D, int64_t D_it, float* gq, int64_t gq_it,
                                   int64_t gq_batch, int64_t gq_head, int64_t gq_row, float* gk, int64_t gk_batch, int64_t gk_head,
                                   int64_t gk_row, float* gv, int64_t gv_batch, int64_t gv_head, int64_t gv_row, int B, int H, int Lq,
                                   int Lk, int dh, int n_it, hipStream_t s, float* gq_part, float drop_p, const uint32_t* seeds,
                                   unsigned int* absmax, unsigned int* kv_absmax = nullptr,    // kv_absmax: out, max |dK|, |dV| (float bits)
                                   void* pack = nullptr,
                                   float* mat_scratch = nullptr,
                                   const void* kvcache = nullptr, int cache_terms = 0, int cache_kind = 0);   // head dim 64: K / V from the 16-bit cache
                                                                   // pack: attn_bwd_pack_floats(...) floats of scratch -> second-version kernel;
                                                                   // mat_scratch (dh == 256): attn_bwd_batched256_scratch_floats(n_it, Lq, Lk) floats
size_t attn_bwd_pack_floats(int B, int H, int Lq, int n_it);
// kvproj_bwd.hip: dW_kv / db_kv of the hoisted projection on the fp16 matrix pipe (hi/lo split), C = 256
bool kvproj_bwd_split_supported(int C);
// x_type / tok_type: element type of x / tokens (kTokF32 / kTokF16 / kTokBF16); fp16 runs two MFMAs per product (its lo half is zero)
hipError_t launch_tn_split_512x256(const float* g, int64_t ldg, const void* x, int64_t ldx, int64_t M, float* out, int64_t ldo,
                                   float* db, const unsigned int* absmax_bits, float* scale_scratch, hipStream_t s, int x_type = kTokF32);
hipError_t launch_kvproj_bwd_split(const float* g, const void* tokens, int64_t M, int C, float* dW, float* db,
                                   const unsigned int* absmax_bits, float* scale_scratch, hipStream_t s, int tok_type = kTokF32);
// dst = dropout(src): keep mask of stream `seed` over the (M, N) index space, scaled by 1 / (1 - p)
hipError_t launch_dropout_apply(const float* src, float* dst, int M, int N, float p, uint32_t seed, hipStream_t s);
size_t attn_bwd_dq_partial_floats(int B, int H, int Lq, int Lk, int dh, bool grouped = false);      // grouped: the batched kernel's slots
int attn_bwd_kb_group(int B, int H, int Lk);
size_t attn_bwd_batched256_scratch_floats(int n_it, int Lq, int Lk);
hipError_t launch_absmax(const float* x, int64_t n, unsigned int* out, hipStream_t s);
hipError_t launch_attn_bwd_rowdot(const float* dO, const float* O, int64_t batch, int64_t row, int B, int H, int Lq, int dh, float* D,
                                  hipStream_t s);
// postproc.hip: parse_pred + 3-D NMS on the device
hipError_t launch_parse_pred(const float* center, const float* size, const float* rot6, const float* prob, int B, int Q, int ncls,
                             int num_semcls, const float* track_scale6, int for_vis, int enable_nms, float* obbs,
                             unsigned char* mask, hipStream_t s);
// obb_iou.hip: the tracker's oriented-box IoU, S segments of (n_a x n_b) pairs in one launch (total >= 1)
hipError_t launch_obb_iou(const double* boxes_a, const double* boxes_b, const int64_t* seg, int S, int64_t total, int64_t n_a_total,
                          int64_t n_b_total, double* iou3, double* iou2, hipStream_t s);
// tracks.hip: the rectangular assignment solver (one wave per segment, S >= 1, sides <= 2048; duals: S * (max_rows + max_cols) doubles)
// and the device-resident track store's update for scenes [b0, b0 + nb) of a batch (nb <= kTrackChunk; three launches)
constexpr int kTrackChunk = 64;
hipError_t launch_assign_max(const float* m, int64_t m_total, const int64_t* seg, int S, int max_rows, int max_cols, double* duals,
                             int32_t* row_to_col, int64_t out_total, hipStream_t s);
size_t tracks_update_workspace_bytes(int B, int Q, int max_tracks);
hipError_t launch_tracks_update(int32_t* store, int max_tracks, const int32_t* slots_host, int b0, int nb, const float* corners_world,
                                const float* prob, const unsigned char* mask, int Q, int K, float conf, float iou_thresh, void* ws,
                                int32_t* track_id, float* iou_out, hipStream_t s);
// the ground-truth store's update (parq_gt_tracks_update): a select launch of its own (valid rows, jittered corners, score 1), then
// launch_tracks_update's IoU and assignment launches.  ws: gt_tracks_update_workspace_bytes, 16-byte aligned
size_t gt_tracks_update_workspace_bytes(int B, int P, int max_tracks);
hipError_t launch_gt_tracks_update(int32_t* store, int max_tracks, const int32_t* slots_host, const int32_t* visits_host, int b0, int nb, int B,
                                   const float* corners_world, const int32_t* labels, const unsigned char* valid, int P, float iou_thresh,
                                   uint32_t seed_lo, uint32_t seed_hi, void* ws, float* iou_out, hipStream_t s);
// track_life.hip: the life record beside the track store (uid, hits, first, last per track) for scenes [b0, b0 + nb) of a call
// (nb <= kTrackChunk): one update noted, and the tracks unseen for too long removed in place; one launch each
hipError_t launch_tracks_note(const int32_t* store, int32_t* life, int max_tracks, const int32_t* slots_host, int b0, int nb,
                              const int32_t* track_id, int Q, int32_t* uid_out, int32_t* hits_out, hipStream_t s);
hipError_t launch_tracks_retire(int32_t* store, int32_t* life, int max_tracks, const int32_t* slots_host, int b0, int nb, int min_hits,
                                int max_age, int tentative_age, int32_t* remap_out, hipStream_t s);
// f1_counts.hip: per-class ground-truth / prediction / true-positive counts of S scenes from a prediction and a ground-truth track
// store (two launches); ws: f1_counts_workspace_bytes
constexpr int kF1MaxThresholds = 8, kF1MaxClasses = 32;
size_t f1_counts_workspace_bytes(int S, int gt_max_tracks, int T, int K);
struct F1Thresholds {
    double thr[kF1MaxThresholds];
};
hipError_t launch_f1_counts(const int32_t* pred_store, int pred_max_tracks, const int32_t* gt_store, int gt_max_tracks, int S,
                            const F1Thresholds& thr, int T, int K, void* ws, int64_t* counts, int64_t* invalid, double* best_iou,
                            hipStream_t s);
// avg_precision.hip: average precision per (threshold, class) of S scenes from the same two stores (target pass, counts, true-positive
// flags, a bitonic sort of S * pred_max_tracks keys padded to a power of two, the curves); ws: average_precision_workspace_bytes.
// The five optional outputs are all given or all NULL.
constexpr int kApMaxPositions = 1 << 20;
size_t average_precision_workspace_bytes(int S, int pred_max_tracks, int T, int K);
hipError_t launch_average_precision(const int32_t* pred_store, int pred_max_tracks, const int32_t* gt_store, int gt_max_tracks, int S,
                                    const F1Thresholds& thr, int T, int K, void* ws, double* ap, int64_t* counts, int64_t* invalid,
                                    int32_t* order, int32_t* class_start, int32_t* cum_tp, double* pred_best, int32_t* pred_target,
                                    hipStream_t s);
// setmatch.hip: the set loss's matcher for all I * B (iteration, scene) problems (cost, launch_assign_max, pairs, finish: four
// launches; I * B >= 1, Q and nmax in [1, 2048]); ws: set_match_workspace_bytes, 16-byte aligned
size_t set_match_workspace_bytes(int I, int B, int Q, int nmax);
hipError_t launch_set_match(const float* logits, const float* coord, int I, int B, int Q, int ncls, const float* t_center,
                            const int32_t* t_label, const int32_t* t_count, int nmax, float cost_class, float cost_bbox, float ratio,
                            int max_padding, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void* ws, int32_t* row_to_col,
                            int32_t* pairs, float* coef, float* row_weight, int32_t* stats, float* cost_out, unsigned char* near_out,
                            hipStream_t st);
// draw.hip: boxes drawn into the normalised views.  Workspace = the min / max parts (draw_minmax_bytes, a multiple of 16 bytes)
// followed by the (B, T, M, 12) edge slots of 8 bytes each
size_t draw_minmax_bytes(int B, int T);
hipError_t launch_draw_minmax(const float* images, int B, int T, int H, int W, void* parts, hipStream_t s);
hipError_t launch_draw_project(const float* camera, const float* T_cp, const float* T_wp, const float* corners, const int32_t* labels,
                               const unsigned char* keep, const int32_t* count, int num_classes, int B, int T, int M, void* slots,
                               hipStream_t s);
hipError_t launch_draw_raster(const float* images, const void* parts, const void* slots, const int32_t* labels, const float* colors, int B,
                              int T, int H, int W, int M, void* out, int out_uint8, hipStream_t s);
// frames.hip: raw uint8 frames resized by Pillow's 8-bit bilinear rule (one launch).  frames_sizes_ok: the sizes the launch takes
bool frames_sizes_ok(int N, int H_in, int W_in, int pl, int pt, int pr, int pb, int H_out, int W_out);
hipError_t launch_frames_resize(const unsigned char* frames, int N, int H_in, int W_in, int pl, int pt, int pr, int pb, const int32_t* plan_x,
                                const int32_t* plan_y, int H_out, int W_out, void* out, int out_uint8, hipStream_t s);
// snippets.hip: a snippet's training targets from depth and poses (count + finalise: two launches).  ws: snippet_workspace_bytes
bool snippet_sizes_ok(int B, int T, int Hd, int Wd, int N);
size_t snippet_workspace_bytes(int B, int T, int Hd, int Wd, int N);
hipError_t launch_snippet_targets(const uint16_t* depth, int B, int T, int Hd, int Wd, const float* kinv, const float* kcolor, int color_h,
                                  int color_w, const double* poses, const float* obbs, const double* corners, const void* sym, int sym_is_int,
                                  int S, int N, int max_box, const int32_t* level_counts, const float* level_ratios, int n_levels,
                                  int max_level, float depth_scale, void* ws, float* obbs_out, void* sym_out, int32_t* num_valid,
                                  int32_t* frame_points, float* frame_trunc, int32_t* points, float* trunc, int32_t* difficulty,
                                  int32_t* valid, hipStream_t s);
hipError_t launch_gemm_split(const float* X, int64_t ldx, const void* Whi, const void* Wlo, const float* bias, float* Y,
                             int64_t ldy, int M, int N, int K, int relu, const float* feat, int hw, hipStream_t s,
                             const float* scale_dev = nullptr, float scale_mul = 1.f, const float* xscale_dev = nullptr,
                             int accumulate = 0,    // Y (+)= ((x * *xscale_dev) W^T) * scale_mul / *scale_dev + bias
                             int out16 = kTokF32,   // Y as kTokF16 / kTokBF16 elements (rounded to nearest; not with accumulate)
                             const FpnDev* fpn = nullptr);   // epilogue adds the pyramid's gathered features (feat == nullptr)

// ------------------------------------------------------------------ elementwise / gather kernels
hipError_t launch_camera_local(const float* T_cp, const float* T_wp, const float* T_wl, int B, int V,
                               float* T_cl, hipStream_t s);
hipError_t launch_camera_local_f64(const float* T_cp, const float* T_wp, const float* T_wl, int B, int V,
                                   double* T_cl, hipStream_t s);
hipError_t launch_initial_ref(const float* refpoint_w, int B, int Q, float* ref, hipStream_t s);
// Per-call pointers of a captured forward (api.hip parq_forward_replay): the recorded iterations must not hold the caller's token and
// output pointers themselves, so the prologue launch of every call (never part of the graph) leaves them in a block of the workspace —
// [0] tokens, [1..5] pred_logits, centre, size, ortho6d, sem_cls_prob, [6] coord_pos — and copies the cameras beside it; the kernels of
// the iterations that touch them (project + sample, box decode) load the pointers from that block when given one (`ind`).
struct CallPtrs { const void* p[8]; };
struct PrologueCall { const float* cam_src; float* cam_dst; int ncam; const void** ind; CallPtrs ptrs; };   // ind == nullptr: nothing to leave
hipError_t launch_forward_prologue(const float* T_cp, const float* T_wp, const float* T_wl, int B, int V, double* T_cl, const float* w, int Q,
                                   float* ref, const float* dim_t, float* emb, float* flags, int nflags, hipStream_t s,
                                   const PrologueCall* call = nullptr);
hipError_t launch_posemb(const float* ref, const float* dim_t, int M, float* emb, hipStream_t s);
hipError_t launch_zero_f64(double* p, int n, hipStream_t s);
hipError_t launch_project_sample(const float* tokens, const float* T_cl, const float* cam, const float* ref,
                                 ScaleBox sb, int B, int V, int h, int w, int C, int Q, float* tgt,
                                 float* coord_pos, hipStream_t s);
// zero_f64/zero_n: accumulators (GroupNorm moments) this kernel clears for later kernels of the iteration
// ind / coord_off: tokens = ind[0] and coord_pos = (float*)ind[6] + coord_off instead of the two pointer arguments (CallPtrs)
// tok_type: element type of the token rows (kTokF32 / kTokF16 / kTokBF16), widened to fp32 as they are read
hipError_t launch_project_sample_f64(const void* tokens, const double* T_cl, const float* cam, const float* ref,
                                     ScaleBox sb, int B, int V, int h, int w, int C, int Q, float* tgt,
                                     float* coord_pos, double* zero_f64, int zero_n, hipStream_t s, float* raw_count = nullptr,
                                     const void* const* ind = nullptr, int64_t coord_off = 0, int tok_type = kTokF32);
hipError_t launch_pe1_sample(const LinearArgs& pe1, const void* tokens, const double* T_cl, const float* cam, const float* ref, ScaleBox sb,
                             int B, int V, int h, int w, int C, int Q, float* tgt, float* coord_pos, double* zero_f64, int zero_n,
                             float* raw_count, hipStream_t s, const void* const* ind = nullptr, int64_t coord_off = 0, int tok_type = kTokF32);
hipError_t launch_sample_finalize(const float* sums, const float* counts, int64_t M, int C, float* tgt, hipStream_t s,
                                  const float* range_sum = nullptr, int* range_flag = nullptr);
hipError_t launch_shard_range_flag(const int* range_flag, float* out, hipStream_t s);
hipError_t launch_attn_combine(const float* parts, int R, int64_t rec, int B, int H, int Q, int Lq_pad, int dh, float* out, hipStream_t s);
// self-attention of the Q queries in one launch (8 key slices per workgroup combined through LDS)
hipError_t launch_self_attn(const float* qkv, int64_t row_stride, int B, int H, int Lq, int dh, float* out,
                            int64_t out_row, hipStream_t s, float* lse = nullptr, float drop_p = 0.f, uint32_t drop_seed = 0);
hipError_t launch_layernorm(const float* X, const float* gamma, const float* beta, float* Y, int M, int C,
                            float eps, hipStream_t s);
// mean / rstd over (rows_per_scene x ncols) blocks: stats[(b * ngroups + g) * 2 + {0,1}]
hipError_t launch_gn_stats(const float* X, int64_t ldx, int col0, int ncols, int ngroups, int B,
                           int rows_per_scene, float eps, float* stats, hipStream_t s);
// Last kernel of an iteration, one wave per query row: GroupNorm+ReLU of the second hidden layer,
// the two output layers (centre 3, rotation 6), softmax / arg-max size gather / centre update
// (transformer_parq.py:242-279), next reference point and its 384-d sine embedding (:45-64).
struct BoxDecodeArgs {
    const float* h1; int64_t ld1;      // [M][..]: logits at cols [0,ncls), size_raw at [ncls, ncls+3)
    const float* h2; int64_t ld2;      // [M][2C]: centre hidden | rotation hidden (pre-GroupNorm)
    const double* gn_sums;             // [B][2][gn_slots][2] moments of h2 per scene and head
    const float* gn_gamma; const float* gn_beta;       // [2][C]
    const float* w3; const float* b3;  // [2][6][C] (centre rows 0..2 of group 0), [2][6]
    int C; int rows_per_scene; float eps;
    const float* ref;                  // [M][3] normalised reference points of this iteration
    const float* mean_sizes; int n_mean;
    const float* dim_t;                // [128]
    ScaleBox sb; int M; int ncls;
    float *logits, *center, *size, *rot, *prob;     // outputs (coord_pos is written by project_sample)
    float* ref_next;                   // [M][3] or nullptr
    float* emb_next;                   // [M][384] or nullptr: pos2posemb3d(ref_next)
    int* poison_mirror;                // optional host-visible int: bit 0 set when outputs are poisoned by a range violation, bit 1 when
                                       // *peaky is set, bits 8 + h: head h of *peaky
    const int* peaky;                  // optional device int raised by the cross-attention merge of attention mode 4 (FlashArgs::peaky):
                                       // bit h = head h ran the mode-4 kernel on a row that rests on too few keys
    int peaky_poison;                  // non-zero: such an iteration's outputs are written as NaN too (never plausible wrong numbers)
    const int* poison;                 // optional device int: non-zero (fp16 operand range exceeded while the K/V cache was built; bit 2:
                                       // an in-launch hand-off timed out) -> every output of the iteration is written as NaN instead of
                                       // a plausible wrong number
    int poison_mask;                   // the bits of *poison that count (all of them in the fp16-operand cache modes, else only bit 2)
    const void* const* ind;            // optional CallPtrs block: the five output pointers are ind[1..5] + out_row0 rows (a captured forward)
    int64_t out_row0;
    int gn_slots;                      // slots per (scene, head) of gn_sums (a multiple of 64; 0 is read as kGnSlots)
    int geom_M;                        // batch-invariant inference: rows per workgroup are chosen from this many rows (0: from M)
};
hipError_t launch_box_decode(const BoxDecodeArgs& a, hipStream_t s);
// weight packing helpers
hipError_t launch_copy_rows(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int rows, int cols,
                            hipStream_t s);
hipError_t launch_fill(float* dst, float value, int64_t n, hipStream_t s);

}  // namespace parq
