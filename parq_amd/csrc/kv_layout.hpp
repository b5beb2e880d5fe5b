// The K/V cache layouts: the contract between the producers (K/V projection epilogues of kvproj_split.hip / kvproj_big.hip, convert
// kernels of flash_split.hip / flash_split8.hip) and the consumers (cross-attention flash_split*.hip, attention maps attn_map.hip,
// attention backward attn_bwd.hip, the fp32 rebuild kvsplit_to_f32_kernel); included by common.hpp.  Sizes, plane offsets and index maps are defined HERE only
// and held to each other by the compile-time checks at the end.  The helpers return indices and chunk positions, never whole
// addresses: a call site keeps its own association of the address sum (folded into a helper, the re-associated pointer arithmetic
// moves hipcc's schedule of the hot kernels), and a kernel that hoists a row's swizzle term writes kv_kswz(row, 0) and c ^ term.
//
// A cache HEAD is 64 dims (a model head of 64 c dims = c consecutive cache heads); per (scene, cache head) the keys come in BLOCKS of
// 32.  Every layout is "fragment-ready": the LDS image of a block equals its global image (staging is a linear 16-byte copy) and a
// lane's 8 contraction elements of an MFMA operand are one 16-byte chunk.
//   split cache    KvBlk<3>, 16 KB per block [K_hi|K_lo|V_hi|V_lo]: x = hi + lo, hi = fp16(x), lo = fp16(x - hi)
//   one-term cache KvBlk<1>, 8 KB per block [K|V]: one fp16 / bf16 value per element, rounded to nearest
//   K plane [32 keys][8 chunks][8 x 16 bit]: chunk c = 4 kh + s holds d = kv_dmap(kh, s, e) and sits at chunk position kv_kswz(key, c)
//           (conflict-free ds_read_b128 across keys);  V plane [64 d][4 chunks][8 x 16 bit]: chunk c = 2 m + kh holds keys
//           kv_kmap(m, kh, e) and sits at position kv_vswz(d, c)
// kv_dmap and kv_kmap are the row enumeration of the 32 x 32 MFMA accumulator (mfma32_row): the projection GEMM stores its accumulators
// as 16-byte chunks without a shuffle, and the softmax probabilities (S^T accumulator registers) are directly the B operand of V^T P^T.
//   mode-4 "stage" cache (flash_split8.hip; N % 64 == 0): a STAGE = 64 keys = two blocks = 24 KB; byte offsets inside a stage:
//     kS8Kh16      0  K hi16 [2 blocks][K plane]                 hi = fp16(x) rounded toward zero
//     kS8K8hi   8192  K hi8  [2 blocks][2 c][2 h][32 keys][16 B] e4m3(x); piece kv_piece8(b2, c, h, key): byte 8 m + e <-> d = kv_dmap(h, 2 m + c, e)
//     kS8K8lo  12288  K lo8  same, e4m3((x - hi16) 2^10)
//     kS8Vh16  16384  V fp16 [2 blocks][V plane]                 round to nearest
//   (the fp8 byte order is the accumulator's register order again; MX operand semantics: tools/bench_src/mx_probe.hip)
#pragma once
namespace parq {
// Row of a 32x32 MFMA C/D tile held in register `reg` of lane `lane` (col = lane & 31): what the layouts below are built around
__host__ __device__ constexpr __forceinline__ int mfma32_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

constexpr int kKvBlkKeys = 32;                                  // keys per cache block
constexpr int kKvHeadDim = 64;                                  // dims per cache head
constexpr int kKvChunk = 8;                                     // 16-bit elements per 16-byte chunk
constexpr int kKvPlaneHalfs = kKvBlkKeys * kKvHeadDim;          // 16-bit units of one K or V plane of a block (4 KB)
// a 32-key block: TERMS = 3 -> [K_hi|K_lo|V_hi|V_lo]; TERMS = 1 -> [K|V] (plane offsets in 16-bit units; K_hi / K at 0)
template <int TERMS>
struct KvBlk {
    static_assert(TERMS == 3 || TERMS == 1, "split or one-term cache");
    static constexpr int halfs = (TERMS == 3 ? 4 : 2) * kKvPlaneHalfs;
    static constexpr int bytes = halfs * 2;
    static constexpr int k_lo = kKvPlaneHalfs;                  // TERMS = 3 only
    static constexpr int v_hi = TERMS == 3 ? 2 * kKvPlaneHalfs : kKvPlaneHalfs;
    static constexpr int v_lo = 3 * kKvPlaneHalfs;              // TERMS = 3 only
};
// a 64-key stage of the mode-4 cache (bytes)
constexpr int kS8Keys = 2 * kKvBlkKeys;
constexpr int kS8Blk16Bytes = kKvPlaneHalfs * 2;                // one block inside a 16-bit plane (K hi16, V fp16)
constexpr int kS8PieceBytes = 16;                               // one fp8 piece
constexpr int kS8Plane8Bytes = 2 * 2 * 2 * kKvBlkKeys * kS8PieceBytes;       // K hi8 or K lo8 of a stage
constexpr int kS8Kh16 = 0, kS8K8hi = kS8Kh16 + 2 * kS8Blk16Bytes, kS8K8lo = kS8K8hi + kS8Plane8Bytes, kS8Vh16 = kS8K8lo + kS8Plane8Bytes;
constexpr int kStage8Bytes = kS8Vh16 + 2 * kS8Blk16Bytes;
// ---- index maps: dim of element e of K chunk 4 kh + s | key of element e of V chunk 2 m + kh
__host__ __device__ constexpr __forceinline__ int kv_dmap(int kh, int s, int e) { return 32 * (s >> 1) + 16 * (s & 1) + 4 * kh + (e & 3) + 8 * (e >> 2); }
__host__ __device__ constexpr __forceinline__ int kv_kmap(int m, int kh, int e) { return 16 * m + 4 * kh + (e & 3) + 8 * (e >> 2); }
// stored position of chunk c inside row `key` of a K plane (8 chunks) | row d of a V plane (4 chunks)
__host__ __device__ constexpr __forceinline__ int kv_kswz(int key, int c) { return c ^ ((key >> 1) & 7); }
__host__ __device__ constexpr __forceinline__ int kv_vswz(int d, int c) { return c ^ ((d >> 2) & 3); }
// fp8 piece (c, h) of key `key` of block b2 inside a K hi8 / K lo8 plane
__host__ __device__ constexpr __forceinline__ int kv_piece8(int b2, int c, int h, int key) { return ((b2 * 2 + c) * 2 + h) * 32 + key; }
// ---- host sizing: bytes of one (scene, cache head) region
__host__ __device__ constexpr int64_t kv_blk_head_bytes(int N, int terms) {
    return (int64_t)((N + kKvBlkKeys - 1) / kKvBlkKeys) * (terms == 3 ? KvBlk<3>::bytes : KvBlk<1>::bytes);
}
__host__ __device__ constexpr int64_t kv_stage_head_bytes(int N) { return (int64_t)(N / kS8Keys) * kStage8Bytes; }

// ---- the contract, checked in every build
namespace kv_check {
template <class F>
constexpr bool permutation(int n, F at) {                       // at(0..n-1) hits each of 0..n-1 exactly once (n <= 256)
    bool seen[256] = {};
    for (int i = 0; i < n; ++i) {
        const int v = at(i);
        if (v < 0 || v >= n || seen[v]) return false;
        seen[v] = true;
    }
    return true;
}
constexpr bool dmap_ok() { return permutation(64, [](int i) { return kv_dmap(i >> 5, (i >> 3) & 3, i & 7); }); }
constexpr bool kmap_ok() { return permutation(32, [](int i) { return kv_kmap(i >> 4, (i >> 3) & 1, i & 7); }); }
constexpr bool piece8_ok() { return permutation(256, [](int i) { return kv_piece8(i >> 7, (i >> 6) & 1, (i >> 5) & 1, i & 31); }); }
constexpr bool swizzles_ok() {                                  // permutations of a row's chunks, and involutions
    for (int key = 0; key < kKvBlkKeys; ++key) {
        if (!permutation(8, [key](int c) { return kv_kswz(key, c); })) return false;
        for (int c = 0; c < 8; ++c)
            if (kv_kswz(key, kv_kswz(key, c)) != c) return false;
    }
    for (int d = 0; d < kKvHeadDim; ++d) {
        if (!permutation(4, [d](int c) { return kv_vswz(d, c); })) return false;
        for (int c = 0; c < 4; ++c)
            if (kv_vswz(d, kv_vswz(d, c)) != c) return false;
    }
    return true;
}
constexpr bool acc_rows_ok() {                                  // the maps enumerate accumulator rows: register 8 m + e of lane half kh
    for (int kh = 0; kh < 2; ++kh)
        for (int e = 0; e < 8; ++e) {
            for (int m = 0; m < 2; ++m)
                if (kv_kmap(m, kh, e) != mfma32_row(8 * m + e, 32 * kh)) return false;
            for (int s = 0; s < 4; ++s)
                if (kv_dmap(kh, s, e) != 32 * (s >> 1) + mfma32_row(8 * (s & 1) + e, 32 * kh)) return false;
        }
    return true;
}
static_assert(dmap_ok(), "kv_dmap is a permutation of the 64 dims of a cache head");
static_assert(kmap_ok(), "kv_kmap is a permutation of the 32 keys of a block");
static_assert(piece8_ok(), "kv_piece8 is a permutation of the 256 pieces of an fp8 plane");
static_assert(swizzles_ok(), "kv_kswz / kv_vswz permute a row's chunks and are their own inverses");
static_assert(acc_rows_ok(), "kv_dmap / kv_kmap are the row enumeration of the 32 x 32 MFMA accumulator");
static_assert(kKvChunk * 2 == 16 && kKvHeadDim / kKvChunk == 8 && kKvBlkKeys / kKvChunk == 4, "8 K chunks per key, 4 V chunks per dim");
// the planes tile a block ...
static_assert(KvBlk<3>::k_lo == kKvPlaneHalfs && KvBlk<3>::v_hi == KvBlk<3>::k_lo + kKvPlaneHalfs &&
              KvBlk<3>::v_lo == KvBlk<3>::v_hi + kKvPlaneHalfs && KvBlk<3>::halfs == KvBlk<3>::v_lo + kKvPlaneHalfs, "split block");
static_assert(KvBlk<1>::v_hi == kKvPlaneHalfs && KvBlk<1>::halfs == KvBlk<1>::v_hi + kKvPlaneHalfs, "one-term block");
static_assert(KvBlk<3>::bytes == 16384 && KvBlk<1>::bytes == 8192, "16 KB / 8 KB per block");
// ... and a stage
static_assert(kS8Plane8Bytes == 256 * kS8PieceBytes && kS8K8hi == 8192 && kS8K8lo == 12288 && kS8Vh16 == 16384 && kStage8Bytes == 24576 &&
              kStage8Bytes == 3 * (2 * kS8Keys * kKvHeadDim), "mode-4 stage: 3 bytes per element of K and V");
// a mode-4 head fits the region the split cache has for the same keys (per-head tiers put either layout there)
static_assert(kStage8Bytes <= 2 * KvBlk<3>::bytes, "stage inside two split blocks");
}  // namespace kv_check
}  // namespace parq
