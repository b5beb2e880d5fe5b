// Oriented-box IoU of the evaluation tracker on the device: parq_amd/f1_eval.py iou3d (the reference's
// utils/f1_eval.py:77-175) for every pair of S independent (n_a x n_b) segments in one launch, one lane per pair.  The per-pair
// routine, and why this file is compiled with floating-point contraction off, are in obb_pair.hpp (shared with tracks.hip).
#include "obb_pair.hpp"

#pragma clang fp contract(off)

namespace parq {

namespace {

constexpr int kLanes = kObbLanes;

__global__ __launch_bounds__(kLanes) void obb_iou_kernel(const double* __restrict__ boxes_a, const double* __restrict__ boxes_b,
                                                         const int64_t* __restrict__ seg, int S, int64_t total, int64_t n_a_total,
                                                         int64_t n_b_total, double* __restrict__ iou3, double* __restrict__ iou2) {
    __shared__ ObbPolyLds lds;
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * kLanes + lane;
    if (p >= total) return;
    // the segment of this pair: the last one whose output offset is <= p (offsets ascend; empty segments share an offset with
    // the next non-empty one and sort before it)
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[(int64_t)mid * 5 + 4] <= p) lo = mid; else hi = mid - 1;
    }
    const int64_t a_off = seg[(int64_t)lo * 5], n_a = seg[(int64_t)lo * 5 + 1], b_off = seg[(int64_t)lo * 5 + 2],
                  n_b = seg[(int64_t)lo * 5 + 3], local = p - seg[(int64_t)lo * 5 + 4];
    // a table that does not describe the arrays it came with writes nothing rather than reading outside them
    if (local < 0 || n_a < 0 || n_b <= 0 || local >= n_a * n_b || a_off < 0 || b_off < 0 || a_off + n_a > n_a_total ||
        b_off + n_b > n_b_total)
        return;
    const int64_t ia = a_off + local / n_b, ib = b_off + local % n_b;
    Corners c1, c2;
    const bool nan1 = load_box(boxes_a + ia * 24, c1), nan2 = load_box(boxes_b + ib * 24, c2);
    double r3, r2;
    obb_pair_iou(c1, nan1, c2, nan2, lds, lane, r3, r2);
    iou3[p] = r3;
    if (iou2) iou2[p] = r2;
}

}  // namespace

hipError_t launch_obb_iou(const double* boxes_a, const double* boxes_b, const int64_t* seg, int S, int64_t total, int64_t n_a_total,
                          int64_t n_b_total, double* iou3, double* iou2, hipStream_t s) {
    const int64_t blocks = (total + kLanes - 1) / kLanes;
    if (S < 1 || total < 1 || blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(obb_iou_kernel, dim3((unsigned)blocks), dim3(kLanes), 0, s, boxes_a, boxes_b, seg, S, total, n_a_total, n_b_total,
                       iou3, iou2);
    return hipGetLastError();
}

}  // namespace parq
