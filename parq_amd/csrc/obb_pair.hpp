// The per-pair routine of the tracker's oriented-box IoU, shared by obb_iou.hip (parq_obb_iou: float64 canonical corners) and
// tracks.hip / f1_counts.hip (parq_tracks_update, parq_f1_counts: float32 world corners made canonical on the fly, load_canonical
// below): ONE text, so the entries cannot drift.
//   boxes: the 8 corners f1_eval.canonical() produces, float64; footprint polygon = corners 3, 2, 1, 0 in (x, z);
//   Sutherland-Hodgman clip of footprint A against footprint B with the host routine's strict inside test and crossing formula in
//   the same operation order, shoelace area, overlap height min(y of corner 0) - max(y of corner 4), volumes from three edges.
// Every file that includes this is compiled with floating-point contraction off (the pragma below): an inside test is
// `e_x * d_y > e_y * d_x`, and for a box clipped against itself or a near-copy its sign is a rounding question that a fused
// multiply-add answers differently from Python's floats.
// The two polygon buffers of a lane live in LDS (a column per lane: bank-conflict free, and indexed at run time without scratch);
// the calling kernel declares them (ObbPolyLds) and runs workgroups of kObbLanes lanes.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace parq {

constexpr int kObbLanes = 64;
// A convex 4-gon clipped by four half-planes has at most 8 vertices; inside flags that rounding makes inconsistent can add a few.
// Writes beyond the capacity are dropped (memory safety only: no geometry the tracker meets comes near it).
constexpr int kMaxV = 12;

struct Corners {
    double v[15];                           // corners 0..4, (x, y, z) each: all that the routine reads besides the NaN scan
};

__device__ __forceinline__ bool load_box(const double* p, Corners& c) {
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        const double x = p[i];
        nan |= x != x;
        if (i < 15) c.v[i] = x;
    }
    return nan;
}

constexpr double kCosHalfPi = 6.123233995736766e-17;

// f1_eval.canonical() of float32 world corners (a track store's, or a batch's): corners [4,0,1,5,7] (the first five of the
// re-ordering, all the routine reads), (x, y, z) -> (x, c y - z, y + c z); true when any of the 24 values is not finite
__device__ __forceinline__ bool load_canonical(const float* p, Corners& c) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        const float x = p[i];
        bad |= !(fabsf(x) <= 3.402823466e38f);
    }
    constexpr int face[5] = {4, 0, 1, 5, 7};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double x = (double)p[3 * face[i]], y = (double)p[3 * face[i] + 1], z = (double)p[3 * face[i] + 2];
        c.v[3 * i] = x;
        c.v[3 * i + 1] = kCosHalfPi * y - z;
        c.v[3 * i + 2] = y + kCosHalfPi * z;
    }
    return bad;
}

__device__ __forceinline__ double edge_len(const Corners& c, int i, int j) {
    const double dx = c.v[3 * i] - c.v[3 * j], dy = c.v[3 * i + 1] - c.v[3 * j + 1], dz = c.v[3 * i + 2] - c.v[3 * j + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// 0.5 * |sum x_i y_{i-1} - sum y_i x_{i-1}| of the 4-gon (corners 3, 2, 1, 0 in (x, z))
__device__ __forceinline__ double quad_area(const Corners& c) {
    const double x0 = c.v[9], y0 = c.v[11], x1 = c.v[6], y1 = c.v[8], x2 = c.v[3], y2 = c.v[5], x3 = c.v[0], y3 = c.v[2];
    const double s1 = ((x0 * y3 + x1 * y0) + x2 * y1) + x3 * y2;
    const double s2 = ((y0 * x3 + y1 * x0) + y2 * x1) + y3 * x2;
    return 0.5 * fabs(s1 - s2);
}

struct ObbPolyLds {
    double px[2][kMaxV][kObbLanes], py[2][kMaxV][kObbLanes];
};

// (3-D IoU, footprint IoU) of boxes c1, c2; nan1 / nan2: the box has a NaN corner (-> (0, 0)).  `lds`: the workgroup's polygon
// buffers, `lane` this lane's column of them.
__device__ __forceinline__ void obb_pair_iou(const Corners& c1, bool nan1, const Corners& c2, bool nan2, ObbPolyLds& lds, int lane,
                                             double& r3, double& r2) {
    double (&px)[2][kMaxV][kObbLanes] = lds.px;
    double (&py)[2][kMaxV][kObbLanes] = lds.py;
    r3 = 0.0;
    r2 = 0.0;
    if (!(nan1 || nan2)) {
        // subject = footprint of A, clip = footprint of B (corner 3, 2, 1, 0; x and z)
        int cur = 0, n = 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[0][k][lane] = c1.v[3 * (3 - k)];
            py[0][k][lane] = c1.v[3 * (3 - k) + 2];
        }
        const double a1 = quad_area(c1), a2 = quad_area(c2);
        bool empty = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (empty) continue;
            const int ka = 3 - ((e + 3) & 3), kb = 3 - e;                 // clip[e - 1] -> clip[e] as corner numbers
            const double ax = c2.v[3 * ka], ay = c2.v[3 * ka + 2], bx = c2.v[3 * kb], by = c2.v[3 * kb + 2];
            const double ex = bx - ax, ey = by - ay;
            const int dst = cur ^ 1;
            int m = 0;
            double qx = px[cur][n - 1][lane], qy = py[cur][n - 1][lane];   // prev
            bool q_in = ex * (qy - ay) > ey * (qx - ax);
            for (int k = 0; k < n; ++k) {
                const double cx = px[cur][k][lane], cy = py[cur][k][lane];
                const bool c_in = ex * (cy - ay) > ey * (cx - ax);
                if (c_in != q_in) {
                    const double dcx = ax - bx, dcy = ay - by;
                    const double dpx = qx - cx, dpy = qy - cy;
                    const double n1 = ax * by - ay * bx;
                    const double n2 = qx * cy - qy * cx;
                    const double inv = 1.0 / (dcx * dpy - dcy * dpx);
                    if (m < kMaxV) {
                        px[dst][m][lane] = (n1 * dpx - n2 * dcx) * inv;
                        py[dst][m][lane] = (n1 * dpy - n2 * dcy) * inv;
                    }
                    ++m;
                }
                if (c_in) {
                    if (m < kMaxV) {
                        px[dst][m][lane] = cx;
                        py[dst][m][lane] = cy;
                    }
                    ++m;
                }
                qx = cx; qy = cy; q_in = c_in;
            }
            n = m < kMaxV ? m : kMaxV;
            cur = dst;
            empty = n == 0;
        }
        bool zero = false;                                               // the host's early `return 0.0, 0.0`
        double inter_area = 0.0;
        if (!empty) {
            if (n < 3) {
                zero = true;
            } else {
                double s1 = 0.0, s2 = 0.0;
                double lx = px[cur][n - 1][lane], ly = py[cur][n - 1][lane];
                for (int k = 0; k < n; ++k) {
                    const double x = px[cur][k][lane], y = py[cur][k][lane];
                    s1 = s1 + x * ly;
                    s2 = s2 + y * lx;
                    lx = x; ly = y;
                }
                inter_area = 0.5 * fabs(s1 - s2);
                if (!(inter_area > 1e-14 * (a1 > a2 ? a1 : a2))) zero = true;
            }
        }
        if (!zero) {
            const double union_2d = (a1 + a2) - inter_area;
            r2 = union_2d > 0.0 ? inter_area / union_2d : __longlong_as_double(0x7ff8000000000000LL);
            const double top = c2.v[1] < c1.v[1] ? c2.v[1] : c1.v[1];                   // min(c1[0, 1], c2[0, 1])
            const double bottom = c2.v[13] > c1.v[13] ? c2.v[13] : c1.v[13];            // max(c1[4, 1], c2[4, 1])
            const double h = top - bottom;
            const double inter_vol = inter_area * (h > 0.0 ? h : 0.0);
            const double v1 = (edge_len(c1, 0, 1) * edge_len(c1, 1, 2)) * edge_len(c1, 0, 4);
            const double v2 = (edge_len(c2, 0, 1) * edge_len(c2, 1, 2)) * edge_len(c2, 0, 4);
            const double uni = (v1 + v2) - inter_vol;
            r3 = uni > 0.0 ? inter_vol / uni : 0.0;
        }
    }
}

}  // namespace parq
