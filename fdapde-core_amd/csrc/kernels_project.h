// kernels_project.h -- nearest-cell projection (fdapde_project): for every point the cell of the mesh closest to it, the closest point of that
// cell, the distance and the basis values there.  Stands in for the reference's Projection<Triangulation> (geometry/project.h) and
// Simplex::nearest (geometry/simplex.h:156-181), with the TRUE closest point of a cell (the reference drops the farthest vertex and recurses,
// which is not the closest point of an obtuse cell: DESIGN.md 13).
//
// One lane per point, as in k_eval_pointwise.  The search walks the bin grid of point location (dev_build_bin_grid) in Chebyshev shells
// around the bin of the point clamped into the grid box and stops once the best squared distance found is below a lower bound for every
// cell it has not seen; the shells are bounded by the grid, so it ends on every input.  No atomics, no LDS, no traffic between workgroups;
// every index of a local array is a compile-time constant after unrolling (no scratch).
#ifndef FDAPDE_KERNELS_PROJECT_H
#define FDAPDE_KERNELS_PROJECT_H

#include "kernels_assembly.h"

namespace fdapde_hip {

// ---- closest point of one cell: barycentric coordinates lam (all in [0, 1] exactly), the point q, the squared distance -------------------
// A vertex region returns the vertex itself (bit for bit) and lam = a unit vector; a point inside a cell of full dimension (M == N)
// returns p itself and 0.

// segment [a, b]: the clamped parameter.  The two ends are tested through d1 = ab . (p - a) <= 0 and d3 = ab . (p - b) >= 0, which are exact
// zeros for p = a and p = b (a quotient num / |ab|^2 is not); between them t = d1 / (d1 - d3)
template <int N> __device__ __forceinline__ double closest_on_segment(const double* p, const double* a, const double* b, double* lam, double* q) {
    double ab[N], d1 = 0, d3 = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) ab[c] = b[c] - a[c], d1 += ab[c] * (p[c] - a[c]), d3 += ab[c] * (p[c] - b[c]);
    if (d1 <= 0.0) {
        lam[0] = 1.0, lam[1] = 0.0;
#pragma unroll
        for (int c = 0; c < N; ++c) q[c] = a[c];
    } else if (d3 >= 0.0) {
        lam[0] = 0.0, lam[1] = 1.0;
#pragma unroll
        for (int c = 0; c < N; ++c) q[c] = b[c];
    } else {
        const double t = fmin(d1 / (d1 - d3), 1.0);
        lam[0] = 1.0 - t, lam[1] = t;
#pragma unroll
        for (int c = 0; c < N; ++c) q[c] = N == 1 ? p[c] : a[c] + t * ab[c];   // (an interior point of an interval is its own projection)
    }
    double d2 = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) d2 += (p[c] - q[c]) * (p[c] - q[c]);
    return d2;
}

// triangle (a, b, c) in R^2 or R^3: the Voronoi regions of its three vertices, three edges and its face, tested through dot products only
// (C. Ericson, Real-Time Collision Detection, 5.1.5); the region gives the barycentric coordinates directly
template <int N>
__device__ __forceinline__ double closest_on_triangle(const double* p, const double* a, const double* b, const double* c, double* lam, double* q) {
    double ab[N], ac[N];
    double d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0, d6 = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        ab[k] = b[k] - a[k], ac[k] = c[k] - a[k];
        const double ap = p[k] - a[k], bp = p[k] - b[k], cp = p[k] - c[k];
        d1 += ab[k] * ap, d2 += ac[k] * ap, d3 += ab[k] * bp, d4 += ac[k] * bp, d5 += ab[k] * cp, d6 += ac[k] * cp;
    }
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {   // vertex a
        lam[0] = 1.0, lam[1] = 0.0, lam[2] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) q[k] = a[k];
    } else if (d3 >= 0.0 && d4 <= d3) {   // vertex b
        lam[0] = 0.0, lam[1] = 1.0, lam[2] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) q[k] = b[k];
    } else if (d6 >= 0.0 && d5 <= d6) {   // vertex c
        lam[0] = 0.0, lam[1] = 0.0, lam[2] = 1.0;
#pragma unroll
        for (int k = 0; k < N; ++k) q[k] = c[k];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {   // edge ab
        const double v = fmin(fmax(d1 / (d1 - d3), 0.0), 1.0);
        lam[0] = 1.0 - v, lam[1] = v, lam[2] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) q[k] = a[k] + v * ab[k];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {   // edge ac
        const double w = fmin(fmax(d2 / (d2 - d6), 0.0), 1.0);
        lam[0] = 1.0 - w, lam[1] = 0.0, lam[2] = w;
#pragma unroll
        for (int k = 0; k < N; ++k) q[k] = a[k] + w * ac[k];
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {   // edge bc
        const double w = fmin(fmax((d4 - d3) / ((d4 - d3) + (d5 - d6)), 0.0), 1.0);
        lam[0] = 0.0, lam[1] = 1.0 - w, lam[2] = w;
#pragma unroll
        for (int k = 0; k < N; ++k) q[k] = b[k] + w * (c[k] - b[k]);
    } else {   // the face
        const double denom = 1.0 / (va + vb + vc);
        const double v = fmin(fmax(vb * denom, 0.0), 1.0), w = fmin(fmax(vc * denom, 0.0), 1.0);
        lam[0] = fmax(1.0 - v - w, 0.0), lam[1] = v, lam[2] = w;
#pragma unroll
        for (int k = 0; k < N; ++k) q[k] = N == 2 ? p[k] : a[k] + v * ab[k] + w * ac[k];   // (a point inside a planar triangle is its own projection)
    }
    double dd = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) dd += (p[k] - q[k]) * (p[k] - q[k]);
    return dd;
}

// tetrahedron: p itself where all four barycentric coordinates are >= 0, else the best of the closest points of its four faces (the first
// face in the order opposite-to-vertex 0, 1, 2, 3 on equal squared distances)
__device__ __forceinline__ double closest_on_tetrahedron(const double* p, const double* x0, const double* x1, const double* x2, const double* x3,
                                                         double* lam, double* q) {
    Geo<3> g;
    geo_from_vertices<3>(x0, x1, x2, x3, g);
    double xi[3], l0 = 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double v = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) v += g.invJ[r][c] * (p[c] - x0[c]);
        xi[r] = v, l0 -= v;
    }
    if (l0 >= 0.0 && xi[0] >= 0.0 && xi[1] >= 0.0 && xi[2] >= 0.0) {
        lam[0] = fmin(l0, 1.0), lam[1] = fmin(xi[0], 1.0), lam[2] = fmin(xi[1], 1.0), lam[3] = fmin(xi[2], 1.0);
        q[0] = p[0], q[1] = p[1], q[2] = p[2];
        return 0.0;
    }
    double fl[3], fq[3];
    double best = closest_on_triangle<3>(p, x1, x2, x3, fl, q);   // opposite to vertex 0
    lam[0] = 0.0, lam[1] = fl[0], lam[2] = fl[1], lam[3] = fl[2];
    double d = closest_on_triangle<3>(p, x0, x2, x3, fl, fq);   // ... vertex 1
    if (d < best) best = d, lam[0] = fl[0], lam[1] = 0.0, lam[2] = fl[1], lam[3] = fl[2], q[0] = fq[0], q[1] = fq[1], q[2] = fq[2];
    d = closest_on_triangle<3>(p, x0, x1, x3, fl, fq);   // ... vertex 2
    if (d < best) best = d, lam[0] = fl[0], lam[1] = fl[1], lam[2] = 0.0, lam[3] = fl[2], q[0] = fq[0], q[1] = fq[1], q[2] = fq[2];
    d = closest_on_triangle<3>(p, x0, x1, x2, fl, fq);   // ... vertex 3
    if (d < best) best = d, lam[0] = fl[0], lam[1] = fl[1], lam[2] = fl[2], lam[3] = 0.0, q[0] = fq[0], q[1] = fq[1], q[2] = fq[2];
    return best;
}

// The search.  Grid axis d has dims[d] bins of width 1 / inv_h[d] from lo[d]; an axis of zero extent has inv_h[d] == 0 and every cell in its
// bin 0 (dev_build_bin_grid): it is searched as ONE bin and contributes no bound -- every cell has the coordinate lo[d] there, so
// (p[d] - lo[d])^2 is part of every distance.
// The bound after shells 0 .. r.  Let p' be p clamped into the grid box B, t' its position in bin units, b its bin.  A cell is registered in every
// bin its bounding box touches, the box widened by 1e-9 of a bin (bin_range), so a cell seen in none of the bins of the cube [b - r, b + r] has
// an axis d on which all of it lies beyond the cube: above (b_d + r + 1) or below (b_d - r) in bin units, each by at least the 1e-9 it was
// widened by (the slack only moves an unseen cell farther; the bound gives the 1e-9 away and another 1e-9 for the rounding of the two
// positions).  Hence |x - p'| >= gap(r) = min over the axes and sides that still have bins of that axis distance, and since the cells lie in
// B, |p - x|^2 >= |p - p'|^2 + |p' - x|^2 >= |p - p'|^2 + gap(r)^2 for every point x of an unseen cell.  |p - p'| is taken 4 u max(|lo|, |hi|)
// short per axis (the box is known to the rounding of its corners) and the sum 8 u short.  The search stops when best < bound (strictly:
// a cell that ties with the best one has been seen) or when the cube covers the grid.
// Ties in the computed squared distance go to the lowest reference cell id.
template <int M, int R, int N>
static __global__ __launch_bounds__(256) void k_project(AsmArgs a, int64_t n_pts, const double* pts /*col-major n_pts x N*/, const double* lo,
                                                      const double* inv_h, const int32_t* dims, const int32_t* bin_ptr, const int32_t* bin_cells,
                                                      const int32_t* cell_i2e, int32_t* cell_out, double* proj /*col-major n_pts x N*/,
                                                      double* dist, double* values /*n_pts x NB or nullptr*/) {
    constexpr int NB = kNB<M, R>;
    constexpr int NP = N <= 2 ? 2 : 4;
    constexpr double kU = 1.1102230246251565e-16;
    constexpr double kBinSlack = 2e-9;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pts) return;
    double p[N], tc[N], ih[N];
    int b[N], nd[N], dm[N];
    double out2 = 0;
    int rmax = 0;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        p[d] = pts[(int64_t)d * n_pts + i];
        ih[d] = inv_h[d], dm[d] = dims[d];
        nd[d] = ih[d] > 0.0 ? dm[d] : 1;
        const double l = lo[d], h = ih[d] > 0.0 ? l + (double)nd[d] / ih[d] : l;
        const double t = (p[d] - l) * ih[d];
        tc[d] = fmin(fmax(t, 0.0), ih[d] > 0.0 ? (double)nd[d] : 0.0);
        const int bb = (int)floor(tc[d]);
        b[d] = bb > nd[d] - 1 ? nd[d] - 1 : bb;
        const double o = (p[d] < l ? l - p[d] : (p[d] > h ? p[d] - h : 0.0)) - 4.0 * kU * fmax(fabs(l), fabs(h));
        if (o > 0.0) out2 += o * o;
        const int far = b[d] > nd[d] - 1 - b[d] ? b[d] : nd[d] - 1 - b[d];
        rmax = far > rmax ? far : rmax;
    }
    double best = 1e300;
    int32_t best_ref = 0x7fffffff;
    double blam[M + 1], bq[N];
#pragma unroll
    for (int v = 0; v <= M; ++v) blam[v] = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) bq[d] = 0.0;
    const int bx = b[0], by = N >= 2 ? b[1] : 0, bz = N >= 3 ? b[2] : 0;
    const int nx = nd[0], ny = N >= 2 ? nd[1] : 1, nz = N >= 3 ? nd[2] : 1;
    const int64_t sx = dm[0], sy = N >= 2 ? dm[1] : 1;   // (the bin index runs over the grid's own dims, empty bins of a flat axis included)
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = bz - r < 0 ? 0 : bz - r, z1 = bz + r > nz - 1 ? nz - 1 : bz + r;
        const int y0 = by - r < 0 ? 0 : by - r, y1 = by + r > ny - 1 ? ny - 1 : by + r;
        const int x0 = bx - r < 0 ? 0 : bx - r, x1 = bx + r > nx - 1 ? nx - 1 : bx + r;
        for (int z = z0; z <= z1; ++z) {
            const bool zs = z - bz == r || bz - z == r;
            for (int y = y0; y <= y1; ++y) {
                // a row of the cube on the shell in y or z: all of its bins; any other row: its two end bins.  The lists of consecutive bins
                // are consecutive in bin_cells: one range per piece.
                const bool whole = zs || y - by == r || by - y == r;
                const int64_t row = ((int64_t)z * sy + y) * sx;
                for (int s = 0; s < 2; ++s) {
                    int xa, xb;
                    if (whole) {
                        if (s == 1) break;
                        xa = x0, xb = x1;
                    } else {
                        if (s == 1 && r == 0) break;
                        xa = xb = s == 0 ? bx - r : bx + r;
                        if (xa < 0 || xa > nx - 1) continue;
                    }
                    const int32_t k1 = bin_ptr[row + xb + 1];
                    for (int32_t k = bin_ptr[row + xa]; k < k1; ++k) {
                        const int32_t cell = bin_cells[k];
                        const int32_t* cv = a.cverts + (int64_t)cell * (M + 1);
                        double lam[M + 1], q[N], d2;
                        if constexpr (M == 1)
                            d2 = closest_on_segment<N>(p, a.vcoords + (int64_t)cv[0] * NP, a.vcoords + (int64_t)cv[1] * NP, lam, q);
                        else if constexpr (M == 2)
                            d2 = closest_on_triangle<N>(p, a.vcoords + (int64_t)cv[0] * NP, a.vcoords + (int64_t)cv[1] * NP,
                                                        a.vcoords + (int64_t)cv[2] * NP, lam, q);
                        else
                            d2 = closest_on_tetrahedron(p, a.vcoords + (int64_t)cv[0] * NP, a.vcoords + (int64_t)cv[1] * NP,
                                                        a.vcoords + (int64_t)cv[2] * NP, a.vcoords + (int64_t)cv[3] * NP, lam, q);
                        if (d2 <= best) {
                            const int32_t ref = cell_i2e[cell];
                            if (d2 < best || ref < best_ref) {
                                best = d2, best_ref = ref;
#pragma unroll
                                for (int v = 0; v <= M; ++v) blam[v] = lam[v];
#pragma unroll
                                for (int d = 0; d < N; ++d) bq[d] = q[d];
                            }
                        }
                    }
                }
            }
        }
        double gap = 1e300;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            if (ih[d] > 0.0) {
                if (b[d] + r < nd[d] - 1) gap = fmin(gap, ((double)(b[d] + r + 1) - tc[d] - kBinSlack) / ih[d]);
                if (b[d] - r > 0) gap = fmin(gap, (tc[d] - (double)(b[d] - r) - kBinSlack) / ih[d]);
            }
        }
        if (gap == 1e300) break;   // the cube covers the grid
        gap = fmax(gap, 0.0);
        if (best < (out2 + gap * gap) * (1.0 - 8.0 * kU)) break;
    }
    cell_out[i] = best_ref;
    dist[i] = sqrt(best);
#pragma unroll
    for (int d = 0; d < N; ++d) proj[(int64_t)d * n_pts + i] = bq[d];
    if (values != nullptr) {
        double val[NB];
        eval_basis_bary<M, R>(blam, val);
#pragma unroll
        for (int h = 0; h < NB; ++h) values[i * NB + h] = val[h];
    }
}

}  // namespace fdapde_hip
#endif
