// Quad -> Bezier control points (python -m gomatching_amd.prepare): what datasets/vts.py:154-162 derives from a `poly` quad on
// every load -- polygon2rbox, the orientation test, cpt_bezier_pts -- for ALL quads of a dataset in one launch.  The rule is
// written out in include/gomatching_hip.h ("Quad -> Bezier control points"); tests/prepare_statement.py states it in plain
// Python and prepare.quad_bezier_host in numpy, and all three give the same 16 integers.
//
// Arithmetic contract: integers where the rule has integers (int64 cross products, shoelace sum and squared lengths), fp64
// for the rest with the statement's operations in the statement's order, each rounded once.  The pragma keeps hipcc from
// fusing this file's products and sums (it contracts by default); fp64 `/` and `sqrt` are the correctly rounded expansions.
// No trigonometry: the corners come straight from the edge's unit vector, so nothing depends on a libm's last bit.
//
// One lane per quad, everything in registers: no LDS, no atomics, no scratch.  The four points, the hull and the rectangle
// live in arrays that are only ever indexed by unrolled loop counters; an index that is data (the monotone chain's stack, a
// sort's permutation) goes through pick4, a chain of selects, and the two stacks are 2-bit fields of one register each.
// The quad is read as two 16-byte loads and the result written as four 16-byte stores.  Memory-sized work: 40 bytes in and
// 64 bytes out per quad against a few hundred VALU instructions, two fp64 divisions and a square root per hull edge.
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

template <typename T>
__device__ __forceinline__ T pick4(const T (&v)[4], int i) {
    return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

__device__ __forceinline__ void cswap(int& ax, int& ay, int& bx, int& by) {     // (a, b) -> sorted by (x, y)
    if (bx < ax || (bx == ax && by < ay)) {
        const int tx = ax, ty = ay;
        ax = bx, ay = by;
        bx = tx, by = ty;
    }
}

// One step of the monotone chain: pop while the top two and point i do not turn left, then push i.  The stack is `st`, newest
// entry in the low two bits, `sz` entries.  At most two pops: the stack holds three points or fewer.
__device__ __forceinline__ void chain_step(const int (&sx)[4], const int (&sy)[4], int i, unsigned& st, int& sz) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (sz >= 2) {
            const int a = (st >> 2) & 3, b = st & 3;
            const long long ox = pick4(sx, a), oy = pick4(sy, a);
            const long long cr = (pick4(sx, b) - ox) * (sy[i] - oy) - (pick4(sy, b) - oy) * (sx[i] - ox);
            if (cr <= 0) {
                st >>= 2;
                --sz;
            }
        }
    }
    st = (st << 2) | (unsigned)i;
    ++sz;
}

__global__ __launch_bounds__(256) void quad_bezier_kernel(const int* __restrict__ quads, const int* __restrict__ hw, int n,
                                                          int* __restrict__ out) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const i32x4 q0 = *reinterpret_cast<const i32x4*>(quads + k * 8);
    const i32x4 q1 = *reinterpret_cast<const i32x4*>(quads + k * 8 + 4);
    const i32x2 sz2 = *reinterpret_cast<const i32x2*>(hw + k * 2);
    const int H = sz2[0], W = sz2[1];

    // ---- 1. sorted(set(points)): a five-comparator network, then a repeat is equal to its left neighbour
    int sx[4] = {q0[0], q0[2], q1[0], q1[2]}, sy[4] = {q0[1], q0[3], q1[1], q1[3]};
    cswap(sx[0], sy[0], sx[1], sy[1]);
    cswap(sx[2], sy[2], sx[3], sy[3]);
    cswap(sx[0], sy[0], sx[2], sy[2]);
    cswap(sx[1], sy[1], sx[3], sy[3]);
    cswap(sx[1], sy[1], sx[2], sy[2]);
    bool valid[4];
    valid[0] = true;
    int nu = 1;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        valid[i] = sx[i] != sx[i - 1] || sy[i] != sy[i - 1];
        nu += valid[i] ? 1 : 0;
    }

    // ---- monotone chain, `cross <= 0` pops, hull = lower[:-1] + upper[:-1] (two distinct points come out as themselves)
    unsigned lo = 0, up = 0;
    int nl = 0, nup = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (valid[i]) chain_step(sx, sy, i, lo, nl);
#pragma unroll
    for (int i = 3; i >= 0; --i)
        if (valid[i]) chain_step(sx, sy, i, up, nup);
    const int nh = nu == 1 ? 1 : nl + nup - 2;
    double hx[4], hy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // entry j from the bottom of a stack of s entries sits at bits 2 (s - 1 - j)
        const int from_lo = (int)(lo >> (2 * ((nl - 1 - j) & 3))) & 3;
        const int from_up = (int)(up >> (2 * ((nup - 1 - (j - (nl - 1))) & 3))) & 3;
        const int idx = nu == 1 ? 0 : (j < nl - 1 ? from_lo : from_up);
        hx[j] = (double)pick4(sx, idx);
        hy[j] = (double)pick4(sy, idx);
    }

    // ---- 2. minimum-area rectangle over the hull's edges in hull order, the first strict minimum wins
    double bux = 0, buy = 0, bumin = 0, bumax = 0, bvmin = 0, bvmax = 0, best = 0;
    bool has = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (nh < 2 || i >= nh) continue;
        const bool wrap = i + 1 == nh;
        const double nx = (wrap || i == 3) ? hx[0] : hx[i == 3 ? 0 : i + 1];
        const double ny = (wrap || i == 3) ? hy[0] : hy[i == 3 ? 0 : i + 1];
        const double ex = nx - hx[i], ey = ny - hy[i];
        const double norm = sqrt(ex * ex + ey * ey);
        if (norm == 0) continue;
        const double ux = ex / norm, uy = ey / norm;
        double umax = 0, umin = 0, vmax = 0, vmin = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double pu = hx[j] * ux + hy[j] * uy;
            const double pv = hy[j] * ux - hx[j] * uy;
            if (j == 0) {
                umax = umin = pu;
                vmax = vmin = pv;
            } else if (j < nh) {
                if (pu > umax) umax = pu;
                if (pu < umin) umin = pu;
                if (pv > vmax) vmax = pv;
                if (pv < vmin) vmin = pv;
            }
        }
        const double area = (umax - umin) * (vmax - vmin);
        if (!has || area < best) {
            has = true;
            best = area;
            bux = ux, buy = uy, bumin = umin, bumax = umax, bvmin = vmin, bvmax = vmax;
        }
    }

    // ---- 3. corners from the unit vector: (umin,vmin), (umax,vmin), (umax,vmax), (umin,vmax), truncated toward zero
    int cx[4], cy[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double u = (c == 0 || c == 3) ? bumin : bumax, v = c < 2 ? bvmin : bvmax;
        cx[c] = nh == 1 ? sx[0] : (int)(u * bux - v * buy);
        cy[c] = nh == 1 ? sy[0] : (int)(u * buy + v * bux);
    }

    // ---- 4. get_tight_rect: stable sort by x (rank by counting), the two `>` comparisons on y, the clamp
    int px[4] = {0, 0, 0, 0}, py[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) rank += (cx[j] < cx[c] || (cx[j] == cx[c] && j < c)) ? 1 : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (rank == r) {
                px[r] = cx[c];
                py[r] = cy[c];
            }
    }
    const bool left = py[1] > py[0], right = py[3] > py[2];
    int rx[4] = {left ? px[0] : px[1], right ? px[2] : px[3], right ? px[3] : px[2], left ? px[1] : px[0]};
    int ry[4] = {left ? py[0] : py[1], right ? py[2] : py[3], right ? py[3] : py[2], left ? py[1] : py[0]};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        rx[c] = min(max(rx[c], 1), W - 1);
        ry[c] = min(max(ry[c], 1), H - 1);
    }

    // ---- 5. orientation: reversed iff the shoelace sum is negative
    long long s = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int d = (c + 1) & 3;
        s += (long long)rx[c] * ry[d] - (long long)rx[d] * ry[c];
    }
    if (s < 0) {
        int t;
        t = rx[0], rx[0] = rx[3], rx[3] = t;
        t = rx[1], rx[1] = rx[2], rx[2] = t;
        t = ry[0], ry[0] = ry[3], ry[3] = t;
        t = ry[1], ry[1] = ry[2], ry[2] = t;
    }

    // ---- 6. cpt_bezier_pts: the two longest edges (integer squared lengths, ties to the lower index), thirds truncated
    long long len2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long long dx = (long long)rx[(c + 1) & 3] - rx[c], dy = (long long)ry[(c + 1) & 3] - ry[c];
        len2[c] = dx * dx + dy * dy;
    }
    int e0 = 0, e1 = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) rank += (len2[j] > len2[c] || (len2[j] == len2[c] && j < c)) ? 1 : 0;
        if (rank == 0) e0 = c;
        if (rank == 1) e1 = c;
    }
    constexpr double T1 = 1.0 / 3.0, T2 = 2.0 / 3.0;
    int* row = out + k * 16;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int a = e == 0 ? e0 : e1, b = (a + 1) & 3;
        const int ax = pick4(rx, a), ay = pick4(ry, a), bx = pick4(rx, b), by = pick4(ry, b);
        const double dax = ax, day = ay, dbx = bx, dby = by;
        const i32x4 first = {ax, ay, (int)((1.0 - T1) * dax + T1 * dbx), (int)((1.0 - T1) * day + T1 * dby)};
        const i32x4 second = {(int)((1.0 - T2) * dax + T2 * dbx), (int)((1.0 - T2) * day + T2 * dby), bx, by};
        *reinterpret_cast<i32x4*>(row + 8 * e) = first;
        *reinterpret_cast<i32x4*>(row + 8 * e + 4) = second;
    }
}

}  // namespace

extern "C" int gom_quad_bezier_i32(const int32_t* quads, const int32_t* hw, int n, int32_t* out, void* stream) {
    GOM_CHECK_ARG(n >= 0);
    if (n == 0) return GOM_OK;
    GOM_CHECK_ARG(quads && hw && out);
    GOM_CHECK_ARG(((uintptr_t)quads & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)hw & 7) == 0);
    hipLaunchKernelGGL(quad_bezier_kernel, dim3((unsigned)cdiv((long)n, 256L)), dim3(256), 0, (hipStream_t)stream, quads, hw, n,
                       (int*)out);
    return gom_launch_status();
}
