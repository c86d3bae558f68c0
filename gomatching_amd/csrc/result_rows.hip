// Result rows: the per-instance work of `results.frame_lines` for ALL instances of a clip in one launch --
// the closed polygon of `boundary_to_polygon` truncated to integers, the CTC emit mask of `TextDecoder.decode`, and the
// minimum-area-rectangle SEARCH of `results.min_area_rect` (convex hull as `results._convex_hull` builds it, then the hull
// edge whose enclosing rectangle is smallest, first index winning ties).  Centre, size, angle and corners are NOT computed
// here: they need hypot / arctan2 / cos / sin, whose last bit differs between the host's libm and the device's, so the host
// finishes the one chosen edge per instance with the numpy expressions it has always used (results.finish_rows).
//
// Arithmetic contract: fp64, the host code's operations in the host code's order, each rounded once.  The pragma below
// keeps hipcc from fusing this file's own products and sums (it contracts by default); fp64 `/` and `sqrt` are the
// correctly rounded expansions.  The edge length is sqrt(ex*ex + ey*ey), as in the statement the tests carry.
//
// One wave64 per instance, one polygon point per lane (50 of 64), 4 instances per 256-thread block.  Latency-sized work:
// the sort is a rank-by-counting over LDS, the monotone chain is serial on lane 0, the edge search is one edge per lane.
// Inputs are expected finite (NaN / Inf coordinates have no defined row on the host either).
#include "common.h"

#pragma clang fp contract(off)

#define RR_PTS 50
#define RR_P 25
#define RR_WAVES 4

namespace {

struct RowsLds {
    double px[64], py[64];                  // polygon points, widened
    double sx[RR_PTS], sy[RR_PTS];          // unique points sorted by (x, y)
    int sidx[RR_PTS];                       // polygon index (first occurrence) of each sorted point
    int lo[RR_PTS], up[RR_PTS];             // monotone-chain stacks (indices into the sorted list)
    double hx[2 * RR_PTS], hy[2 * RR_PTS];  // hull points in `lower[:-1] + upper[:-1]` order
    int hp[2 * RR_PTS];                     // polygon index of each hull point
    int nh;
    unsigned mask_lo, mask_hi;
};

__device__ __forceinline__ double cross3(const RowsLds& L, int o, int a, int b) {
    return (L.sx[a] - L.sx[o]) * (L.sy[b] - L.sy[o]) - (L.sy[a] - L.sy[o]) * (L.sx[b] - L.sx[o]);
}

// Where instance k's operands come from.  `Packed`: instance k is row k of bd / recs / track_ids, as a clip's concatenated
// fields are (gom_result_rows_i32).  `Gathered`: a descriptor names a row of a ring of cap rows, the track id and the frame's
// scale pair, and the point is scaled here as scale_xy_kernel (elementwise.hip) scales it: one fp32 product per coordinate,
// rounded once (gom_result_rows_gather_i32).
struct Packed {
    const float* __restrict__ bd;
    const int64_t* __restrict__ recs;
    const int64_t* __restrict__ track_ids;
    __device__ __forceinline__ long row(long k) const { return k; }
    __device__ __forceinline__ void point(long k, const float* p, float& fx, float& fy) const {
        fx = p[0];
        fy = p[1];
    }
    __device__ __forceinline__ long long track_id(long k) const { return track_ids ? track_ids[k] : 0; }
};

struct Gathered {
    const float* __restrict__ bd;
    const int64_t* __restrict__ recs;
    const int* __restrict__ desc;                    // [n][GOM_RR_DESC_WORDS]
    long cap;
    __device__ __forceinline__ long row(long k) const {          // never outside the ring, whatever the descriptor holds
        const long r = desc[k * GOM_RR_DESC_WORDS];
        return r < 0 ? 0 : (r >= cap ? cap - 1 : r);
    }
    __device__ __forceinline__ void point(long k, const float* p, float& fx, float& fy) const {
        fx = p[0] * __int_as_float(desc[k * GOM_RR_DESC_WORDS + 3]);
        fy = p[1] * __int_as_float(desc[k * GOM_RR_DESC_WORDS + 4]);
    }
    __device__ __forceinline__ long long track_id(long k) const {
        const unsigned long long lo = (unsigned)desc[k * GOM_RR_DESC_WORDS + 1], hi = (unsigned)desc[k * GOM_RR_DESC_WORDS + 2];
        return (long long)(lo | (hi << 32));
    }
};

template <class Src>
__global__ __launch_bounds__(64 * RR_WAVES) void result_rows_kernel(const Src src, int n, int voc_size, int* __restrict__ out,
                                                                    int ld) {
    __shared__ RowsLds lds[RR_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long k = (long)blockIdx.x * RR_WAVES + w;
    const bool active = k < n;                       // a tail wave recomputes the last instance and stores nothing,
    const long kk = active ? k : (long)n - 1;        // so that every wave reaches every barrier
    const long src_row = src.row(kk);
    RowsLds& L = lds[w];
    int* row = out + kk * (long)ld;

    // ---- polygon: top points, then bottom points reversed (predictor.boundary_to_polygon)
    float fx = 0.f, fy = 0.f;
    if (lane < RR_PTS) {
        const int r = lane < RR_P ? lane : RR_PTS - 1 - lane;
        src.point(kk, src.bd + src_row * (RR_P * 4) + r * 4 + (lane < RR_P ? 0 : 2), fx, fy);
        if (active) {
            row[GOM_RR_POLY_I32 + 2 * lane] = (int)fx;                     // astype(int): truncation toward zero
            row[GOM_RR_POLY_I32 + 2 * lane + 1] = (int)fy;
            row[GOM_RR_POLY_F32 + 2 * lane] = __float_as_int(fx);
            row[GOM_RR_POLY_F32 + 2 * lane + 1] = __float_as_int(fy);
        }
    }
    const double x = fx, y = fy;
    L.px[lane] = x;
    L.py[lane] = y;

    // ---- CTC emit mask (TextDecoder.decode): a character that follows a blank or differs from its predecessor
    long long id = 0;
    if (lane < RR_P) id = src.recs[src_row * RR_P + lane];
    const long long prev = __shfl_up(id, 1);
    const bool is_char = lane < RR_P && id < (long long)voc_size - 1;
    const bool prev_char = lane > 0 && prev < (long long)voc_size - 1;
    const unsigned long long emit = __ballot(is_char && (!prev_char || id != prev));
    if (active && lane < RR_P) {
        const long long c = id < -2147483647LL - 1 ? -2147483647LL - 1 : (id > 2147483647LL ? 2147483647LL : id);
        row[GOM_RR_RECS + lane] = (int)c;
    }
    __syncthreads();

    // ---- sorted(set(points)): drop repeats (the first occurrence stays), rank the rest by (x, y)
    bool dup = false;
    for (int j = 0; j < RR_PTS; ++j)
        if (j < lane && L.px[j] == x && L.py[j] == y) dup = true;
    const unsigned long long uniq = __ballot(lane < RR_PTS && !dup);
    const int nu = __popcll(uniq);
    int rank = 0;
    for (int j = 0; j < RR_PTS; ++j) {
        const double qx = L.px[j], qy = L.py[j];
        if (((uniq >> j) & 1ull) && (qx < x || (qx == x && qy < y))) ++rank;
    }
    if (lane < RR_PTS && !dup) {
        L.sx[rank] = x;
        L.sy[rank] = y;
        L.sidx[rank] = lane;
    }
    __syncthreads();

    // ---- monotone chain, `cross <= 0` pops, hull = lower[:-1] + upper[:-1]; two or fewer points are their own hull
    if (lane == 0) {
        int nh = 0;
        unsigned long long hm = 0;
        if (nu <= 2) {
            for (int i = 0; i < nu; ++i) L.hp[nh++] = i;
        } else {
            int nl = 0, nup = 0;
            for (int i = 0; i < nu; ++i) {
                while (nl >= 2 && cross3(L, L.lo[nl - 2], L.lo[nl - 1], i) <= 0) --nl;
                L.lo[nl++] = i;
            }
            for (int i = nu - 1; i >= 0; --i) {
                while (nup >= 2 && cross3(L, L.up[nup - 2], L.up[nup - 1], i) <= 0) --nup;
                L.up[nup++] = i;
            }
            for (int i = 0; i < nl - 1; ++i) L.hp[nh++] = L.lo[i];
            for (int i = 0; i < nup - 1; ++i) L.hp[nh++] = L.up[i];
        }
        for (int i = 0; i < nh; ++i) {
            const int s = L.hp[i];
            L.hx[i] = L.sx[s];
            L.hy[i] = L.sy[s];
            L.hp[i] = L.sidx[s];
            hm |= 1ull << L.sidx[s];
        }
        L.nh = nh;
        L.mask_lo = (unsigned)hm;
        L.mask_hi = (unsigned)(hm >> 32);
    }
    __syncthreads();

    // ---- edge search: one hull edge per lane, then the first minimum over the wave
    const int nh = L.nh;
    double best = 0.0;
    int bi = -1;
    if (nh >= 2) {
        for (int i = lane; i < nh; i += 64) {
            const int i1 = i + 1 == nh ? 0 : i + 1;
            const double ex = L.hx[i1] - L.hx[i], ey = L.hy[i1] - L.hy[i];
            const double norm = sqrt(ex * ex + ey * ey);
            if (norm == 0) continue;
            const double ux = ex / norm, uy = ey / norm;
            double umax = 0, umin = 0, vmax = 0, vmin = 0;
            for (int j = 0; j < nh; ++j) {
                const double qx = L.hx[j], qy = L.hy[j];
                const double pu = qx * ux + qy * uy;
                const double pv = -qx * uy + qy * ux;
                if (j == 0) {
                    umax = umin = pu;
                    vmax = vmin = pv;
                } else {
                    if (pu > umax) umax = pu;
                    if (pu < umin) umin = pu;
                    if (pv > vmax) vmax = pv;
                    if (pv < vmin) vmin = pv;
                }
            }
            const double area = (umax - umin) * (vmax - vmin);
            if (bi < 0 || area < best) {
                best = area;
                bi = i;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (oi >= 0 && (bi < 0 || ob < best || (ob == best && oi < bi))) {
                best = ob;
                bi = oi;
            }
        }
    }
    if (active && lane == 0) {
        row[GOM_RR_EMIT] = (int)(unsigned)emit;
        row[GOM_RR_NHULL] = nh;
        row[GOM_RR_HULL_MASK] = (int)L.mask_lo;
        row[GOM_RR_HULL_MASK + 1] = (int)L.mask_hi;
        row[GOM_RR_EDGE] = bi >= 0 ? L.hp[bi] : -1;
        row[GOM_RR_EDGE + 1] = bi >= 0 ? L.hp[bi + 1 == nh ? 0 : bi + 1] : -1;
        row[GOM_RR_EDGE + 2] = 0;
        const long long t = src.track_id(kk);
        row[GOM_RR_TRACK_ID] = (int)(unsigned)((unsigned long long)t & 0xffffffffull);
        row[GOM_RR_TRACK_ID + 1] = (int)(unsigned)((unsigned long long)t >> 32);
    }
}

}  // namespace

extern "C" int gom_result_rows_i32(const float* bd, const int64_t* recs, const int64_t* track_ids, int n, int voc_size,
                                   int32_t* out, int ld, void* stream) {
    GOM_CHECK_ARG(n >= 0 && voc_size >= 2 && ld >= GOM_RESULT_ROWS_WORDS);
    if (n == 0) return GOM_OK;
    GOM_CHECK_ARG(bd && recs && out);
    hipLaunchKernelGGL(result_rows_kernel<Packed>, dim3((unsigned)cdiv((long)n, (long)RR_WAVES)), dim3(64 * RR_WAVES), 0,
                       (hipStream_t)stream, Packed{bd, recs, track_ids}, n, voc_size, (int*)out, ld);
    return gom_launch_status();
}

extern "C" int gom_result_rows_gather_i32(const float* bd, const int64_t* recs, long cap, const int32_t* desc, int n,
                                          int voc_size, int32_t* out, int ld, void* stream) {
    GOM_CHECK_ARG(n >= 0 && voc_size >= 2 && ld >= GOM_RESULT_ROWS_WORDS);
    if (n == 0) return GOM_OK;
    GOM_CHECK_ARG(cap >= 1 && bd && recs && desc && out);
    hipLaunchKernelGGL(result_rows_kernel<Gathered>, dim3((unsigned)cdiv((long)n, (long)RR_WAVES)), dim3(64 * RR_WAVES), 0,
                       (hipStream_t)stream, Gathered{bd, recs, (const int*)desc, cap}, n, voc_size, (int*)out, ld);
    return gom_launch_status();
}
