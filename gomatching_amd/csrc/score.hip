// Scoring: the pairwise measure between the ground-truth and the detected quadrilaterals of a whole video -- what
// the DSText protocol's `distance_fn` (IoU) and `overlapping_fn` (intersection over the detection's area) compute per pair in a
// Python double loop -- as the count pass and the emit pass of a stream compaction, so that only the pairs above the threshold
// (a few per ground-truth object) travel back to the host's CLEAR-MOT bookkeeping (gomatching_amd/score.py).
//
// Geometry per pair, as tests/score_statement.py states it in numpy float64:
//   * convex hull of each 4-gon: the four points sorted by (x, y), then Andrew's monotone chain with 64-bit integer cross
//     products, popping on cross <= 0 -- any point order is accepted (bow-ties included), duplicate and collinear points
//     collapse.  For four points the chain reduces to: the first and the last sorted point are hull points, each of the two
//     middle points is one when it lies strictly off the line through them, and two on the same side keep the turn convex.
//     The hull lives in FOUR slots, counter-clockwise from the first sorted point, a dropped point's slot repeating a
//     neighbour: a repeated vertex adds nothing to a shoelace sum and is a clip edge that every point is inside of.
//   * either hull without area (twice the area, exact in int64) -> 0.
//   * the detection hull clipped by each edge of the ground-truth hull (Sutherland-Hodgman; inside = cross >= 0; a crossing at
//     prev + t (cur - prev), t = dp / (dp - dc)); at most 4 + 4 = 8 vertices; the shoelace area of the result.
// Arithmetic: fp64, the statement's operations in its order, each rounded once (the pragma keeps hipcc from contracting).
// Side tests are fp64 cross products: exact -- equal to the int64 value -- while the vertex is an integer one below 2^25.
//
// One wave64 per ground-truth object; its lanes stride over the detections of the object's frame.  The clip polygon (up to 8
// vertices, written at a running index) ping-pongs between two per-lane LDS slots [vertex][lane] -- as a private array it
// would be runtime-indexed and go to scratch; hulls and the four clip edges are unrolled over registers.  Counts and write
// positions come from a ballot and a popcount prefix: no atomics, so the output is bitwise reproducible and does not depend
// on the launch geometry.  Offsets, scan and total are device data the host cannot see: every index made from them is clamped.
// The per-pair device functions (hull, clip, measure) live in quad_geom.h, which score_det.hip shares.
#include "quad_geom.h"

#pragma clang fp contract(off)

#define SC_WAVES 2

namespace {

template <bool EMIT>
__global__ __launch_bounds__(64 * SC_WAVES) void quad_pairs_kernel(
    const int* __restrict__ gt_quads, const int* __restrict__ det_quads, const int* __restrict__ gt_off,
    const int* __restrict__ det_off, const int* __restrict__ gt_key, const int* __restrict__ det_key, int G, int D, int F,
    int measure, double threshold, int* __restrict__ counts, const long long* __restrict__ scan, long long total,
    int* __restrict__ out_det, double* __restrict__ out_val) {
    __shared__ ClipLds lds[SC_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long gl = (long long)blockIdx.x * SC_WAVES + w;
    if (gl >= G) return;                                               // no barrier below: the LDS slots are per lane
    const int g = (int)gl;
    ClipLds& L = lds[w];

    // the object's frame: the largest f with gt_off[f] <= g
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gt_off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    int d0 = det_off[lo], d1 = det_off[lo + 1];
    d0 = d0 < 0 ? 0 : (d0 > D ? D : d0);
    d1 = d1 < d0 ? d0 : (d1 > D ? D : d1);
    const int nd = d1 - d0;

    const Hull hg = quad_hull(gt_quads + (long long)g * 8);
    const int kg = gt_key[g];
    int gx0 = hg.x[0], gx1 = hg.x[0], gy0 = hg.y[0], gy1 = hg.y[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        gx0 = min(gx0, hg.x[i]);
        gx1 = max(gx1, hg.x[i]);
        gy0 = min(gy0, hg.y[i]);
        gy1 = max(gy1, hg.y[i]);
    }

    long long pos = EMIT ? scan[g] : 0;
    int kept = 0;
    for (int base = 0; base < nd; base += 64) {
        const int j = base + lane;
        bool keep = false;
        double v = 0.0;
        if (j < nd && det_key[d0 + j] == kg) {
            const Hull hd = quad_hull(det_quads + (long long)(d0 + j) * 8);
            int dx0 = hd.x[0], dx1 = hd.x[0], dy0 = hd.y[0], dy1 = hd.y[0];
#pragma unroll
            for (int i = 1; i < 4; ++i) {
                dx0 = min(dx0, hd.x[i]);
                dx1 = max(dx1, hd.x[i]);
                dy0 = min(dy0, hd.y[i]);
                dy1 = max(dy1, hd.y[i]);
            }
            // bounding boxes that do not meet: the intersection is empty, the value 0 (never above a positive threshold)
            if (dx0 <= gx1 && gx0 <= dx1 && dy0 <= gy1 && gy0 <= dy1) v = pair_value(hg, hd, measure, L, lane);
            keep = v > threshold;
        }
        const unsigned long long b = __ballot(keep);
        if (EMIT) {
            const long long p = pos + __popcll(b & ((1ull << lane) - 1ull));
            if (keep && p >= 0 && p < total) {
                out_det[p] = j;
                out_val[p] = v;
            }
            pos += __popcll(b);
        } else {
            kept += __popcll(b);
        }
    }
    if (!EMIT && lane == 0) counts[g] = kept;
}

int check_args(const void* gt_quads, const void* det_quads, const void* gt_off, const void* det_off, const void* gt_key,
               const void* det_key, int G, int D, int F, long pairs, int measure, double threshold) {
    GOM_CHECK_ARG(G >= 0 && D >= 0 && F >= 0);
    GOM_CHECK_ARG(F > 0 || (G == 0 && D == 0));
    GOM_CHECK_ARG(measure == 0 || measure == 1);
    GOM_CHECK_ARG(threshold > 0.0 && threshold < 1.0);                 // (a NaN fails both)
    GOM_CHECK_ARG(pairs >= 0 && pairs <= 2147483647L && pairs <= (long)G * (long)D);
    if (F > 0) GOM_CHECK_ARG(gt_off && det_off);
    if (G > 0) GOM_CHECK_ARG(gt_quads && gt_key);
    if (D > 0) GOM_CHECK_ARG(det_quads && det_key);
    return GOM_OK;
}

}  // namespace

extern "C" int gom_quad_pairs_count_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                                        const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D,
                                        int F, long pairs, int measure, double threshold, int32_t* counts, void* stream) {
    const int rc = check_args(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, pairs, measure, threshold);
    if (rc != GOM_OK) return rc;
    if (G == 0) return GOM_OK;
    GOM_CHECK_ARG(counts);
    hipLaunchKernelGGL(quad_pairs_kernel<false>, dim3((unsigned)cdiv((long)G, (long)SC_WAVES)), dim3(64 * SC_WAVES), 0,
                       (hipStream_t)stream, gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, measure, threshold,
                       (int*)counts, (const long long*)nullptr, 0LL, (int*)nullptr, (double*)nullptr);
    return gom_launch_status();
}

extern "C" int gom_quad_pairs_emit_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                                       const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D,
                                       int F, long pairs, int measure, double threshold, const int64_t* scan, long total,
                                       int32_t* out_det, double* out_val, void* stream) {
    const int rc = check_args(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, pairs, measure, threshold);
    if (rc != GOM_OK) return rc;
    GOM_CHECK_ARG(total >= 0 && total <= pairs);
    if (G == 0 || total == 0) return GOM_OK;
    GOM_CHECK_ARG(scan && out_det && out_val);
    hipLaunchKernelGGL(quad_pairs_kernel<true>, dim3((unsigned)cdiv((long)G, (long)SC_WAVES)), dim3(64 * SC_WAVES), 0,
                       (hipStream_t)stream, gt_quads, det_quads, gt_off, det_off, gt_key, det_key, G, D, F, measure, threshold,
                       (int*)nullptr, (const long long*)scan, (long long)total, (int*)out_det, (double*)out_val);
    return gom_launch_status();
}
