// Scoring, the DSText detection protocol: per frame, which detections lie on "don't care" regions, the greedy
// one-to-one matching of the care objects to the remaining detections, and the three counts the protocol's precision /
// recall / hmean are made of -- what `evaluate_method` of the reference's ICDAR15-style script does per frame with a full
// IoU matrix and a double loop.  Composing it from the pair compaction of score.hip works (two count / emit calls and a sweep
// on the host) but ships every pair above the threshold back only to reduce it to three integers per frame; here nothing but
// det_care [D], match [G] and frame_stats [F,3] leaves the device.  The rule is in include/gomatching_hip.h; the geometry of
// a pair is quad_geom.h's, the same device functions as the pair compaction, so a pair has the same bits in both.
//
// One wave64 owns a frame (the matching is sequential over the frame's ground truth and parallel over its detections: one
// wavefront's work), DM_WAVES frames per workgroup.
//   1. lanes stride over the frame's ground truth and count the don't-care objects (ballot + popcount).
//   2. per chunk of 64 detections, lane = detection: its hull stays in registers while the don't-care objects go by
//      (wave-uniform); a lane leaves when one covers it.  The ballot of the lanes that stay is the chunk's FREE MASK, kept in
//      a register of lane `chunk` -- 64 chunks, hence at most DM_MAX_DET = 4096 detections of a frame take part in the
//      matching (the host refuses longer frames before the launch; the kernel itself stays in bounds and leaves such
//      detections unmatched).
//   3. ground truth ascending, care objects only: chunks ascending, the chunk's free mask broadcast from its lane; the free
//      lanes compute the IoU, the lowest set bit of the ballot of the passing ones is the match, its bit leaves the mask, the
//      object is closed.  Chunks without a free detection cost one shuffle.  A bit matrix in LDS, built first and swept
//      afterwards, would compute all G x D values; this computes the pairs up to each object's first hit only, and the
//      sequential step is a ballot and a find-first-set either way.
// No atomics, no scratch for the clip polygon (per-lane LDS slots, see score.hip), every output word has one writer: the lane
// that owns the detection, lane 0 for an object and for the frame.  Nothing depends on the launch geometry.  Offsets are device
// data: every index made from them is clamped.
#include "quad_geom.h"

#pragma clang fp contract(off)

#define DM_WAVES 2
#define DM_MAX_DET 4096

namespace {

__device__ __forceinline__ bool boxes_meet(const HullBox& a, const HullBox& b) {
    return a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1;
}

__global__ __launch_bounds__(64 * DM_WAVES) void quad_det_match_kernel(
    const int* __restrict__ gt_quads, const int* __restrict__ det_quads, const int* __restrict__ gt_off,
    const int* __restrict__ det_off, const int* __restrict__ gt_care, int G, int D, int F, double iou_thr, double area_thr,
    int* __restrict__ det_care, int* __restrict__ match, int* __restrict__ frame_stats) {
    __shared__ ClipLds lds[DM_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long fl = (long long)blockIdx.x * DM_WAVES + w;
    if (fl >= F) return;                                               // no barrier below: the LDS slots are per lane
    const int f = (int)fl;
    ClipLds& L = lds[w];

    int g0 = gt_off[f], g1 = gt_off[f + 1], d0 = det_off[f], d1 = det_off[f + 1];
    g0 = g0 < 0 ? 0 : (g0 > G ? G : g0);
    g1 = g1 < g0 ? g0 : (g1 > G ? G : g1);
    d0 = d0 < 0 ? 0 : (d0 > D ? D : d0);
    d1 = d1 < d0 ? d0 : (d1 > D ? D : d1);
    const int ng = g1 - g0, nd = d1 - d0;

    // 1. the frame's don't-care objects
    int ndc = 0;
    for (int base = 0; base < ng; base += 64) {
        const int i = base + lane;
        ndc += __popcll(__ballot(i < ng && gt_care[g0 + i] == 0));
    }

    // 2. detections on don't-care regions; the free mask of chunk c in lane c
    unsigned long long avail = 0;
    int care_dets = 0;
    for (int base = 0, c = 0; base < nd; base += 64, ++c) {
        const int j = base + lane;
        bool care = j < nd;
        if (ndc > 0) {
            const Hull hd = quad_hull(det_quads + (long long)(d0 + (care ? j : nd - 1)) * 8);
            const HullBox bd = hull_box(hd);
            for (int i = 0; i < ng; ++i) {
                if (gt_care[g0 + i] != 0) continue;
                if (__ballot(care) == 0) break;                        // every detection of the chunk has left
                const Hull hg = quad_hull(gt_quads + (long long)(g0 + i) * 8);
                // bounding boxes that do not meet: the intersection is empty, the value 0 (never above a positive threshold)
                if (care && boxes_meet(hull_box(hg), bd) && pair_value(hg, hd, 1, L, lane) > area_thr) care = false;
            }
        }
        if (j < nd) det_care[d0 + j] = care ? 1 : 0;
        const unsigned long long b = __ballot(care);
        care_dets += __popcll(b);
        if (base < DM_MAX_DET && lane == c) avail = b;
    }

    // 3. greedy matching: ground truth ascending, the lowest free detection that passes
    const int nchunk = ((nd < DM_MAX_DET ? nd : DM_MAX_DET) + 63) >> 6;
    int matched = 0;
    for (int i = 0; i < ng; ++i) {
        int m = -1;
        if (gt_care[g0 + i] != 0) {
            const Hull hg = quad_hull(gt_quads + (long long)(g0 + i) * 8);
            const HullBox bg = hull_box(hg);
            for (int c = 0; c < nchunk; ++c) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane(__shfl((int)(unsigned)avail, c));
                const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane(__shfl((int)(unsigned)(avail >> 32), c));
                const unsigned long long a = ((unsigned long long)hi << 32) | lo;
                if (a == 0) continue;
                bool pass = false;
                if ((a >> lane) & 1ull) {                              // (a free bit is a detection below nd)
                    const Hull hd = quad_hull(det_quads + (long long)(d0 + c * 64 + lane) * 8);
                    if (boxes_meet(bg, hull_box(hd))) pass = pair_value(hg, hd, 0, L, lane) > iou_thr;
                }
                const unsigned long long b = __ballot(pass);
                if (b != 0) {
                    const int bit = __ffsll((long long)b) - 1;
                    m = c * 64 + bit;
                    if (lane == c) avail &= ~(1ull << bit);
                    break;
                }
            }
            matched += m >= 0;
        }
        if (lane == 0) match[g0 + i] = m;
    }
    if (lane == 0) {
        frame_stats[(long long)f * 3 + 0] = matched;
        frame_stats[(long long)f * 3 + 1] = ng - ndc;
        frame_stats[(long long)f * 3 + 2] = care_dets;
    }
}

}  // namespace

extern "C" int gom_quad_det_match_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                                      const int32_t* det_off, const int32_t* gt_care, int G, int D, int F, double iou_thr,
                                      double area_thr, int32_t* det_care, int32_t* match, int32_t* frame_stats, void* stream) {
    GOM_CHECK_ARG(G >= 0 && D >= 0 && F >= 0);
    GOM_CHECK_ARG(F > 0 || (G == 0 && D == 0));
    GOM_CHECK_ARG(iou_thr > 0.0 && iou_thr < 1.0);                     // (a NaN fails both)
    GOM_CHECK_ARG(area_thr > 0.0 && area_thr < 1.0);
    if (F > 0) GOM_CHECK_ARG(gt_off && det_off && frame_stats);
    if (G > 0) GOM_CHECK_ARG(gt_quads && gt_care && match);
    if (D > 0) GOM_CHECK_ARG(det_quads && det_care);
    if (F == 0) return GOM_OK;
    hipLaunchKernelGGL(quad_det_match_kernel, dim3((unsigned)cdiv((long)F, (long)DM_WAVES)), dim3(64 * DM_WAVES), 0,
                       (hipStream_t)stream, gt_quads, det_quads, gt_off, det_off, gt_care, G, D, F, iou_thr, area_thr,
                       (int*)det_care, (int*)match, (int*)frame_stats);
    return gom_launch_status();
}
