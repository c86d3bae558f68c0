// The corner arithmetic of the gather form of fused MSDA (msda_fused_lanes_kernel, msda.hip), stated once: from a sample's offset
// pair, its query's reference point and the level's map size to the four map positions the kernel LOADS and the terms of their
// bilinear weights.  Its second user is the decoder's row marking (dec_value_rows.hip), which must name exactly the rows that kernel
// loads: with one function the marked set IS the loaded set, not a second derivation of it.
//
// A load happens for all four corners of every sample, whatever its weight: a corner beyond the map's border is clamped onto the
// border and carries weight 0, and a sample outside the (-1, H) x (-1, W) acceptance window reads the map's first pixel (h_low =
// w_low = 0) with weight 0 -- 0 * finite = 0 is what the reference's zero padding computes, so those rows must hold finite values.
#pragma once
#include <hip/hip_runtime.h>

struct MsdaCorners {
    int yc0, yc1, xc0, xc1;                                  // clamped rows / columns of the four loads: (yc0|yc1) x (xc0|xc1)
    bool inside, y0, y1, x0, x1;                             // the sample is in the window; the corner row / column is on the map
    float lh, lw, hh, hw;                                    // bilinear terms: corner (y0, x0) weighs hh * hw, (y0, x1) hh * lw, ...
};

// (ox, oy): the sample's offsets in pixels; (rx, ry): the reference point in [0, 1] (already scaled by the level's valid ratio for
// padded batches); H x W the level map, Hf = (float)H, Wf = (float)W, rW = 1.f / Wf, rH = 1.f / Hf.
// off / W and off / H (ms_deform_attn.py:141-147) are divisions by per-level constants: q = x * (1/W) followed by one residual
// correction, r = fma(-q, W, x), q += r * (1/W).
__device__ __forceinline__ MsdaCorners msda_corners(const float ox, const float oy, const float rx, const float ry, const int H,
                                                    const int W, const float Hf, const float Wf, const float rW, const float rH) {
    MsdaCorners c;
    float qx = ox * rW, qy = oy * rH;
    qx = fmaf(fmaf(-qx, Wf, ox), rW, qx);
    qy = fmaf(fmaf(-qy, Hf, oy), rH, qy);
    const float lx = rx + qx, ly = ry + qy;
    const float h_im = ly * H - 0.5f, w_im = lx * W - 0.5f;
    c.inside = h_im > -1.f && w_im > -1.f && h_im < Hf && w_im < Wf;
    const float hf = floorf(h_im), wf = floorf(w_im);
    c.lh = h_im - hf;
    c.lw = w_im - wf;
    c.hh = 1.f - c.lh;
    c.hw = 1.f - c.lw;
    const int h_low = c.inside ? (int)hf : 0, w_low = c.inside ? (int)wf : 0;
    c.y0 = h_low >= 0;
    c.y1 = h_low + 1 <= H - 1;
    c.x0 = w_low >= 0;
    c.x1 = w_low + 1 <= W - 1;
    c.yc0 = c.y0 ? h_low : 0;
    c.yc1 = c.y1 ? h_low + 1 : H - 1;
    c.xc0 = c.x0 ? w_low : 0;
    c.xc1 = c.x1 ? w_low + 1 : W - 1;
    return c;
}
