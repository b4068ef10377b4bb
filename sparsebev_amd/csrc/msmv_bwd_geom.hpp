// The tap geometry of the sampler's backward, stated once: shared by the atomic kernels (msmv_sampling_bwd.hip) and the tap list of the
// atomics-free feature gradient (msmv_sampling_det.hip), so that both decide "is this level read" and "which pixel is this corner" from
// the same expressions (msmv_sampling_backward.cu:29-105 / the forward's msmv_sampling_forward.cu:41-66).
// The bilinear fractions differ between the two: msmv_sampling_bwd.hip forms each fraction and its complement with one explicit fma on
// the exact product (corner_frac there: one rounding each) and does not read lh / lw below; msmv_sampling_det.hip is built with
// -ffp-contract=off, so every product and difference of its tap list is individually rounded.  The two agree on every decision
// (lvl_ok, floors, corners: all of them read the fp32 product) and differ by at most one rounding in the bilinear fractions.
#pragma once
#include <cmath>

namespace sbev {

// loc.z -> camera index: round(z * (N - 1)), clamped to the rig (nm1 = (float)(N - 1))
__device__ __forceinline__ int msmv_view(float z, float nm1, int N) {
    int view = (int)roundf(z * nm1);
    view = min(max(view, 0), N - 1);
    return view;
}

// one sample point at one level: its pixel coordinates and whether the level is read at all (false for a NaN coordinate) ...
struct MsmvLevelPos {
    float h_im, w_im;
    bool lvl_ok;
};
__device__ __forceinline__ MsmvLevelPos msmv_level_pos(float x, float y, int H, int W) {
    MsmvLevelPos t;
    t.h_im = y * (float)(H - 1);
    t.w_im = x * (float)(W - 1);
    t.lvl_ok = t.h_im > -1.f && t.w_im > -1.f && t.h_im < (float)H && t.w_im < (float)W;
    return t;
}
// ... and its floors and bilinear fractions: corner (kh, kw) is pixel ((int)hf + kh, (int)wf + kw), inside the map or not
struct MsmvLevelFrac {
    float hf, wf, lh, lw;
};
__device__ __forceinline__ MsmvLevelFrac msmv_level_frac(const MsmvLevelPos& t) {
    MsmvLevelFrac f;
    f.hf = floorf(t.h_im);
    f.wf = floorf(t.w_im);
    f.lh = t.h_im - f.hf;
    f.lw = t.w_im - f.wf;
    return f;
}

}  // namespace sbev
