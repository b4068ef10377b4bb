// Shared host-side helpers of libsbev_hip.so (error slot, launch checks).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "../../include/sbev_hip.h"

namespace sbev {

void set_error(const char* fmt, ...);
int box_convention();    // SBEV_BOX_* (process-wide, like the reference's VERSION global)

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return SBEV_ELAUNCH;
    }
    return SBEV_OK;
}

#define SBEV_REQUIRE(cond, ...)                 \
    do {                                        \
        if (!(cond)) {                          \
            ::sbev::set_error(__VA_ARGS__);     \
            return SBEV_EINVAL;                 \
        }                                       \
    } while (0)

constexpr int kWave = 64;  // CDNA wavefront

// gemm_regtile.hip: the split-K partial-slab GEMM of sbev_linear_splitk_f32 for N % 128 == 0, K % 32 == 0
// (writes *slabs_written = splits / fold partial slabs: fold = regtile_fold(splits) is 2 when pairs of K splits are summed inside
// the kernel -- splits even and the SBEV_NO_SPLIT_FOLD switch unset -- else 1)
int regtile_fold(int splits);
int launch_splitk_regtile(const float* X, const float* W, float* slabs, int64_t M, int N, int K, int64_t ldx, int64_t ldw,
                          int splits, int fold, int* slabs_written, hipStream_t stream);

int regtile_plan(int64_t M, int N, int K);

// gemm.hip: the GEMM half of sbev_linear_splitk_f32 (*used partial slabs [used, M, N], not reduced)
int launch_splitk_slabs(const float* X, const float* W, int64_t M, int N, int K, int64_t ldx, int64_t ldw, int splits,
                        float* workspace, int* used, hipStream_t s);

int launch_splitk_slabs_bf16x3(const float* X, const uint16_t* W2, int64_t M, int N, int K, int64_t ldx, int splits,
                               float* workspace, int* used, hipStream_t s);

// grad_scale.hip: the scaled domain of the neck's and the backbone's backward.  Two launches on `s`: the four 32-bit words at `ws_head`
// ([0] 2^e  [1] 2^-e  [2] amax bits  [3] ticket) are cleared -- that launch is checked before anything else is enqueued -- then amax over
// the n tensors grads[i] of counts[i] elements (a multiple of 8; all fp32 or all fp16, 16-byte aligned) writes the pair.  Returns the status.
constexpr int kGradScaleMaxTensors = SBEV_FPN_MAX_OUT > 4 ? SBEV_FPN_MAX_OUT : 4;      // the neck's outputs, the backbone's four stage maps
int launch_grad_scale(const char* who, const void* const* grads, const long long* counts, int n, bool f32, void* ws_head, hipStream_t s);

// Every process-wide switch that influences what a decoder step enqueues, read ONCE per step (decoder.hip: read_switches) and handed
// down from there.  sbev_decoder_switches() copies this struct out field by field IN THIS ORDER (include/sbev_hip.h lists it), so a
// switch added here is part of every caller's graph key: int32_t fields only.
struct Switches {
    int32_t row_chain, chain_pair, fuse_sample_mix, fuse_l5_f32, query_order, lazy_scan_launch, out_fold, gen_weight_stationary,
        out8_min_rows, msmv_buffer_taps, box_convention;
};
bool msmv_buffer_taps_enabled();      // msmv_sampling.hip (read by the sampler launchers themselves: public entry points of their own)

// The feature pyramid + sample points that every sampler entry point is given (include/sbev_hip.h: sbev_msmv_fwd), as ONE value: the
// extern "C" functions build it from their positional arguments, decoder.hip once per step from its config.  Strides in elements.
struct PyramidDesc {
    const void* const* feats;       // [L] level bases
    const int32_t* hw;              // {H0, W0, H1, W1, ...}
    int L, feat_dtype, N, C, Q, P, gdiv;
    const int64_t* stride_bo;       // [L] per (sample-batch / gdiv) -- or per ring slot
    int64_t stride_g;
    const int64_t* stride_v;        // [L] per view
    int64_t stride_px;
    const float *loc, *weights;
    const int32_t* frame_slots;     // online frame ring (null: none): logical frame t lives in slot frame_slots[t] of n_slots
    int n_slots;
    const int32_t* slot_table;      // keyed frame pool (null: none): DEVICE int32 [B, T], frame t of sample b lives in slot slot_table[b*T + t]
                                    // of n_slots; at most one of frame_slots / slot_table

    // elements from the base of one (sample-batch) slab of level l to the last pixel of its last view; a limit adds its own tail
    int64_t slab_span(int l) const { return (int64_t)(N - 1) * stride_v[l] + ((int64_t)hw[2 * l] * hw[2 * l + 1] - 1) * stride_px; }
};
// what all three implementations ask first (`who`: the entry point, the prefix of every message)
inline int check_pyramid(const PyramidDesc& d, const char* who) {
    SBEV_REQUIRE(d.feats && d.hw && d.stride_bo && d.stride_v, "%s: null descriptor array", who);
    SBEV_REQUIRE(d.L >= 1 && d.L <= SBEV_MAX_LEVELS, "%s: L=%d not in 1..%d", who, d.L, SBEV_MAX_LEVELS);
    SBEV_REQUIRE(d.P >= 1 && d.P <= SBEV_MAX_POINTS, "%s: num_point exceed limits (P=%d > %d)", who, d.P, SBEV_MAX_POINTS);
    return SBEV_OK;
}
// the forward's and the fused launch's 16-byte taps: non-empty maps, strides in multiples of 4 elements (the backward asks neither)
inline int check_levels(const PyramidDesc& d, bool need_feats, const char* who) {
    for (int l = 0; l < d.L; ++l) {
        SBEV_REQUIRE(!need_feats || d.feats[l] != nullptr, "%s: feats[%d] is null", who, l);
        SBEV_REQUIRE(d.hw[2 * l] >= 1 && d.hw[2 * l + 1] >= 1, "%s: level %d has empty map", who, l);
        SBEV_REQUIRE(d.stride_bo[l] % 4 == 0 && d.stride_v[l] % 4 == 0, "%s: level %d strides must be multiples of 4 elements", who, l);
    }
    return SBEV_OK;
}
// the description -> a kernel argument block (MsmvArgs, BwdArgs: the same member names)
template <typename Args>
inline void fill_pyramid(Args& a, const PyramidDesc& d) {
    for (int l = 0; l < d.L; ++l) {
        a.feat[l] = static_cast<std::decay_t<decltype(a.feat[0])>>(d.feats[l]);
        a.H[l] = d.hw[2 * l];
        a.W[l] = d.hw[2 * l + 1];
        a.stride_bo[l] = d.stride_bo[l];
        a.stride_v[l] = d.stride_v[l];
    }
    a.stride_g = d.stride_g; a.stride_px = d.stride_px;
    a.loc = d.loc; a.w = d.weights;
    a.N = d.N; a.C = d.C; a.Q = d.Q; a.P = d.P; a.gdiv = d.gdiv;
}
// msmv_sampling.hip / mixing.hip: the implementations behind sbev_msmv_fwd[_ring / _pool] (B' sample batches) and the sbev_sample_mix_*
// (B samples; out_up 0: y is fp32, 2^e: fp16 pairs; order may be null), for callers that hold a description (decoder.hip)
int msmv_fwd(const PyramidDesc& d, int64_t Bp, float* out, int out_layout, int T, int G, sbev_stream_t stream);
int sample_mix(const PyramidDesc& d, int64_t B, int T, int G, const float* params, float* y, int Pout, float eps, float out_up,
               const int32_t* order, sbev_stream_t stream);

// gemm_bf16s.hip: the GEMM half of sbev_linear_splitk_bf16s / _f16s / _f16s_xdev as ONE description (the entry points build it from
// their positional arguments, decoder.hip once per layer): `used` partial slabs [used, M, 256], not reduced
struct SplitImageX {      // the X operand [M, ldx], exactly one form
    enum Form {
        F32_HOST_EXP,     // fp32, multiplied by 2^up_log2 and split in the kernel (bf16 modes: up_log2 = 0)
        F16_PAIRS,        // (fp16 hi, fp16 lo) of x 2^up_log2 in 32-bit slots, split by the producer (fp16 modes only)
        F32_DEV_SCALE     // fp32, dev_scale = {2^e, 2^-e} in device memory (fp16 modes only)
    } form;
    const float* x;
    int64_t ldx;
    int up_log2;
    const float* dev_scale;
};
struct OutProj {
    SplitImageX X;
    const uint16_t* Wp;
    const float* nscale;       // null in the bf16 modes; [256] per-column factors of the slabs (F32_DEV_SCALE: W's down-scales)
    int64_t M;
    int K, nimg;               // nimg 2 / 3: bf16x3 / bf16x6; 4 / 5: fp16 with 3 / 4 image products
    float* slabs;
    int out8_min_rows;         // the caller's reading of sbev_linear_out8_min_rows (F16_PAIRS only: rows from which the 256-row tiles run)
    // F16_PAIRS only, both null unless the caller WANTS the fold: the S chunk-workgroups of a row tile fold their slabs INSIDE the launch
    // into `folded` [M, 256] -- taken only where out_fold_shape_ok(M, K) (every workgroup of the launch resident at once) and the 128-row
    // kernel runs; fold_sync: one zeroed word per row tile (<= 64).  A row tile that never completes within the poll bound raises the
    // decoder's fault word.
    unsigned* fold_sync;
    float* folded;
};
struct OutProjResult {
    int used;                  // slabs to sum
    bool folded;               // the launch folded them: ONE slab, in OutProj::folded instead of OutProj::slabs
};
int launch_out_proj_slabs(const OutProj& o, OutProjResult* r, hipStream_t s);
bool out_fold_shape_ok(long long M, int K);
bool out_fold_enabled();              // sbev_decoder_out_fold's current setting
bool out_fold_install(void* host_word_dev);
long long out_fold_timeouts();
int out_fold_switch(int enable);
int out8_min_rows(int rows);
int out8_min_rows_setting();          // sbev_linear_out8_min_rows' current setting
int out_fold_drop(int enable);
bool gen_weight_stationary_enabled(); // sbev_linear_gen_weight_stationary's current setting

// layout.hip: on-demand relayout of the units the sample points mark (sample_point.hpp::TouchMap); need / done: one 4-byte word per tile
struct LazyPlan {
    int n_levels, R;
    long long n_images;
    int S[SBEV_MAX_LEVELS];
    unsigned tiles[SBEV_MAX_LEVELS];
    unsigned base[SBEV_MAX_LEVELS + 1];      // base[n_levels] = tiles of the pyramid
};
bool lazy_plan(int n_levels, const int32_t* hw, long long n_images, int channels, LazyPlan* p);
// one layer's move as ONE value: the stand-alone launch's argument, and the scan of layers 1..5 riding in the generator GEMM's prologue
// (gemm_bf16s.hip).  Sources: table[index[l]] (replayable step; src unused) or src[l]
struct LazyScan {
    const LazyPlan* plan;
    const void* const* table;
    const int32_t* index;
    const void* const* src;
    void* const* out;
    int esize;
    uint32_t *need, *done;
    bool last;
};
// gemm_bf16s.hip: the split-image generator GEMM Y [M, ldy] = X W^T + bias behind sbev_linear_bf16s_gen (nimg 2 / 3) and
// sbev_linear_f16s_gen (nimg 4 / 5) as ONE description (the entry points build it from their positional arguments, decoder.hip once
// per layer).  An operand is its image fragments WITH its fp16 scale (read in the fp16 modes only)
struct SplitFrags {
    const uint16_t* frags;     // [ceil(rows/32)][K/16][images][64][8] (sbev_pack_bf16s_frags / sbev_pack_f16s_frags)
    const float* scale;        // X: {2^ex, 2^-ex} in device memory; W: the [N] down-scales 2^-ew of its rows
};
struct GenGemm {
    SplitFrags X, W;
    const float* bias;         // [N] or null
    float* Y;
    int64_t M;
    int N, K;
    int64_t ldy;
    int relu, nimg;            // nimg 2 / 3: bf16x3 / bf16x6; 4 / 5: fp16 with 3 / 4 image products
    bool weight_stationary;    // the caller's reading of sbev_linear_gen_weight_stationary: that kernel runs where it is set AND gen_ws_shape_ok
    const LazyScan* scan;      // non-null: this layer's relayout scan in the kernel's prologue (weight-stationary kernel only)
    const uint32_t* skip_hdr;  // non-null: layer 0 of a step with a prefix cache (weight-stationary kernel only, never with scan): prefix_clean
};
bool gen_ws_shape_ok(int64_t M, int K, int64_t ldy, int nimg);
int launch_gen_gemm(const GenGemm& g, hipStream_t s);
int launch_lazy_relayout(const LazyScan& scan, bool first, hipStream_t s);      // first: the step's first move (every marked unit is new)

// row_chain.hip: the row-local op chains of a decoder layer as single launches (weights pre-packed: sbev_decoder_chain_pack)
bool row_chain_supported(const sbev_decoder_config& c);
bool row_chain_pays(long long rows);
int launch_chain_front(const sbev_decoder_config& c, const sbev_decoder_weights& w, const float* bbox, const float* feat, float* x,
                       float* qkvt, float eps, hipStream_t s, uint32_t* skip_hdr = nullptr);      // skip_hdr: see prefix_clean
// attention.hip: sbev_sasa_f32 for callers that hold a prefix cache (skip_hdr, mask == null only)
int launch_sasa(const float* qkvt, int64_t ld, const float* query_bbox, const double* pc_range, const uint8_t* mask, float* out, int B, int Q,
                int H, int head_dim, const uint32_t* skip_hdr, hipStream_t s);
int launch_chain_attn(const sbev_decoder_config& c, const sbev_decoder_weights& w, const float* att, const float* x, float* x1,
                      const float* bbox, const float* time_diff, const float* lidar2img, float* loc_bp, float* w_bp, float eps,
                      hipStream_t s, uint16_t* x1_frag = nullptr, const float* x1_scale = nullptr, uint32_t* pair_sync = nullptr,
                      const LazyPlan* touch = nullptr, uint32_t* touch_need = nullptr);
// project.hip: sbev_sample_and_project that also marks the relayout units its points read (touch != null)
int launch_sample_and_project(const float* query_bbox, const float* offset, int64_t ld_offset, const float* scale_logits, int64_t ld_logits,
                              const float* time_diff, const float* lidar2img, const double* pc_range, int B, int Q, int T, int N, int G, int P,
                              int L, float image_h, float image_w, float eps, float* loc_bp, float* weights_bp, const LazyPlan* touch,
                              uint32_t* touch_need, const int32_t (*hw)[2], hipStream_t stream);
int launch_chain_tail(const sbev_decoder_config& c, const sbev_decoder_weights& w, const float* slabs, int splits, const float* x1,
                      const float* bbox, const float* vel_div, float* x3, float* cls_out, float* box_out, int with_front, float* x,
                      float* qkvt, float eps, hipStream_t s, float* pair_x = nullptr, uint32_t* pair_sync = nullptr);
long long chain_pair_floats(long long rows);         // pair mode of the tail: exchange rows / arrival counters for `rows` rows
long long chain_pair_sync_words(long long rows);
long long chain_fold_sync_offset(long long rows);    // the out-projection's fold counters inside the same zeroed block (64 words)
bool chain_pair_enabled();                           // sbev_decoder_chain_pair's current setting (the in-launch hand-offs' master switch)
bool chain_pair_install(void* host_word_dev);        // the pair hand-off's end of the fault word (as out_fold_install / out_fold_timeouts)
long long chain_pair_timeouts();

// fault_word.hip: the decoder's sticky host-mapped fault word (the pair hand-off and the out-projection's fold report into it)
bool chain_fault_word_ready();                       // the host-mapped fault word is installed on the current device (never under capture: sbev_init)
void chain_pair_prepare();                          // install the pair tail's host-mapped fault word for the current device (outside any capture)
unsigned chain_pair_faults_pending();               // pair hand-offs that timed out and were not acknowledged (host word, no sync)

// gemm.hip: pairs of independent small ops of a decoder layer's tail in ONE launch (see pair_kernel)
bool small_linear_shape(int64_t M, int N, int K);
int launch_ln_and_linear(const float* X, const float* ln_w, const float* ln_b, float eps, int ln_relu, float* Yln, int64_t M, int N,
                         const float* Xg, const float* W, const float* bias, float* Yg, int Ng, int K, int relu, hipStream_t s);
int launch_ln_and_refine(const float* X, const float* ln_w, const float* ln_b, float eps, int ln_relu, float* Yln, int64_t M, int N,
                         const float* bbox, const float* reg, const float* vel_div, float* out, int Q, int code, hipStream_t s);
int launch_linear_and_lin3(const float* Xg, const float* W, const float* bias, float* Yg, int64_t M, int Ng, int K, int relu,
                           const float* x3, int64_t ldx3, const float* w3, const float* b3, const float* ln_w, const float* ln_b,
                           float eps, float* y3, int N3, hipStream_t s);

// gemm.hip: LayerNorm as the PROLOGUE of the small-tile linears that consume it (sbev_ln_linear_f32); a group launch
// shares one prologue between its problems (they all read the same X)
struct LnPrologue {
    const float* g;
    const float* b;
    float eps;
    int relu;
    const float* add;   // [M, 256] or null: added after LayerNorm (+ ReLU)
    float* xn;          // [M, 256]: the normalised rows, written once (problem 0's column-tile-0 workgroups)
};
int launch_linear_group(const sbev_linear_problem* probs, int n, const LnPrologue* ln, hipStream_t s);
bool ln_linear_fusable(int64_t M, int N, int K);

// attention_bwd_mfma.hip: the MFMA flash backward behind sbev_sasa_bwd_f32 (lse / dvec: [B, H, Q] scratch each)
int launch_sasa_bwd_mfma(const float* qkvt, int64_t ld, const float* bbox, const float* lo, const float* span, const uint8_t* mask,
                         const float* out, const float* grad_out, float* grad_qkvt, float* lse, float* dvec,
                         int B, int Q, int H, float scale, float p_drop, uint64_t seed, const uint64_t* seed_dev, hipStream_t s);

// optional HIP-event bracket around sampler launches (decoder.hip; switched by sbev_profile_sampler)
bool profile_begin(hipStream_t s, hipEvent_t* e0, hipEvent_t* e1, int kind = 0);
void profile_end(hipStream_t s, hipEvent_t e0, hipEvent_t e1, int kind = 0);   // kind: 0 sampler, 1 generator GEMM, 2 out-projection GEMM

// Prefix cache (decoder.hip): the header of the caller's cache block, 32-bit words.  The step's first launch (prefix_watch_kernel)
// rewrites every dirty word on every step; the three launches of layer 0 that read only the queries and the weights leave at once
// where none is set.
constexpr int PFX_ARMED = 0, PFX_FORCE = 1, PFX_HITS = 2, PFX_MISSES = 3, PFX_DIRTY = 4, PFX_NW = 64;
// nothing this step's queries changed: the OR of the dirty words, read with wave-uniform loads (hdr is a kernel argument); the caller
// returns on true before its first barrier, LDS-DMA request or store
__device__ __forceinline__ bool prefix_clean(const uint32_t* hdr) {
    const uint4* d = reinterpret_cast<const uint4*>(hdr + PFX_DIRTY);
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < PFX_NW / 4; ++i) {
        const uint4 v = d[i];
        acc |= (v.x | v.y) | (v.z | v.w);
    }
    return acc == 0;
}

// Sum over the 64 lanes of a wave without LDS traffic (ds_bpermute-based __shfl_xor costs an LDS round trip per
// step, which is pure exposed latency when only a few waves share a SIMD): 4 DPP steps reduce each 16-lane row
// (row_mirror, row_half_mirror, two quad permutes), then the 4 row sums are combined with v_readlane.
// Every lane receives the total.
__device__ __forceinline__ float wave_sum_dpp(float v) {
#define SBEV_DPP_F(x, ctrl) __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), ctrl, 0xf, 0xf, true))
    v += SBEV_DPP_F(v, 0x140);
    v += SBEV_DPP_F(v, 0x141);
    v += SBEV_DPP_F(v, 0x4e);
    v += SBEV_DPP_F(v, 0xb1);
#undef SBEV_DPP_F
    const int b = (int)__float_as_uint(v);
    const float r0 = __uint_as_float((unsigned)__builtin_amdgcn_readlane(b, 0));
    const float r1 = __uint_as_float((unsigned)__builtin_amdgcn_readlane(b, 16));
    const float r2 = __uint_as_float((unsigned)__builtin_amdgcn_readlane(b, 32));
    const float r3 = __uint_as_float((unsigned)__builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

}  // namespace sbev
