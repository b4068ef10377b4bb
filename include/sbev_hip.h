/*
 * sbev_hip.h -- C ABI of libsbev_hip.so: the MI355X (gfx950) implementation of SparseBEV's
 * adaptive spatio-temporal sampling + adaptive mixing decoder hot path.
 *
 * This is the drop-in boundary.  Every entry point is plain C:
 * raw DEVICE pointers, sizes, an explicit hipStream_t (passed as void*), an int status.
 *   - 0 on success, a negative SBEV_E* code on failure; sbev_last_error() returns the message of the
 *     last failure on the calling thread.  No C++ exception crosses this boundary.
 *   - No hidden allocation and no synchronisation: outputs and workspaces are caller-allocated, all
 *     work is enqueued on `stream` (NULL = the legacy default stream, which is what the reference's
 *     `<<<grid, block>>>` launches use: models/csrc/msmv_sampling/msmv_sampling_forward.cu:290).
 *   - Stateless and thread-safe for distinct streams.
 *   - Feature addressing is 64-bit at the sample-batch level (base = b' * stride_bo, so pyramids beyond 2^31 elements
 *     work; the reference's 32-bit offsets overflow at B'*N*H*W*C >= 2^31: msmv_sampling_forward.cu:127).  The
 *     offset of a tap INSIDE one sample-batch slab, (N-1)*stride_v + (H*W-1)*stride_px + C, is 32-bit and
 *     host-checked (SBEV_EINVAL beyond 2^31 - 1), as are item / row counts (B'*Q < 2^31).
 * Reference interfaces replaced are cited per function as file:line inside the reference checkout.
 */
#ifndef SBEV_HIP_H
#define SBEV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBEV_ABI_VERSION 1
#define SBEV_MAX_LEVELS 5   /* c2345 and c23456 variants: models/csrc/msmv_sampling/msmv_sampling.cpp:362-369 */
#define SBEV_MAX_POINTS 32  /* MAX_POINT: models/csrc/msmv_sampling/msmv_sampling.cpp:3,125 */
#define SBEV_MAX_FRAMES 16  /* frames per sample in the online feature ring (the reference evicts its cache at 16: models/sparsebev.py:286-292) */

typedef void* sbev_stream_t; /* hipStream_t */

enum sbev_status {
    SBEV_OK = 0,
    SBEV_EINVAL = -1,  /* bad argument (the reference raises AT_ASSERTM -> RuntimeError: msmv_sampling.cpp:106-125) */
    SBEV_ELAUNCH = -2, /* hipLaunch / hipGetLastError failure (the reference only printf's: msmv_sampling_forward.cu:295-298) */
    SBEV_ENODEV = -3,  /* no gfx950 device visible */
    SBEV_EFAULT = -4   /* an EARLIER decoder step's result is invalid (a pair-mode hand-off timed out: sbev_decoder_chain_pair_faults) */
};

enum sbev_dtype { SBEV_F32 = 0, SBEV_BF16 = 1, SBEV_F16 = 2, SBEV_U8 = 3 };   /* SBEV_U8: the source of sbev_image_front only.  Otherwise: feature STORAGE types of the sampler (fp32 math throughout): bf16 and fp16 taps are widened exactly.
                                                                   * fp16 is what the reference's eval mode produces before its out_fp32 cast (val.py:115, models/sparsebev.py:46) */
enum sbev_gemm_mode {
    SBEV_GEMM_F32 = 0,      /* exact: f32-input MFMA */
    SBEV_GEMM_BF16X3 = 1,   /* opt-in 3 x bf16 split (rounds 1-2 kernels, gemm_bf16x3.hip) */
    SBEV_GEMM_BF16X6 = 2,   /* fp32-class: hi + mid + lo bf16 images, 6 products, fp32 accumulate (gemm_bf16s.hip) */
    SBEV_GEMM_BF16X3S = 3,  /* 3 x bf16 split on the gemm_bf16s.hip kernels */
    SBEV_GEMM_F16X3 = 4,    /* fp32-class: scaled fp16 hi + lo images, 3 products (hl, lh, hh), fp32 accumulate (gemm_bf16s.hip) */
    SBEV_GEMM_F16X4 = 5     /* the same with all 4 products */
};

/* Output layouts of the sampler. */
enum sbev_out_layout {
    SBEV_OUT_REF = 0, /* [B', Q, C, P]  -- what _ms_deform_attn_cuda_c2345_forward returns (msmv_sampling.cpp:136) */
    SBEV_OUT_MIX = 1  /* [B, Q, G, T*P, C] with b' = (b*T + t)*G + g, point index t*P + p -- the layout
                         sampling_4d hands to AdaptiveMixing (models/sparsebev_sampling.py:125-128), written
                         directly so the [B',Q,C,P] -> [B,Q,G,T*P,C] permute never touches HBM */
};

int sbev_abi_version(void);
const char* sbev_last_error(void);
/* Number of visible HIP devices whose arch is gfx950 (0 if none / no driver). */
int sbev_device_count(void);

/*
 * Box / rotation convention of the checkpoint, a process-wide switch like the reference's `VERSION` global
 * (models/utils.py:320-325, set from checkpoint['version'] in val.py:128-129): it changes the rotation sign of the sample
 * offsets (rotation_3d_in_axis, models/utils.py:66-77) and the box layout SparseBEVHead.get_bboxes returns
 * (models/sparsebev_head.py:472-476).  Read at launch time by sbev_sampling_front, sbev_sample_and_project,
 * sbev_decoder_forward and sbev_nms_free_decode (bottom_center != 0).  Default SBEV_BOX_V1_0_0.
 */
enum { SBEV_BOX_V1_0_0 = 0, SBEV_BOX_V0_17_1 = 1 };
int sbev_set_box_convention(int convention);
int sbev_get_box_convention(void);

/*
 * Multi-scale multi-view bilinear sampling, forward.
 * Replaces: _ms_deform_attn_cuda_c2345_forward / _ms_deform_attn_cuda_c23456_forward
 *           (models/csrc/msmv_sampling/msmv_sampling.cpp:98-210, kernels msmv_sampling_forward.cu:75-267)
 *           and their Python entry msmv_sampling() (models/csrc/wrapper.py:87-93).
 *
 *   out[b',q,c,p] = sum_l w[b',q,p,l] * bilinear(feat_l[b', view, :, :, c]; y*(H_l-1), x*(W_l-1))
 *   view = round(loc.z*(N-1)); align_corners=True; a level contributes only if -1 < h_im < H_l and
 *   -1 < w_im < W_l; each of the 4 corners is zero outside the map.
 *
 * feats[l]      device pointer of level l (fp32 or bf16 per feat_dtype), channel-last.  Element offset of
 *               (b', view, h, w, c) = (b'/gdiv)*stride_bo[l] + (b'%gdiv)*stride_g + view*stride_v[l]
 *                                     + (h*W_l + w)*stride_px + c.
 *               The reference layout [B',N,H,W,C] is gdiv=1, stride_bo=N*H*W*C, stride_v=H*W*C, stride_px=C.
 *               A zero-copy NHWC pyramid [B*T, N, H, W, G*C] (no regroup copy) is
 *               gdiv=G, stride_bo=N*H*W*G*C, stride_g=C, stride_v=H*W*G*C, stride_px=G*C.
 * hw            host int32 [L][2] = (H_l, W_l)
 * loc           device fp32 [B',Q,P,3] = (x, y in [0,1], view/(N-1));  weights device fp32 [B',Q,P,L]
 * out           device fp32, layout per out_layout; T and G are only read for SBEV_OUT_MIX (B' = B*T*G)
 * Constraints: 1 <= L <= 5, 1 <= P <= 32, C % 4 == 0.
 */
int sbev_msmv_fwd(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                  int64_t Bp, int N, int C, int Q, int P,
                  int gdiv, const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                  const float* loc, const float* weights, float* out,
                  int out_layout, int T, int G, sbev_stream_t stream);

/*
 * sbev_msmv_fwd over an ONLINE FRAME RING (streaming inference).
 * Replaces: the per-call `torch.cat` of cached per-frame features (models/sparsebev.py:297-303) plus the decoder's
 *           regroup copy (models/sparsebev_transformer.py:73-85): features of every frame stay where they were
 *           written -- level l is ONE resident NHWC buffer [B, n_slots, N, H_l, W_l, G*C] -- and logical frame t
 *           (0 = current, T-1 = oldest) of sample batch b' = (b*T + t)*G + g is read from slot frame_slots[t].
 *           Per step only the newest frame's 6 images are relayouted into the slot of the evicted frame.
 * Same arguments as sbev_msmv_fwd except: stride_slot[l] = elements between consecutive slots (N*H_l*W_l*G*C);
 * gdiv must equal G; frame_slots = host int32 [T], values in [0, n_slots); 1 <= T <= SBEV_MAX_FRAMES.
 */
int sbev_msmv_fwd_ring(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                       int64_t Bp, int N, int C, int Q, int P,
                       int gdiv, const int64_t* stride_slot, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                       const float* loc, const float* weights, float* out,
                       int out_layout, int T, int G, const int32_t* frame_slots, int n_slots, sbev_stream_t stream);

/*
 * sbev_msmv_fwd over a KEYED FRAME POOL: the ring's resident buffers [B, n_slots, N, H_l, W_l, G*C], with the mapping (sample b, logical
 * frame t) -> slot in DEVICE memory instead of the kernel arguments: slot_table_dev = device int32 [B, T], frame t of sample b is read
 * from slot slot_table_dev[b*T + t] of sample b.
 * Replaces: the file-name keyed cache of simple_test_online (models/sparsebev.py:255-321): every sample has its own row (streams at
 *           different phases of different scenes share a batch), a frame that appears twice in a window is ONE slot read twice (so
 *           n_slots < T is legal), and the table's ADDRESS is what a captured launch holds -- refresh its contents in place and one
 *           hipGraph serves every step.
 * Same arguments as sbev_msmv_fwd_ring except the table; gdiv must equal G, 1 <= T <= SBEV_MAX_FRAMES, n_slots >= 1.  The table is read
 * by the kernel (one scalar load per wave and item): the host cannot validate it, so an entry outside [0, n_slots) is CLAMPED to the
 * nearest end -- a bad table reads the wrong frame, never memory outside the buffers.  Results are bit-identical to sbev_msmv_fwd on a
 * dense pyramid holding the same frames.
 */
int sbev_msmv_fwd_pool(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                       int64_t Bp, int N, int C, int Q, int P,
                       int gdiv, const int64_t* stride_slot, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                       const float* loc, const float* weights, float* out,
                       int out_layout, int T, int G, const int32_t* slot_table_dev, int n_slots, sbev_stream_t stream);

/* sbev_msmv_fwd / _ring / _pool gather through raw BUFFER loads whenever every level's (sample-batch) slab is below 2 GiB: an out-of-map
 * bilinear corner is an out-of-range buffer offset, answered with zeros by the hardware and never read -- the reference's semantics
 * (msmv_sampling_forward.cu:47-66) also for Inf / NaN border pixels.  Larger slabs take 64-bit global loads + a select (same
 * results).  sbev_msmv_buffer_taps(0) forces that path (tests, A/B; env SBEV_MSMV_NO_BUF=1); returns the previous setting. */
int sbev_msmv_buffer_taps(int enable);


/*
 * Multi-scale multi-view bilinear sampling, backward (fp32 features).
 * Replaces: _ms_deform_attn_cuda_c2345_backward / _c23456_backward (models/csrc/msmv_sampling/msmv_sampling.cpp:212-360,
 *           kernels msmv_sampling_backward.cu:29-361) = MSMVSamplingC2345.backward (models/csrc/wrapper.py:51-61).
 * Same feature addressing as sbev_msmv_fwd.  grad_feats[l] (fp32, same layout as feats[l]) is ACCUMULATED into with
 * float atomics -- the caller zero-fills it (the reference's host code does `zeros_like`, :244-249).
 * grad_out [B',Q,C,P]; grad_loc [B',Q,P,3] (x, y scaled by (W_l-1), (H_l-1) like :102-104; the view component is
 * written as 0) and grad_weights [B',Q,P,L] are fully overwritten, without atomics.  A point with a non-finite x or y (NaN, +-Inf)
 * reads no level, like the reference's (:170): its grad_loc and grad_weights rows are exactly 0 and it writes no feature gradient.
 */
int sbev_msmv_bwd(const void* const* feats, void* const* grad_feats, const int32_t* hw, int L,
                  int64_t Bp, int N, int C, int Q, int P,
                  int gdiv, const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                  const float* loc, const float* weights, const float* grad_out,
                  float* grad_loc, float* grad_weights, sbev_stream_t stream);

/*
 * Projection of 3-D sample points into all T*N cameras, camera-hit mask, first-hit view selection.
 * Replaces: the front half of sampling_4d (models/sparsebev_sampling.py:49-114) and its DUMP taps (:82-86).
 *
 * BIT-EXACT contract (vs. the reference's native-PyTorch path on CPU): homogeneous coordinates are
 * ((m0*x + m1*y) + m2*z) + m3 with separately rounded fp32 multiplies and adds (no FMA), followed by two
 * IEEE divisions (by max(homo, eps), then by image_w / image_h);
 * valid = homo > eps && 0 < v < 1 && 0 < u < 1; view = first valid view, 0 if none.
 *
 * sample_points device fp32 [B,Q,T,G*P,3] (metres);  lidar2img device fp32 [B,T*N,4,4] (image index t*N+n)
 * loc_bp        device fp32 [B*T*G, Q, P, 3] = (u, v, view/(N-1)) -- the sampler's `loc` operand
 * dump_uvh      optional (may be NULL) device fp32 [B,T,N,Q,G*P,3] = (u, v, max(homo,eps))   (DUMP tap)
 * dump_valid    optional device uint8 [B,T,N,Q,G*P]                                          (DUMP tap)
 * i_view        optional device int32 [B,T,Q,G*P]
 */
int sbev_project_select(const float* sample_points, const float* lidar2img,
                        int B, int Q, int T, int N, int G, int P,
                        float image_h, float image_w, float eps,
                        float* loc_bp, float* dump_uvh, uint8_t* dump_valid, int32_t* i_view,
                        sbev_stream_t stream);

/*
 * Sample-point generation and scale-weight softmax (everything in SparseBEVSampling.inner_forward between
 * the two Linear layers and sampling_4d).
 * Replaces: make_sample_points (models/sparsebev_sampling.py:8-24), decode_bbox (models/bbox/utils.py:63-77),
 *           rotation_3d_in_axis v1.0.0 (models/utils.py:49-84), the velocity warp and the level softmax
 *           (models/sparsebev_transformer.py:279-300), and the weight reorder of sampling_4d (:117-119)
 *           INCLUDING its (b,g,t)-vs-(b,t,g) flattening quirk.
 *
 * query_bbox    device fp32 [B,Q,10] (cx,cy,cz in [0,1], log w,l,h, sin, cos, vx, vy)
 * offset        device fp32 [B*Q, ld_offset]: first G*P*3 columns = output of the sampling_offset Linear
 * scale_logits  device fp32 [B*Q, ld_logits]: first G*P*L columns = output of the scale_weights Linear (pre-softmax)
 *               (row strides let both live in ONE packed GEMM output: the two Linears are fused into N = G*P*(3+L))
 * time_diff     device fp32 [B,T];  pc_range host double [6] (x0,y0,z0,x1,y1,z1)
 * sample_points device fp32 [B,Q,T,G*P,3] (out; may be NULL)
 * weights_bp    device fp32 [B*G*T, Q, P, L] (out; may be NULL): row b' holds softmax(scale_logits)[b,q,g',p,:]
 *               with g' = ((b' % (T*G))) / T  -- the weights the reference actually applies to sample batch b'.
 */
int sbev_sampling_front(const float* query_bbox, const float* offset, int64_t ld_offset,
                        const float* scale_logits, int64_t ld_logits,
                        const float* time_diff, const double* pc_range,
                        int B, int Q, int T, int G, int P, int L,
                        float* sample_points, float* weights_bp, sbev_stream_t stream);

/*
 * nn.Linear on the matrix cores, exact fp32 (v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate).
 *   Y[m,n] = act( sum_k X[m,k] * W[n,k] + bias[n] ) + residual[m,n]
 * Replaces: every torch.nn.Linear / F.linear of the decoder layer (models/sparsebev_transformer.py:116-153,
 *           203,262-263,343-344,358,378; mmcv MultiheadAttention in/out projections and FFN, :7,125,202).
 * X [M,ldx], W [N,ldw] (both K-contiguous, 16-byte aligned, ld % 4 == 0), bias [N] or NULL,
 * residual [M,ldy] or NULL (added AFTER the activation, the `identity + out` form of mmcv FFN / MHA),
 * relu != 0 applies max(.,0) before the residual.
 */
int sbev_linear_f32(const float* X, const float* W, const float* bias, const float* residual, float* Y,
                    int64_t M, int N, int K, int64_t ldx, int64_t ldw, int64_t ldy, int relu,
                    sbev_stream_t stream);
/* Which kernel sbev_linear_f32 launches for a call (a pure host function; the launcher switches on it): has_residual = residual != NULL,
 * y_bias_aligned = Y and a non-NULL bias are 16-byte aligned.  SBEV_EINVAL for M, N or K < 1 or ldy < N. */
enum sbev_linear_path {
    SBEV_LINEAR_STRIP = 0,     /* K == 256, N % 128 == 0, N >= 24576, ldy % 4 == 0, aligned, no residual: W strips stationary in registers */
    SBEV_LINEAR_RAGGED64 = 1,  /* K % 32 != 0: 64 x 64 tiles, the K tail staged element by element */
    SBEV_LINEAR_BIG128 = 2,    /* at least 256 tiles of 128 x 128 */
    SBEV_LINEAR_SMALL256 = 3,  /* K == 256: 32 x 32 tiles, K split over the 4 waves */
    SBEV_LINEAR_SMALL512 = 4,  /* K == 512: the same */
    SBEV_LINEAR_TILE64 = 5     /* every other K % 32 == 0: 64 x 64 tiles */
};
int sbev_linear_f32_path(int64_t M, int N, int K, int64_t ldy, int has_residual, int y_bias_aligned);

/*
 * Up to 3 independent small Linear layers (K = 256 or 512, same K) in ONE launch, e.g. the classification and the
 * regression branch of a decoder layer (models/sparsebev_transformer.py:174-175), which both consume the layer output.
 * Each problem has exactly the semantics of sbev_linear_f32.
 */
typedef struct sbev_linear_problem {
    const float* X; const float* W; const float* bias; const float* residual; float* Y;
    int64_t M; int32_t N, K; int64_t ldx, ldw, ldy; int32_t relu;
} sbev_linear_problem;
int sbev_linear_group_f32(const sbev_linear_problem* probs, int n, sbev_stream_t stream);

/*
 * Split-K variant for long reductions with a small output (AdaptiveMixing.out_proj: K = 32768, N = 256,
 * models/sparsebev_transformer.py:344,378), with the whole epilogue of that call site fused into the slab
 * reduction: + bias, optional ReLU, + residual (`query + out`, :379), optional LayerNorm(N) (norm2, :171).
 * workspace: device buffer of sbev_linear_splitk_workspace(M, N, splits) bytes.  N % 4 == 0, N <= 1024.
 */
/* Recommended number of K splits for sbev_linear_splitk_f32 at this shape (fills the GPU once). */
int sbev_linear_splitk_plan(int64_t M, int N, int K);
int64_t sbev_linear_splitk_workspace(int64_t M, int N, int splits);
int sbev_linear_splitk_f32(const float* X, const float* W, const float* bias, const float* residual,
                           const float* ln_w, const float* ln_b, float ln_eps, float* Y,
                           int64_t M, int N, int K, int64_t ldx, int64_t ldw, int relu,
                           int splits, float* workspace, sbev_stream_t stream);
/* Which kernel writes the partial slabs of sbev_linear_splitk_f32 for a call, and into *used (may be NULL) how many slabs the reducer
 * then sums (a pure host function; the launcher switches on it; reads the SBEV_NO_SPLIT_FOLD switch as the launcher does).
 * SBEV_EINVAL for M, N, K or splits < 1. */
enum sbev_linear_splitk_path_id {
    SBEV_SPLITK_REGTILE_FOLD2 = 0,    /* N % 128 == 0, K % 32 == 0, K >= 2048, splits <= K / 32 and even: register tiles, pairs of splits summed */
    SBEV_SPLITK_REGTILE_FOLD1 = 1,    /* the same with an odd splits: one slab per split */
    SBEV_SPLITK_SPLIT128 = 2,         /* every other K % 32 == 0: 128 x 128 tiles x ceil(K / (32 ceil(K / splits / 32))) <= splits slabs */
    SBEV_SPLITK_SPLIT128_RAGGED = 3   /* K % 32 != 0: the same tiles, the K tail staged element by element */
};
int sbev_linear_splitk_path(int64_t M, int N, int K, int splits, int32_t* used);

/* Row LayerNorm (+ optional ReLU) (+ optional add_after [M,N], e.g. query_feat + position encoding, :167) of X [M,N],
 * N % 4 == 0, N <= 1024.
 * Replaces: nn.LayerNorm(embed_dims) (+ nn.ReLU) at models/sparsebev_transformer.py:117-121,127-129,132-136,169-172. */
int sbev_layer_norm_f32(const float* X, const float* ln_w, const float* ln_b, float eps,
                        const float* add_after, float* Y, int64_t M, int N, int relu, sbev_stream_t stream);

/*
 * LayerNorm as the prologue of the Linear that consumes it:
 *   Xn = relu?(LayerNorm(X; ln_w, ln_b, eps)) (+ ln_add),   Y = act(Xn W^T + bias) (+ residual);  Xn is also stored.
 * Replaces: a norm immediately followed by a Linear on its output -- the position encoder's last LayerNorm + ReLU, the
 *           `query_feat + query_pos` add and the attention in_proj (models/sparsebev_transformer.py:117-121,166-169;
 *           mmcv MultiheadAttention in_proj), norm1 + the sampling offset / scale-weight Linear (:169-170,262-268), norm3 +
 *           the first Linear of the cls / reg branches (:172-175,132-147).
 * X, Xn [M, K] dense; ln_add [M, K] or NULL; W [N, ldw]; Y / residual [M, ldy].  One launch when K == 256, M <= 2048 and
 * the shape is one sbev_linear_f32 runs on its 32 x 32 small-tile kernel (each column tile re-normalises its rows, so the
 * prologue only pays while rows are few); otherwise sbev_layer_norm_f32 + sbev_linear_f32.  Pointers 16-byte aligned.
 */
int sbev_ln_linear_f32(const float* X, const float* ln_w, const float* ln_b, float ln_eps, int ln_relu,
                       const float* ln_add, float* Xn, const float* W, const float* bias, const float* residual,
                       float* Y, int64_t M, int N, int K, int64_t ldw, int64_t ldy, int relu, sbev_stream_t stream);

/*
 * sbev_sampling_front + sbev_project_select fused into one launch (what the decoder runtime uses): the intermediate
 * [B,Q,T,G*P,3] sample-point tensor never exists.  Same arithmetic in the same no-FMA translation unit, so loc_bp and
 * weights_bp are bit-identical to the two-call path (tested).  No DUMP outputs: use the two calls for the debug taps.
 */
int sbev_sample_and_project(const float* query_bbox, const float* offset, int64_t ld_offset,
                            const float* scale_logits, int64_t ld_logits,
                            const float* time_diff, const float* lidar2img, const double* pc_range,
                            int B, int Q, int T, int N, int G, int P, int L,
                            float image_h, float image_w, float eps,
                            float* loc_bp, float* weights_bp, sbev_stream_t stream);

/*
 * Adaptive mixing core: per (query, group)  y = relu(LN_[Pout,C]( S @ relu(LN_[Pin,C]( x @ M )) )).
 * Replaces: the two dynamic matmuls + F.layer_norm + ReLU of AdaptiveMixing.inner_forward
 *           (models/sparsebev_transformer.py:362-374).  The parameter generator (:358) and the out-projection
 *           (:377-379) around it are sbev_linear_f32 / sbev_linear_splitk_f32.
 * x       device fp32 [BQ, G, Pin, C]          (= the sampler's SBEV_OUT_MIX output)
 * params  device fp32 [BQ, G, C*C + Pout*Pin]  (per (q,g): M[C_in,C_out] then S[Pout,Pin]; the generator's output)
 * y       device fp32 [BQ, G, Pout, C]         (flattened [g][o][c] it is the out-projection's input row)
 * Built for C = 64, Pout = 128 (hard-coded in the reference: sparsebev_transformer.py:124); Pin % 4 == 0, Pin <= 120.
 */
int sbev_adaptive_mixing_f32(const float* x, const float* params, float* y,
                             int64_t BQ, int G, int Pin, int C, int Pout, float eps, sbev_stream_t stream);

/*
 * Scale-adaptive self attention core (flash-style; the [B,H,Q,Q] bias is never materialised).
 * Replaces: SparseBEVSelfAttention.inner_forward's distance/tau mask construction
 *           (models/sparsebev_transformer.py:215-227,236-248) and the softmax(QK^T/sqrt(d) + mask)V core of
 *           the mmcv/torch MultiheadAttention it calls (:228).
 * qkvt    device fp32 [B,Q,ld]: columns [0,HD*H) = q, [HD*H,2HD*H) = k, [2HD*H,3HD*H) = v (the packed in_proj
 *         output), [3HD*H, 3HD*H+H) = tau (gen_tau output; one GEMM with the 8 tau rows appended to in_proj)
 * query_bbox device fp32 [B,Q,10]; the box centres in metres, c = bbox[:, 0:2] * (range_max - range_min) + range_min
 *         (decode_bbox, models/bbox/utils.py:63-71), are formed inside the kernel from pc_range (host double [6])
 * mask    optional device uint8 [Q,Q], 1 = masked (-inf), the query-denoising mask (:224-225); NULL at inference
 * out     device fp32 [B,Q,H*HD] (input of the out-projection)
 * Built for head_dim = 32.
 */
int sbev_sasa_f32(const float* qkvt, int64_t ld, const float* query_bbox, const double* pc_range,
                  const uint8_t* mask, float* out, int B, int Q, int H, int head_dim, sbev_stream_t stream);

/*
 * Box refinement of one decoder layer.
 * Replaces: refine_bbox (models/sparsebev_transformer.py:155-160) with inverse_sigmoid (models/utils.py:87-102)
 *           and the velocity / time_diff division (:179-183).
 * out[:, 0:3] = sigmoid(reg[:, 0:3] + logit(clamp(query_bbox[:, 0:3]))), out[:, 3:] = reg[:, 3:],
 * out[:, 8:] /= vel_div[b] when vel_div != NULL (vel_div[b] = time_diff[b,1], values < 1e-5 replaced by 1).
 */
int sbev_refine_bbox(const float* query_bbox, const float* reg, const float* vel_div, float* out,
                     int B, int Q, int code_size, sbev_stream_t stream);

/* ---- detection head pre / post-processing -------------------------------------------------- */

/*
 * Decoder inputs at inference (no query denoising).
 * Replaces: SparseBEVHead.forward's `init_query_bbox.weight.clone()` + the eval branch of prepare_for_dn_input
 *           (models/sparsebev_head.py:70,123-126,209-211).
 * query_bbox[b] = init_query_bbox [Q,10];  query_feat[b,q] = [label_row (D-1 values = label_enc.weight[num_classes]), 0].
 */
int sbev_head_prepare(const float* init_query_bbox, const float* label_row, float* query_bbox, float* query_feat,
                      int B, int Q, int D, sbev_stream_t stream);

/*
 * Decoder boxes -> head output format.
 * Replaces: models/sparsebev_head.py:85-95 -- xyz * (pc_max - pc_min) + pc_min (two fp32 roundings each, as the
 *           reference's separate mul and add) and the column reorder to (cx, cy, w, l, cz, h, sin, cos, vx, vy).
 * bbox_norm / out: [n, 10] rows (n = num_layers * B * Q); in place (out == bbox_norm) is allowed.
 */
int sbev_head_denorm(const float* bbox_norm, const double* pc_range, float* out, int64_t n, sbev_stream_t stream);

/*
 * NMS-free box decoding of the last decoder layer.
 * Replaces: NMSFreeCoder.decode_single (models/bbox/coders/nms_free_coder.py:37-88) with denormalize_bbox
 *           (models/bbox/utils.py:26-47), per sample of NMSFreeCoder.decode (:90-111); with bottom_center != 0 also
 *           the gravity-centre -> bottom-centre shift of SparseBEVHead.get_bboxes (models/sparsebev_head.py:471).
 * cls_scores [B,Q,num_classes] logits, bbox_preds [B,Q,10] in the head format above.
 * Top max_num of the Q*num_classes sigmoid scores (score descending; equal scores: lower flat index first -- torch.topk
 * leaves that order unspecified), label = index % num_classes, box = bbox_preds[index / num_classes] denormalised to
 * (cx, cy, cz, w, l, h, rot, vx, vy); kept iff the centre lies inside post_center_range [6] (required, like the
 * reference) and, when use_score_threshold != 0, score > score_threshold.  Kept rows are compacted in order into
 * boxes [B,max_num,9] / scores [B,max_num] / labels [B,max_num] (int32), the rest zero-filled; count[b] = rows kept.
 * Limits: Q * num_classes <= 16384 (the per-sample sort lives in one CU's LDS), max_num <= 1024.
 */
int sbev_nms_free_decode(const float* cls_scores, const float* bbox_preds, int B, int Q, int num_classes, int max_num,
                         float score_threshold, int use_score_threshold, const double* post_center_range,
                         int bottom_center, float* boxes, float* scores, int32_t* labels, int32_t* count,
                         sbev_stream_t stream);

/* ---- detection head, training side (csrc/head_train.hip): fp32, no float atomics, bit-equal from run to run -------- */

/*
 * Decoder inputs in training: denoising queries in front of the matching queries, and the attention mask.
 * Replaces: SparseBEVHead.prepare_for_dn_input's training branch (models/sparsebev_head.py:124-207) with encode_bbox
 *           (models/bbox/utils.py:46-60): ~40 torch ops and two Python loops become one launch.
 * Ground truth of the batch concatenated sample-major: gt_boxes [G,9] (gravity centre, w, l, h, rot, vx, vy), gt_labels [G],
 * gt_offsets [B+1] (device; prefix sums of the per-sample counts).  Noise, one row per known query j = r*G + i (group r, gt i):
 * u_box [N*G,3] in [-1,1), u_lab [N*G] in [0,1), new_lab [N*G] in [0,num_classes).  single = the largest per-sample count,
 * pad = single*N.  At a fixed capacity (sbev_head_capacity_plan): single = the capacity per sample and G = B*capacity >= gt_offsets[B];
 * the rows of gt_boxes / gt_labels / the noise behind gt_offsets[B] are not read and their noised_label words are not written.  query_bbox [B,pad+Q,10], query_feat [B,pad+Q,D]: row (b, r*single + k) for the k-th gt of sample b holds
 * the centre c + (u * (wlh / 2)) * box_noise_scale, encoded with pc_range and clamped to [0,1], log(wlh), sin, cos, velocity;
 * feature [label_enc[lab'], 1] with lab' = new_lab if u_lab < label_noise_scale else the gt label (written to noised_label [N*G]).
 * A scale of 0 switches that noise off.  Unused pad rows are zero; rows pad.. are sbev_head_prepare's.
 * attn_mask [pad+Q, pad+Q] bytes, 1 = may not attend: a matching row sees no dn column, a dn row its own group's and all matching ones.
 */
int sbev_head_dn_prepare(const float* init_query_bbox, const float* label_enc, const float* gt_boxes, const int32_t* gt_labels,
                         const int32_t* gt_offsets, const float* u_box, const float* u_lab, const int32_t* new_lab,
                         const double* pc_range, float box_noise_scale, float label_noise_scale, int B, int Q, int D,
                         int num_classes, int G, int N, int single, float* query_bbox, float* query_feat,
                         int32_t* noised_label, uint8_t* attn_mask, sbev_stream_t stream);

/*
 * Backward of sbev_head_dn_prepare for its two parameters (ground truth and noise get no gradient).
 * Replaces: autograd through the embedding lookup, cat, repeat and index_put of models/sparsebev_head.py:126-127,175-193.
 * grad_init_query_bbox [Q,10] = sum over b of the matching rows of grad_query_bbox; grad_label_enc [num_classes+1, D-1]: row
 * num_classes = sum over all matching rows of grad_query_feat[..., :D-1], row c = sum over the known queries with noised label c.
 * One owner per output element, sums in a fixed order over the N * gt_offsets[B] known queries (not over N * G: the order does not
 * depend on a capacity behind gt_offsets[B]).
 */
int sbev_head_dn_prepare_bwd(const float* grad_query_bbox, const float* grad_query_feat, const int32_t* noised_label,
                             const int32_t* gt_offsets, int B, int Q, int D, int num_classes, int G, int N, int single,
                             float* grad_init_query_bbox, float* grad_label_enc, sbev_stream_t stream);

/*
 * Matching cost of every decoder layer and sample in one launch.
 * Replaces: HungarianAssigner3D.assign steps 2-3 up to the nan_to_num (models/bbox/assigners/hungarian_assigner_3d.py:54-74)
 *           with BBox3DL1Cost (models/bbox/match_costs/match_cost.py:6-27), normalize_bbox (models/bbox/utils.py:4-20) and
 *           mmdet's FocalLossCost, called per layer and sample by _get_target_single (models/sparsebev_head.py:301-311).
 * cls_scores / bbox_preds: [L,B,ld_rows,*] with the pointer at the first of the Q matching rows of each sample (ld_rows >= Q).
 * cost [L,B,Q,Gmax] = w_cls * (pos(p) - neg(p)) + w_reg * sum_k |pred_k*cw_k - ngt_k*cw_k|, nan -> 100, +inf -> 100, -inf -> -100;
 * columns g >= the sample's count are 0.
 */
int sbev_head_match_cost(const float* cls_scores, const float* bbox_preds, int64_t ld_rows, const float* gt_boxes,
                         const int32_t* gt_labels, const int32_t* gt_offsets, const float* code_weights, float w_cls,
                         float w_reg, float alpha, float gamma, int L, int B, int Q, int num_classes, int Gmax, float* cost,
                         sbev_stream_t stream);

/*
 * Rectangular linear sum assignment on the host (no GPU call): shortest augmenting paths (Jonker-Volgenant).
 * Replaces: scipy.optimize.linear_sum_assignment in HungarianAssigner3D.assign (hungarian_assigner_3d.py:80).
 * cost: row-major [n_rows, ld >= n_cols].  col_of_row [n_rows]: the column of each row, -1 for unmatched; min(n_rows, n_cols)
 * pairs at minimum total cost.  SBEV_EINVAL on a non-finite cost or ld < n_cols.
 */
int sbev_lsa_solve(const float* cost, int64_t ld, int n_rows, int n_cols, int32_t* col_of_row);

/*
 * The assignment table of a step from the host copy of sbev_head_match_cost's output (no GPU call).
 * Replaces: the per-layer, per-sample solver calls and index bookkeeping of hungarian_assigner_3d.py:80-91 / sparsebev_head.py:329-347.
 * cost [L,B,Q,Gmax], gt_counts [B] (host).  assign [L,B,Q]: -1 = background, g = index of the matched gt of that sample.
 */
int sbev_head_assign(const float* cost, const int32_t* gt_counts, int L, int B, int Q, int Gmax, int32_t* assign);

/*
 * The same table solved on the device: one launch, one workgroup per problem (l, b), no device -> host copy and no synchronisation,
 * so the launch can sit inside a captured graph.
 * Replaces: sbev_head_assign together with the copy of the costs to the host, the stream synchronisation in front of it and the
 *           upload of the table behind it (scipy.optimize.linear_sum_assignment on .cpu() costs in hungarian_assigner_3d.py:74-91).
 * It is sbev_lsa_solve's algorithm restated in parallel with the same fp64 arithmetic in the same order and the same tie rule (among
 * equally short columns the last free one in scan order, otherwise the first), so the table is sbev_head_assign's bit for bit.
 * cost [L,B,Q,Gmax] (device, as sbev_head_match_cost writes it), gt_offsets [B+1] (device): the counts are read there, and one that
 * is negative or above Gmax is clamped into 0..Gmax and flagged.  Only the Q x count block of a problem is read.
 * assign [L,B,Q] int32: -1 background, g = matched gt of that sample.
 * status [L*B] int32 (may be null): 0 solved; 1 non-finite cost in the block, a count out of range, or no feasible assignment:
 * that problem's row is all -1 and the other problems are untouched.
 * workspace: sbev_head_assign_device_workspace(L, B, Q, Gmax) bytes (-1 on bad sizes), 16-byte aligned; may be null where that is 0.
 * sbev_head_assign_device_plan(Q, Gmax): what the launch will do -- 0: the per-problem solver state (29 bytes per column, 13 per row)
 * stays in LDS, 1: it lives in the workspace, -1: bad sizes.  Both are pure host functions.
 * Checked before any GPU call: sizes >= 0, Q <= 32767, Q * Gmax < 2^31, null pointers at non-zero sizes; L*B*Q == 0 is SBEV_OK
 * without a launch.
 */
int64_t sbev_head_assign_device_workspace(int L, int B, int Q, int Gmax);
int sbev_head_assign_device_plan(int Q, int Gmax);
int sbev_head_assign_device(const float* cost, const int32_t* gt_offsets, int L, int B, int Q, int Gmax,
                            int32_t* assign, int32_t* status, void* workspace, sbev_stream_t stream);

/*
 * The training step's plan at a fixed ground-truth capacity, from the per-sample counts in gt_offsets on the device: one launch, no
 * host value follows the counts, so the launch can sit inside a captured graph whose ground truth changes between replays.
 * Replaces: prepare_for_dn_loss's gather indices (models/sparsebev_head.py:224-237) and the host arithmetic of num_total_pos /
 *           cls_avg_factor / num_tgt (:247,371-384,:239-275) that SparseBEVTrainHead.loss() does with numpy at a dynamic shape.
 * gt_offsets [B+1] (device).  count[b] = offsets[b+1] - offsets[b], clamped into 0..capacity for everything written here.
 * codes [B, N*capacity] int32: k at (b, r*capacity + k) for k < count[b], -2 elsewhere -- sbev_head_set_loss's codes of the denoising rows.
 * avg_factors [2,2] fp32: row 0 = (num_pos + num_neg * bg_cls_weight, num_pos) with num_pos = sum_b min(count[b], Q) and
 * num_neg = B*Q - num_pos; row 1 = (N * sum_b count[b]) twice.  Integer sums, the factors formed in double and rounded once.
 * status [1] int32: 0, or the sum of 1 (a count above capacity), 2 (offsets[0] != 0 or a negative count), 4 (offsets[B] > B*capacity).
 * One owner per output, plain stores, no atomics.  Checked before any GPU call: B, Q, capacity >= 0, N >= 1, B*N*capacity < 2^31,
 * null pointers (codes may be null where B*N*capacity == 0).
 */
int sbev_head_capacity_plan(const int32_t* gt_offsets, int B, int Q, int capacity, int N, double bg_cls_weight, int32_t* codes,
                            float* avg_factors, int32_t* status, sbev_stream_t stream);

/*
 * AdamW with global-norm gradient clipping, a static loss scale and the skip of a non-finite step over a list of fp32 tensors: three
 * launches per step on `stream` -- no host synchronisation, no device -> host copy, no atomics -- so the step can be captured.
 * Replaces: the optimizer and optimizer_config of the training recipe (configs/r50_nuimg_704x256.py:186-200: AdamW, grad_clip
 *           max_norm 35, static loss scale 512 with the step skipped on overflow), i.e. torch.optim.AdamW.step,
 *           torch.nn.utils.clip_grad_norm_ and the overflow check of mmcv's Fp16OptimizerHook.
 * Tensor addresses and sizes are host arrays that travel BY VALUE in the launches' argument blocks (at most SBEV_OPTIM_MAX_TENSORS per
 * call; a longer list is several calls of _sumsq and _adamw, each with its own slice of `partials`).  What changes between steps is
 * read from device memory:
 *   hyper  [SBEV_OPTIM_HYPER_FLOATS] fp32: [0] inv_scale (1 / loss scale), [1] max_norm (<= 0: no clipping), [2] hold (non-zero: the
 *          step is skipped whatever the norm), [3] unused, then per group g at [4 + 4g]: lr, weight_decay, lr multiplier, unused.
 *   header SBEV_OPTIM_HEADER_BYTES, 8-byte aligned, written by sbev_optim_finish only: double beta1^t, beta2^t (running products; the
 *          caller initialises both to 1); int64 step t, skipped; float norm, clip, 1 - beta1^t, sqrt(1 - beta2^t); int32 skip; 12 unused.
 * A chunk is SBEV_OPTIM_CHUNK consecutive elements of one tensor.  sbev_optim_plan (pure host): out[0] = chunks of the list,
 * out[1] = calls of _sumsq / _adamw that launch (groups of SBEV_OPTIM_MAX_TENSORS tensors with any element), out[2] = bytes of `partials`.
 *
 * sbev_optim_sumsq:  partials[c] = sum over chunk c of (g * inv_scale)^2, summed in fp64 in a fixed order, rounded once.
 * sbev_optim_finish: norm = sqrt(sum of the n_partials partials in index order, fp64); clip = min(1, max_norm / (norm + 1e-6));
 *                    skip = norm not finite, or hold.  Not skipped: t += 1 and the beta powers advance.  Skipped: skipped += 1 only.
 * sbev_optim_adamw:  with g' = g * inv_scale * clip and lr = lr_g * multiplier_g:  p *= 1 - lr * wd;  m += (g' - m) * (1 - beta1);
 *                    v = v * beta2 + g' * g' * (1 - beta2);  p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps),
 *                    every operation rounded to fp32 on its own.  Nothing is stored when the header says skip.
 * Bit-reproducible: neither the chunking nor any order of summation depends on the device or on the alignment of a tensor.
 * Checked before any GPU call (SBEV_EINVAL): null arrays / pointers, n > SBEV_OPTIM_MAX_TENSORS, a negative numel, a base that is not
 * 4-byte aligned, a group outside 0..n_groups-1, n_groups > SBEV_OPTIM_MAX_GROUPS, betas outside [0, 1).  A list without elements is
 * SBEV_OK without a launch.  p / m / v of the list must not overlap each other.
 */
#define SBEV_OPTIM_CHUNK 8192
#define SBEV_OPTIM_MAX_TENSORS 64
#define SBEV_OPTIM_MAX_GROUPS 16
#define SBEV_OPTIM_HYPER_FLOATS 68
#define SBEV_OPTIM_HEADER_BYTES 64
int sbev_optim_plan(const int64_t* numel, int n, int64_t* out);
int sbev_optim_sumsq(const void* const* g, const int64_t* numel, int n, const float* hyper, float* partials, sbev_stream_t stream);
int sbev_optim_finish(const float* partials, int64_t n_partials, const float* hyper, void* header, double beta1, double beta2,
                      sbev_stream_t stream);
int sbev_optim_adamw(void* const* p, const void* const* g, void* const* m, void* const* v, const int64_t* numel, const int32_t* group,
                     int n, int n_groups, double beta1, double beta2, double eps, const float* hyper, const void* header,
                     sbev_stream_t stream);

/* Bytes of workspace PER LAYER for sbev_head_set_loss (-1 on bad sizes). */
int64_t sbev_head_set_loss_workspace(int B, int rows);

/*
 * Sigmoid focal loss + L1 loss of all decoder layers and their gradients for unit upstream gradient: two launches.
 * Replaces: loss_single / dn_loss_single with the target construction of _get_target_single and prepare_for_dn_loss's gather
 *           (models/sparsebev_head.py:224-275,301-402) and mmdet's FocalLoss (sigmoid) and L1Loss.
 * cls_scores / bbox_preds: [L,B,ld_rows,*] with the pointer at the first of the `rows` rows of each sample.  codes: int32
 * [B,rows] per layer (layer l at codes + l*code_layer_stride; 0 = one table for all layers): -2 skip the row, -1 background,
 * g >= 0 target gt g of sample b (class gt_labels, box normalize_bbox(gt_boxes)).  A code at or above the sample's gt count, or below
 * -2, is a caller's error: it is treated as -2 (the row is skipped, its gradients are zero) so that nothing is read out of bounds.
 * loss [L,2]: scale * nan_to_num(w_focal * sum focal / max(A_cls,1)), scale * nan_to_num(w_l1 * sum_{g >= 0, target finite}
 * sum_k |pred_k - ngt_k| * cw_k / max(A_box,1)) with A_cls, A_box = avg_factors[0..1] read on the device; loss_finite [L,2] = 1
 * where the value was finite before nan_to_num.  grad_cls [L,B,rows,NC], grad_bbox [L,B,rows,10]: d loss / d input, every
 * element written by one thread.  workspace: L * sbev_head_set_loss_workspace(B, rows) bytes.
 */
int sbev_head_set_loss(const float* cls_scores, const float* bbox_preds, int64_t ld_rows, const int32_t* codes,
                       int64_t code_layer_stride, const float* gt_boxes, const int32_t* gt_labels, const int32_t* gt_offsets,
                       const float* code_weights, const float* avg_factors, float w_focal, float alpha, float gamma,
                       float w_l1, float scale, int L, int B, int rows, int num_classes, float* loss, float* loss_finite,
                       float* grad_cls, float* grad_bbox, float* workspace, sbev_stream_t stream);


/*
 * Batched NCHW -> NHWC relayout of one pyramid level: in [n_images, channels, hw] -> out [n_images, hw, channels].
 * Replaces: the permute + contiguous feature regroup of the decoder (models/sparsebev_transformer.py:73-85); the
 *           per-group split of that regroup is not needed (sbev_msmv_fwd addresses group g as a channel slice).
 */
int sbev_nchw_to_nhwc_f32(const float* in, float* out, int64_t n_images, int channels, int hw, sbev_stream_t stream);

/* Staging launches of a REPLAYABLE step (sparsebev_amd/runtime.py StepGraphs): the source pointer is table[index], read on the
 * device when the kernel starts.  `table` is a device array of 64-bit pointers that the host refreshes before every launch of the
 * captured graph, so a caller that passes newly allocated tensors of the same shape every step -- how the reference's loops feed
 * model(...) (timing.py:77-96, val.py) -- replays ONE graph.  Sources must be 16-byte aligned.
 * sbev_nchw_to_nhwc_f32_indirect = sbev_nchw_to_nhwc_f32 with in = table[index]; sbev_copy_indirect: nseg <= 4 contiguous copies in one
 * launch, segment k = nbytes[k] bytes from table[index[k]] to dst[k] (index, dst, nbytes: host arrays). */
int sbev_nchw_to_nhwc_f32_indirect(const void* const* table, int index, float* out, int64_t n_images, int channels, int hw,
                                   sbev_stream_t stream);
/* All levels of one pyramid in ONE launch (round 5): level l = [n_images, channels, hw[l]] from table[index[l]] to out[l]; the coarse
 * levels' few tiles run in the tail of the finest level's instead of in short launches of their own.  Needs hw[l] % 4 == 0, channels % 4
 * == 0 and 16-byte aligned buffers (SBEV_EINVAL otherwise: launch the per-level form). */
int sbev_nchw_to_nhwc_f32_multi_indirect(const void* const* table, int n_levels, const int32_t* index, float* const* out,
                                         int64_t n_images, int channels, const int32_t* hw, sbev_stream_t stream);
/* The same relayouts for 2-byte channels -- bf16 or fp16 feature STORAGE (enum sbev_dtype; bytes are moved, never interpreted): what
 * an fp16 backbone (the reference's eval mode, val.py:115, before the out_fp32 cast of models/sparsebev.py:46) or a bf16 neck emits
 * goes to the sampler's layout at half the traffic of the fp32 relayout.  128-channel x 64-pixel tiles; any sizes (channels % 8,
 * hw % 4 and 8- / 16-byte alignment select the vector path). */
int sbev_nchw_to_nhwc_b16(const void* in, void* out, int64_t n_images, int channels, int hw, sbev_stream_t stream);
int sbev_nchw_to_nhwc_b16_indirect(const void* const* table, int index, void* out, int64_t n_images, int channels, int hw,
                                   sbev_stream_t stream);
int sbev_copy_indirect(const void* const* table, int nseg, const int32_t* index, void* const* dst, const int64_t* nbytes,
                       sbev_stream_t stream);

/* The decoder step's LAST launch (round 5): the stacked outputs cls [n_cls floats] / bbox [n_box floats] copied out of the runtime's
 * buffers into the caller's, nan_to_num'ed on the way (NaN -> 0, +-Inf -> +-FLT_MAX, every other value bit for bit) -- both tensors
 * in one launch.  Replaces: the two torch.nan_to_num launches of SparseBEVTransformer.forward (models/sparsebev_transformer.py:35-36)
 * and, for a replayed step graph, the clones out of the graph's buffers.  _indirect: destinations = table[idx_cls] / table[idx_box]
 * (device pointer table, see above), so that a captured step writes straight into tensors allocated per call.  Sources and
 * destinations must not overlap. */
int sbev_finish_outputs(const float* cls_src, const float* box_src, float* cls_dst, float* box_dst, int64_t n_cls, int64_t n_box,
                        sbev_stream_t stream);
int sbev_finish_outputs_indirect(const void* const* table, int idx_cls, int idx_box, const float* cls_src, const float* box_src,
                                 int64_t n_cls, int64_t n_box, sbev_stream_t stream);


/*
 * y = relu(LayerNorm(x[:, 0:3] @ w^T + b)): the first half of the position encoder
 * (nn.Linear(3, D), nn.LayerNorm(D), nn.ReLU: models/sparsebev_transformer.py:116-119).  x [M, ldx], w [N,3].
 */
int sbev_linear3_ln_relu_f32(const float* x, int64_t ldx, const float* w, const float* b,
                             const float* ln_w, const float* ln_b, float eps, float* y,
                             int64_t M, int N, sbev_stream_t stream);

/* Split-K slab reducer: Y = LayerNorm?( relu?( sum_z slabs[z] + bias ) + residual ), slabs [splits, M, N]. */
int sbev_splitk_reduce_f32(const float* slabs, int splits, const float* bias, const float* residual,
                           const float* ln_w, const float* ln_b, float ln_eps, float* Y,
                           int64_t M, int N, int relu, sbev_stream_t stream);

/*
 * Opt-in "3 x bf16" Linear for the two large GEMMs of AdaptiveMixing (models/sparsebev_transformer.py:358,378):
 * both fp32 operands are split into bf16 (hi, lo) pairs and Y = Xhi.Whi + Xhi.Wlo + Xlo.Whi is accumulated in
 * fp32 on v_mfma_f32_32x32x16_bf16.  fp32-class accuracy (about 2^-16 relative per product; 1.2e-5 max abs error on
 * the reference's AdaptiveMixing fixture), ~3-5x the speed of the exact-fp32 MFMA path; NOT bit-equal to fp32 math,
 * hence never the default.  sbev_split_bf16x3_weights converts W [N,K] fp32 once into W2 [N, K/8, 2, 8] bf16
 * (same byte count); K % 32 == 0.
 */
int sbev_split_bf16x3_weights(const float* W, uint16_t* W2, int64_t N, int K, sbev_stream_t stream);
int sbev_linear_bf16x3(const float* X, const uint16_t* W2, const float* bias, const float* residual, float* Y,
                       int64_t M, int N, int K, int64_t ldx, int64_t ldy, int relu, sbev_stream_t stream);
/* The parameter generator's shape (K = 256, N % 128 == 0, N >= 1024; sbev_linear_bf16x3_strip_ok) with the activation split
 * ONCE by the caller (X2 = sbev_split_bf16x3_weights(X [M, 256])): W-stationary strips in registers, X2 streamed from L2. */
int sbev_linear_bf16x3_strip_ok(int64_t M, int N, int K);
int sbev_linear_bf16x3_strip(const uint16_t* X2, const uint16_t* W2, const float* bias, float* Y, int64_t M, int N, int K,
                             int64_t ldy, int relu, sbev_stream_t stream);
int sbev_linear_splitk_bf16x3(const float* X, const uint16_t* W2, const float* bias, const float* residual,
                              const float* ln_w, const float* ln_b, float ln_eps, float* Y,
                              int64_t M, int N, int K, int64_t ldx, int relu, int splits, float* workspace,
                              sbev_stream_t stream);

/*
 * Split-bf16 Linears on the bf16 matrix core, round 3 (gemm_bf16s.hip).  nimg = 3 ("bf16x6"): every fp32 operand is the exact
 * sum of three RNE bf16 images (hi + mid + lo) and Y accumulates, in fp32 on v_mfma_f32_32x32x16_bf16, the six image products of
 * weight >= 2^-16 (hh, hm, mh, mm, hl, lh); the dropped ones are <= 2^-23 |a b| per product, i.e. below what an fp32 fma chain
 * rounds away per step -- fp32-class, not bit-equal to fp32 math.  nimg = 2 ("bf16x3"): hi + lo, three products, 2^-16 class.
 * Replaces: torch.nn.Linear of AdaptiveMixing.parameter_generator / out_proj (models/sparsebev_transformer.py:358,378).
 *
 *   sbev_split_bf16s_rows   X [rows, ldx] fp32 -> out [nimg][rows][K] bf16 row-major planes (rows * K * nimg elements): the
 *                           images themselves (image i = RNE_bf16 of what images < i left over).  K % 8 == 0.
 *   sbev_pack_bf16s_frags   W [N, ldw] fp32 -> out [ceil(N/32)][K/16][nimg][64][8] bf16 (sbev_bf16s_image_elems(N, K, nimg)
 *                           elements): the same images in v_mfma_f32_32x32x16_bf16 operand order -- lane l of fragment (nf, ks)
 *                           holds row 32 nf + (l & 31), k = 16 ks + 8 (l >> 5) + 0..7; a ragged last block repeats row N - 1.
 *                           The operand format of both kernels (weights once per weight update, the generator's X once per
 *                           call); K % 16 == 0.
 *   sbev_linear_bf16s_gen   Y [M, ldy] = X W^T + bias (ReLU optional) from the fragment images Xs / Ws.  N % 256 == 0,
 *                           K % 32 == 0, K <= 4096 (sbev_linear_bf16s_gen_ok).
 *   sbev_linear_splitk_bf16s  Y = LayerNorm?(relu?(X W^T + bias) + residual) for N == 256, K % 32 == 0 (sbev_linear_bf16s_out_ok):
 *                           X stays fp32 [M, ldx] and is split inside the kernel; workspace = sbev_linear_bf16s_out_plan(M, N, K)
 *                           partial slabs [plan, M, 256] fp32, summed in a fixed order (bit-reproducible) by sbev_splitk_reduce_f32.
 */
int64_t sbev_bf16s_image_elems(int64_t rows, int K, int nimg);
int sbev_split_bf16s_rows(const float* X, int64_t ldx, uint16_t* out, int64_t rows, int K, int nimg, sbev_stream_t stream);
int sbev_pack_bf16s_frags(const float* W, int64_t ldw, uint16_t* out, int N, int K, int nimg, sbev_stream_t stream);
int sbev_linear_bf16s_gen_ok(int64_t M, int N, int K);
int sbev_linear_bf16s_gen(const uint16_t* Xs, const uint16_t* Ws, const float* bias, float* Y, int64_t M, int N, int K,
                          int64_t ldy, int relu, int nimg, sbev_stream_t stream);
int sbev_linear_bf16s_out_ok(int64_t M, int N, int K);
int sbev_linear_bf16s_out_plan(int64_t M, int N, int K);
/* What a generator call of this shape launches (sbev_linear_bf16s_gen: nimg 2 / 3; sbev_linear_f16s_gen: nimg = nprod + 1), a pure host
 * function: weight_stationary = the setting of sbev_linear_gen_weight_stationary to plan for, cus = the device's compute units
 * (0: ask the current device).  Writes 7 + 4 L int32 words and returns their count; SBEV_EINVAL for a shape the kernels do not
 * cover or capacity < that count.
 *   out[0]  kernel: 0 = weight-stationary, 2 / 4 = tiled with 128- / 256-row tiles (row fragments per wave)
 *   out[1]  row splits (weight-stationary) / row tiles, over which the ceil(M / 32) row fragments are spread:
 *   out[2], out[3]  base, rem -- the first rem own base + 1 fragments, the others base
 *   out[4]  weight-stationary: tasks (column tiles x row splits); tiled: workgroups per row tile
 *   out[5]  tiled: column tiles a workgroup may walk in one launch (weight-stationary: 0)
 *   out[6]  L launches, each out[7 + 4 i ..]: first column tile (of 256 columns), column tiles, workgroups, dynamic LDS bytes */
int sbev_linear_gen_plan(int64_t M, int N, int K, int64_t ldy, int nimg, int weight_stationary, int cus, int32_t* out, int capacity);
int sbev_linear_splitk_bf16s(const float* X, const uint16_t* Wp, const float* bias, const float* residual,
                             const float* ln_w, const float* ln_b, float ln_eps, float* Y,
                             int64_t M, int N, int K, int64_t ldx, int relu, int nimg, float* workspace,
                             sbev_stream_t stream);

/*
 * fp16 hi + lo Linears on the same kernels (gemm_mode f16x3 / f16x4, round 3): an operand row (or the whole X) is multiplied by
 * 2^e -- a power of two, exact -- so that its largest |value| lands in [2^14, 2^15), then split into hi = RNE_fp16 and
 * lo = RNE_fp16(remainder): 11 + 11 significand bits + lo's sign = the fp32 value to <= 2^-23 relative for elements within 2^-17
 * of that maximum, to 2^-40 of the maximum below.  Products hl + lh + hh (nprod = 3; the dropped lo x lo is <= 2^-24 |a b|) or all
 * four (nprod = 4) on v_mfma_f32_32x32x16_f16, fp32 accumulation; the result is multiplied by 2^-(ex + ew) (exact).
 * tests/test_gpu_bf16s.py: max and rms error against fp64 <= the exact f32-MFMA kernels' at both AdaptiveMixing shapes.
 *   sbev_pack_f16s_frags     W [N, ldw] fp32 -> out [ceil(N/32)][K/16][2][64][8] fp16 (sbev_bf16s_image_elems(N, K, 2) elements) and
 *                            scales: per row [2][N] (2^e, then 2^-e) or, per_tensor = 1, [2] for the whole matrix (one extra pass over
 *                            it); per_tensor = 2: scales [2] is an input (a power of two from the caller's bound on |W|)
 *   sbev_linear_f16s_gen     as sbev_linear_bf16s_gen; xscale = X's [2] scales, wdown = W's 2^-e row [N]
 *   sbev_linear_splitk_f16s  as sbev_linear_splitk_bf16s; X fp32 is multiplied by 2^x_up_log2 inside the kernel (x_is_pairs = 0) -- the caller's bound
 *                            (|X| 2^x_up_log2 < 65504; an overflow shows as Inf / NaN, never silently); nscale = sbev_f16s_out_scale
 *   sbev_f16s_out_scale      nscale[n] = wdown[n] 2^-x_up_log2
 */
int sbev_pack_f16s_frags(const float* W, int64_t ldw, uint16_t* out, float* scales, int N, int K, int per_tensor, sbev_stream_t stream);
int sbev_linear_f16s_gen(const uint16_t* Xs, const float* xscale, const uint16_t* Ws, const float* wdown, const float* bias, float* Y,
                         int64_t M, int N, int K, int64_t ldy, int relu, int nprod, sbev_stream_t stream);

/* K = 256 with two images per operand (f16x3 / f16x4 / bf16x3s) runs on the WEIGHT-STATIONARY generator kernel: a wave keeps the
 * weights of its 32 output columns in registers for the whole launch, only X streams (LDS-DMA ring), persistent workgroups walk
 * (column tile, row split) tasks -- half the operand bytes per MFMA of the tiled kernel, bit-identical results.  0 restores the tiled
 * ping-pong kernel everywhere (A/B, tests; env SBEV_NO_GEN_WS=1); returns the previous setting. */
int sbev_linear_gen_weight_stationary(int enable);

int sbev_linear_splitk_f16s(const float* X, int x_is_pairs, int x_up_log2, const uint16_t* Wp, const float* nscale, const float* bias, const float* residual,
                            const float* ln_w, const float* ln_b, float ln_eps, float* Y,
                            int64_t M, int N, int K, int64_t ldx, int relu, int nprod, float* workspace, sbev_stream_t stream);
int sbev_f16s_out_scale(const float* wdown, int x_up_log2, float* nscale, int N, sbev_stream_t stream);
/* sbev_linear_splitk_f16s with X's scale in device memory (x_scale = {2^e, 2^-e}, e.g. sbev_f16s_tensor_scale) instead of a host-side
 * bound; wdown = W's [N] down-scales (sbev_pack_f16s_frags scales + N).  X fp32 only. */
int sbev_linear_splitk_f16s_xdev(const float* X, const float* x_scale, const uint16_t* Wp, const float* wdown, const float* bias,
                                 const float* residual, const float* ln_w, const float* ln_b, float ln_eps, float* Y,
                                 int64_t M, int N, int K, int64_t ldx, int relu, int nprod, float* workspace, sbev_stream_t stream);
/* The pre-split operand: out[i] = (fp16 hi, fp16 lo) of X[i] 2^up_log2 packed in one 32-bit slot (hi in the low half).  With
 * x_is_pairs = 1 sbev_linear_splitk_f16s takes X in this format (same [M, ldx] geometry) and only de-interleaves it.  The mixing
 * launches can emit it directly: sbev_adaptive_mixing_pairs_f16 / sbev_sample_mix_pairs_f16 = sbev_adaptive_mixing_f32 /
 * sbev_sample_mix_f32 with y written as pairs of y 2^up_log2 (what sbev_decoder_forward does in the fp16 GEMM modes). */
int sbev_f16s_pairs(const float* X, void* out, int64_t n, int up_log2, sbev_stream_t stream);
/* updown[0..1] = {2^e, 2^-e} with max |X| 2^e in [2^14, 2^15) over X [rows, ldx] (K columns): the operand scale of sbev_gemm_tn_f16s */
int sbev_f16s_tensor_scale(const float* X, int64_t ldx, int64_t rows, int K, float* updown, sbev_stream_t stream);
int sbev_adaptive_mixing_pairs_f16(const float* x, const float* params, void* y, int64_t BQ, int G, int Pin, int Cg, int Pout, float eps,
                                   int up_log2, sbev_stream_t stream);
int sbev_sample_mix_pairs_f16(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                              int64_t B, int N, int Q, int T, int G, int P, int Cg,
                              const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                              const float* loc, const float* weights, const int32_t* frame_slots, int n_slots,
                              const float* params, void* y, int Pout, float eps, int up_log2, sbev_stream_t stream);

/* dst[i] = (float)src[i] over a contiguous run; src_dtype: 0 fp32, 1 bf16, 2 fp16.  How the online frame ring takes
 * channels-last frames (sparsebev_amd/cache.py); replaces the torch.cat of cached frames, models/sparsebev.py:297-303. */
int sbev_copy_widen_f32(const void* src, int src_dtype, float* dst, int64_t n, sbev_stream_t stream);

/*
 * Gather + adaptive mixing in ONE launch: the workgroup of item (b*Q + q, g) samples its own x[T*P, 64] (the arithmetic of
 * sbev_msmv_fwd / sbev_msmv_fwd_ring with out_layout SBEV_OUT_MIX, frames spread over its four waves) into LDS and runs
 * sbev_adaptive_mixing_f32 on it -- bit-identical to the two launches, without the [B,Q,G,T*P,C] round trip through HBM.
 * Replaces: sampling_4d's gather + the middle of AdaptiveMixing.inner_forward (models/sparsebev_sampling.py:122-128,
 *           models/sparsebev_transformer.py:362-374).
 * Shapes covered: sbev_sample_mix_supported(L, C, P, T, gdiv, G) != 0  (L in {4,5}, C = 64, P in {4,8}, gdiv = G, T*P in
 * 4..64 or 116..120); feats / strides / loc / weights as for sbev_msmv_fwd with B' = B*T*G; frame_slots NULL = dense
 * pyramid, else the online ring (n_slots, see sbev_msmv_fwd_ring); params [B*Q, G, C*C + Pout*T*P]; y [B*Q, G, Pout, C].
 */
int sbev_sample_mix_supported(int L, int C, int P, int T, int gdiv, int G);
/* The fused kernel's taps are 31-bit BUFFER byte offsets (an out-of-map bilinear corner is a hardware-zeroed out-of-range load, never a
 * read: msmv_sampling_forward.cu:47-66), so every level's (sample-batch) slab -- N views of H_l x W_l pixels -- must stay below 2 GiB;
 * 1 if so.  hw = {H_0, W_0, H_1, W_1, ...}, strides in elements.  sbev_msmv_fwd itself has a 64-bit path for larger slabs. */
int sbev_sample_mix_slabs_ok(const int32_t* hw, int L, int feat_dtype, int N, int C, const int64_t* stride_v, int64_t stride_px);
int sbev_sample_mix_f32(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                        int64_t B, int N, int Q, int T, int G, int P, int C,
                        const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                        const float* loc, const float* weights, const int32_t* frame_slots, int n_slots,
                        const float* params, float* y, int Pout, float eps, sbev_stream_t stream);
/* sbev_decoder_forward uses the fused launch where supported (default 1); 0 restores sampler + mixing as two launches. */
int sbev_decoder_fuse_sample_mix(int enable);

/*
 * Launch order of the fused gather + mixing items (round 4).  The gather's fabric traffic is set by WHICH items share an XCD's
 * private L2 and WHEN they run: in launch order (block b = item (row b / G, group b % G) on XCD b % 8) every group is split
 * over two XCDs by row parity and both fetch the whole group's coarse levels, and rows far apart on the BEV grid evict each
 * other's lines (tools/sampler_footprint.py: 172 MB of fabric reads per launch at config 2 against 124 MB of distinct tap
 * segments; 800 against 503 MB at the 1600-query config).  sbev_query_order sorts each sample's rows by the direction of the
 * box centre around the ego origin -- order [B*Q] int32, sample b's rows b*Q + q in slots [b*Q, (b+1)*Q), one workgroup per
 * sample, Q <= sbev_query_order_max() -- and sbev_sample_mix_*_ordered walk the GROUP-major list (g, position) in eight
 * contiguous pieces, one per XCD: one group and one arc of the camera ring per L2.  A placement hint only: results are
 * bit-identical for ANY permutation (order = NULL: launch order).  query_bbox rows: ld floats apart, columns 0, 1 = normalised
 * centre (decode_bbox, models/bbox/utils.py:69-70; the reference has no counterpart: its CUDA op takes the launch order).
 * Measured (round 4, config 2): fabric reads of the launch 290 -> 232 MB, L2 hit 0.39 -> 0.47, duration unchanged (85.6 -> 87.7 us:
 * the launch is bound by each workgroup's chain of memory latencies, not by fabric bytes), plus 17 us for the sort -- so
 * sbev_decoder_forward keeps the launch order unless sbev_decoder_query_order(1) (env SBEV_QUERY_ORDER=1; returns the previous
 * setting): then every layer's input boxes are sorted in front of its self attention and the fused launch walks that order;
 * sbev_decoder_query_order(2) (SBEV_QUERY_ORDER=2) sorts the step's INPUT boxes once and every layer walks that order.
 */
int sbev_query_order_max(void);
int sbev_query_order(const float* query_bbox, int64_t ld, const double* pc_range, int B, int Q, int32_t* order, sbev_stream_t stream);
int sbev_sample_mix_f32_ordered(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                                int64_t B, int N, int Q, int T, int G, int P, int C,
                                const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                                const float* loc, const float* weights, const int32_t* frame_slots, int n_slots,
                                const float* params, float* y, int Pout, float eps, const int32_t* order, sbev_stream_t stream);
int sbev_sample_mix_pairs_f16_ordered(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                                      int64_t B, int N, int Q, int T, int G, int P, int Cg,
                                      const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                                      const float* loc, const float* weights, const int32_t* frame_slots, int n_slots,
                                      const float* params, void* y, int Pout, float eps, int up_log2, const int32_t* order,
                                      sbev_stream_t stream);
int sbev_decoder_query_order(int enable);
/* The fused launch in its general form, and the one that takes a keyed frame pool (sbev_msmv_fwd_pool): slot_table_dev = device int32
 * [B, T] (entries clamped to [0, n_slots) by the kernel; n_slots >= 1, may be below T) -- or frame_slots as for sbev_sample_mix_f32 --
 * or neither (dense pyramid); both together are refused.  y_pairs == 0: y fp32 (sbev_sample_mix_f32); != 0: (fp16 hi, fp16 lo) pairs of
 * y 2^up_log2 (sbev_sample_mix_pairs_f16); order: NULL or as for the _ordered forms.  Bit-identical to those four on the same frames;
 * the slot of a frame is requested one unit ahead, with the unit's sample points.  Messages carry the sbev_sample_mix_f32 prefix. */
int sbev_sample_mix_pool(const void* const* feats, const int32_t* hw, int L, int feat_dtype,
                         int64_t B, int N, int Q, int T, int G, int P, int C,
                         const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                         const float* loc, const float* weights, const int32_t* frame_slots, const int32_t* slot_table_dev, int n_slots,
                         const float* params, void* y, int Pout, float eps, int y_pairs, int up_log2, const int32_t* order,
                         sbev_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training: backward passes of the decoder layer.
 * Replaces: torch autograd through SparseBEVTransformerDecoderLayer.forward and the activation-checkpointed
 *           inner_forward()s (models/sparsebev_transformer.py:162-193,231-234,313-317,383-387).  Every entry point is the
 *           hand-written backward of one forward entry point above; sparsebev_amd/autograd.py chains them.
 * ---------------------------------------------------------------------------------------------------------- */

/* Layout-generic fp32 MFMA GEMM:  C[M,N] (+)= sum_k A(m,k) B(k,n),  A(m,k) = a_kmajor ? A[k*lda+m] : A[m*lda+k],
 * B(k,n) = b_kmajor ? B[k*ldb+n] : B[n*ldb+k].  For nn.Linear y = x W^T:  grad_x = sbev_gemm_f32(grad_y, 0, ., W, 1, .),
 * grad_W = sbev_gemm_f32(grad_y, 1, ., x, 1, .).  `workspace` (sbev_gemm_f32_workspace bytes, may be NULL when that is 0)
 * holds split-K slabs for few-tile / long-K shapes; results are bit-reproducible (no atomics). */
int64_t sbev_gemm_f32_workspace(int64_t M, int N, int64_t K);
int sbev_gemm_f32(const float* A, int a_kmajor, int64_t lda, const float* B, int b_kmajor, int64_t ldb,
                  float* C, int64_t ldc, int64_t M, int N, int64_t K, int accumulate,
                  float* workspace, sbev_stream_t stream);
/* The same reduction over up to 8 operand pairs of identical layout and shape in ONE launch (+ the slab sum): C (+)= sum_s A_s B_s --
 * the weight gradient of a Linear shared by several decoder layers.  A / B: host arrays of nseg device pointers;
 * workspace: sbev_gemm_f32_multi_workspace(M, N, K, nseg) bytes (always needed).  Bit-reproducible.  K = 0 is an empty sum in both:
 * C = 0, or C unchanged under accumulate. */
int64_t sbev_gemm_f32_multi_workspace(int64_t M, int N, int64_t K, int nseg);
int sbev_gemm_f32_multi(const float* const* A, int a_kmajor, int64_t lda, const float* const* B, int b_kmajor, int64_t ldb,
                        int nseg, float* C, int64_t ldc, int64_t M, int N, int64_t K, int accumulate,
                        float* workspace, sbev_stream_t stream);

/* grad_W-shaped product on the fp16 matrix core (gemm_tn_f16s.hip): C[M,N] (+)= sum_k A[k*lda + m] B[k*ldb + n], both operands
 * k-major (grad_W = grad_y^T . x of a Linear, reduced over the B*Q rows; replaces sbev_gemm_f32(a_kmajor = b_kmajor = 1) where
 * sbev_gemm_tn_f16s_ok: M, N multiples of 4 and >= 256 tiles of 128 x 128).  Operands are multiplied by a_scale[0] / b_scale[0]
 * (device, {2^e, 2^-e}: sbev_f16s_tensor_scale or a caller's bound), split into fp16 hi + lo inside the kernel, 3 products
 * (hl, lh, hh), fp32 accumulation, result times a_scale[1] b_scale[1].  Error vs fp64 <= the exact f32-MFMA kernel's. */
int sbev_gemm_tn_f16s_ok(int64_t M, int64_t N, int64_t K);
int sbev_gemm_tn_f16s(const float* A, int64_t lda, const float* a_scale, const float* B, int64_t ldb, const float* b_scale,
                      float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int accumulate, sbev_stream_t stream);

/* dZ = dY * (Y > 0) (Y = a ReLU's forward output, NULL: dZ = dY; dZ may be NULL or alias dY) and db[n] = sum_m dZ[m,n]
 * (NULL: skipped).  Rows have stride ld.  workspace: sbev_colsum_workspace(M, N) bytes (needed when db != NULL);
 * column sums are added in a fixed order (bit-reproducible). */
int64_t sbev_colsum_workspace(int64_t M, int N);
int sbev_bias_relu_bwd(const float* dY, const float* Y, float* dZ, float* db, int64_t M, int N, int64_t ld,
                       float* workspace, sbev_stream_t stream);

/* LayerNorm(+ReLU) backward over the last dim (N % 4 == 0, N <= 1024): X is the LayerNorm INPUT;
 * workspace: sbev_layer_norm_bwd_workspace(M, N) bytes. */
int64_t sbev_layer_norm_bwd_workspace(int64_t M, int N);
int sbev_layer_norm_bwd(const float* dY, const float* X, const float* gamma, const float* beta, float eps, int relu,
                        float* dX, float* dgamma, float* dbeta, float* workspace, int64_t M, int N, sbev_stream_t stream);
/* sbev_bias_relu_bwd / sbev_layer_norm_bwd with the parameter gradients (db; dgamma, dbeta) ADDED to their buffers when accumulate != 0:
 * a parameter shared by the layers of a decoder call collects its gradient in one buffer, no separate summation launches. */
/* LayerNorm backward in two halves for parameters shared by several layers: sbev_layer_norm_bwd_rows = dX and the [M, 2] (mean, rstd)
 * rows (workspace >= 2 M floats); sbev_layer_norm_param_group = dgamma / dbeta of ng <= 8 LayerNorms, each summed over <= 8
 * (dY, X, stats) triples, in ONE launch.  Pointer tables are host arrays [ng][8]; the per-LayerNorm arrays [ng]. */
int sbev_layer_norm_bwd_rows(const float* dY, const float* X, const float* gamma, const float* beta, float eps, int relu,
                             float* dX, float* workspace, int64_t M, int N, sbev_stream_t stream);
int sbev_layer_norm_param_group(const float* const* dYs, const float* const* Xs, const float* const* stats,
                                const float* const* gammas, const float* const* betas, float* const* dgammas, float* const* dbetas,
                                const int32_t* Ns, const int32_t* nsegs, const int32_t* relus, const int32_t* accumulate,
                                int ng, int64_t M, sbev_stream_t stream);
/* Grouped bias gradients: out_b[n] (+)= sum_s colsum(seg_b[s] [M, N_b]) for ng <= 16 biases with <= 8 gradient matrices each (the
 * layers of a call sharing the bias) in ONE launch.  segs: host array [ng][8] of device pointers; outs / Ns / nsegs / accumulate: [ng]. */
int sbev_colsum_group(const float* const* segs, float* const* outs, const int32_t* Ns, const int32_t* nsegs,
                      const int32_t* accumulate, int ng, int64_t M, sbev_stream_t stream);
int sbev_bias_relu_bwd_acc(const float* dY, const float* Y, float* dZ, float* db, int64_t M, int N, int64_t ld,
                           float* workspace, int accumulate, sbev_stream_t stream);
int sbev_layer_norm_bwd_acc(const float* dY, const float* X, const float* gamma, const float* beta, float eps, int relu,
                            float* dX, float* dgamma, float* dbeta, float* workspace, int64_t M, int N, int accumulate, sbev_stream_t stream);

/* sbev_linear3_ln_relu_f32 that also stores the Linear's pre-LayerNorm output `pre` [M,N] (may be NULL). */
int sbev_linear3_ln_relu_ex_f32(const float* x, int64_t ldx, const float* w, const float* b,
                                const float* ln_w, const float* ln_b, float eps, float* y, float* pre,
                                int64_t M, int N, sbev_stream_t stream);

/* Backward of sbev_adaptive_mixing_f32 (the forward is recomputed inside): grad_y [BQ,G,Pout,C] ->
 * grad_x [BQ,G,Pin,C], grad_params [BQ,G,C*C+Pout*Pin]. */
int sbev_adaptive_mixing_bwd_f32(const float* x, const float* params, const float* grad_y, float* grad_x, float* grad_params,
                                 int64_t BQ, int G, int Pin, int C, int Pout, float eps, sbev_stream_t stream);
/* the same, also writing item_max[BQ*G][4]: four partial maxima of |grad_params| per (row, group), their maximum = that item's
 * maximum: sbev_f16s_tensor_scale of the array is the fp16 scale of grad_params without another pass over its 118 MB */
int sbev_adaptive_mixing_bwd_max_f32(const float* x, const float* params, const float* grad_y, float* grad_x, float* grad_params,
                                     float* item_max, int64_t BQ, int G, int Pin, int C, int Pout, float eps, sbev_stream_t stream);

/* Training forward of sbev_sasa_f32 with attention dropout (mmcv MultiheadAttention attn_drop; keep decisions are a
 * hash of (seed, b, h, i, j)), and the backward of either forward: grad_out [B,Q,H*32] -> grad_qkvt [B,Q,ld]
 * (q | k | v | tau columns, padding zeroed).  `out` is the forward output; workspace = 2*B*H*Q floats. */
int sbev_sasa_train_fwd_f32(const float* qkvt, int64_t ld, const float* query_bbox, const double* pc_range,
                            const uint8_t* mask, float* out, int B, int Q, int H, int head_dim,
                            float attn_drop, uint64_t seed, sbev_stream_t stream);
int sbev_sasa_bwd_f32(const float* qkvt, int64_t ld, const float* query_bbox, const double* pc_range,
                      const uint8_t* mask, const float* out, const float* grad_out, float* grad_qkvt,
                      float* workspace, int B, int Q, int H, int head_dim, float attn_drop, uint64_t seed,
                      sbev_stream_t stream);

/* sbev_msmv_bwd with (a) grad_out in either output layout of sbev_msmv_fwd (SBEV_OUT_REF / SBEV_OUT_MIX with T, G) and
 * (b) grad_feats == NULL when the features need no gradient (no atomics are issued at all). */
int sbev_msmv_bwd_ex(const void* const* feats, void* const* grad_feats, const int32_t* hw, int L,
                     int64_t Bp, int N, int C, int Q, int P,
                     int gdiv, const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                     const float* loc, const float* weights, const float* grad_out, int grad_out_layout, int T, int G,
                     float* grad_loc, float* grad_weights, sbev_stream_t stream);

/* The feature gradient of sbev_msmv_bwd_ex WITHOUT float atomics, bit-reproducible (msmv_sampling_det.hip).  Replaces the grad_value
 * atomics of ms_deformable_col2im_bilinear_gm (models/csrc/msmv_sampling/msmv_sampling_backward.cu:29-105) in three steps; grad_loc and
 * grad_weights come from sbev_msmv_bwd_ex with grad_feats == NULL, as before.
 *   Taps of a call are numbered i = (((b'*Q + q)*P + p)*L + l)*4 + k, k = 2*kh + kw the bilinear corner; n = sbev_msmv_bwd_tap_count.
 *   Tap i is LIVE iff sbev_msmv_bwd would issue its atomic: level l passes the -1 < h_im < H, -1 < w_im < W test and the corner lies
 *   inside the map.  Its destination is (l, off), off the element offset of the corner's channel row in grad_feats[l]; its scalar is
 *   coef_i = (ch * cwid) * wl (two fp32 roundings).
 *   Result, for every destination and channel c:  acc = +0;  for the destination's live taps in ascending i:
 *   acc = acc + coef_i * grad_out[b', q, p, c] (product rounded, then the sum);  grad_feats[l][off + c] += acc  (ONE addition: the call
 *   accumulates, like the atomic path).  Nothing else -- launch geometry, CU count, other streams, eager or graph replay -- reaches
 *   the bits.
 * sbev_msmv_bwd_tap_count: pure host function, n = B'*Q*P*L*4; -1 for negative sizes, P > SBEV_MAX_POINTS, L outside
 *   1..SBEV_MAX_LEVELS, or n > INT64_MAX / 4.
 * sbev_msmv_bwd_taps: the pyramid arguments of sbev_msmv_bwd_ex (feats[l] are not read) -> keys[n] (device int64: (l << 56) | off of a
 *   live tap, INT64_MAX of a dead one) and coefs[n] (device fp32; 0 of a dead tap).  Needs stride_px >= C, stride_g >= C where
 *   gdiv > 1, no negative stride and offsets below 2^56: every destination row has one writer.
 * sbev_msmv_bwd_sum_sorted: sorted_keys[n] = the keys in ascending order, order[n] = the tap index at each sorted position (device
 *   int64 both).  They MUST come from a STABLE sort of keys (ties in ascending tap index): that order is the summation order.  This
 *   library does not sort; torch.sort(keys, stable=True) does.  grad_out as in sbev_msmv_bwd_ex (either layout; T, G read for
 *   SBEV_OUT_MIX), any C >= 1; n must equal sbev_msmv_bwd_tap_count(Bp, Q, P, L). */
int64_t sbev_msmv_bwd_tap_count(int64_t Bp, int Q, int P, int L);
int sbev_msmv_bwd_taps(const void* const* feats, const int32_t* hw, int L,
                       int64_t Bp, int N, int C, int Q, int P,
                       int gdiv, const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                       const float* loc, const float* weights, int64_t* keys, float* coefs, sbev_stream_t stream);
int sbev_msmv_bwd_sum_sorted(void* const* grad_feats, int L, const int64_t* sorted_keys, const int64_t* order,
                             const float* coefs, int64_t n, const float* grad_out, int grad_out_layout,
                             int64_t Bp, int C, int Q, int P, int T, int G, sbev_stream_t stream);

/* Backward of sbev_project_select: grad_loc [B*T*G,Q,P,3] -> grad_points [B,Q,T,G*P,3] through the camera the forward
 * selected (re-selected bit-exactly).  models/sparsebev_sampling.py:49-114. */
int sbev_project_select_bwd(const float* sample_points, const float* lidar2img, const float* grad_loc,
                            int B, int Q, int T, int N, int G, int P, float image_h, float image_w, float eps,
                            float* grad_points, sbev_stream_t stream);

/* Backward of sbev_sampling_front: grad_points [B,Q,T,G*P,3] and grad_weights_bp [B*G*T,Q,P,L] (either may be NULL) ->
 * grad_offset (first G*P*3 columns) and grad_logits (first G*P*L columns) of rows with stride ld_grad -- e.g. the two
 * column blocks of one packed [B*Q, G*P*(3+L)] gradient --, grad_bbox [B*Q,10] (or NULL; velocity is detached). */
int sbev_sampling_front_bwd(const float* query_bbox, const float* offset, int64_t ld_off, const float* logits, int64_t ld_logit,
                            const double* pc_range, int B, int Q, int T, int G, int P, int L,
                            const float* grad_points, const float* grad_weights_bp,
                            float* grad_offset, float* grad_logits, int64_t ld_grad, float* grad_bbox, sbev_stream_t stream);

/* Backward of sbev_refine_bbox (code_size 10): grad_out, the forward's `out` and the proposal -> grad_reg, grad_bbox (NULL ok). */
int sbev_refine_bbox_bwd(const float* grad_out, const float* out, const float* query_bbox, const float* vel_div,
                         float* grad_reg, float* grad_bbox, int B, int Q, sbev_stream_t stream);

/* y = x * keep / (1 - p), keep_i = hash(seed, i) >= p: the mmcv FFN dropouts; the backward is the same call on grad_y. */
int sbev_dropout_f32(const float* x, float* y, int64_t n, uint64_t seed, float p, sbev_stream_t stream);

/* The three dropout launches with a part of the seed in DEVICE memory (round 4): the keep decisions hash `seed + *seed_dev` (seed_dev
 * null: `seed` alone, i.e. the calls above).  A training step captured as a hipGraph freezes every by-value argument, so the host
 * seeds of its dropout sites stay what they were at capture; the word behind `seed_dev` is what the caller changes between replays
 * (sparsebev_amd/train_graph.py refreshes it with one small launch before each replay).  Forward and backward of a site must see the
 * same word: change it only between steps. */
int sbev_sasa_train_fwd_f32_ds(const float* qkvt, int64_t ld, const float* query_bbox, const double* pc_range, const uint8_t* mask,
                               float* out, int B, int Q, int H, int head_dim, float attn_drop, uint64_t seed, const uint64_t* seed_dev,
                               sbev_stream_t stream);
int sbev_sasa_bwd_f32_ds(const float* qkvt, int64_t ld, const float* query_bbox, const double* pc_range, const uint8_t* mask,
                         const float* out, const float* grad_out, float* grad_qkvt, float* workspace, int B, int Q, int H, int head_dim,
                         float attn_drop, uint64_t seed, const uint64_t* seed_dev, sbev_stream_t stream);
int sbev_dropout_f32_ds(const float* x, float* y, int64_t n, uint64_t seed, const uint64_t* seed_dev, float p, sbev_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Whole-decoder runtime: ONE call enqueues every kernel of every layer (18 launches per layer, DESIGN_HISTORY.md section 4) on `stream`.
 * Replaces: the Python control flow of SparseBEVTransformerDecoder.forward / ...DecoderLayer.forward
 *           (models/sparsebev_transformer.py:56-101,162-193) at inference.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct sbev_decoder_config {
    int32_t B, Q, T, N, G, P, L;        /* batch, queries, frames, views (6), groups (4), points, levels */
    int32_t D, H, ffn;                  /* embed dims (256), heads (8), FFN hidden (512) */
    int32_t num_classes, code_size, num_layers, out_points;
    int32_t attn_in_rows;               /* rows of attn_in_w: 3*D + H rounded up to a multiple of 4 */
    int32_t feat_dtype;                 /* enum sbev_dtype of the pyramid */
    int32_t hw[SBEV_MAX_LEVELS][2];     /* (H_l, W_l) */
    float image_h, image_w, eps_homo;   /* img_shape and the 1e-5 of sampling_4d */
    int32_t gemm_mode;                  /* enum sbev_gemm_mode for the two large mixing GEMMs (0 = exact fp32) */
    int32_t n_slots;                    /* 0: feats_nhwc[l] = [B*T*N, H, W, D] (dense); > 0: online frame ring / keyed frame pool [B, n_slots, N, H, W, D] */
    int32_t frame_slots[SBEV_MAX_FRAMES]; /* ring only: physical slot of logical frame t (see sbev_msmv_fwd_ring) */
    int32_t overlap;                    /* != 0: run the parameter-generator GEMM and the classification branch on an
                                           internal second stream (created once per process) beside the sampling chain /
                                           regression branch, joined back into `stream` with events.  The side stream and
                                           its events are process-wide: calls with overlap != 0 must not run concurrently
                                           from several host threads (overlap == 0, the default, has no shared state) */
    double pc_range[6];
    const int32_t* slot_table;          /* NULL: frame_slots above (or dense).  Else the keyed frame pool (sbev_msmv_fwd_pool): DEVICE int32
                                           [B, T], frame t of sample b is read from slot slot_table[b*T + t]; needs n_slots > 0 (may be
                                           below T), frame_slots is ignored.  The pointer is what a captured step holds: refresh the table
                                           in place and one capture serves every step */
} sbev_decoder_config;

/* Device pointers of the shared decoder layer's parameters (reference state-dict names in comments, prefix
 * decoder.decoder_layer.).  Linear weights are [out, in] row-major exactly as nn.Linear stores them. */
typedef struct sbev_decoder_weights {
    const float *pe0_w, *pe0_b, *pe1_g, *pe1_b, *pe3_w, *pe3_b, *pe4_g, *pe4_b;  /* position_encoder.{0,1,3,4} */
    const float *attn_in_w, *attn_in_b;   /* rows: self_attn.attention.attn.in_proj_{weight,bias}, then self_attn.gen_tau.*, then zero padding */
    const float *attn_out_w, *attn_out_b; /* self_attn.attention.attn.out_proj.* */
    const float *samp_w, *samp_b;         /* rows: sampling.sampling_offset.*, then sampling.scale_weights.* */
    const float *pg_w, *pg_b, *op_w, *op_b;                       /* mixing.parameter_generator.*, mixing.out_proj.* */
    const uint16_t *pg_w2, *op_w2;                                /* their sbev_split_bf16x3_weights images (gemm_mode 1; else NULL) */
    const float *ffn0_w, *ffn0_b, *ffn1_w, *ffn1_b;               /* ffn.layers.0.0.*, ffn.layers.1.* */
    const float *norm1_g, *norm1_b, *norm2_g, *norm2_b, *norm3_g, *norm3_b;
    const float *cls0_w, *cls0_b, *cls1_g, *cls1_b, *cls3_w, *cls3_b, *cls4_g, *cls4_b, *cls6_w, *cls6_b;  /* cls_branch.* */
    const float *reg0_w, *reg0_b, *reg2_w, *reg2_b, *reg4_w, *reg4_b;                                        /* reg_branch.* */
    const float *chain_pack;   /* sbev_decoder_chain_pack image of the small Linears' weights, or NULL (op-by-op launches) */
    const uint16_t *pg_ws;     /* gemm_mode 2 / 3: sbev_pack_bf16s_frags image of pg_w (3 / 2 images); else NULL */
    const uint16_t *op_wp;     /* gemm_mode 2 / 3: sbev_pack_bf16s_frags image of op_w (3 / 2 images); else NULL */
    /* gemm_mode 4 / 5 (fp16 hi + lo): pg_ws / op_wp are the sbev_pack_f16s_frags images (per-row scales) and */
    const float *pg_wdown;     /*   the 2^-e row of pg_w's scales [G * (C*C + out_points * T*P)] */
    const float *op_nscale;    /*   sbev_f16s_out_scale(op_w's 2^-e row, sbev_decoder_mixed_up_log2(cfg)) [embed_dims] */
    const float *pg_xscale;    /*   {2^e, 2^-e} (device memory) for the generator's input, norm1's output: the largest e with
                                *   (sqrt(embed_dims - 1) max|norm1_g| + max|norm1_b|) 2^e < 65504 */
} sbev_decoder_weights;

/*
 * Row chains.  Every op of a decoder layer except the self attention, the sampler and the two big mixing GEMMs is
 * row-local (position_encoder, attention in/out projections, norm1-3, sampling Linear, ffn, cls_branch, reg_branch,
 * refine_bbox: models/sparsebev_transformer.py:166-183), so with `chain_pack` set sbev_decoder_forward runs them as three
 * launches per layer with the rows in LDS (6 launches per layer instead of 17; the sample-point projection runs inside too).  The kernels stream the weights in a
 * lane-ordered layout: sbev_decoder_chain_pack writes that image (sbev_decoder_chain_pack_floats floats, 16-byte aligned,
 * 0 = config not covered: needs embed_dims 256, ffn 512, code_size 10) from the weight pointers of `weights`; re-pack when
 * the weights change.  Results agree with the op-by-op launches to fp32 round-off (different summation order), not bit for bit.
 * sbev_decoder_row_chain(0) makes sbev_decoder_forward ignore chain_pack (default 1).
 */
int64_t sbev_decoder_chain_pack_floats(const sbev_decoder_config* cfg);
int sbev_decoder_chain_pack(const sbev_decoder_config* cfg, const sbev_decoder_weights* weights, float* out, sbev_stream_t stream);
int sbev_decoder_row_chain(int enable);
/* What one row-chain launch of `cfg` (B * Q = 1 .. 4096 rows) does, decided on the host from plain values: no device is touched, no
 * pointer is needed.  kind: 0 = tail, 1 = front, 2 = attention chain; with_front: the tail goes on with the next layer's front;
 * pair_ok: pair mode is allowed (switch on, fault word installed, workspace given); cus: the device's compute units (0: none -- no
 * pairs).  Writes int32 words to out[0 .. capacity) and returns their number, -1 (SBEV_EINVAL) on an uncovered config or a short buffer:
 *    0 pre (= kind)   1 rg: row groups of 4 rows per row block (1, 2, 4)   2 pair (0 / 1)   3 grid (workgroups)   4 dynamic LDS bytes
 *    5 n_units        6 n_pairs (0 without pair mode)
 *    7 warm: float offset into the sbev_decoder_chain_pack image of the weight span the launch streams   8 its 128-byte lines
 *    9 float offset in the image of the launch's small vectors, copied to   10 vec_off,  11 vec_n: floats [vec_off, vec_off + vec_n)
 *      of the kernels' LDS parameter block
 * then the unit table of member 0 and, with pair = 1, of member 1 (the same number of units), 18 words per unit:
 *    epilogue (0 ffn.0, 1 ffn.1, 2 / 3 branch layers, 4 output + refine_bbox, 5 position encoder, 6 in-projection, 7 attention
 *    out-projection, 8 sampling Linear), first output column (in-projection), then the unit's two Linears a | b, 8 words each:
 *    weights (float offset into the image, -1: none), LDS float offset and row stride of the input rows, KH (k-pieces per 64-column
 *    group), items (= column groups x KH), chunks (16-k chunks per item), kh0, KHT (the Linear covers pieces [kh0, kh0 + KH) of KHT). */
int sbev_decoder_chain_plan(const sbev_decoder_config* cfg, int kind, int with_front, int pair_ok, int cus, int32_t* out, int capacity);
/* Fixed plans.  A launch's unit tables depend on the chain, rg, pair, with_front and the column-group counts of the in-projection and of
 * the sampling Linear only; for the keys of config 2's launches (tail on pairs with / without front, attention chain, front: rg as
 * planned, 13 and 2 column groups) the library holds kernels with the table compiled in -- no table in the kernel arguments, no scalar
 * load of one between two units.  A launch takes such a kernel when its key is covered and its planned table equals the compiled one
 * (always, unless SBEV_CHAIN_TIE_SMALL / _PAIR_Q0 / _RG / _PAIR16 is set in the environment); results are bit-identical either way.
 * sbev_decoder_chain_fixed(0 / 1) switches them (returns the previous setting; default 1, SBEV_CHAIN_FIXED=0 in the environment starts
 * with 0).  The switch is NOT one of sbev_decoder_switches: a captured step keeps the kernels it was recorded with.
 * sbev_decoder_chain_fixed_plan: sbev_decoder_chain_plan's words (same arguments, same layout) with the unit tables taken from the
 * compiled-in table of the fixed kernel that covers the launch's key, or 0 = none covers it (also: config not covered by the row
 * chains at all); -1 on a short buffer.  Touches no device.
 * sbev_decoder_chain_fixed_launches: row-chain launches since the library was loaded that took a fixed kernel (a captured launch counts
 * once, at its capture). */
int sbev_decoder_chain_fixed(int enable);
int64_t sbev_decoder_chain_fixed_launches(void);
int sbev_decoder_chain_fixed_plan(const sbev_decoder_config* cfg, int kind, int with_front, int pair_ok, int cus, int32_t* out, int capacity);

/* Pair mode of the tail chain (round 4).  A chain workgroup streams every weight of its chain through its CU's ~60 GB/s L2 path, so
 * where two workgroups per row block fit the device in ONE round (<= ~1000 rows at 8 rows per pair, <= ~2000 at 16, on 256 CUs) the
 * tail runs on PAIRS: the members split ffn.layers.0 by columns and ffn.layers.1 by k (partial sums exchanged), take one branch each
 * (classification | regression + refine_bbox + the next position encoder) and split the attention in-projection by columns -- half
 * the weight stream per CU, two hand-offs through write-through stores and one arrival counter per pair in the decoder workspace
 * (zeroed by the layer's attention chain; bounded polls).  Results equal the single-workgroup chain to fp32 round-off.
 * sbev_decoder_chain_pair(0 / 1) switches it (returns the previous setting; default 1, SBEV_NO_CHAIN_PAIR=1 in the environment
 * starts with 0).  sbev_decoder_chain_pair_timeouts: hand-offs whose partner did not arrive within the poll bound (~1 s) since the
 * library was loaded -- 0 unless something kept half of a pair off the GPU; the results of such a launch are undefined; synchronises
 * the device; -1 on a HIP error. */
int sbev_decoder_chain_pair(int enable);
int64_t sbev_decoder_chain_pair_timeouts(void);
/* The same event on the NORMAL path (round 5): a timed-out hand-off also bumps a sticky word in pinned host memory, read without
 * synchronising anything.  While sbev_decoder_chain_pair_faults() > 0, sbev_decoder_forward (and sbev_graph_launch of a captured
 * step) refuses with SBEV_EFAULT: the step that faulted -- the PREVIOUS one or an earlier one, its launches were asynchronous -- holds
 * wrong rows and must be repeated.  The refusing call switches pair mode off (single-workgroup tail from here on: no hand-offs, no
 * faults); the caller acknowledges with sbev_decoder_chain_pair_faults_ack() (returns the count) and re-runs.  A caller that
 * synchronises on its own can ask sbev_decoder_chain_pair_faults() right after its synchronisation and learn about the CURRENT step.
 * Pair mode is only used when the word could be installed (hipHostMalloc). */
int64_t sbev_decoder_chain_pair_faults(void);
int64_t sbev_decoder_chain_pair_faults_ack(void);
/* In-launch fold of the out-projection's split-K slabs (round 6; fp16 GEMM modes, row chains on, every workgroup of the out-projection
 * resident at once: <= ~1000 rows on 256 CUs).  The S chunk-workgroups of a row tile write their slab through, meet at a counter in the
 * decoder workspace (zeroed by the layer's attention chain, like the pair counters) and each sums ceil(rows / S) rows of the tile over all
 * slabs in slab order -- bit-identical to the tail's own sum -- so the tail reads ONE row block instead of S (32 x 8 rows x 1 KB per
 * workgroup, twice per pair: 59 MB per layer at 900 rows).  Polls are bounded like the pair hand-off's; a row tile that never completes
 * raises the same fault word (sbev_decoder_chain_pair_faults) and counts in sbev_decoder_chain_pair_timeouts.  Follows the pair switch
 * (sbev_decoder_chain_pair(0) turns both off); sbev_decoder_out_fold(0 / 1) switches it alone (returns the previous setting).  DEFAULT 0:
 * measured at config 2 the fold costs the out-projection 12.6 us and saves the tail 4 -- an A/B switch, not the
 * product path; SBEV_OUT_FOLD=1 in the environment starts with 1.  sbev_debug_out_fold_drop: test hook, never set in production. */
int sbev_decoder_out_fold(int enable);
/* Rows from which the fp16-mode out-projection with the pre-split operand (the decoder's path) runs on 256-row tiles
 * (gemm_bf16s_out8_kernel: two row halves as phase groups sharing one W ring -- a third less operand delivery per product than the 128-row
 * kernel; default 1024: the batch configs and the 1600-query config; env SBEV_OUT8_MIN_ROWS; 0 = never, other values are raised to 1024).  Returns the previous threshold. */
int sbev_linear_out8_min_rows(int rows);
int sbev_debug_out_fold_drop(int enable);
/* Per-device setup that is illegal under stream capture (hipHostMalloc + hipMemcpyToSymbol of the fault word above): call once per device
 * before the first capture that may contain a decoder step -- the ctypes binding does when it loads the library in a process that already has its device context.  Without it
 * sbev_decoder_workspace_bytes attempts the same; an attempt that fails (e.g. made inside a torch.cuda.graph capture) is retried by later
 * calls, with one message on stderr / sbev_last_error(), and pair mode stays off meanwhile.  The word is shared by all devices of a process. */
int sbev_init(void);
/* Test hook for the poll bound: with 1, one member of the first pair of every pair-mode tail exits at once; its partner must time out
 * (sbev_decoder_chain_pair_timeouts grows, the launch ends after about a second per hand-off, only that pair's 8 rows are wrong).
 * Returns the previous setting.  Never set in production. */
int sbev_debug_chain_pair_drop(int enable);

/* Kernel launches per layer sbev_decoder_forward enqueues for this config and weight set under the current process-wide switches
 * (row chains, gather + mixing fusion), -1 on an invalid config: 6 with the row chains, 17 op by op, + 1 for the two-launch gather
 * + mixing, + 1 for the activation split of the split-bf16 GEMM modes. */
int sbev_decoder_launches_per_layer(const sbev_decoder_config* cfg, const sbev_decoder_weights* weights);

/* The process-wide switches a decoder step is planned from, as the library holds them now -- whichever way each was set (its setter,
 * its environment variable at load, the library itself after a pair fault).  sbev_decoder_forward / _lazy / _capture read exactly this
 * set, once per call; a step captured under one reading must only be replayed under an equal one, so a caller that caches captured
 * steps puts ALL returned values into its key.  Fills out[0 .. min(n, capacity)) and returns n, the number of values (11 today; later
 * versions only append).  Needs no device.  Order:
 *    0 sbev_decoder_row_chain            1 sbev_decoder_chain_pair          2 sbev_decoder_fuse_sample_mix
 *    3 fused gather + mixing for 5 fp32 levels (no setter: SBEV_NO_FUSE_L5F32 in the environment clears it)
 *    4 sbev_decoder_query_order (0 / 1 / 2)   5 sbev_decoder_lazy_scan_launch    6 sbev_decoder_out_fold
 *    7 sbev_linear_gen_weight_stationary      8 sbev_linear_out8_min_rows (rows)  9 sbev_msmv_buffer_taps
 *   10 sbev_get_box_convention */
int sbev_decoder_switches(int32_t* out, int capacity);

/* fp16 GEMM modes: log2 of the power of two the out-projection's input (relu(LayerNorm) over out_points * embed_dims / G elements:
 * |x| <= sqrt(n - 1)) is multiplied by before its fp16 split inside sbev_decoder_forward: 9 for n = 8192. */
int sbev_decoder_mixed_up_log2(const sbev_decoder_config* cfg);

/* Bytes of scratch sbev_decoder_forward needs for this config (-1 on an invalid config). */
int64_t sbev_decoder_workspace_bytes(const sbev_decoder_config* cfg);

/*
 * feats_nhwc  host array [L] of device pointers, level l = [B*T*N, H_l, W_l, D] channels-last (fp32 / bf16)
 * query_bbox  [B,Q,10], query_feat [B,Q,D], time_diff [B,T], lidar2img [B,T*N,4,4], vel_div [B] (or NULL if T == 1),
 * attn_mask   optional uint8 [Q,Q] (query denoising), NULL at inference
 * cls_out     [num_layers,B,Q,num_classes], bbox_out [num_layers,B,Q,code_size]  (NOT nan_to_num'ed)
 * workspace   256-byte aligned device scratch of >= sbev_decoder_workspace_bytes(cfg) bytes
 */
int sbev_decoder_forward(const sbev_decoder_config* cfg, const sbev_decoder_weights* weights,
                         const void* const* feats_nhwc, const float* query_bbox, const float* query_feat,
                         const float* time_diff, const float* lidar2img, const float* vel_div,
                         const uint8_t* attn_mask, float* cls_out, float* bbox_out,
                         void* workspace, int64_t workspace_bytes, sbev_stream_t stream);

/*
 * On-demand relayout (round 6).  The reference regroups EVERY pixel of every level on every call (models/sparsebev_transformer.py:73-85);
 * the gather reads the 4 bilinear corners of each sample point per level (models/csrc/msmv_sampling/msmv_sampling_forward.cu:41-66,
 * sparsebev_sampling.py:88-109) -- under half of the pyramid.  sbev_decoder_forward_lazy takes the reference's NCHW maps
 * [B*T*N, 256, H_l, W_l] as SOURCES (direct pointers, or entries of a device pointer table read at launch time: the replayable form)
 * and channels-last buffers of the same sizes as destinations (feats_nhwc; contents arbitrary): every layer's camera selection marks
 * the 64-pixel x 64-channel units its points read, one launch behind it moves the marked units this step has not moved yet.  Outputs are
 * bit-identical to sbev_nchw_to_nhwc_* followed by sbev_decoder_forward.  Dense pyramids of 4 groups x 64 channels
 * (sbev_decoder_lazy_supported); fp32 / bf16 / fp16 storage; 16-byte aligned sources and destinations.  Every argument after `lazy` as in
 * sbev_decoder_forward.
 */
typedef struct sbev_lazy_feats {
    const void* const* table;              /* device array of source pointers, or NULL */
    int32_t index[SBEV_MAX_LEVELS];        /* table != NULL: level l's NCHW source is table[index[l]] */
    const void* src[SBEV_MAX_LEVELS];      /* table == NULL: level l's NCHW source */
} sbev_lazy_feats;
int sbev_decoder_lazy_supported(const sbev_decoder_config* cfg);
/* Layers 1.. find and move the units their points marked and no earlier launch moved ("scan").  Up to 1024 rows in the fp16 GEMM modes that
 * scan rides in the generator GEMM's prologue (every generator workgroup takes its share before its first request: five launches per step
 * less at config 2); sbev_decoder_lazy_scan_launch(1) (env SBEV_LAZY_SCAN_LAUNCH=1) keeps it a launch of its own.  Bit-identical; returns
 * the previous setting.  Read when a step is enqueued / captured. */
int sbev_decoder_lazy_scan_launch(int enable);
int sbev_decoder_forward_lazy(const sbev_decoder_config* cfg, const sbev_decoder_weights* weights, void* const* feats_nhwc,
                              const sbev_lazy_feats* lazy, const float* query_bbox, const float* query_feat,
                              const float* time_diff, const float* lidar2img, const float* vel_div,
                              const uint8_t* attn_mask, float* cls_out, float* bbox_out,
                              void* workspace, int64_t workspace_bytes, sbev_stream_t stream);
/*
 * Prefix cache.  Three launches of layer 0 -- the position encoder + attention in-projection, the self attention and the parameter
 * generator GEMM -- read the queries and the weights and nothing of the frame.  The reference builds the queries from two weight tensors
 * on every call at eval (models/sparsebev_head.py:126-127, 217-218), so in real use they repeat bit for bit, in freshly allocated tensors.
 * sbev_decoder_forward_cached is sbev_decoder_forward (lazy == NULL) / sbev_decoder_forward_lazy with `cache`: device memory of the
 * caller's, 256-byte aligned, >= sbev_prefix_cache_bytes(cfg) bytes, NOT part of the workspace (workspaces may be shared between steps
 * with other queries).  A first launch of the step compares this call's queries with the copy in the cache, 16 bytes at a time as
 * integers, and refreshes the copy; where nothing differed the three launches return at once and the step reads their results of the
 * step that stored them.  Outputs are bit-identical either way.  The cache is used only on row-chain steps with the weight-stationary
 * generator, without attn_mask, without launch profiling and with 16-byte aligned queries (sbev_decoder_prefix_planned); on any other
 * step it is not touched at all, so its contents always belong to the stored query copy.
 * Layout: 32-bit words 0..3 are `armed`, `force`, `hits`, `misses`; the rest is private to the library.  The caller zeroes `armed`
 * (with the device idle on the cache, or in stream order) before the first use and whenever ANYTHING but the queries and the frame changes
 * under the same cache: weights, config, gemm mode, switches, pc_range, stream -- the next step then recomputes whatever the rest holds.
 * `force` != 0 makes every step recompute (the uncached step with the same launches); `hits` / `misses` count the steps that skipped /
 * recomputed.  cache == NULL: exactly sbev_decoder_forward / _lazy.  sbev_prefix_cache_bytes: -1 on an invalid config.
 */
int64_t sbev_prefix_cache_bytes(const sbev_decoder_config* cfg);
int sbev_decoder_forward_cached(const sbev_decoder_config* cfg, const sbev_decoder_weights* weights, void* const* feats_nhwc,
                                const sbev_lazy_feats* lazy, const float* query_bbox, const float* query_feat,
                                const float* time_diff, const float* lidar2img, const float* vel_div,
                                const uint8_t* attn_mask, float* cls_out, float* bbox_out,
                                void* workspace, int64_t workspace_bytes, sbev_stream_t stream, void* cache, int64_t cache_bytes);
/* Whether a step of this config / weight set under the current switches and profiling state would use a cache, given that one is passed
 * (cache_given), a mask is (mask_given) and the on-demand relayout is (lazy_given).  Pure host function; -1 on an invalid config. */
int sbev_decoder_prefix_planned(const sbev_decoder_config* cfg, const sbev_decoder_weights* weights, int cache_given, int mask_given,
                                int lazy_given);
/* The pieces, for callers that run the layers themselves: tiles of a pyramid (one 4-byte word of `need` and of `done` each; -1: shape not
 * covered); the marking form of sbev_sample_and_project (hw: [L][2] = (H_l, W_l); byte g of a tile's `need` word := 1 when a point of
 * group g reads one of its pixels); the move (first != 0: the step's first launch -- one workgroup per tile, `done` rebuilt from `need`;
 * else only need & ~done; last != 0 additionally clears `need` for the next step).  A stale `need` only moves more units. */
int64_t sbev_lazy_relayout_tiles(int n_levels, const int32_t* hw_pixels, int64_t n_images, int channels);
int sbev_sample_and_project_touch(const float* query_bbox, const float* offset, int64_t ld_offset,
                                  const float* scale_logits, int64_t ld_logits,
                                  const float* time_diff, const float* lidar2img, const double* pc_range,
                                  int B, int Q, int T, int N, int G, int P, int L,
                                  float image_h, float image_w, float eps,
                                  float* loc_bp, float* weights_bp, const int32_t* hw, uint32_t* need, sbev_stream_t stream);
int sbev_nchw_to_nhwc_lazy(const void* const* table, const int32_t* index, const void* const* src, void* const* out, int n_levels,
                           const int32_t* hw_pixels, int64_t n_images, int channels, int dtype, uint32_t* need, uint32_t* done, int first,
                           int last, sbev_stream_t stream);

/*
 * hipGraph capture of one decoder step: the launch sequence of sbev_decoder_forward is static per (config, pointer
 * set), so it can be recorded once on `stream` (explicit, non-default; nothing executes during the capture) and
 * replayed per sample.  The graph reads its inputs through the captured device pointers: refresh them in place
 * (cfg->slot_table is one of them; cfg->frame_slots is captured BY VALUE: a new ring order needs a new capture).
 * The workspace and every input / output buffer must outlive the graph.  Replaces per-call Python/launch overhead
 * of the reference's eager module chain (models/sparsebev_transformer.py:86-97).
 */
typedef struct sbev_graph sbev_graph;
int sbev_decoder_capture(const sbev_decoder_config* cfg, const sbev_decoder_weights* weights,
                         const void* const* feats_nhwc, const float* query_bbox, const float* query_feat,
                         const float* time_diff, const float* lidar2img, const float* vel_div,
                         const uint8_t* attn_mask, float* cls_out, float* bbox_out,
                         void* workspace, int64_t workspace_bytes, sbev_stream_t stream, sbev_graph** out);
/* Capture of ANY sequence of this library's launches on `stream` (explicit, non-default) between the two calls -- e.g. the per-level
 * NCHW -> NHWC relayout followed by sbev_decoder_forward: the whole per-sample step as one replayable graph.  Nothing executes
 * during the capture; every buffer the recorded launches read or write must outlive the graph.  sbev_capture_end(stream, NULL)
 * abandons a capture (after a failed call inside it). */
int sbev_capture_begin(sbev_stream_t stream);
int sbev_capture_end(sbev_stream_t stream, sbev_graph** out);
int sbev_graph_launch(sbev_graph* graph, sbev_stream_t stream);
int64_t sbev_graph_num_nodes(const sbev_graph* graph);   /* kernel nodes recorded (-1 for NULL) */
int sbev_graph_destroy(sbev_graph* graph);

/* Bracket launches with HIP events on their stream -- `enable` is a bit mask of kinds: 1 = every sbev_msmv_fwd launch,
 * 2 = the parameter-generator GEMM, 4 = the out-projection GEMM, 8 = the fused gather + mixing launch, 0 = off -- and read back + clear the elapsed times in ms
 * (blocks until those launches finished).  Measurement aid for bench.py's roofline figures. */
int sbev_profile_sampler(int enable);
int sbev_profile_sampler_read(float* ms, int max_n);
/* The events are not free (two records around a launch leave ~5.6 us of idle stream each -- 2 % of a decoder step for the
 * six sampler launches): bracket the launches of only every n-th sbev_decoder_forward call (n = 1: every call, the default).
 * Resets the call counter, so the first call after it is a bracketed one. */
int sbev_profile_stride(int every_n_calls);
/* Same for the other bracketed launches: kind 0 = sampler, 1 = parameter-generator GEMM, 2 = out-projection GEMM, 3 = fused gather + mixing. */
int sbev_profile_read(int kind, float* ms, int max_n);

/*
 * The keyed frame pool's insert: a step's NEW frames into their slots, in the memory the backbone emits, recordable inside a captured step:
 * one launch for n_frames frame sets x n_levels levels x B samples.  Source (k, l) -- frame set k of the step's offered window positions,
 * level l -- is src[k * n_levels + l] (table == NULL) or table[index[k * n_levels + l]] read on the device when the kernel starts (src ==
 * NULL; the device pointer table of a replayable step, see sbev_nchw_to_nhwc_f32_indirect); exactly one of the two forms,
 * 1 <= n_frames <= SBEV_MAX_FRAMES, 1 <= n_levels <= SBEV_MAX_LEVELS; index and src are host arrays of n_frames * n_levels entries, out and
 * hw_pixels of n_levels.  src_layout (enum sbev_frames_layout), one value per call: SBEV_FRAMES_NCHW = [B, n_views, channels,
 * hw_pixels[l]], SBEV_FRAMES_NHWC = channels-last [B, n_views, hw_pixels[l], channels].  insert is a device int32 [n_frames, B], refreshed
 * by the host per step like the slot table of sbev_msmv_fwd_pool: sample b's frame of set k goes to slot insert[k * B + b] of the pool's
 * resident buffer out[l] = [B, n_slots, n_views, hw_pixels[l], channels]; an entry outside [0, n_slots) --
 * use -1 -- means none: nothing of that (k, b) is read or written.  Entries are NOT clamped: this launch writes.  Two live entries of one
 * sample must name DIFFERENT slots -- the host planner's duty (cache.SlotBook.plan_frames); the kernel cannot check it, and two frame
 * sets writing one slot race.  src_dtype -> dst_dtype (enum sbev_dtype): fp32 -> fp32; fp16 -> fp16 and bf16 -> bf16, moved as bytes;
 * fp16 -> fp32 and bf16 -> fp32, widened exactly.  Everything else is SBEV_EINVAL: fp32 into 2-byte slots would be lossy, as would fp16
 * into bf16.  Any sizes: per level the vector form where hw and channels allow it (NCHW: hw % 4 == 0 and channels % 4 == 0, % 8 for a
 * 2-byte source; channels-last: one sample's n_views * hw * channels source bytes a multiple of 16), else a scalar form.  Sources and
 * destinations 16-byte aligned.  B == 0 is an empty call.
 * Replaces: the reference's per-frame extract-then-cat (models/sparsebev.py:255-321) for every missing frame of a window, and this library's
 *           own B x L eager sbev_nchw_to_nhwc_* / sbev_copy_widen_f32 launches in front of a replayed step.
 */
enum sbev_frames_layout { SBEV_FRAMES_NCHW = 0, SBEV_FRAMES_NHWC = 1 };
int sbev_pool_insert_frames(const void* const* table, const int32_t* index, const void* const* src, void* const* out, int n_frames,
                            int n_levels, const int32_t* hw_pixels, int B, int n_views, int channels, int src_layout, int src_dtype,
                            int dst_dtype, const int32_t* insert, int n_slots, sbev_stream_t stream);

/*
 * One frame per sample: sbev_pool_insert_frames with n_frames = 1, SBEV_FRAMES_NCHW, src_dtype = dst_dtype = dtype and insert = [B] -- the
 * same kernel, the same bytes.  Its refusals are worded for itself ("sbev_pool_insert: ...", "dtype", "level l", "plane too large"), and
 * its size bound is channels * hw_pixels[l] <= INT32_MAX where the frames entry bounds channels * hw_pixels[l] * n_views.
 */
int sbev_pool_insert(const void* const* table, const int32_t* index, const void* const* src, void* const* out, int n_levels,
                     const int32_t* hw_pixels, int B, int n_views, int channels, int dtype, const int32_t* insert, int n_slots,
                     sbev_stream_t stream);

/*
 * The detector's GPU-side image stage as ONE launch for all n = B * N images of a step: load, photometric distortion, BGR -> RGB,
 * normalise, zero pad to a multiple of `div`, GridMask, store.
 * Replaces: the pre-backbone lines of SparseBEV.extract_feat (models/sparsebev.py:61-100: .float(), color_aug, mean / std, pad_multiple)
 *           and the GridMask in front of the backbone (models/sparsebev.py:48-49), i.e. GpuPhotoMetricDistortion, rgb_to_hsv, hsv_to_rgb,
 *           pad_multiple and GridMask of models/utils.py -- a few dozen torch passes over the fp32 image tensor.
 * src [n, 3, H, W] contiguous, SBEV_U8 or SBEV_F32; dst [n, 3, Hp, Wp] contiguous, SBEV_F32 or SBEV_F16, Hp = ceil(H / div) * div and Wp
 * likewise; every element of dst is stored by this launch, the padding as zeros.  mean, std: HOST arrays of 3, passed on by value;
 * to_rgb: img_norm_cfg's flag.  Per pixel, in fp32, every operation rounded on its own and in the reference's order: float(src) read as
 * RGB; + delta; * alpha (mode 0); rgb_to_hsv; s * sat; h + hue; h > 360 -> h - 360, then h < 0 -> h + 360; hsv_to_rgb; * alpha (mode 1);
 * the channel permutation; RGB -> BGR; the to_rgb flip; - mean[c]; / std[c] (a division); the pad; the mask; the cast.  No clamp.
 * colour_on == 0 skips everything up to the to_rgb flip (the reference outside training); with colour_on != 0 EVERY image takes the HSV
 * round trip, whatever its flags (as in the reference).
 * table: device memory, 16-byte aligned, SBEV_FRONT_ROW_BYTES per image, read when the kernel runs (a captured launch serves every step:
 * refresh the table in place).  NULL: no distortion, no mask -- the inference call (colour_on must be 0).  One row, 16 little-endian
 * 32-bit words:
 *    0 int32  flags: bit 0 brightness, 1 contrast, 2 saturation, 3 hue, 4 channel swap -- "this transform is applied"
 *    1 int32  contrast mode: 0 = before the HSV round trip, 1 = after it
 *    2 float  delta   3 float alpha   4 float saturation factor   5 float hue shift (degrees)
 *    6..8 int32  the permutation p: channel k of the distorted RGB image becomes channel p[k] of the old one (imgs[idx, p])
 *    9 int32  GridMask applied   10 int32 d   11 int32 l   12 int32 st_h   13 int32 st_w     (built on the padded size; a pixel is KEPT
 *             iff it lies on a row stripe or a column stripe, models/utils.py:15-46; d < 1 is "not applied")
 *    14, 15 unused (zero)
 * sbev_image_front_plan (pure host): out[0] = Hp, out[1] = Wp, out[2] = elements of dst, out[3] = bytes of the table, out[4] = workgroups.
 * Checked before any GPU call (SBEV_EINVAL): null src / dst / mean / std, n, H, W or div < 1, a dtype not listed above, std[c] == 0, a
 * table that is not 16-byte aligned, colour_on without a table, src / dst not aligned to their element size, a padded size or grid
 * beyond 32 bits.
 */
#define SBEV_FRONT_ROW_BYTES 64
int sbev_image_front_plan(int n, int H, int W, int div, int64_t* out);
int sbev_image_front(const void* src, int src_dtype, void* dst, int dst_dtype, int n, int H, int W, int div, const float* mean,
                     const float* std, int to_rgb, int colour_on, const void* table, sbev_stream_t stream);

/*
 * The loader's image geometry as ONE launch for all n images of a step: decoded camera frames in, the front end's input out.
 * Replaces: RandomTransformImage of loaders/pipelines/transforms.py (PIL resize -- bicubic, antialiased --, crop with black fill,
 *           FLIP_LEFT_RIGHT) and the format bundle's HWC -> CHW, which run on the host at 19-28 ms per 900 x 1600 frame.
 * src [n, H, W, 3] uint8 contiguous (4-byte aligned); dst [n, 3, fH, fW] uint8 contiguous; every byte of dst is stored.  The result
 * equals Pillow's at every byte: Pillow's 8-bit resampler is integer arithmetic (coefficients rounded to 22 fractional bits, an int
 * accumulator from 1 << 21, >> 22, clamp, uint8 between the horizontal and the vertical pass) and the kernel does the same.
 * Output pixel (y, x) of image i reads resized pixel (crop_y + y, crop_x + x'), x' = fW - 1 - x if mirrored, else x; a coordinate
 * outside the resized image gives 0.
 * table: device memory, 16-byte aligned: n_transforms blocks written by sbev_image_geom_plan, one per sample; image_rows: int32 [n] on
 * the device, the block of each image (clamped to [0, n_transforms)).  Both are read when the kernel runs: a captured launch serves
 * every step, refresh them in place.  A block, in little-endian int32 words (block bytes = out[0] of the plan, a multiple of 16):
 *    0 newW   1 newH   2 crop_x   3 crop_y   4 flip   5 ksize_x   6 ksize_y   7 unused (zero)
 *    8 ..                 (first, count) of the fW kept columns: source columns first .. first + count - 1; count 0 = outside
 *    8 + 2 fW ..          (first, count) of the fH kept rows
 *    xk = round up to 4 words of (8 + 2 fW + 2 fH) ..   int32 coefficients [fW, SBEV_GEOM_KMAX], zero beyond count
 *    xk + 16 fW ..        int32 coefficients [fH, SBEV_GEOM_KMAX]
 * sbev_image_geom_plan (pure host) writes one block into table_out (host memory; NULL: sizes only) for the source H x W resized to
 * resize_w x resize_h and cropped at (crop_x, crop_y) to fW x fH.  Coefficients in double, in Pillow's order: scale = in / out,
 * filterscale = max(scale, 1), support = 2 * filterscale, center = (xx + 0.5) * scale, xmin = (int)(center - support + 0.5) clamped to
 * 0, xmax likewise clamped to the input size, weights bicubic((x + xmin - center + 0.5) * (1 / filterscale)) with a = -0.5, summed in
 * order, divided by the sum, (int)(+-0.5 + w * 2^22) by sign.  ksize = 2 * ceil(support) + 1.
 *    out[0] block bytes   out[1] workgroups per image   out[2] ksize_x   out[3] ksize_y   out[4] source bytes the taps read per image
 *    (0 without table_out)   out[5], out[6] the kernel's output tile (width, height)   out[7] source rows read (0 without table_out)
 * Checked before any GPU call (SBEV_EINVAL): null pointers, sizes < 1 or above 2^22 - 1, a ksize above SBEV_GEOM_KMAX (an axis shrunk
 * by more than 3.5: refused, never truncated), a misaligned table / image_rows / src, a grid beyond 31 bits.
 */
#define SBEV_GEOM_KMAX 16
int sbev_image_geom_plan(int H, int W, int fH, int fW, int resize_w, int resize_h, int crop_x, int crop_y, int flip, int32_t* table_out,
                         int64_t* out);
int sbev_image_geom(const void* src, void* dst, int n, int H, int W, int fH, int fW, const void* table, const void* image_rows,
                    int n_transforms, sbev_stream_t stream);

/*
 * The FPN neck between the backbone and the decoder (its backward: sbev_fpn_backward below): L + 1 launches for L input levels on v_mfma_f32_32x32x16_f16.
 * Replaces: mmdet's FPN forward as the detector configures it (in_channels = the backbone's stages, out_channels = 256, num_outs levels,
 *           no extra convolutions) under fp16 autocast (models/sparsebev.py:46): 2 L convolutions, L - 1 interpolate + add pairs and
 *           the casts around them, each a launch of its own, and the NCHW -> channels-last relayout in front of the decoder.
 * Levels l = 0 .. L - 1, finest first, described by chw = {Cin_0, H_0, W_0, Cin_1, ...}; n images.  Everything is channels-last:
 *   inputs[l]  [n, H_l, W_l, Cin_l]  SBEV_F16 or SBEV_F32 (one dtype for all levels)
 *   outs[o]    [n, H_o, W_o, 256]    SBEV_F16 or SBEV_F32, o = 0 .. num_outs - 1; every element is stored by the call
 *   workspace  the merged laterals M_l as fp16 [n, H_l, W_l, 256], level after level (out[2] bytes of the plan); left valid for the caller
 * Arithmetic: operands are fp16 -- fp32 inputs and the fp32 weights are rounded once, to nearest even --, products are accumulated in
 * fp32 on the matrix core, biases are fp32.
 *   M_{L-1} = fp16(conv1x1(C_{L-1}) + b);   M_l = fp16((conv1x1(C_l) + b_l) + float(M_{l+1}[nearest])), the sum in fp32, one rounding
 *   nearest: F.interpolate(size = (H_l, W_l), mode = 'nearest') for any pair of sizes: source index min(floor(dst * float32(in / out)),
 *            in - 1) with the product rounded in float32
 *   outs[l] = conv3x3(M_l, zero pad 1) + b_l in fp32, stored as it is or rounded once to fp16
 *   outs[L - 1 + e], e = 1 .. num_outs - L: rows 0, 2^e, .. and columns 0, 2^e, .. of outs[L - 1] (F.max_pool2d(prev, 1, stride = 2)
 *            applied e times), [n, ceil(H / 2^e), ceil(W / 2^e), 256], written by the same launch
 * Weights: sbev_fpn_pack_weights rounds lateral_w[l] [256, Cin_l, 1, 1] and fpn_w[l] [256, 256, 3, 3] (contiguous, w_dtype SBEV_F32 or
 * SBEV_F16, device memory) to fp16 in MFMA fragment order into `pack` (out[1] bytes of the plan, device memory); 2 L small launches,
 * to be repeated whenever a weight changes.  Biases are read as they are: lateral_bias[l], fpn_bias[l] fp32 [256] on the device.
 * The pointer lists are host arrays, read during the call.
 * sbev_fpn_plan (pure host): out[SBEV_FPN_PLAN_WORDS]:
 *    0 launches of a forward (L + 1; 0 for n == 0)   1 pack bytes   2 workspace bytes   3 pixels of all merged laterals
 *    4 workgroups of the convolution launch   5 .. 8 workgroups of the lateral launch of level 0 .. 3 (128 pixels each)
 *    9 extra levels   10 + 2 (e - 1), 11 + 2 (e - 1): height and width of extra level e   the rest zero
 * Checked before any GPU call (SBEV_EINVAL): L outside 1 .. SBEV_FPN_MAX_IN, num_outs outside L .. SBEV_FPN_MAX_OUT, n < 0, Cin_l not a
 * multiple of 32 in 32 .. 65536, an empty plane or a side above 32767, more pixels than 32-bit indices hold, a dtype not listed; then
 * n == 0 answers SBEV_OK; then null pointers; then 16-byte alignment of inputs, outs, pack and workspace (4-byte of the biases).
 */
#define SBEV_FPN_MAX_IN 4
#define SBEV_FPN_MAX_OUT 5
#define SBEV_FPN_PLAN_WORDS 18
int sbev_fpn_plan(int n_levels, const int32_t* chw, int64_t n, int num_outs, int64_t* out);
int sbev_fpn_pack_weights(int n_levels, const int32_t* chw, const void* const* lateral_w, const void* const* fpn_w, int w_dtype, void* pack,
                          sbev_stream_t stream);
int sbev_fpn_forward(int n_levels, const int32_t* chw, int64_t n, int num_outs, const void* const* inputs, int in_dtype, const void* pack,
                     const float* const* lateral_bias, const float* const* fpn_bias, void* workspace, void* const* outs, int out_dtype,
                     sbev_stream_t stream);

/*
 * The FPN neck's backward: from the output gradients to the gradients of the inputs, weights and biases, 4 L + 1 launches (5 L + 1 with
 * input gradients) and one tiny launch that clears the 16 head bytes (a kernel, not a memset node), all four GEMM families on v_mfma_f32_32x32x16_f16 with fp32 accumulation.
 * Replaces: autograd through mmdet's FPN under fp16 autocast (the backward of 2 L convolutions, the interpolate / add / cast nodes).
 * The forward is sbev_fpn_forward's; the rounding to fp16 in M_l is straight-through (derivative 1), as under autocast.
 *   grad_outs[o]   gP_o [n, H_o, W_o, 256] channels-last, g_dtype SBEV_F32 or SBEV_F16, o = 0 .. num_outs - 1
 *   inputs[l]      C_l as the forward read them (in_dtype); merged: the forward's workspace (M_l, fp16, level after level)
 *   grad_inputs    null (no input gradient), or per level a [n, H_l, W_l, Cin_l] destination of in_dtype (a null entry skips the level)
 *   grad_lateral_w[l] [256, Cin_l], grad_lateral_bias[l] [256], grad_fpn_w[l] [256, 256, 3, 3], grad_fpn_bias[l] [256]: fp32, every
 *                  element is stored by the call (nothing is accumulated into)
 * Definition (tests/fpn_bwd_cases.py restates it in fp64):
 *   scale   amax = max |gP_o| over all outputs, found on the device; (2^e, 2^-e) with 2^e amax in [2^W, 2^(W+1)), W =
 *           SBEV_FPN_GRAD_WINDOW_LOG2 = 3, e capped at 126, is written to the first 8 bytes of the workspace and read from there by every
 *           consumer: no host read, no synchronisation, the call can be captured.  amax zero or non-finite: e = 0.  This is ONE rule
 *           with sbev_resnet_backward's scale (one implementation; SBEV_RESNET_GRAD_WINDOW_LOG2 is the same constant).  Workspace head,
 *           32-bit words: [0] 2^e  [1] 2^-e  (floats)  [2] amax bits  [3] ticket.  Every gradient
 *           operand is fp16 in the scaled domain: 2^12 of headroom below 65504, full fp16 precision down to 2^-18 amax.  A non-finite
 *           gP or an fp16 overflow of an intermediate travels as inf / NaN into the parameter gradients, never as a wrong finite value.
 *   G_l     = gP_l for l < L - 1; G_{L-1} = gP_{L-1} + gP_L + gP_{L+1} .. at the pixels with y, x multiples of 2, 4, .. (the extra
 *           levels' sources), added in that order in fp32.  g_l = fp16(2^e G_l), rounded once on the way into LDS.
 *   D_l     = conv3x3(g_l, W3_l'), W3'[ci, co, ky, kx] = fp16(W3[co, ci, 2 - ky, 2 - kx]), fp32 accumulation
 *   gM_0    = fp16(D_0);  gM_l = fp16(D_l + S), S = the fp32 sum, row-major from zero, of gM_{l-1} over the pixel's children: the (y, x)
 *           of level l - 1 whose nearest source under the forward's float32 rule is this pixel (any ratio).  No atomics.
 *   gC_l    = 2^-e gM_l . fp16(Wlat_l), stored in in_dtype
 *   gW3_l[co, ci, ky, kx] = 2^-e sum_p g_l[p, co] M_l[p + (ky - 1, kx - 1), ci] (zero outside the plane)
 *   gWlat_l[co, ci]       = 2^-e sum_p gM_l[p, co] fp16(C_l[p, ci])
 *   gc_l = 2^-e sum_p g_l[p, :],  gblat_l = 2^-e sum_p gM_l[p, :]
 *           The reductions over pixels p (all images of the level, row-major) are split into slabs of slab_len pixels: the matrix
 *           products accumulate a slab in fp32 on the matrix core, the bias sums add a slab pixel after pixel in fp32; the slabs'
 *           partials are then added in order 0, 1, .. and multiplied by 2^-e.  Bit-reproducible.
 * sbev_fpn_pack_weights_bwd: the flipped / transposed 3x3 images and the transposed lateral images, fp16 in fragment order, into `pack`
 * (out[2] bytes of the plan: as many as the forward's image); 2 L small launches, repeated whenever a weight changes.
 * sbev_fpn_backward_plan (pure host): out[SBEV_FPN_BWD_PLAN_WORDS]:
 *    0 launches of a backward (0 for n == 0)   1 workspace bytes   2 pack bytes   3 .. 6 slabs of level 0 .. 3   7 .. 10 their slab_len
 *    (max(512, ceil(pixels / 16) rounded up to 256))   11, 12, 13 byte offsets in the workspace of gM (fp16, all levels, as `merged`),
 *    of D_1 .. D_{L-1} (fp32) and of the slab partials   the rest zero.  Workspace bytes 0 .. 7 hold (2^e, 2^-e) after a call.
 * Checked before any GPU call, like sbev_fpn_forward: the plan's refusals, the dtypes; n == 0 answers SBEV_OK; null pointers; 16-byte
 * alignment of inputs, merged, grad_outs, grad_inputs, pack and workspace (4-byte of the fp32 gradients).
 */
#define SBEV_FPN_GRAD_WINDOW_LOG2 3
#define SBEV_FPN_BWD_PLAN_WORDS 16
int sbev_fpn_backward_plan(int n_levels, const int32_t* chw, int64_t n, int num_outs, int want_input_grads, int64_t* out);
int sbev_fpn_pack_weights_bwd(int n_levels, const int32_t* chw, const void* const* lateral_w, const void* const* fpn_w, int w_dtype,
                              void* pack, sbev_stream_t stream);
int sbev_fpn_backward(int n_levels, const int32_t* chw, int64_t n, int num_outs, const void* const* inputs, int in_dtype,
                      const void* merged, const void* const* grad_outs, int g_dtype, const void* pack_bwd, void* workspace,
                      void* const* grad_inputs, float* const* grad_lateral_w, float* const* grad_lateral_bias, float* const* grad_fpn_w,
                      float* const* grad_fpn_bias, sbev_stream_t stream);

/*
 * The ResNet backbone between the image front end and the FPN neck, inference only: the Bottleneck nets (depth 50 / 101 / 152, style
 * 'pytorch': the stage's stride on the 3 x 3), BatchNorm in eval mode folded into the convolutions, on v_mfma_f32_32x32x16_f16.
 * Replaces: mmdet's ResNet forward with norm_eval=True under fp16 autocast (configs/r50_nuimg_704x256.py:31-40): per convolution a
 *           convolution, a BatchNorm, a ReLU / add and the casts around them, each a launch of its own.
 * The net: depth picks the blocks per stage ((3,4,6,3), (3,4,23,3), (3,8,36,3)); stage_blocks, when not null, overrides them
 * (num_stages entries); stage s has mid = base_channels 2^s channels, 4 mid output channels, stride 1 (s = 0) or 2 on its first block.
 *   x          [n, 3, H, W] NCHW contiguous, SBEV_F32 or SBEV_F16
 *   outs[k]    [n, h, w, C] channels-last fp16: the output of stage out_indices[k] (increasing), every element stored by the call
 *   workspace  out[2] bytes of the plan: the activations between the launches
 * Plane sizes: stem floor((H + 6 - 7) / 2) + 1; pool and every stride-2 3 x 3 floor((H + 2 - 3) / 2) + 1; stride-2 1 x 1 floor((H - 1) / 2) + 1.
 * Arithmetic.  The fold, per output channel, in fp32 with every operation rounded on its own (true division, true square root):
 *   s = gamma / sqrt(var + eps),   w' = fp16(w * s),   b' = beta - mean * s
 * Every convolution: operands fp16 (w' and the previous activation; the stem rounds an fp32 image once, to nearest even), products
 * accumulated in fp32 on the matrix core, y = acc + b' [+ float(residual)] [then max(y, 0)] in fp32, rounded once to fp16, stored
 * channels-last.  Zero padding.  A block: conv1 1 x 1 + ReLU; conv2 3 x 3 (pad 1, the block's stride) + ReLU; conv3 1 x 1 + residual +
 * ReLU; on a stage's first block the residual is downsample = 1 x 1 (the block's stride), no ReLU, else the block's input.  The stem:
 * 7 x 7 / 2 / pad 3 + ReLU, K = 147 in the weight's own (c, ky, kx) order padded with zeros to 160.  The max-pool 3 x 3 / 2 / pad 1
 * ignores its padding: a true maximum, exact.  K split: where the plan says 3, the chunks of 64 reduction indices (tap-major, then channels)
 * are dealt to three groups of waves in turn (chunk c to group c mod 3), each accumulates its own on the matrix core, and acc = (g0 + g1) + g2
 * in fp32, in that order.  One lane owns each stored element, no atomics: bit-reproducible.
 * Launch order (the order of the plan's layers, of sbev_resnet_pack_weights' lists for a whole net, and of keep): stem, pool, then per
 * block conv1, conv2, [downsample], conv3: 2 + 3 blocks + num_stages launches (54 for ResNet-50), all enqueued by one call on one stream,
 * nothing allocated, nothing synchronised.
 *
 * sbev_resnet_plan (pure host): out[SBEV_RESNET_PLAN_WORDS]:
 *    0 launches of a forward (0 for n == 0)   1 pack bytes   2 workspace bytes   3 layers   4 multiply-adds of a forward   5 outputs
 *    6 + 3 k .. 8 + 3 k: C, h, w of outs[k]   then from word SBEV_RESNET_PLAN_HEAD, SBEV_RESNET_LAYER_WORDS per layer:
 *    kind (0 stem, 1 pool, 2 convolution), Cin, Cout, taps (49: the stem), stride, h, w (the output plane), row tiles (128 output pixels),
 *    column tiles, K split (1 or 3), where the output lives (a byte offset in the workspace, or -(1 + k): outs[k]), epilogue
 *    the rest zero.  keep != 0: every layer's output has a workspace region of its own (tests read them back); keep == 0: five regions,
 *    reused (two for block outputs, conv1's, conv2's and downsample's).  Column tiles: the widest of 256 / 128 / 64 channels that divides
 *    Cout and still gives at least 256 workgroups, 64 where none does.  K split: 3 where 64-channel tiles give fewer than 256 workgroups
 *    and K has 6 chunks or more (the split is inside the workgroup: no workspace, no extra launch), else 1.
 * sbev_resnet_pack_weights: fold and pack n_layers convolutions, desc = {Cin, Cout, taps} each (taps 1, 9, or 49 with Cin = 3 for the
 *    stem), w[i] [Cout, Cin, kh, kw] contiguous (w_dtype SBEV_F32 or SBEV_F16), gamma / beta / mean / var fp32 [Cout], all device memory;
 *    layer after layer into `pack`: fragment-order fp16 w' (taps Cin Cout halves; the stem 160 Cout), then fp32 b' [Cout].  One small
 *    launch per layer on the stream; to be repeated whenever a weight or a statistic changes.
 * sbev_conv_f16: ONE convolution of the family on raw pointers: x [n, H, W, Cin], y [n, h, w, Cout], residual as y (epilogue 2 only),
 *    pack = one layer's image; taps 1 or 9, stride 1 or 2, epilogue 0 bias / 1 + ReLU / 2 + residual + ReLU, col_tile 0 (the plan's choice)
 *    or 64 / 128 / 256; the K split follows the plan's rule for the shape and the column tile.
 * Checked before any GPU call (SBEV_EINVAL): a depth other than 50 / 101 / 152 (18 / 34 are BasicBlock nets), num_stages outside 1 .. 4,
 * base_channels / Cin / Cout not a multiple of 64, n < 0, an empty plane or a side above 32767, more output pixels in a layer than 32-bit
 * row indices hold, out_indices not increasing stage numbers, a dtype / taps / stride / epilogue / col_tile not listed; then n == 0
 * answers SBEV_OK; then null pointers; then 16-byte alignment of x, pack, workspace, outs, residual, y (element alignment of the
 * tensors sbev_resnet_pack_weights reads).
 */
#define SBEV_RESNET_MAX_LAYERS 160
#define SBEV_RESNET_PLAN_HEAD 18
#define SBEV_RESNET_LAYER_WORDS 12
#define SBEV_RESNET_PLAN_WORDS (SBEV_RESNET_PLAN_HEAD + SBEV_RESNET_LAYER_WORDS * SBEV_RESNET_MAX_LAYERS)
int sbev_resnet_plan(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                     const int32_t* out_indices, int keep, int64_t* out);
int sbev_resnet_pack_weights(int n_layers, const int32_t* desc, const void* const* w, const float* const* gamma, const float* const* beta,
                             const float* const* mean, const float* const* var, float eps, int w_dtype, void* pack, sbev_stream_t stream);
int sbev_conv_f16(const void* x, const void* pack, const void* residual, void* y, int64_t n, int H, int W, int Cin, int Cout, int taps,
                  int stride, int epilogue, int col_tile, sbev_stream_t stream);
int sbev_resnet_forward(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                        const int32_t* out_indices, int keep, const void* x, int x_dtype, const void* pack, void* workspace,
                        void* const* outs, sbev_stream_t stream);

/*
 * The ResNet backbone's backward: from the gradients of the stage maps to the gradients of the convolution weights and the BatchNorm
 * gamma / beta of the trainable stages, on v_mfma_f32_32x32x16_f16 with fp32 accumulation.  BatchNorm stays in eval mode (norm_eval=True:
 * running statistics), so its backward is the backward of the fold.
 * Replaces: autograd through mmdet's ResNet under fp16 autocast with frozen_stages = first_trainable_stage - 1 and norm_eval=True.
 * first_trainable_stage is 1 .. num_stages (mmdet's frozen_stages + 1): the stem, the pool and the stages before it get no gradient of any
 * kind, and no image gradient is ever produced.  0 (a trainable stem: the 7 x 7 weight gradient and the max-pool backward) is refused.
 *
 * sbev_resnet_forward_train: sbev_resnet_forward's launches and arithmetic, bit for bit, but every activation from the output of the last
 *   frozen launch (`first_kept`: the pool, or the last frozen stage's output) onward lives in the caller's `acts` buffer (plan word 3
 *   bytes), each launch at its own 256-byte aligned offset in launch order; the stage maps still go to outs[k]; the frozen launches
 *   ping-pong in `workspace` (sbev_resnet_plan's bytes with keep = 0) as before.
 *
 * Definition (tests/resnet_bwd_cases.py restates it in fp64).  A block with input x: a1 = relu(conv1(x)), a2 = relu(conv2(a1)),
 * r = x or downsample(x), out = relu(conv3(a2) + r), all stored fp16 by the forward; w' = fp16(w s), s = gamma / sqrt(var + eps).  The
 * roundings of w' and of the stored activations are straight-through (derivative 1).  A ReLU's derivative is read from the stored fp16
 * activation: 1 where it is > 0, else 0 (a select, not a product: a masked inf is 0).
 *   scale   amax = max |gP_k| over grad_outs, found on the device; (2^e, 2^-e) with 2^e amax in [2^W, 2^(W+1)), W =
 *           SBEV_RESNET_GRAD_WINDOW_LOG2 = 3, e capped at 126, e = 0 for a zero or non-finite amax; the pair is written to the first 8
 *           bytes of the workspace and read from there by every consumer: no host read, no synchronisation.  ONE rule with
 *           sbev_fpn_backward's scale (one implementation, the same workspace head; SBEV_FPN_GRAD_WINDOW_LOG2 is the same constant).
 *           A non-finite gP or an fp16
 *           overflow of an intermediate travels as inf / NaN into the parameter gradients, never as a wrong finite value.
 *   blocks, last to first, in the scaled domain, G_out the fp32 gradient of a block's out:
 *     g3 = fp16(G_out [out > 0])                        (the gradient at conv3's output and at r)
 *     g2 = fp16(dgrad_1x1(g3, w3') [a2 > 0])
 *     g1 = fp16(dgrad_3x3,stride(g2, w2') [a1 > 0])
 *     G_x = dgrad_1x1(g1, w1') + R, the previous block's G_out.  Identity residual: R = float(g3), added to the finished accumulator.
 *           First block of a stage: the downsample's products dgrad_1x1,stride(g3, wd') -- they land on the pixels (S y, S x) the strided
 *           1 x 1 read and are zero elsewhere -- CONTINUE conv1's accumulation in the same fp32 accumulator (K = conv1's output
 *           channels first, then the downsample's).  Where x is a stage output listed in out_indices, 2^e float(gP_k) (the product
 *           rounded on its own) is added last.  So the order is ((conv1 products, then downsample products) + float(g3)) + 2^e gP.
 *     The net's last block starts from G_out = 2^e gP (zero when the last stage is not in out_indices); a stage output that is not in
 *     out_indices gets no addend.  In the first trainable stage's first block no data gradient leaves conv1 or the downsample.
 *     A data gradient multiplies the fp16 w' transposed (for a 3 x 3 also flipped: tap (ky, kx) -> (2 - ky, 2 - kx)); at stride 2 an input
 *     pixel sums only the taps whose source (Y + 1 - ky, X + 1 - kx) is even in both coordinates.  K runs tap-major, then channels, in
 *     chunks of 64 on the matrix core; every stored element is rounded once.
 *   per trainable convolution, g_y the stored fp16 gradient at its output, x_in its stored fp16 input:
 *     gW'[co, ci, ky, kx] = 2^-e sum_p g_y[p, co] x_in[S p + (ky - 1, kx - 1), ci] (zero outside the plane; a 1 x 1 reads S p),
 *     gb'[co] = 2^-e sum_p g_y[p, co].  The reduction over the output pixels p (all images, row-major) is cut into slabs of slab_len =
 *     max(512, ceil(pixels / 16) rounded up to 256) pixels: the products accumulate a slab in fp32 on the matrix core in steps of 32
 *     pixels, the bias sums add a slab pixel after pixel in fp32; the partials are added in slab order 0, 1, .. and then multiplied by 2^-e.
 *   fold backward, fp32, every operation rounded on its own, root = sqrt(var + eps), s = gamma / root, rinv = 1 / root:
 *     g_w = s gW'      g_beta = gb'      g_gamma = rinv (D - mean gb'),  D = sum_k w[co, k] gW'[co, k]  (= sum_p g_y z for the raw convolution z)
 *     D's order: lane t of 256 adds its products from zero, tap after tap (tap 0 first) and within a tap ci = t, t + 256, .. ascending;
 *     then for h = 128, 64, .. 1: lane t < h adds lane t + h's sum to its own.
 *   All results are fp32 and every element is stored by the call; nothing is accumulated into.  Bit-reproducible: one owner per stored
 *   element, no float atomics.
 *
 * sbev_resnet_backward: one call enqueues everything on one stream, allocates nothing and synchronises nothing (it can be captured):
 *   a clear of the 16 head bytes (a launch, not a memset node), the amax, the seed of the last block, then per block (last first) weight gradient + fold of conv3, the data
 *   gradient to a2, the same for conv2 and a1, weight gradient + fold of conv1 and of the downsample, the data gradient to x.
 *   acts / outs as sbev_resnet_forward_train left them; grad_outs[k] [n, h, w, C] channels-last of g_dtype (SBEV_F32 or SBEV_F16);
 *   w / gamma / mean / var / grad_w / grad_gamma / grad_beta: one entry per CONVOLUTION in launch order as sbev_resnet_pack_weights
 *   lists a whole net (entry 0 the stem, entry j the launch j + 1); entries of frozen convolutions are not read; a null grad_gamma[j] /
 *   grad_beta[j] skips that result (a frozen norm).
 * sbev_resnet_pack_weights_bwd: n_layers images, desc = {Cin, Cout, taps} each, layer after layer into `pack`: the fragment image of
 *   W^T[ci][co][tap'] = fp16(w[co][ci][8 - tap'] s[co]) (a 1 x 1: tap 0), [tap'][Cout / 16][Cin / 32][64 lanes][8 halves] -- the forward's
 *   lane map with the channel roles swapped and the forward's own fp32 fold, so the w' bits are the forward's; taps Cin Cout halves each.
 *   A whole net packs the launches that send a data gradient in the order of their plan offsets (per block: conv3, conv2, conv1,
 *   downsample).
 * sbev_resnet_backward_plan (pure host): out[SBEV_RESNET_BWD_PLAN_WORDS]:
 *    0 launches of a backward (0 for n == 0)   1 workspace bytes   2 backward-pack bytes   3 activation-buffer bytes   4 the forward's
 *    workspace bytes   5 layers   6 first_kept   7, 8 byte offsets in the workspace of the two g3 buffers   9, 10 of g2 and g1
 *    11 of the slab partials   12 the forward's pack bytes; then from word SBEV_RESNET_BWD_PLAN_HEAD, SBEV_RESNET_BWD_LAYER_WORDS per launch:
 *    slabs, slab_len, where its output is kept (a byte offset in acts, -(2 + k): outs[k], -1: not kept), byte offset of its image in the
 *    backward's pack (-1: none), trainable (0 / 1), sends a data gradient (0 / 1).
 * Single operations on raw pointers (tests, tools):
 *   sbev_conv_dgrad_f16: gx [n, H, W, Cin] = fp16(select(mask > 0, ((acc + float(res)) + scale[0] gp), 0)), acc = the products of
 *     gy [n, h, w, Cout] (taps 1 or 9, stride 1 or 2) and then, with Cout2 != 0, of gy2 [n, h2, w2, Cout2] (a 1 x 1 of stride2) over the
 *     images in `pack` (gy's, then gy2's); mask / res / gp may be null; col_tile 0 (the forward's rule on Cin) or 64 / 128 / 256.
 *   sbev_conv_wgrad_f16: the slab partials of one convolution into part [slabs][taps Cout Cin + Cout] (tap-major [tap][co][ci], then the
 *     column sums), unscaled; slab_len 0: the rule above, else a multiple of 32.
 *   sbev_bn_fold_backward: partials of `slabs` slabs -> grad_w [Cout, Cin, kh, kw], grad_gamma, grad_beta (null: skipped); scale null: 1,
 *     else scale[1] multiplies the slab sum.
 * Checked before any GPU call (SBEV_EINVAL), like sbev_resnet_forward: the plan's refusals, first_trainable_stage, dtypes, taps / stride /
 * channel counts / col_tile / slab_len not listed; then n == 0 answers SBEV_OK; then null pointers; then 16-byte alignment of
 * activations, gradients, packs and workspace (element alignment of the fp32 tensors and the weights).
 */
#define SBEV_RESNET_GRAD_WINDOW_LOG2 3
#define SBEV_RESNET_BWD_PLAN_HEAD 16
#define SBEV_RESNET_BWD_LAYER_WORDS 6
#define SBEV_RESNET_BWD_PLAN_WORDS (SBEV_RESNET_BWD_PLAN_HEAD + SBEV_RESNET_BWD_LAYER_WORDS * SBEV_RESNET_MAX_LAYERS)
int sbev_resnet_backward_plan(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                              const int32_t* out_indices, int first_trainable_stage, int64_t* out);
int sbev_resnet_forward_train(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                              const int32_t* out_indices, int first_trainable_stage, const void* x, int x_dtype, const void* pack,
                              void* workspace, void* acts, void* const* outs, sbev_stream_t stream);
int sbev_resnet_pack_weights_bwd(int n_layers, const int32_t* desc, const void* const* w, const float* const* gamma, const float* const* var,
                                 float eps, int w_dtype, void* pack, sbev_stream_t stream);
int sbev_resnet_backward(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                         const int32_t* out_indices, int first_trainable_stage, const void* acts, const void* const* outs,
                         const void* const* grad_outs, int g_dtype, const void* pack_bwd, void* workspace, const void* const* w, int w_dtype,
                         const float* const* gamma, const float* const* mean, const float* const* var, float eps, float* const* grad_w,
                         float* const* grad_gamma, float* const* grad_beta, sbev_stream_t stream);
int sbev_conv_dgrad_f16(const void* gy, const void* gy2, const void* pack, const void* mask, const void* res, const void* gp, int gp_dtype,
                        const float* scale, void* gx, int64_t n, int H, int W, int Cin, int Cout, int taps, int stride, int Cout2, int stride2,
                        int col_tile, sbev_stream_t stream);
int sbev_conv_wgrad_f16(const void* gy, const void* x, float* part, int64_t n, int H, int W, int Cin, int Cout, int taps, int stride,
                        int slab_len, sbev_stream_t stream);
int sbev_bn_fold_backward(const float* part, int slabs, const float* scale, const void* w, int w_dtype, const float* gamma, const float* mean,
                          const float* var, float eps, int Cin, int Cout, int taps, float* grad_w, float* grad_gamma, float* grad_beta,
                          sbev_stream_t stream);

/*
 * Both weight images of the ResNet backbone by ONE launch that takes no host array, so that it records into a graph and a replay folds
 * the weights as they are then (a captured training step after an optimizer update).
 * Replaces, inside a captured step: one sbev_resnet_pack_weights launch per convolution plus one sbev_resnet_pack_weights_bwd launch per
 * convolution that sends a data gradient (about 100 launches for ResNet-50); those entries stay the eager path and this one's reference.
 *
 * sbev_resnet_repack_plan (pure host): the net as the other resnet plans describe it; first_trainable_stage 1 .. num_stages as
 *   sbev_resnet_backward_plan takes it, or num_stages + 1: nothing trains, the backward image is empty.  w / gamma / beta / mean / var:
 *   one DEVICE pointer per convolution in launch order (entry 0 the stem), only looked at, never read through.  Fills `table`
 *   (SBEV_RESNET_REPACK_WORDS words of host memory; the caller uploads the first out[0] of them to the device):
 *     0 convolutions   1 work items   2 forward-image bytes   3 backward-image bytes   4 w_dtype   the rest of the head zero; then from
 *     word SBEV_RESNET_REPACK_HEAD, SBEV_RESNET_REPACK_LAYER_WORDS per convolution: the addresses of w, gamma, beta, mean, var; Cin, Cout,
 *     taps (49: the stem); the byte offset of its forward fragments and of its fp32 bias (exactly where sbev_resnet_pack_weights puts
 *     them for the whole net); the byte offset of its backward image (sbev_resnet_backward_plan's, -1: none); its first work item.
 *   A work item is 32 output channels x 64 reduction indices x all taps; a workgroup finds an item's convolution by a binary search over
 *   the first-item column.  out[4]: table words, work items (the grid of a launch with one workgroup per item), forward-image bytes
 *   (sbev_resnet_plan's pack bytes), backward-image bytes (sbev_resnet_backward_plan's).
 *   Checked (SBEV_EINVAL): null table / out, w_dtype, the plans' refusals, first_trainable_stage, a null or misaligned tensor (element
 *   alignment, as the pack entries ask).
 * sbev_resnet_repack: one kernel launch on the stream -- a fixed number of workgroups striding over the table's work items, so the call
 *   needs no host copy of the table.  fwd_image / bwd_image: the plan's bytes, 16-byte aligned; bwd_image may be null when the backward
 *   image is empty; where it is null although the table gives convolutions a backward offset, those images are silently NOT written
 *   (the table lives on the device: the host entry cannot see it; the caller sizes bwd_image from the plan's word 3).  Bit for bit what sbev_resnet_pack_weights and sbev_resnet_pack_weights_bwd write (s = gamma / sqrt(var + eps),
 *   b' = beta - mean s, w' = fp16(w s), each operation rounded on its own; w' is computed once and feeds both images).  Every weight
 *   element is read once; every 16-byte piece of both images is stored exactly once, whole; no atomics; nothing else is written.
 */
#define SBEV_RESNET_REPACK_HEAD 8
#define SBEV_RESNET_REPACK_LAYER_WORDS 12
#define SBEV_RESNET_REPACK_WORDS (SBEV_RESNET_REPACK_HEAD + SBEV_RESNET_REPACK_LAYER_WORDS * SBEV_RESNET_MAX_LAYERS)
int sbev_resnet_repack_plan(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int first_trainable_stage,
                            const void* const* w, const float* const* gamma, const float* const* beta, const float* const* mean,
                            const float* const* var, int w_dtype, int64_t* table, int64_t* out);
int sbev_resnet_repack(const int64_t* table_dev, void* fwd_image, void* bwd_image, float eps, sbev_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SBEV_HIP_H */
