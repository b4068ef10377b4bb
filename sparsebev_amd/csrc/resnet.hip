// The ResNet backbone (Bottleneck nets, style 'pytorch', BatchNorm in eval mode folded into the convolutions) for inference on
// v_mfma_f32_32x32x16_f16: NCHW images in, the FPN neck's channels-last fp16 stage maps out.  One launch per convolution (BatchNorm,
// ReLU, the residual add and the fp16 cast ride in its epilogue), one for the stem, one for the max-pool: 54 launches for ResNet-50.
//
// Arithmetic (include/sbev_hip.h: sbev_resnet_forward states it in full): w' = fp16(w * s), b' = beta - mean * s, s = gamma / sqrt(var + eps),
// every operation rounded on its own in fp32 (this unit is built with -ffp-contract=off); operands fp16, products accumulated in fp32 on
// the matrix core, y = fp16(acc + b' [+ float(residual)] [max 0]) rounded once.
//
// The convolution kernel is fpn.hip's implicit GEMM with a column-tile grid dimension: rows = output pixels of all images (128 per
// workgroup), columns = 64 WN output channels (WN = 1, 2, 4: 2 WN waves per K group, wave (wm, wn) owns rows 64 wm .. + 64 and channels 64 wn .. + 64 of
// the tile as 2 x 2 accumulators of 32 x 32), K = taps x Cin walked in chunks of 64 channels of one tap.
//   A (pixels): 128 WN threads stage the 128 x 64 chunk -- global -> registers one chunk ahead of the MFMAs, registers -> LDS -- and the
//      waves read their fragments back with 16-byte LDS reads (row pitch 72 halves).  Row r is output pixel (image, oy, ox); tap (ky, kx)
//      of a 3 x 3 reads source pixel (S oy + ky - 1, S ox + kx - 1), a 1 x 1 reads (S oy, S ox); a tap outside the plane, or a row beyond
//      the layer, stages zeros.  A tile spans images freely.
//   B (weights): folded and packed once per weight version by sbev_resnet_pack_weights into fragment order,
//      [tap][Kpad / 16][Cout / 32][64 lanes][8 halves]: lane l of fragment nt holds channel co = 64 (nt / 2) + 2 (l & 31) + (nt & 1),
//      k = 16 ks + 8 (l >> 5) + j (fpn.hip's lane map, for any Cout).  A wave reads its two fragments straight from global memory.
//      The 64-channel tiles (WN = 1) load the next chunk's fragments before the current chunk's MFMAs: they run a few waves per CU, so
//      nothing else hides that latency; the wider tiles load at use (fpn.hip measured the prefetch as a loss there).
// The stem is the same GEMM with K = 3 x 7 x 7 = 147 (order c, ky, kx: the weight's own) padded with zeros to 160, staged whole from the
// NCHW image (fp32 rounded to fp16, nearest even, on the way into LDS).
//
// Where a launch cannot give every CU a workgroup even at 64-channel tiles (the late stages: tens of workgroups walking K = 1024 .. 4608
// chunk after chunk), the workgroup splits K instead of the grid: kSplit = 3 groups of waves stage and multiply chunks g, g + 3, .. each and
// their partial sums are added through LDS in the fixed order (g0 + g1) + g2 before the epilogue.
//
// Who writes what: every stored element has one owning lane; no atomics; the K split folds in a fixed order: bit-reproducible.
//
// Training: sbev_resnet_forward_train (at the end of this file) is the same launches with every activation the backward reads kept in a
// caller-owned buffer; resnet_train.hpp hands the net's table to the backward, resnet_bwd.hip.
#include "fpn_common.hpp"
#include "resnet_train.hpp"

namespace {

using namespace sbev_fpn;

constexpr int kKC = 64, kPitch = kKC + 8;
constexpr int kStemK = 147, kStemKpad = 160, kStemPitch = kStemKpad + 8;
constexpr int kMaxLayers = SBEV_RESNET_MAX_LAYERS;
constexpr int kSplit = 3;              // K groups of a workgroup where the launch cannot fill the CUs (pick_k_split)
enum { EPI_BIAS = 0, EPI_RELU = 1, EPI_RES_RELU = 2 };
enum { KIND_STEM = 0, KIND_POOL = 1, KIND_CONV = 2 };

// ---------------------------------------------------------------- the convolution family
struct ConvArgs {
    const _Float16* x;        // [n, H, W, Cin]
    const uint4* wp;          // packed w'
    const float* bias;        // b' [Cout]
    const _Float16* res;      // [rows, Cout] or null
    _Float16* y;              // [rows, Cout]
    int rows, Cin, Cout, H, W, h, w;
};

template <int TAPS, int STRIDE, int EPI, int WN, int KS>
__global__ __launch_bounds__(128 * WN * KS) void resnet_conv_kernel(const ConvArgs a) {
    constexpr int PER = 8 / WN;           // 16-byte pieces of a row's 64-channel chunk per thread
    constexpr int GT = 128 * WN;          // threads of one K group
    __shared__ __attribute__((aligned(16))) _Float16 tile[KS * kTileM * kPitch];
    static_assert(KS == 1 || 2 * WN * 64 * 64 * 4 <= KS * kTileM * kPitch * 2, "the fold reuses the staging tiles");

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = KS == 1 ? 0 : wave / (2 * WN), wg = KS == 1 ? wave : wave % (2 * WN);      // K group (chunks g, g + KS, ..), wave inside it
    const int wm = wg / WN, wn = wg % WN;
    const int tg = tid - g * GT;
    const int srow = tg / WN, q = tg % WN;
    const long long r = (long long)blockIdx.x * kTileM + srow;
    const bool valid = r < a.rows;
    const int plane = a.h * a.w;
    const int img = valid ? (int)(r / plane) : 0, rem = valid ? (int)(r % plane) : 0;
    const int oy = rem / a.w, ox = rem % a.w;
    const int iy0 = STRIDE * oy - (TAPS == 9 ? 1 : 0), ix0 = STRIDE * ox - (TAPS == 9 ? 1 : 0);
    const _Float16* src = a.x + (size_t)img * a.H * a.W * a.Cin + q * (8 * PER);
    _Float16* mine = tile + g * (kTileM * kPitch);
    uint4* dst = reinterpret_cast<uint4*>(mine + srow * kPitch + q * (8 * PER));

    const int NF = a.Cout / 32;
    const int group = (int)blockIdx.y * WN + wn;          // the wave's 64 output channels
    const int per_tap = a.Cin / kKC, nchunks = TAPS * per_tap;
    f32x16 acc[2][2];
    zero_acc(acc);
    uint4 raw[PER];
    // chunk c: tap c / per_tap = (ky, kx), channels 64 (c % per_tap) ..; this group's next chunk is (tap, kc)
    int tap = g / per_tap, kc = g % per_tap;
    auto fetch = [&]() {
        const int iy = iy0 + (TAPS == 9 ? tap / 3 : 0), ix = ix0 + (TAPS == 9 ? tap % 3 : 0);
        const bool in = valid && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
#pragma unroll
        for (int i = 0; i < PER; ++i) raw[i] = make_uint4(0u, 0u, 0u, 0u);
        if (in) {
            const uint4* p = reinterpret_cast<const uint4*>(src + ((size_t)iy * a.W + ix) * a.Cin + kc * kKC);
#pragma unroll
            for (int i = 0; i < PER; ++i) raw[i] = p[i];
        }
        if constexpr (KS == 1) {
            if (++kc == per_tap) { kc = 0; ++tap; }
        } else {
            kc += KS;
            while (kc >= per_tap) { kc -= per_tap; ++tap; }
        }
    };
    // the narrow tiles run a few waves per CU: nothing hides the weight loads' latency there, so they too are issued a chunk ahead
    constexpr bool PB = WN == 1;
    uint4 bcur[PB ? 2 * (kKC / 16) : 1], bnext[PB ? 2 * (kKC / 16) : 1];
    auto load_b = [&](int c, uint4* b) {
        const uint4* bw = a.wp + ((size_t)c * (kKC / 16) * NF + 2 * group) * 64 + lane;
#pragma unroll
        for (int kk = 0; kk < kKC / 16; ++kk) {
            b[2 * kk] = bw[(size_t)kk * NF * 64];
            b[2 * kk + 1] = bw[(size_t)kk * NF * 64 + 64];
        }
    };
    if (g < nchunks) {
        fetch();
        if constexpr (PB) load_b(g, bcur);
    }
    const _Float16* arow = mine + (64 * wm + (lane & 31)) * kPitch + 8 * (lane >> 5);
    for (int c = g; c - g < nchunks; c += KS) {          // every group walks ceil(nchunks / KS) steps: the barriers are the workgroup's
        const bool have = KS == 1 || c < nchunks;
        if (have) {
#pragma unroll
            for (int i = 0; i < PER; ++i) dst[i] = raw[i];
        }
        __syncthreads();
        if (c + KS < nchunks) {
            fetch();
            if constexpr (PB) load_b(c + KS, bnext);
        }
        if (have) {
            uint4 bnow[2 * (kKC / 16)];
            if constexpr (PB) {
#pragma unroll
                for (int i = 0; i < 2 * (kKC / 16); ++i) bnow[i] = bcur[i];
            } else {
                load_b(c, bnow);
            }
#pragma unroll
            for (int kk = 0; kk < kKC / 16; ++kk) {
                const uint4 a0 = *reinterpret_cast<const uint4*>(arow + 16 * kk);
                const uint4 a1 = *reinterpret_cast<const uint4*>(arow + 32 * kPitch + 16 * kk);
                const f16x8 fa0 = __builtin_bit_cast(f16x8, a0), fa1 = __builtin_bit_cast(f16x8, a1);
                const f16x8 fb0 = __builtin_bit_cast(f16x8, bnow[2 * kk]), fb1 = __builtin_bit_cast(f16x8, bnow[2 * kk + 1]);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
        if constexpr (PB) {
#pragma unroll
            for (int i = 0; i < 2 * (kKC / 16); ++i) bcur[i] = bnext[i];
        }
    }
    if constexpr (KS > 1) {
        // fold the groups' partial sums in the fixed order (g0 + g1) + g2 ..: group s hands its accumulators over through the (now idle)
        // staging tiles, [wave of the group][register][lane], and group 0 adds them; one owner per element, no atomics
        float* fold = reinterpret_cast<float*>(tile) + (size_t)wg * (64 * 64) + lane;
        for (int s = 1; s < KS; ++s) {
            if (g == s) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int rr = 0; rr < 16; ++rr) fold[((i * 2 + j) * 16 + rr) * 64] = acc[i][j][rr];
            }
            __syncthreads();
            if (g == 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int rr = 0; rr < 16; ++rr) acc[i][j][rr] += fold[((i * 2 + j) * 16 + rr) * 64];
            }
            __syncthreads();
        }
        if (g != 0) return;
    }

    const int c0 = 64 * group + 2 * (lane & 31);
    const float b0 = a.bias[c0], b1 = a.bias[c0 + 1];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const long long row = (long long)blockIdx.x * kTileM + acc_row(wm, mb, rr, lane);
            if (row >= a.rows) continue;
            const size_t o = (size_t)row * a.Cout + c0;
            float v0 = acc[mb][0][rr] + b0, v1 = acc[mb][1][rr] + b1;
            if constexpr (EPI == EPI_RES_RELU) {
                const f16x2 pv = *reinterpret_cast<const f16x2*>(a.res + o);
                v0 += (float)pv.x;
                v1 += (float)pv.y;
            }
            if constexpr (EPI != EPI_BIAS) {
                v0 = fmaxf(v0, 0.f);
                v1 = fmaxf(v1, 0.f);
            }
            *reinterpret_cast<unsigned*>(a.y + o) = pack_h2(v0, v1);
        }
    }
}

template <int TAPS, int STRIDE, int EPI>
void launch_conv_wn(int ct, int ks, dim3 grid, hipStream_t s, const ConvArgs& a) {
    if (ct == 64 && ks == kSplit) hipLaunchKernelGGL((resnet_conv_kernel<TAPS, STRIDE, EPI, 1, kSplit>), grid, dim3(128 * kSplit), 0, s, a);
    else if (ct == 64) hipLaunchKernelGGL((resnet_conv_kernel<TAPS, STRIDE, EPI, 1, 1>), grid, dim3(128), 0, s, a);
    else if (ct == 128) hipLaunchKernelGGL((resnet_conv_kernel<TAPS, STRIDE, EPI, 2, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((resnet_conv_kernel<TAPS, STRIDE, EPI, 4, 1>), grid, dim3(512), 0, s, a);
}

template <int TAPS, int STRIDE>
void launch_conv_epi(int epi, int ct, int ks, dim3 grid, hipStream_t s, const ConvArgs& a) {
    if (epi == EPI_BIAS) launch_conv_wn<TAPS, STRIDE, EPI_BIAS>(ct, ks, grid, s, a);
    else if (epi == EPI_RELU) launch_conv_wn<TAPS, STRIDE, EPI_RELU>(ct, ks, grid, s, a);
    else launch_conv_wn<TAPS, STRIDE, EPI_RES_RELU>(ct, ks, grid, s, a);
}

// ks: pick_k_split's answer for this shape (1, or kSplit with ct == 64)
void launch_conv(int taps, int stride, int epi, int ct, int ks, const ConvArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows + kTileM - 1) / kTileM), (unsigned)(a.Cout / ct));
    if (taps == 1 && stride == 1) launch_conv_epi<1, 1>(epi, ct, ks, grid, s, a);
    else if (taps == 1) launch_conv_epi<1, 2>(epi, ct, ks, grid, s, a);
    else if (stride == 1) launch_conv_epi<9, 1>(epi, ct, ks, grid, s, a);
    else launch_conv_epi<9, 2>(epi, ct, ks, grid, s, a);
}

// ---------------------------------------------------------------- the stem: 7 x 7 / 2 / pad 3 from NCHW, bias + ReLU
struct StemArgs {
    const void* x;            // [n, 3, H, W] fp32 or fp16
    const uint4* wp;
    const float* bias;
    _Float16* y;              // [rows, Cout]
    int rows, Cout, H, W, h, w;
};

template <bool F32>
__global__ __launch_bounds__(128) void resnet_stem_kernel(const StemArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 tile[kTileM * kStemPitch];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long r = (long long)blockIdx.x * kTileM + tid;
    const bool valid = r < a.rows;
    const int plane = a.h * a.w;
    const int img = valid ? (int)(r / plane) : 0, rem = valid ? (int)(r % plane) : 0;
    const int oy = rem / a.w, ox = rem % a.w;
    _Float16* mine = tile + tid * kStemPitch;
    for (int c = 0; c < 3; ++c) {
        const size_t base = ((size_t)img * 3 + c) * a.H * a.W;
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = 2 * oy + ky - 3;
            const bool iny = valid && (unsigned)iy < (unsigned)a.H;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const int ix = 2 * ox + kx - 3;
                _Float16 v = (_Float16)0.f;
                if (iny && (unsigned)ix < (unsigned)a.W) {
                    const size_t e = base + (size_t)iy * a.W + ix;
                    v = F32 ? (_Float16) static_cast<const float*>(a.x)[e] : static_cast<const _Float16*>(a.x)[e];
                }
                mine[c * 49 + ky * 7 + kx] = v;
            }
        }
    }
    for (int k = kStemK; k < kStemKpad; ++k) mine[k] = (_Float16)0.f;
    __syncthreads();

    const int NF = a.Cout / 32, group = (int)blockIdx.y;
    f32x16 acc[2][2];
    zero_acc(acc);
    const _Float16* arow = tile + (64 * wm + (lane & 31)) * kStemPitch + 8 * (lane >> 5);
    const uint4* bw = a.wp + (size_t)(2 * group) * 64 + lane;
#pragma unroll
    for (int kk = 0; kk < kStemKpad / 16; ++kk) {
        const uint4 b0 = bw[(size_t)kk * NF * 64], b1 = bw[(size_t)kk * NF * 64 + 64];
        const uint4 a0 = *reinterpret_cast<const uint4*>(arow + 16 * kk);
        const uint4 a1 = *reinterpret_cast<const uint4*>(arow + 32 * kStemPitch + 16 * kk);
        const f16x8 fa0 = __builtin_bit_cast(f16x8, a0), fa1 = __builtin_bit_cast(f16x8, a1);
        const f16x8 fb0 = __builtin_bit_cast(f16x8, b0), fb1 = __builtin_bit_cast(f16x8, b1);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb1, acc[1][1], 0, 0, 0);
    }
    const int c0 = 64 * group + 2 * (lane & 31);
    const float b0 = a.bias[c0], b1 = a.bias[c0 + 1];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const long long row = (long long)blockIdx.x * kTileM + acc_row(wm, mb, rr, lane);
            if (row >= a.rows) continue;
            const float v0 = fmaxf(acc[mb][0][rr] + b0, 0.f), v1 = fmaxf(acc[mb][1][rr] + b1, 0.f);
            *reinterpret_cast<unsigned*>(a.y + (size_t)row * a.Cout + c0) = pack_h2(v0, v1);
        }
    }
}

// ---------------------------------------------------------------- max-pool 3 x 3 / 2 / pad 1, channels-last fp16, 8 channels per lane
struct PoolArgs {
    const _Float16* x;        // [n, H, W, C]
    _Float16* y;              // [n, h, w, C]
    long long items;          // n h w C / 8
    int C8, H, W, h, w;
};

__global__ __launch_bounds__(256) void resnet_pool_kernel(const PoolArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.items) return;
    const int g = (int)(i % a.C8);
    const long long p = i / a.C8;
    const int plane = a.h * a.w;
    const int img = (int)(p / plane), rem = (int)(p % plane);
    const int oy = rem / a.w, ox = rem % a.w;
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
        if ((unsigned)iy >= (unsigned)a.H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox + kx - 1;
            if ((unsigned)ix >= (unsigned)a.W) continue;      // the padding is ignored: tap (1, 1) is always inside
            const uint4 v = *reinterpret_cast<const uint4*>(a.x + ((((size_t)img * a.H + iy) * a.W + ix) * a.C8 + g) * 8);
            const f16x8 h = __builtin_bit_cast(f16x8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], (float)h[j]);
        }
    }
    *reinterpret_cast<uint4*>(a.y + (size_t)i * 8) =
        make_uint4(pack_h2(m[0], m[1]), pack_h2(m[2], m[3]), pack_h2(m[4], m[5]), pack_h2(m[6], m[7]));
}

// ---------------------------------------------------------------- fold BatchNorm into the weights -> fragment order fp16, fp32 bias
struct FoldArgs {
    const void* w;            // [Cout, Cin, taps] contiguous (the stem: [Cout, 147], taps = 1), fp32 or fp16
    const float *gamma, *beta, *mean, *var;
    uint4* dst;
    float* bias;
    float eps;
    int Cin, Kpad, Cout, taps, f32;
    long long frags;          // taps * (Kpad / 16) * (Cout / 32) * 64
};

__global__ __launch_bounds__(256) void resnet_fold_pack_kernel(const FoldArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.frags) return;
    if (i < a.Cout) {
        const float s = sbev_resnet::bn_fold_scale(a.gamma[i], a.var[i], a.eps);
        a.bias[i] = a.beta[i] - a.mean[i] * s;
    }
    const int NF = a.Cout / 32, KS = a.Kpad / 16;
    const int lane = (int)(i & 63);
    const long long f = i >> 6;
    const int nt = (int)(f % NF);
    const long long rest = f / NF;
    const int ks = (int)(rest % KS), tap = (int)(rest / KS);
    const int co = 64 * (nt >> 1) + 2 * (lane & 31) + (nt & 1);
    const int k0 = 16 * ks + 8 * (lane >> 5);
    const float s = sbev_resnet::bn_fold_scale(a.gamma[co], a.var[co], a.eps);
    float p[8];      // the eight products first, their second rounding afterwards: all loads in flight (resnet_train.hpp: bn_fold_round)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int k = k0 + t;
        p[t] = 0.f;
        if (k < a.Cin) {
            const size_t e = ((size_t)co * a.Cin + k) * a.taps + tap;
            const float w = a.f32 ? static_cast<const float*>(a.w)[e] : (float)static_cast<const _Float16*>(a.w)[e];
            p[t] = w * s;
        }
    }
    unsigned h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f16x2 v;
        v.x = sbev_resnet::bn_fold_round(p[2 * j]);
        v.y = sbev_resnet::bn_fold_round(p[2 * j + 1]);
        h[j] = __builtin_bit_cast(unsigned, v);
    }
    a.dst[i] = make_uint4(h[0], h[1], h[2], h[3]);
}

// ---------------------------------------------------------------- the plan (pure host)
inline int out_side(int in, int stride) { return (in - 1) / stride + 1; }      // 3 x 3 / pad 1 and 1 x 1 / pad 0 alike
inline long long align256(long long v) { return (v + 255) & ~255LL; }

// bytes of one layer's pack: fragments, then the fp32 bias
inline long long pack_bytes(int Cin, int Cout, int taps) {
    const long long k = taps == 49 ? kStemKpad : (long long)taps * Cin;
    return k * Cout * 2 + (long long)Cout * 4;
}
inline long long frag_bytes(int Cin, int Cout, int taps) { return pack_bytes(Cin, Cout, taps) - (long long)Cout * 4; }

// the widest column tile that still gives every CU a workgroup; 64 where none does (the late stages: small tiles instead of a split K)
inline int pick_col_tile(long long row_tiles, int Cout) {
    for (int ct = 256; ct > 64; ct >>= 1)
        if (Cout % ct == 0 && row_tiles * (Cout / ct) >= 256) return ct;
    return 64;
}

// Where even 64-channel tiles leave CUs without a workgroup the K loop is the launch's critical path: kSplit groups of waves in the
// workgroup then walk every kSplit-th chunk each and fold their partial sums in a fixed order (from 6 chunks on: below that the fold costs
// what it saves)
inline int pick_k_split(long long row_tiles, int Cout, int ct, int taps, int Cin) {
    return ct == 64 && row_tiles * (Cout / 64) < 256 && taps * (Cin / kKC) >= 6 ? kSplit : 1;
}

struct Layer {
    int kind, Cin, Cout, taps, stride, H, W, h, w, epi, col_tile, k_split;
    long long rows, row_tiles, pack_off, macs;
    int in_layer, res_layer;      // producing layers (-1: the image; res: -1 none)
    int role;                     // workspace region, or -2 - k: outs[k]
    long long out_off;            // byte offset in the workspace (role >= 0)
};

struct NetPlan {
    int n_layers, n_out;
    Layer layer[kMaxLayers];
    int out_layer[4];
    long long pack_total, ws_total, macs;
};

int make_net_plan(const char* who, int depth, const int32_t* stage_blocks, int num_stages, int base, int64_t n, int H, int W, int n_out,
                  const int32_t* out_indices, int keep, NetPlan* p) {
    SBEV_REQUIRE(depth != 18 && depth != 34, "%s: depth=%d is a BasicBlock net (the Bottleneck nets 50, 101, 152 are built)", who, depth);
    SBEV_REQUIRE(depth == 50 || depth == 101 || depth == 152, "%s: depth=%d (50, 101, 152 are built)", who, depth);
    SBEV_REQUIRE(num_stages >= 1 && num_stages <= 4, "%s: num_stages=%d not in 1 .. 4", who, num_stages);
    static const int32_t r50[4] = {3, 4, 6, 3}, r101[4] = {3, 4, 23, 3}, r152[4] = {3, 8, 36, 3};
    const int32_t* blocks = stage_blocks != nullptr ? stage_blocks : depth == 50 ? r50 : depth == 101 ? r101 : r152;
    int total_blocks = 0;
    for (int s = 0; s < num_stages; ++s) {
        SBEV_REQUIRE(blocks[s] >= 1 && blocks[s] <= 64, "%s: stage %d has %d blocks (1 .. 64)", who, s, blocks[s]);
        total_blocks += blocks[s];
    }
    SBEV_REQUIRE(3 * total_blocks + num_stages + 2 <= kMaxLayers, "%s: %d blocks: more than %d launches", who, total_blocks, kMaxLayers);
    SBEV_REQUIRE(base >= 64 && base % 64 == 0 && base <= 1024, "%s: base_channels=%d (channel counts are multiples of 64, at most 1024 here)",
                 who, base);
    SBEV_REQUIRE(n >= 0 && n <= (1LL << 20), "%s: n=%lld images", who, (long long)n);
    SBEV_REQUIRE(H >= 1 && W >= 1, "%s: an empty image (%d x %d)", who, H, W);
    SBEV_REQUIRE(H <= 32767 && W <= 32767, "%s: image %d x %d: a side above 32767", who, H, W);
    SBEV_REQUIRE(out_indices != nullptr && n_out >= 1 && n_out <= num_stages, "%s: %d out_indices (1 .. num_stages)", who, n_out);
    for (int k = 0; k < n_out; ++k)
        SBEV_REQUIRE(out_indices[k] >= 0 && out_indices[k] < num_stages && (k == 0 || out_indices[k] > out_indices[k - 1]),
                     "%s: out_indices must be increasing stage numbers below num_stages", who);

    int nl = 0;
    long long pack = 0, macs = 0;
    bool fits = true;
    auto add = [&](int kind, int Cin, int Cout, int taps, int stride, int sH, int sW, int h, int w, int epi, int in_layer, int res_layer,
                   int role) {
        Layer& L = p->layer[nl];
        L.kind = kind; L.Cin = Cin; L.Cout = Cout; L.taps = taps; L.stride = stride; L.H = sH; L.W = sW; L.h = h; L.w = w; L.epi = epi;
        L.rows = (long long)n * h * w;
        fits = fits && L.rows <= 0x7fffffffLL - kTileM;
        L.row_tiles = (L.rows + kTileM - 1) / kTileM;
        L.col_tile = kind == KIND_CONV ? pick_col_tile(L.row_tiles, Cout) : kind == KIND_STEM ? 64 : Cout;
        L.k_split = kind == KIND_CONV ? pick_k_split(L.row_tiles, Cout, L.col_tile, taps, Cin) : 1;
        L.pack_off = pack;
        L.macs = 0;
        if (kind != KIND_POOL) {
            pack += pack_bytes(Cin, Cout, taps);
            L.macs = L.rows * Cout * (kind == KIND_STEM ? kStemK : (long long)taps * Cin);
            macs += L.macs;
        }
        L.in_layer = in_layer; L.res_layer = res_layer;
        L.role = keep && role >= 0 ? nl : role;
        L.out_off = 0;
        return nl++;
    };
    enum { X0 = 0, X1 = 1, T1 = 2, T2 = 3, DS = 4 };
    const int h1 = (H + 6 - 7) / 2 + 1, w1 = (W + 6 - 7) / 2 + 1;          // H >= 1: H - 1 >= 0, no negative division
    int cur = add(KIND_STEM, 3, base, 49, 2, H, W, h1, w1, EPI_RELU, -1, -1, T1);
    int ch = out_side(h1, 2), cw = out_side(w1, 2);
    cur = add(KIND_POOL, base, base, 9, 2, h1, w1, ch, cw, EPI_BIAS, cur, -1, X0);
    int cin = base, next_out = 0;
    for (int s = 0; s < num_stages; ++s) {
        const int mid = base << s, cout = 4 * mid, stride = s == 0 ? 1 : 2;
        for (int b = 0; b < blocks[s]; ++b) {
            const int st = b == 0 ? stride : 1;
            const int oh = out_side(ch, st), ow = out_side(cw, st);
            const int t1 = add(KIND_CONV, cin, mid, 1, 1, ch, cw, ch, cw, EPI_RELU, cur, -1, T1);
            const int t2 = add(KIND_CONV, mid, mid, 9, st, ch, cw, oh, ow, EPI_RELU, t1, -1, T2);
            int res = cur;
            if (b == 0) res = add(KIND_CONV, cin, cout, 1, st, ch, cw, oh, ow, EPI_BIAS, cur, -1, DS);
            int role = p->layer[cur].role == X0 ? X1 : X0;
            if (b == blocks[s] - 1 && next_out < n_out && out_indices[next_out] == s) role = -2 - next_out;
            cur = add(KIND_CONV, mid, cout, 1, 1, oh, ow, oh, ow, EPI_RES_RELU, t2, res, role);
            if (role < 0) p->out_layer[next_out++] = cur;
            cin = cout; ch = oh; cw = ow;
        }
    }
    SBEV_REQUIRE(fits, "%s: %lld images of %d x %d: more pixels in a layer than 32-bit row indices hold", who, (long long)n, H, W);
    p->n_layers = nl;
    p->n_out = n_out;
    p->pack_total = pack;
    p->macs = macs;
    // workspace: one region per role (ping-pong), or per layer (keep): the largest tensor that lives there
    long long size[kMaxLayers];
    for (int i = 0; i < kMaxLayers; ++i) size[i] = 0;
    for (int i = 0; i < nl; ++i) {
        const Layer& L = p->layer[i];
        if (L.role >= 0 && L.rows * L.Cout * 2 > size[L.role]) size[L.role] = L.rows * L.Cout * 2;
    }
    long long off[kMaxLayers], at = 0;
    for (int i = 0; i < kMaxLayers; ++i) { off[i] = at; at += align256(size[i]); }
    for (int i = 0; i < nl; ++i)
        if (p->layer[i].role >= 0) p->layer[i].out_off = off[p->layer[i].role];
    p->ws_total = at;
    return SBEV_OK;
}

int check_conv_shape(const char* who, int Cin, int Cout, int taps) {
    if (taps == 49) {
        SBEV_REQUIRE(Cin == 3, "%s: the 7 x 7 stem has 3 input channels (got %d)", who, Cin);
    } else {
        SBEV_REQUIRE(taps == 1 || taps == 9, "%s: taps=%d (1, 9, or 49 for the stem)", who, taps);
        SBEV_REQUIRE(Cin >= 64 && Cin % 64 == 0 && Cin <= 65536, "%s: %d input channels (a multiple of 64, at most 65536)", who, Cin);
    }
    SBEV_REQUIRE(Cout >= 64 && Cout % 64 == 0 && Cout <= 65536, "%s: %d output channels (a multiple of 64, at most 65536)", who, Cout);
    return SBEV_OK;
}

// every launch of a forward in launch order; where(layer) is the address of that layer's output
template <class Where>
void enqueue_forward(const NetPlan& p, const void* x, int x_dtype, const void* pack, Where where, hipStream_t s) {
    for (int i = 0; i < p.n_layers; ++i) {
        const Layer& L = p.layer[i];
        const char* wl = static_cast<const char*>(pack) + L.pack_off;
        if (L.kind == KIND_STEM) {
            StemArgs a;
            a.x = x;
            a.wp = reinterpret_cast<const uint4*>(wl);
            a.bias = reinterpret_cast<const float*>(wl + frag_bytes(L.Cin, L.Cout, L.taps));
            a.y = static_cast<_Float16*>(where(i));
            a.rows = (int)L.rows; a.Cout = L.Cout; a.H = L.H; a.W = L.W; a.h = L.h; a.w = L.w;
            const dim3 grid((unsigned)L.row_tiles, (unsigned)(L.Cout / 64));
            if (x_dtype == SBEV_F32) hipLaunchKernelGGL(resnet_stem_kernel<true>, grid, dim3(128), 0, s, a);
            else hipLaunchKernelGGL(resnet_stem_kernel<false>, grid, dim3(128), 0, s, a);
        } else if (L.kind == KIND_POOL) {
            PoolArgs a;
            a.x = static_cast<const _Float16*>(where(L.in_layer));
            a.y = static_cast<_Float16*>(where(i));
            a.C8 = L.Cout / 8; a.H = L.H; a.W = L.W; a.h = L.h; a.w = L.w;
            a.items = L.rows * a.C8;
            hipLaunchKernelGGL(resnet_pool_kernel, dim3((unsigned)((a.items + 255) / 256)), dim3(256), 0, s, a);
        } else {
            ConvArgs a;
            a.x = static_cast<const _Float16*>(where(L.in_layer));
            a.wp = reinterpret_cast<const uint4*>(wl);
            a.bias = reinterpret_cast<const float*>(wl + frag_bytes(L.Cin, L.Cout, L.taps));
            a.res = L.res_layer >= 0 ? static_cast<const _Float16*>(where(L.res_layer)) : nullptr;
            a.y = static_cast<_Float16*>(where(i));
            a.rows = (int)L.rows; a.Cin = L.Cin; a.Cout = L.Cout; a.H = L.H; a.W = L.W; a.h = L.h; a.w = L.w;
            launch_conv(L.taps, L.stride, L.epi, L.col_tile, L.k_split, a, s);
        }
    }
}

}  // namespace

extern "C" int sbev_resnet_plan(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                                const int32_t* out_indices, int keep, int64_t* out) {
    const char* who = "sbev_resnet_plan";
    SBEV_REQUIRE(out != nullptr, "%s: null out", who);
    NetPlan p;
    if (int st = make_net_plan(who, depth, stage_blocks, num_stages, base_channels, n, H, W, n_out, out_indices, keep, &p)) return st;
    for (int i = 0; i < SBEV_RESNET_PLAN_WORDS; ++i) out[i] = 0;
    out[0] = n > 0 ? p.n_layers : 0;
    out[1] = p.pack_total;
    out[2] = p.ws_total;
    out[3] = p.n_layers;
    out[4] = p.macs;
    out[5] = p.n_out;
    for (int k = 0; k < p.n_out; ++k) {
        const Layer& L = p.layer[p.out_layer[k]];
        out[6 + 3 * k] = L.Cout; out[7 + 3 * k] = L.h; out[8 + 3 * k] = L.w;
    }
    for (int i = 0; i < p.n_layers; ++i) {
        const Layer& L = p.layer[i];
        int64_t* o = out + SBEV_RESNET_PLAN_HEAD + SBEV_RESNET_LAYER_WORDS * i;
        o[0] = L.kind; o[1] = L.Cin; o[2] = L.Cout; o[3] = L.taps; o[4] = L.stride; o[5] = L.h; o[6] = L.w;
        o[7] = L.row_tiles; o[8] = L.Cout / L.col_tile; o[9] = L.k_split;
        o[10] = L.role >= 0 ? L.out_off : L.role + 1;          // outs[k]: -(1 + k)
        o[11] = L.epi;
    }
    return SBEV_OK;
}

extern "C" int sbev_resnet_pack_weights(int n_layers, const int32_t* desc, const void* const* w, const float* const* gamma,
                                        const float* const* beta, const float* const* mean, const float* const* var, float eps, int w_dtype,
                                        void* pack, sbev_stream_t stream) {
    const char* who = "sbev_resnet_pack_weights";
    SBEV_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "%s: %d layers (at most %d)", who, n_layers, kMaxLayers);
    SBEV_REQUIRE(w_dtype == SBEV_F32 || w_dtype == SBEV_F16, "%s: w_dtype %d (SBEV_F32 or SBEV_F16)", who, w_dtype);
    SBEV_REQUIRE(eps >= 0.f && std::isfinite(eps), "%s: eps=%g", who, (double)eps);
    if (n_layers == 0) return SBEV_OK;
    SBEV_REQUIRE(desc && w && gamma && beta && mean && var && pack, "%s: null pointer", who);
    SBEV_REQUIRE(aligned16(pack), "%s: 16-byte alignment", who);
    for (int i = 0; i < n_layers; ++i) {
        if (int st = check_conv_shape(who, desc[3 * i], desc[3 * i + 1], desc[3 * i + 2])) return st;
        SBEV_REQUIRE(w[i] && gamma[i] && beta[i] && mean[i] && var[i], "%s: layer %d: null pointer", who, i);
        bool al = (reinterpret_cast<uintptr_t>(w[i]) & (w_dtype == SBEV_F32 ? 3u : 1u)) == 0;
        for (const float* q : {gamma[i], beta[i], mean[i], var[i]}) al = al && (reinterpret_cast<uintptr_t>(q) & 3u) == 0;
        SBEV_REQUIRE(al, "%s: layer %d: misaligned tensor", who, i);
    }
    long long at = 0;
    for (int i = 0; i < n_layers; ++i) {
        const int Cin = desc[3 * i], Cout = desc[3 * i + 1], taps = desc[3 * i + 2];
        FoldArgs a;
        a.w = w[i]; a.gamma = gamma[i]; a.beta = beta[i]; a.mean = mean[i]; a.var = var[i];
        a.eps = eps;
        a.Cout = Cout;
        a.f32 = w_dtype == SBEV_F32;
        if (taps == 49) { a.Cin = kStemK; a.Kpad = kStemKpad; a.taps = 1; }
        else { a.Cin = Cin; a.Kpad = Cin; a.taps = taps; }
        a.frags = (long long)a.taps * (a.Kpad / 16) * (Cout / 32) * 64;
        a.dst = reinterpret_cast<uint4*>(static_cast<char*>(pack) + at);
        a.bias = reinterpret_cast<float*>(static_cast<char*>(pack) + at + frag_bytes(Cin, Cout, taps));
        at += pack_bytes(Cin, Cout, taps);
        hipLaunchKernelGGL(resnet_fold_pack_kernel, dim3((unsigned)((a.frags + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    }
    return sbev::check_launch(who);
}

extern "C" int sbev_conv_f16(const void* x, const void* pack, const void* residual, void* y, int64_t n, int H, int W, int Cin, int Cout, int taps,
                             int stride, int epilogue, int col_tile, sbev_stream_t stream) {
    const char* who = "sbev_conv_f16";
    SBEV_REQUIRE(taps == 1 || taps == 9, "%s: taps=%d (1 or 9)", who, taps);
    SBEV_REQUIRE(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", who, stride);
    SBEV_REQUIRE(epilogue >= EPI_BIAS && epilogue <= EPI_RES_RELU, "%s: epilogue=%d (0 bias, 1 + ReLU, 2 + residual + ReLU)", who, epilogue);
    if (int st = check_conv_shape(who, Cin, Cout, taps)) return st;
    SBEV_REQUIRE(col_tile == 0 || ((col_tile == 64 || col_tile == 128 || col_tile == 256) && Cout % col_tile == 0),
                 "%s: col_tile=%d (0, or 64 / 128 / 256 dividing Cout=%d)", who, col_tile, Cout);
    SBEV_REQUIRE(n >= 0 && n <= (1LL << 20), "%s: n=%lld images", who, (long long)n);
    SBEV_REQUIRE(H >= 1 && W >= 1, "%s: an empty plane (%d x %d)", who, H, W);
    SBEV_REQUIRE(H <= 32767 && W <= 32767, "%s: plane %d x %d: a side above 32767", who, H, W);
    const int h = out_side(H, stride), w = out_side(W, stride);
    const long long rows = (long long)n * h * w;
    SBEV_REQUIRE(rows <= 0x7fffffffLL - kTileM, "%s: %lld output pixels: row indices are 32-bit", who, rows);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(x && pack && y && (epilogue != EPI_RES_RELU || residual), "%s: null pointer", who);
    SBEV_REQUIRE(aligned16(x) && aligned16(pack) && aligned16(y) && aligned16(residual), "%s: 16-byte alignment", who);
    ConvArgs a;
    a.x = static_cast<const _Float16*>(x);
    a.wp = static_cast<const uint4*>(pack);
    a.bias = reinterpret_cast<const float*>(static_cast<const char*>(pack) + frag_bytes(Cin, Cout, taps));
    a.res = static_cast<const _Float16*>(residual);
    a.y = static_cast<_Float16*>(y);
    a.rows = (int)rows; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.h = h; a.w = w;
    const int ct = col_tile ? col_tile : pick_col_tile((rows + kTileM - 1) / kTileM, Cout);
    launch_conv(taps, stride, epilogue, ct, pick_k_split((rows + kTileM - 1) / kTileM, Cout, ct, taps, Cin), a, reinterpret_cast<hipStream_t>(stream));
    return sbev::check_launch(who);
}

extern "C" int sbev_resnet_forward(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                                   const int32_t* out_indices, int keep, const void* x, int x_dtype, const void* pack, void* workspace,
                                   void* const* outs, sbev_stream_t stream) {
    const char* who = "sbev_resnet_forward";
    NetPlan p;
    if (int st = make_net_plan(who, depth, stage_blocks, num_stages, base_channels, n, H, W, n_out, out_indices, keep, &p)) return st;
    SBEV_REQUIRE(x_dtype == SBEV_F32 || x_dtype == SBEV_F16, "%s: x_dtype %d (SBEV_F32 or SBEV_F16)", who, x_dtype);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(x && pack && workspace && outs, "%s: null pointer", who);
    for (int k = 0; k < n_out; ++k) SBEV_REQUIRE(outs[k] != nullptr, "%s: output %d: null pointer", who, k);
    bool al = aligned16(x) && aligned16(pack) && aligned16(workspace);
    for (int k = 0; k < n_out; ++k) al = al && aligned16(outs[k]);
    SBEV_REQUIRE(al, "%s: 16-byte alignment", who);

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    auto where = [&](int layer) -> void* {
        const Layer& L = p.layer[layer];
        return L.role >= 0 ? static_cast<void*>(static_cast<char*>(workspace) + L.out_off) : outs[-2 - L.role];
    };
    enqueue_forward(p, x, x_dtype, pack, where, s);
    return sbev::check_launch(who);
}

// ---------------------------------------------------------------- the trainable forward (its backward: resnet_bwd.hip)
int sbev_resnet::train_net(const char* who, int depth, const int32_t* stage_blocks, int num_stages, int base, int64_t n, int H, int W, int n_out,
                           const int32_t* out_indices, int first_trainable_stage, TrainNet* t) {
    NetPlan p;
    if (int st = make_net_plan(who, depth, stage_blocks, num_stages, base, n, H, W, n_out, out_indices, 0, &p)) return st;
    SBEV_REQUIRE(first_trainable_stage != 0, "%s: first_trainable_stage=0 (frozen_stages=-1, a trainable stem: the 7 x 7 weight gradient and the "
                 "max-pool backward are not built)", who);
    SBEV_REQUIRE(first_trainable_stage >= 1 && first_trainable_stage <= num_stages, "%s: first_trainable_stage=%d not in 1 .. num_stages=%d", who,
                 first_trainable_stage, num_stages);
    t->n_layers = p.n_layers;
    t->n_out = p.n_out;
    t->first_trainable_stage = first_trainable_stage;
    t->ws_bytes = p.ws_total;
    t->pack_bytes = p.pack_total;
    for (int k = 0; k < 4; ++k) t->out_layer[k] = k < p.n_out ? p.out_layer[k] : -1;
    static const int32_t r50[4] = {3, 4, 6, 3}, r101[4] = {3, 4, 23, 3}, r152[4] = {3, 8, 36, 3};
    const int32_t* blocks = stage_blocks != nullptr ? stage_blocks : depth == 50 ? r50 : depth == 101 ? r101 : r152;
    int stage = -1, block = 0, which = 3;
    t->first_kept = 1;
    for (int i = 0; i < p.n_layers; ++i) {
        const Layer& L = p.layer[i];
        TLayer& T = t->layer[i];
        T.kind = L.kind; T.Cin = L.Cin; T.Cout = L.Cout; T.taps = L.taps; T.stride = L.stride; T.H = L.H; T.W = L.W; T.h = L.h; T.w = L.w;
        T.in_layer = L.in_layer; T.res_layer = L.res_layer; T.rows = L.rows; T.pack_off = L.pack_off;
        T.out_k = L.role < 0 ? -2 - L.role : -1;
        if (L.kind == KIND_CONV) {
            // launch order inside a block: conv1, conv2, [downsample], conv3
            if (which == 3) { which = 0; if (stage < 0 || block + 1 == blocks[stage]) { ++stage; block = 0; } else { ++block; } }
            else if (which == 0) which = 1;
            else if (which == 1) which = L.epi == EPI_BIAS ? 2 : 3;
            else which = 3;
            T.stage = stage; T.block = block; T.which = which;
            if (which == 0 && block == 0 && stage == first_trainable_stage - 1) t->first_kept = L.in_layer;
        } else {
            T.stage = -1; T.block = 0; T.which = 0;
        }
    }
    long long at = 0;
    for (int i = 0; i < p.n_layers; ++i) {
        TLayer& T = t->layer[i];
        T.act = kNotKept;
        if (i < t->first_kept) continue;
        T.act = 0;
        if (T.out_k >= 0) continue;
        T.act = at;
        at += align256(T.rows * T.Cout * 2);
    }
    t->acts_bytes = at;
    return SBEV_OK;
}

extern "C" int sbev_resnet_forward_train(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W,
                                         int n_out, const int32_t* out_indices, int first_trainable_stage, const void* x, int x_dtype,
                                         const void* pack, void* workspace, void* acts, void* const* outs, sbev_stream_t stream) {
    const char* who = "sbev_resnet_forward_train";
    sbev_resnet::TrainNet t;
    if (int st = sbev_resnet::train_net(who, depth, stage_blocks, num_stages, base_channels, n, H, W, n_out, out_indices, first_trainable_stage, &t))
        return st;
    NetPlan p;
    if (int st = make_net_plan(who, depth, stage_blocks, num_stages, base_channels, n, H, W, n_out, out_indices, 0, &p)) return st;
    SBEV_REQUIRE(x_dtype == SBEV_F32 || x_dtype == SBEV_F16, "%s: x_dtype %d (SBEV_F32 or SBEV_F16)", who, x_dtype);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(x && pack && workspace && acts && outs, "%s: null pointer", who);
    for (int k = 0; k < n_out; ++k) SBEV_REQUIRE(outs[k] != nullptr, "%s: output %d: null pointer", who, k);
    bool al = aligned16(x) && aligned16(pack) && aligned16(workspace) && aligned16(acts);
    for (int k = 0; k < n_out; ++k) al = al && aligned16(outs[k]);
    SBEV_REQUIRE(al, "%s: 16-byte alignment", who);
    auto where = [&](int layer) -> void* {
        const Layer& L = p.layer[layer];
        if (L.role < 0) return outs[-2 - L.role];
        if (layer >= t.first_kept) return static_cast<char*>(acts) + t.layer[layer].act;
        return static_cast<char*>(workspace) + L.out_off;
    };
    enqueue_forward(p, x, x_dtype, pack, where, reinterpret_cast<hipStream_t>(stream));
    return sbev::check_launch(who);
}
