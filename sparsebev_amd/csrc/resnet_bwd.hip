// The ResNet backbone's backward (include/sbev_hip.h: sbev_resnet_backward) on v_mfma_f32_32x32x16_f16: from the gradients of the stage
// maps to the gradients of the convolution weights and of the BatchNorm gamma / beta of the trainable stages.  The forward is
// resnet.hip's with every activation from the last frozen stage's output onward kept (sbev_resnet_forward_train).  Every gradient
// operand goes to the matrix core as fp16 in a SCALED domain (grad_scale.hip, shared with the neck's backward): amax = max |gP_k| is found
// on the device and (2^e, 2^-e) with 2^e amax in [2^3, 2^4) written to the head of the workspace; every consumer reads the pair from there.
//
// Launches: grad_scale.hip's clear (the amax word and its ticket) and amax, seed, then per block, last block first,
//   rb_wgrad + rb_fold_bwd   conv3: A = g3, B = a2
//   rb_dgrad                 g2 = fp16(dgrad(g3, w3') [a2 > 0])
//   rb_wgrad + rb_fold_bwd   conv2: A = g2, B = a1 read at the block's stride, nine taps
//   rb_dgrad                 g1 = fp16(dgrad(g2, w2') [a1 > 0]): nine taps of the flipped image; at stride 2 a tap whose source parity
//                            does not match stages zeros
//   rb_wgrad + rb_fold_bwd   conv1: A = g1, B = x; downsample: A = g3, B = x read at the block's stride
//   rb_dgrad                 the previous block's g3 = fp16((acc + float(g3)) [+ 2^e gP] masked by x > 0); on a first block the
//                            downsample's products continue conv1's accumulation (one K loop over [g1 | g3 at the even pixels])
// rb_dgrad is resnet.hip's implicit GEMM (128 output pixels x 64 WN channels per workgroup, K in chunks of 64 channels of one tap) over
// the transposed / flipped fragment image of w'; rb_wgrad is the pixel-major product of the neck's weight gradients (32 pixels per K step
// staged row-major, read back transposed by fpn_common.hpp's tr_frag; the same slab rule) with both channel counts and the input stride
// as arguments.
//
// Who writes what: every stored element has one owning lane; nothing is read-modify-written except the amax word (integer max) and its
// ticket; slab partials fold in slab order.  Bit-reproducible.  Built with -ffp-contract=off: the fold backward is defined by
// individually rounded fp32 operations.
#include "fpn_common.hpp"
#include "resnet_train.hpp"

namespace {

using namespace sbev_fpn;
using namespace sbev_resnet;

constexpr int kKC = 64, kPitch = kKC + 8;
constexpr int kMaxLayers = SBEV_RESNET_MAX_LAYERS;

// ---------------------------------------------------------------- the last block's g3 = fp16(2^e gP [out > 0]), or zeros without a gP
struct SeedArgs {
    const void* gp;            // [rows, C] fp32 / fp16, or null
    const _Float16* out;       // the stage map
    _Float16* g;
    const float* scale;
    long long items;           // rows C / 8
    int f32;
};

__global__ __launch_bounds__(256) void rb_seed_kernel(const SeedArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.items) return;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (a.gp != nullptr) {
        const float up = a.scale[0];
        const f16x8 m = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(a.out + i * 8));
        if (a.f32) {
            const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(a.gp) + i * 8);
            const float4 lo = p[0], hi = p[1];
            const float t[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)m[j] > 0.f ? t[j] * up : 0.f;
        } else {
            const f16x8 t = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(static_cast<const _Float16*>(a.gp) + i * 8));
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)m[j] > 0.f ? (float)t[j] * up : 0.f;
        }
    }
    *reinterpret_cast<uint4*>(a.g + i * 8) = make_uint4(pack_h2(v[0], v[1]), pack_h2(v[2], v[3]), pack_h2(v[4], v[5]), pack_h2(v[6], v[7]));
}

// ---------------------------------------------------------------- data gradients
// One K segment: the gradient g [n, h, w, C] at the output of a convolution with `taps` taps and stride `stride` whose input plane is the
// launch's H x W.  Input pixel (Y, X) reads, for tap' = (ky', kx') of the FLIPPED image, the virtual pixel (Y + ky' - 1, X + kx' - 1)
// (a 1 x 1: (Y, X)); it is output pixel (vy / stride, vx / stride) where both are non-negative multiples of the stride inside the plane,
// and contributes nothing elsewhere.
struct Seg {
    const _Float16* g;
    int taps, stride, h, w, C;
};

struct DgradArgs {
    Seg s0, s1;                // s1.C == 0: one segment
    const uint4* wp;           // fragment images of the transposed (flipped) w' of s0, then of s1: [tap'][C / 16][N / 32][64 lanes][8 halves]
    const _Float16* mask;      // [rows, N] or null: the stored activation whose sign gates the result
    const _Float16* res;       // [rows, N] or null: added in fp32
    const void* gp;            // [rows, N] or null: a stage map's gradient, x 2^e, added last
    const float* scale;
    _Float16* y;               // [rows, N]
    int rows, N, H, W, gp_f32;
};

template <int WN>
__global__ __launch_bounds__(128 * WN) void rb_dgrad_kernel(const DgradArgs a) {
    constexpr int PER = 8 / WN;           // 16-byte pieces of a row's 64-channel chunk per thread
    __shared__ __attribute__((aligned(16))) _Float16 tile[kTileM * kPitch];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int srow = tid / WN, q = tid % WN;
    const long long r = (long long)blockIdx.x * kTileM + srow;
    const bool valid = r < a.rows;
    const int plane = a.H * a.W;
    const int img = valid ? (int)(r / plane) : 0, rem = valid ? (int)(r % plane) : 0;
    const int Y = rem / a.W, X = rem % a.W;
    uint4* dst = reinterpret_cast<uint4*>(tile + srow * kPitch + q * (8 * PER));

    const int NF = a.N / 32;
    const int group = (int)blockIdx.y * WN + wn;          // the wave's 64 output channels
    const int n0 = a.s0.taps * (a.s0.C / kKC), nchunks = n0 + a.s1.taps * (a.s1.C / kKC);
    f32x16 acc[2][2];
    zero_acc(acc);
    uint4 raw[PER];
    auto fetch = [&](int c) {
        const Seg& s = c < n0 ? a.s0 : a.s1;
        const int cc = c < n0 ? c : c - n0;
        const int per_tap = s.C / kKC, tap = cc / per_tap, kc = cc % per_tap;
        const int vy = Y + (s.taps == 9 ? tap / 3 - 1 : 0), vx = X + (s.taps == 9 ? tap % 3 - 1 : 0);
        const int sh = s.stride - 1;                      // stride 1 or 2
        const int sy = vy >> sh, sx = vx >> sh;
        const bool in = valid && vy >= 0 && vx >= 0 && ((vy | vx) & sh) == 0 && sy < s.h && sx < s.w;
#pragma unroll
        for (int i = 0; i < PER; ++i) raw[i] = make_uint4(0u, 0u, 0u, 0u);
        if (in) {
            const uint4* p = reinterpret_cast<const uint4*>(s.g + (((size_t)img * s.h + sy) * s.w + sx) * s.C + kc * kKC + q * (8 * PER));
#pragma unroll
            for (int i = 0; i < PER; ++i) raw[i] = p[i];
        }
    };
    fetch(0);
    const _Float16* arow = tile + (64 * wm + (lane & 31)) * kPitch + 8 * (lane >> 5);
    for (int c = 0; c < nchunks; ++c) {
#pragma unroll
        for (int i = 0; i < PER; ++i) dst[i] = raw[i];
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1);
        const uint4* bw = a.wp + ((size_t)c * (kKC / 16) * NF + 2 * group) * 64 + lane;
#pragma unroll
        for (int kk = 0; kk < kKC / 16; ++kk) {
            const uint4 b0 = bw[(size_t)kk * NF * 64], b1 = bw[(size_t)kk * NF * 64 + 64];
            const uint4 a0 = *reinterpret_cast<const uint4*>(arow + 16 * kk);
            const uint4 a1 = *reinterpret_cast<const uint4*>(arow + 32 * kPitch + 16 * kk);
            const f16x8 fa0 = __builtin_bit_cast(f16x8, a0), fa1 = __builtin_bit_cast(f16x8, a1);
            const f16x8 fb0 = __builtin_bit_cast(f16x8, b0), fb1 = __builtin_bit_cast(f16x8, b1);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    const int c0 = 64 * group + 2 * (lane & 31);
    const float up = a.gp != nullptr ? a.scale[0] : 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const long long row = (long long)blockIdx.x * kTileM + acc_row(wm, mb, rr, lane);
            if (row >= a.rows) continue;
            const size_t o = (size_t)row * a.N + c0;
            float v0 = acc[mb][0][rr], v1 = acc[mb][1][rr];
            if (a.res != nullptr) {
                const f16x2 pv = *reinterpret_cast<const f16x2*>(a.res + o);
                v0 += (float)pv.x;
                v1 += (float)pv.y;
            }
            if (a.gp != nullptr) {
                float g0, g1;
                if (a.gp_f32) {
                    const float2 t = *reinterpret_cast<const float2*>(static_cast<const float*>(a.gp) + o);
                    g0 = t.x; g1 = t.y;
                } else {
                    const f16x2 t = *reinterpret_cast<const f16x2*>(static_cast<const _Float16*>(a.gp) + o);
                    g0 = (float)t.x; g1 = (float)t.y;
                }
                v0 += g0 * up;
                v1 += g1 * up;
            }
            if (a.mask != nullptr) {
                const f16x2 m = *reinterpret_cast<const f16x2*>(a.mask + o);
                v0 = (float)m.x > 0.f ? v0 : 0.f;
                v1 = (float)m.y > 0.f ? v1 : 0.f;
            }
            *reinterpret_cast<unsigned*>(a.y + o) = pack_h2(v0, v1);
        }
    }
}

void launch_dgrad(int ct, const DgradArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows + kTileM - 1) / kTileM), (unsigned)(a.N / ct));
    if (ct == 64) hipLaunchKernelGGL(rb_dgrad_kernel<1>, grid, dim3(128), 0, s, a);
    else if (ct == 128) hipLaunchKernelGGL(rb_dgrad_kernel<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(rb_dgrad_kernel<4>, grid, dim3(512), 0, s, a);
}

// the forward's rule: the widest column tile that still gives every CU a workgroup, 64 where none does
int pick_col_tile(long long row_tiles, int N) {
    for (int ct = 256; ct > 64; ct >>= 1)
        if (N % ct == 0 && row_tiles * (N / ct) >= 256) return ct;
    return 64;
}

// ---------------------------------------------------------------- weight gradients: part[tap][co][ci] = sum_p gy[p, co] x[S p + tap, ci]
struct WgradArgs {
    const _Float16* gy;        // [pixels, Cout]: the gradient at the convolution's output, n h w pixels
    const _Float16* x;         // [n, H, W, Cin]: its input
    float* part;               // [slab][part_stride]: taps Cout Cin products, then Cout column sums of gy
    long long part_stride;
    int pixels, Cout, Cin, taps, stride, H, W, h, w, slab_len, TI, TJ;
};

__global__ __launch_bounds__(256) void rb_wgrad_kernel(const WgradArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 sA[kWK * kWPitch];
    __shared__ __attribute__((aligned(16))) _Float16 sB[kWK * kWPitch];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int row = tid >> 3, seg = tid & 7;
    const int bx = (int)blockIdx.x;
    const int tap = bx / (a.TI * a.TJ), ti = (bx / a.TJ) % a.TI, tj = bx % a.TJ;
    const int co0 = 128 * ti, ci0 = 128 * tj;
    const int dy = a.taps == 9 ? tap / 3 - 1 : 0, dx = a.taps == 9 ? tap % 3 - 1 : 0;
    const int p_begin = (int)blockIdx.y * a.slab_len, p_end = min(a.pixels, p_begin + a.slab_len);
    const int nchunks = (p_end - p_begin + kWK - 1) / kWK;
    const int plane = a.h * a.w;
    const bool col_sums = tap == (a.taps == 9 ? 4 : 0) && tj == 0;
    const bool a_in = co0 + 16 * seg < a.Cout, b_in = ci0 + 16 * seg < a.Cin;

    Raw<64, false> ra, rb;
    auto fetch = [&](int c) {
        const int p = p_begin + kWK * c + row;
        const bool ok = p < p_end;
        const bool oka = ok && a_in;
        load_raw<64, false>(ra, a.gy + ((size_t)(oka ? p : 0) * a.Cout + (oka ? co0 + 16 * seg : 0)), oka);
        const int q = ok ? p : 0;
        const int img = q / plane, rem = q % plane;
        const int iy = a.stride * (rem / a.w) + dy, ix = a.stride * (rem % a.w) + dx;
        const bool in = ok && b_in && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        load_raw<64, false>(rb, a.x + (in ? (((size_t)img * a.H + iy) * a.W + ix) * a.Cin + ci0 + 16 * seg : 0), in);
    };

    f32x16 acc[2][2];
    zero_acc(acc);
    float colsum = 0.f;
    if (nchunks > 0) fetch(0);
    for (int c = 0; c < nchunks; ++c) {
        store_raw<64, false>(ra, sA + row * kWPitch + 16 * seg);
        store_raw<64, false>(rb, sB + row * kWPitch + 16 * seg);
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1);
#pragma unroll
        for (int ks = 0; ks < kWK / 16; ++ks) {
            const f16x8 a0 = tr_frag(sA, 16 * ks, 64 * wr, lane), a1 = tr_frag(sA, 16 * ks, 64 * wr + 32, lane);
            const f16x8 b0 = tr_frag(sB, 16 * ks, 64 * wc, lane), b1 = tr_frag(sB, 16 * ks, 64 * wc + 32, lane);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (col_sums && tid < 128) {          // the bias gradient's slab sum: pixel after pixel, fp32
#pragma unroll 8
            for (int k = 0; k < kWK; ++k) colsum += (float)sA[k * kWPitch + tid];
        }
        __syncthreads();
    }

    float* part = a.part + (size_t)blockIdx.y * a.part_stride;
    float* wpart = part + (size_t)tap * a.Cout * a.Cin;
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = ci0 + 64 * wc + 32 * j + fr;
            if (ci >= a.Cin) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = co0 + 64 * wr + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fh;
                if (co < a.Cout) wpart[(size_t)co * a.Cin + ci] = acc[i][j][e];
            }
        }
    if (col_sums && tid < 128 && co0 + tid < a.Cout) part[(size_t)a.taps * a.Cout * a.Cin + co0 + tid] = colsum;
}

// ---------------------------------------------------------------- slabs in order, x 2^-e, then the BatchNorm fold's backward: one workgroup per output channel
struct FoldBwdArgs {
    const float* part;         // [slab][part_stride]: [tap][Cout][Cin], then [Cout]
    const float* scale;        // (2^e, 2^-e), or null: 1
    const void* w;             // [Cout, Cin, taps]
    const float *gamma, *mean, *var;
    float *gw, *ggamma, *gbeta;      // gw [Cout, Cin, taps]; ggamma / gbeta [Cout] or null
    long long part_stride;
    float eps;
    int n_slabs, Cin, Cout, taps, w_f32;
};

__global__ __launch_bounds__(256) void rb_fold_bwd_kernel(const FoldBwdArgs a) {
    __shared__ float red[256];
    const int co = (int)blockIdx.x, tid = (int)threadIdx.x;
    const float root = sqrtf(a.var[co] + a.eps);          // bn_fold_scale's denominator
    const float s = bn_fold_scale(a.gamma[co], a.var[co], a.eps);
    const float down = a.scale != nullptr ? a.scale[1] : 1.f;
    const int K = a.Cin * a.taps;
    float dot = 0.f;
    // tap-major like the partials: consecutive lanes read consecutive input channels of one tap
    for (int tap = 0; tap < a.taps; ++tap) {
        for (int ci = tid; ci < a.Cin; ci += 256) {
            const size_t at = ((size_t)tap * a.Cout + co) * a.Cin + ci;
            float sum = a.part[at];
            for (int sl = 1; sl < a.n_slabs; ++sl) sum += a.part[(size_t)sl * a.part_stride + at];
            const float gwp = sum * down;
            const size_t e = (size_t)co * K + (size_t)ci * a.taps + tap;
            const float wv = a.w_f32 ? static_cast<const float*>(a.w)[e] : (float)static_cast<const _Float16*>(a.w)[e];
            a.gw[e] = s * gwp;
            dot += wv * gwp;
        }
    }
    red[tid] = dot;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        const size_t at = (size_t)a.taps * a.Cout * a.Cin + co;
        float sum = a.part[at];
        for (int sl = 1; sl < a.n_slabs; ++sl) sum += a.part[(size_t)sl * a.part_stride + at];
        const float gb = sum * down;
        if (a.gbeta != nullptr) a.gbeta[co] = gb;
        if (a.ggamma != nullptr) a.ggamma[co] = (1.f / root) * (red[0] - a.mean[co] * gb);
    }
}

// ---------------------------------------------------------------- w' transposed (and flipped) -> the data gradients' fragment image, fp16
struct PackBwdArgs {
    const void* w;             // [Cout, Cin, taps]
    const float *gamma, *var;
    uint4* dst;
    float eps;
    int Cin, Cout, taps, f32;
    long long frags;           // taps * (Cout / 16) * (Cin / 32) * 64
};

__global__ __launch_bounds__(256) void rb_pack_bwd_kernel(const PackBwdArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.frags) return;
    const int NF = a.Cin / 32, KS = a.Cout / 16;
    const int lane = (int)(i & 63);
    const long long f = i >> 6;
    const int nt = (int)(f % NF);
    const long long rest = f / NF;
    const int ks = (int)(rest % KS), tapp = (int)(rest / KS);
    const int ci = 64 * (nt >> 1) + 2 * (lane & 31) + (nt & 1);
    const int k0 = 16 * ks + 8 * (lane >> 5);
    const int tap = a.taps == 9 ? 8 - tapp : 0;
    float p[8];      // the eight products first, their second rounding afterwards: all gathers in flight (resnet_train.hpp: bn_fold_round)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int co = k0 + k;
        const float s = bn_fold_scale(a.gamma[co], a.var[co], a.eps);
        const size_t e = ((size_t)co * a.Cin + ci) * a.taps + tap;
        const float w = a.f32 ? static_cast<const float*>(a.w)[e] : (float)static_cast<const _Float16*>(a.w)[e];
        p[k] = w * s;
    }
    unsigned h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f16x2 v;
        v.x = bn_fold_round(p[2 * j]);      // the forward's fold: the same w' bits
        v.y = bn_fold_round(p[2 * j + 1]);
        h[j] = __builtin_bit_cast(unsigned, v);
    }
    a.dst[i] = make_uint4(h[0], h[1], h[2], h[3]);
}

// ---------------------------------------------------------------- the plan (pure host)
int out_side(int in, int stride) { return (in - 1) / stride + 1; }

struct BwdPlan {
    TrainNet t;
    int trainable[kMaxLayers], dgrad[kMaxLayers];      // per launch: has parameter gradients; sends a data gradient to its input
    int slabs[kMaxLayers], slab_len[kMaxLayers];
    long long pack_off[kMaxLayers];                    // byte offset of the launch's image in the backward's pack, -1 without one
    long long ga_off, gb_off, g2_off, g1_off, part_off, bytes, pack_bytes;
    int launches;
};

int make_bwd_plan(const char* who, int depth, const int32_t* stage_blocks, int num_stages, int base, int64_t n, int H, int W, int n_out,
                  const int32_t* out_indices, int fts, BwdPlan* b) {
    if (int st = train_net(who, depth, stage_blocks, num_stages, base, n, H, W, n_out, out_indices, fts, &b->t)) return st;
    const TrainNet& t = b->t;
    long long g3 = 0, g2 = 0, g1 = 0, part = 0, pack = 0;
    int launches = 3;      // clear, amax, seed
    for (int i = 0; i < t.n_layers; ++i) {
        const TLayer& L = t.layer[i];
        b->trainable[i] = L.kind == 2 && L.stage >= fts - 1;
        b->dgrad[i] = 0;
        b->slabs[i] = b->slab_len[i] = 0;
        b->pack_off[i] = -1;
        if (!b->trainable[i]) continue;
        slab_rule(L.rows, &b->slabs[i], &b->slab_len[i]);
        part = std::max(part, b->slabs[i] * ((long long)L.taps * L.Cout * L.Cin + L.Cout));
        // conv1 and the downsample of the first trainable block read a frozen activation: no data gradient leaves them
        const bool first = L.stage == fts - 1 && L.block == 0;
        b->dgrad[i] = L.which == 1 || L.which == 3 || !first;
        launches += 2;
        if (L.which == 3) g3 = std::max(g3, L.rows * L.Cout * 2);
        if (L.which == 1) g2 = std::max(g2, L.rows * L.Cout * 2);
        if (L.which == 0) g1 = std::max(g1, L.rows * L.Cout * 2);
    }
    // the backward's pack, block after block: conv3, conv2, then conv1 with the downsample's image right behind it (one K loop reads both)
    for (int i = 0; i < t.n_layers; ++i) {
        if (!b->trainable[i] || t.layer[i].which != 0) continue;
        const int c1 = i, c2 = i + 1, ds = t.layer[i + 2].which == 2 ? i + 2 : -1, c3 = ds >= 0 ? i + 3 : i + 2;
        for (int j : {c3, c2, c1, ds}) {
            if (j < 0 || !b->dgrad[j]) continue;
            b->pack_off[j] = pack;
            pack += (long long)t.layer[j].taps * t.layer[j].Cin * t.layer[j].Cout * 2;
        }
        launches += 2 + (b->dgrad[c1] ? 1 : 0);
    }
    b->ga_off = 256;
    b->gb_off = b->ga_off + round_up(g3, 256);
    b->g2_off = b->gb_off + round_up(g3, 256);
    b->g1_off = b->g2_off + round_up(g2, 256);
    b->part_off = b->g1_off + round_up(g1, 256);
    b->bytes = n > 0 ? b->part_off + part * 4 : 0;
    b->pack_bytes = pack;
    b->launches = n > 0 ? launches : 0;
    return SBEV_OK;
}

int check_shape(const char* who, int64_t n, int H, int W, int Cin, int Cout, int taps, int stride) {
    SBEV_REQUIRE(taps == 1 || taps == 9, "%s: taps=%d (1 or 9)", who, taps);
    SBEV_REQUIRE(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", who, stride);
    SBEV_REQUIRE(Cin >= 64 && Cin % 64 == 0 && Cin <= 65536, "%s: %d input channels (a multiple of 64, at most 65536)", who, Cin);
    SBEV_REQUIRE(Cout >= 64 && Cout % 64 == 0 && Cout <= 65536, "%s: %d output channels (a multiple of 64, at most 65536)", who, Cout);
    SBEV_REQUIRE(n >= 0 && n <= (1LL << 20), "%s: n=%lld images", who, (long long)n);
    SBEV_REQUIRE(H >= 1 && W >= 1, "%s: an empty plane (%d x %d)", who, H, W);
    SBEV_REQUIRE(H <= 32767 && W <= 32767, "%s: plane %d x %d: a side above 32767", who, H, W);
    SBEV_REQUIRE((long long)n * H * W <= 0x7fffffffLL - kTileM, "%s: %lld pixels: row indices are 32-bit", who, (long long)n * H * W);
    return SBEV_OK;
}

void enqueue_wgrad(const _Float16* gy, const _Float16* x, float* part, const TLayer& L, int slabs, int slab_len, hipStream_t s) {
    WgradArgs w;
    w.gy = gy; w.x = x; w.part = part;
    w.part_stride = (long long)L.taps * L.Cout * L.Cin + L.Cout;
    w.pixels = (int)L.rows; w.Cout = L.Cout; w.Cin = L.Cin; w.taps = L.taps; w.stride = L.stride;
    w.H = L.H; w.W = L.W; w.h = L.h; w.w = L.w;
    w.slab_len = slab_len;
    w.TI = (L.Cout + 127) / 128; w.TJ = (L.Cin + 127) / 128;
    hipLaunchKernelGGL(rb_wgrad_kernel, dim3((unsigned)(L.taps * w.TI * w.TJ), (unsigned)slabs), dim3(256), 0, s, w);
}

void enqueue_fold(const float* part, int slabs, const float* scale, const void* w, int w_f32, const float* gamma, const float* mean,
                  const float* var, float eps, const TLayer& L, float* gw, float* ggamma, float* gbeta, hipStream_t s) {
    FoldBwdArgs f;
    f.part = part; f.scale = scale; f.w = w; f.gamma = gamma; f.mean = mean; f.var = var;
    f.gw = gw; f.ggamma = ggamma; f.gbeta = gbeta;
    f.part_stride = (long long)L.taps * L.Cout * L.Cin + L.Cout;
    f.eps = eps;
    f.n_slabs = slabs; f.Cin = L.Cin; f.Cout = L.Cout; f.taps = L.taps; f.w_f32 = w_f32;
    hipLaunchKernelGGL(rb_fold_bwd_kernel, dim3((unsigned)L.Cout), dim3(256), 0, s, f);
}

Seg seg_of(const _Float16* g, const TLayer& L) { return Seg{g, L.taps, L.stride, L.h, L.w, L.Cout}; }

}  // namespace

extern "C" int sbev_resnet_backward_plan(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W,
                                         int n_out, const int32_t* out_indices, int first_trainable_stage, int64_t* out) {
    const char* who = "sbev_resnet_backward_plan";
    SBEV_REQUIRE(out != nullptr, "%s: null out", who);
    BwdPlan b;
    if (int st = make_bwd_plan(who, depth, stage_blocks, num_stages, base_channels, n, H, W, n_out, out_indices, first_trainable_stage, &b))
        return st;
    for (int i = 0; i < SBEV_RESNET_BWD_PLAN_WORDS; ++i) out[i] = 0;
    out[0] = b.launches;
    out[1] = b.bytes;
    out[2] = b.pack_bytes;
    out[3] = n > 0 ? b.t.acts_bytes : 0;
    out[4] = b.t.ws_bytes;
    out[5] = b.t.n_layers;
    out[6] = b.t.first_kept;
    out[7] = b.ga_off; out[8] = b.gb_off; out[9] = b.g2_off; out[10] = b.g1_off; out[11] = b.part_off;
    out[12] = b.t.pack_bytes;
    for (int i = 0; i < b.t.n_layers; ++i) {
        int64_t* o = out + SBEV_RESNET_BWD_PLAN_HEAD + SBEV_RESNET_BWD_LAYER_WORDS * i;
        const TLayer& L = b.t.layer[i];
        o[0] = n > 0 ? b.slabs[i] : 0;
        o[1] = b.slab_len[i];
        o[2] = L.act == kNotKept ? -1 : L.out_k >= 0 ? -(2 + L.out_k) : L.act;
        o[3] = b.pack_off[i];
        o[4] = b.trainable[i];
        o[5] = b.dgrad[i];
    }
    return SBEV_OK;
}

extern "C" int sbev_resnet_pack_weights_bwd(int n_layers, const int32_t* desc, const void* const* w, const float* const* gamma,
                                            const float* const* var, float eps, int w_dtype, void* pack, sbev_stream_t stream) {
    const char* who = "sbev_resnet_pack_weights_bwd";
    SBEV_REQUIRE(n_layers >= 0 && n_layers <= kMaxLayers, "%s: %d layers (at most %d)", who, n_layers, kMaxLayers);
    SBEV_REQUIRE(w_dtype == SBEV_F32 || w_dtype == SBEV_F16, "%s: w_dtype %d (SBEV_F32 or SBEV_F16)", who, w_dtype);
    SBEV_REQUIRE(eps >= 0.f && std::isfinite(eps), "%s: eps=%g", who, (double)eps);
    if (n_layers == 0) return SBEV_OK;
    SBEV_REQUIRE(desc && w && gamma && var && pack, "%s: null pointer", who);
    SBEV_REQUIRE(aligned16(pack), "%s: 16-byte alignment", who);
    for (int i = 0; i < n_layers; ++i) {
        if (int st = check_shape(who, 1, 1, 1, desc[3 * i], desc[3 * i + 1], desc[3 * i + 2], 1)) return st;
        SBEV_REQUIRE(w[i] && gamma[i] && var[i], "%s: layer %d: null pointer", who, i);
        const bool al = (reinterpret_cast<uintptr_t>(w[i]) & (w_dtype == SBEV_F32 ? 3u : 1u)) == 0 &&
                        ((reinterpret_cast<uintptr_t>(gamma[i]) | reinterpret_cast<uintptr_t>(var[i])) & 3u) == 0;
        SBEV_REQUIRE(al, "%s: layer %d: misaligned tensor", who, i);
    }
    long long at = 0;
    for (int i = 0; i < n_layers; ++i) {
        PackBwdArgs a;
        a.w = w[i]; a.gamma = gamma[i]; a.var = var[i];
        a.eps = eps;
        a.Cin = desc[3 * i]; a.Cout = desc[3 * i + 1]; a.taps = desc[3 * i + 2];
        a.f32 = w_dtype == SBEV_F32;
        a.frags = (long long)a.taps * (a.Cout / 16) * (a.Cin / 32) * 64;
        a.dst = reinterpret_cast<uint4*>(static_cast<char*>(pack) + at);
        at += (long long)a.taps * a.Cin * a.Cout * 2;
        hipLaunchKernelGGL(rb_pack_bwd_kernel, dim3((unsigned)((a.frags + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    }
    return sbev::check_launch(who);
}

extern "C" int sbev_conv_dgrad_f16(const void* gy, const void* gy2, const void* pack, const void* mask, const void* res, const void* gp,
                                   int gp_dtype, const float* scale, void* gx, int64_t n, int H, int W, int Cin, int Cout, int taps, int stride,
                                   int Cout2, int stride2, int col_tile, sbev_stream_t stream) {
    const char* who = "sbev_conv_dgrad_f16";
    if (int st = check_shape(who, n, H, W, Cin, Cout, taps, stride)) return st;
    SBEV_REQUIRE(Cout2 == 0 || (Cout2 >= 64 && Cout2 % 64 == 0 && Cout2 <= 65536), "%s: Cout2=%d (0, or a multiple of 64, at most 65536)", who, Cout2);
    SBEV_REQUIRE(Cout2 == 0 || stride2 == 1 || stride2 == 2, "%s: stride2=%d (1 or 2)", who, stride2);
    SBEV_REQUIRE(gp_dtype == SBEV_F32 || gp_dtype == SBEV_F16, "%s: gp_dtype %d (SBEV_F32 or SBEV_F16)", who, gp_dtype);
    SBEV_REQUIRE(col_tile == 0 || ((col_tile == 64 || col_tile == 128 || col_tile == 256) && Cin % col_tile == 0),
                 "%s: col_tile=%d (0, or 64 / 128 / 256 dividing Cin=%d)", who, col_tile, Cin);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(gy && pack && gx && (Cout2 == 0 || gy2) && (gp == nullptr || scale), "%s: null pointer", who);
    SBEV_REQUIRE(aligned16(gy) && aligned16(gy2) && aligned16(pack) && aligned16(mask) && aligned16(res) && aligned16(gp) && aligned16(gx) &&
                     (reinterpret_cast<uintptr_t>(scale) & 3u) == 0, "%s: 16-byte alignment", who);
    DgradArgs a;
    a.s0 = Seg{static_cast<const _Float16*>(gy), taps, stride, out_side(H, stride), out_side(W, stride), Cout};
    a.s1 = Seg{static_cast<const _Float16*>(gy2), 1, Cout2 ? stride2 : 1, Cout2 ? out_side(H, stride2) : 1, Cout2 ? out_side(W, stride2) : 1, Cout2};
    a.wp = static_cast<const uint4*>(pack);
    a.mask = static_cast<const _Float16*>(mask); a.res = static_cast<const _Float16*>(res); a.gp = gp; a.scale = scale;
    a.y = static_cast<_Float16*>(gx);
    a.rows = (int)(n * H * W); a.N = Cin; a.H = H; a.W = W; a.gp_f32 = gp_dtype == SBEV_F32;
    launch_dgrad(col_tile ? col_tile : pick_col_tile((a.rows + kTileM - 1) / kTileM, Cin), a, reinterpret_cast<hipStream_t>(stream));
    return sbev::check_launch(who);
}

extern "C" int sbev_conv_wgrad_f16(const void* gy, const void* x, float* part, int64_t n, int H, int W, int Cin, int Cout, int taps, int stride,
                                   int slab_len, sbev_stream_t stream) {
    const char* who = "sbev_conv_wgrad_f16";
    if (int st = check_shape(who, n, H, W, Cin, Cout, taps, stride)) return st;
    SBEV_REQUIRE(slab_len == 0 || (slab_len >= kWK && slab_len % kWK == 0), "%s: slab_len=%d (0: the plan's rule, or a multiple of %d)", who,
                 slab_len, kWK);
    TLayer L;
    L.Cin = Cin; L.Cout = Cout; L.taps = taps; L.stride = stride; L.H = H; L.W = W; L.h = out_side(H, stride); L.w = out_side(W, stride);
    L.rows = (long long)n * L.h * L.w;
    int slabs, len;
    slab_rule(L.rows, &slabs, &len);
    if (slab_len) { len = slab_len; slabs = (int)((L.rows + len - 1) / len); }
    SBEV_REQUIRE(slabs <= 65535, "%s: %d slabs (at most 65535)", who, slabs);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(gy && x && part, "%s: null pointer", who);
    SBEV_REQUIRE(aligned16(gy) && aligned16(x) && aligned16(part), "%s: 16-byte alignment", who);
    enqueue_wgrad(static_cast<const _Float16*>(gy), static_cast<const _Float16*>(x), part, L, slabs, len, reinterpret_cast<hipStream_t>(stream));
    return sbev::check_launch(who);
}

extern "C" int sbev_bn_fold_backward(const float* part, int slabs, const float* scale, const void* w, int w_dtype, const float* gamma,
                                     const float* mean, const float* var, float eps, int Cin, int Cout, int taps, float* grad_w,
                                     float* grad_gamma, float* grad_beta, sbev_stream_t stream) {
    const char* who = "sbev_bn_fold_backward";
    if (int st = check_shape(who, 1, 1, 1, Cin, Cout, taps, 1)) return st;
    SBEV_REQUIRE(slabs >= 1 && slabs <= 65535, "%s: slabs=%d (1 .. 65535)", who, slabs);
    SBEV_REQUIRE(w_dtype == SBEV_F32 || w_dtype == SBEV_F16, "%s: w_dtype %d (SBEV_F32 or SBEV_F16)", who, w_dtype);
    SBEV_REQUIRE(eps >= 0.f && std::isfinite(eps), "%s: eps=%g", who, (double)eps);
    SBEV_REQUIRE(part && w && gamma && mean && var && grad_w, "%s: null pointer", who);
    bool al = (reinterpret_cast<uintptr_t>(w) & (w_dtype == SBEV_F32 ? 3u : 1u)) == 0;
    for (const float* q : {part, scale, gamma, mean, var, (const float*)grad_w, (const float*)grad_gamma, (const float*)grad_beta})
        al = al && (reinterpret_cast<uintptr_t>(q) & 3u) == 0;
    SBEV_REQUIRE(al, "%s: misaligned tensor", who);
    TLayer L;
    L.Cin = Cin; L.Cout = Cout; L.taps = taps;
    enqueue_fold(part, slabs, scale, w, w_dtype == SBEV_F32, gamma, mean, var, eps, L, grad_w, grad_gamma, grad_beta,
                 reinterpret_cast<hipStream_t>(stream));
    return sbev::check_launch(who);
}

extern "C" int sbev_resnet_backward(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int64_t n, int H, int W, int n_out,
                                    const int32_t* out_indices, int first_trainable_stage, const void* acts, const void* const* outs,
                                    const void* const* grad_outs, int g_dtype, const void* pack_bwd, void* workspace, const void* const* w,
                                    int w_dtype, const float* const* gamma, const float* const* mean, const float* const* var, float eps,
                                    float* const* grad_w, float* const* grad_gamma, float* const* grad_beta, sbev_stream_t stream) {
    const char* who = "sbev_resnet_backward";
    BwdPlan b;
    if (int st = make_bwd_plan(who, depth, stage_blocks, num_stages, base_channels, n, H, W, n_out, out_indices, first_trainable_stage, &b))
        return st;
    const TrainNet& t = b.t;
    SBEV_REQUIRE(g_dtype == SBEV_F32 || g_dtype == SBEV_F16, "%s: g_dtype %d (SBEV_F32 or SBEV_F16)", who, g_dtype);
    SBEV_REQUIRE(w_dtype == SBEV_F32 || w_dtype == SBEV_F16, "%s: w_dtype %d (SBEV_F32 or SBEV_F16)", who, w_dtype);
    SBEV_REQUIRE(eps >= 0.f && std::isfinite(eps), "%s: eps=%g", who, (double)eps);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(acts && outs && grad_outs && pack_bwd && workspace && w && gamma && mean && var && grad_w && grad_gamma && grad_beta,
                 "%s: null pointer", who);
    for (int k = 0; k < n_out; ++k) SBEV_REQUIRE(outs[k] != nullptr && grad_outs[k] != nullptr, "%s: output %d: null pointer", who, k);
    bool al = aligned16(acts) && aligned16(pack_bwd) && aligned16(workspace);
    for (int k = 0; k < n_out; ++k) al = al && aligned16(outs[k]) && aligned16(grad_outs[k]);
    // the per-convolution lists are indexed like sbev_resnet_pack_weights' for a whole net: convolution j is launch j + 1 (j >= 1; 0: the stem)
    for (int i = 2; i < t.n_layers; ++i) {
        if (!b.trainable[i]) continue;
        const int j = i - 1;
        SBEV_REQUIRE(w[j] && gamma[j] && mean[j] && var[j] && grad_w[j], "%s: convolution %d: null pointer", who, j);
        al = al && (reinterpret_cast<uintptr_t>(w[j]) & (w_dtype == SBEV_F32 ? 3u : 1u)) == 0;
        for (const float* q : {gamma[j], mean[j], var[j], (const float*)grad_w[j], (const float*)grad_gamma[j], (const float*)grad_beta[j]})
            al = al && (reinterpret_cast<uintptr_t>(q) & 3u) == 0;
    }
    SBEV_REQUIRE(al, "%s: 16-byte alignment (4-byte of the fp32 tensors)", who);

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const float* scale = reinterpret_cast<const float*>(ws);
    _Float16* gbuf[2] = {reinterpret_cast<_Float16*>(ws + b.ga_off), reinterpret_cast<_Float16*>(ws + b.gb_off)};
    _Float16* g2 = reinterpret_cast<_Float16*>(ws + b.g2_off);
    _Float16* g1 = reinterpret_cast<_Float16*>(ws + b.g1_off);
    float* part = reinterpret_cast<float*>(ws + b.part_off);
    const bool gf32 = g_dtype == SBEV_F32, wf32 = w_dtype == SBEV_F32;
    auto act = [&](int layer) -> const _Float16* {
        const TLayer& L = t.layer[layer];
        return static_cast<const _Float16*>(L.out_k >= 0 ? outs[L.out_k] : static_cast<const void*>(static_cast<const char*>(acts) + L.act));
    };
    auto image = [&](int layer) { return reinterpret_cast<const uint4*>(static_cast<const char*>(pack_bwd) + b.pack_off[layer]); };
    auto params = [&](int layer, const _Float16* gy, const _Float16* x) {
        const int j = layer - 1;
        enqueue_wgrad(gy, x, part, t.layer[layer], b.slabs[layer], b.slab_len[layer], s);
        enqueue_fold(part, b.slabs[layer], scale, w[j], wf32, gamma[j], mean[j], var[j], eps, t.layer[layer], grad_w[j], grad_gamma[j],
                     grad_beta[j], s);
    };
    auto dgrad = [&](const Seg& s0, const Seg& s1, int layer, const TLayer& in, const _Float16* mask, const _Float16* res, const void* gp,
                     _Float16* y) {
        DgradArgs a;
        a.s0 = s0; a.s1 = s1;
        a.wp = image(layer);
        a.mask = mask; a.res = res; a.gp = gp; a.scale = scale;
        a.y = y;
        a.rows = (int)in.rows; a.N = in.Cout; a.H = in.h; a.W = in.w; a.gp_f32 = gf32;
        launch_dgrad(pick_col_tile((a.rows + kTileM - 1) / kTileM, a.N), a, s);
    };

    {
        long long count[4];
        for (int k = 0; k < n_out; ++k) count[k] = t.layer[t.out_layer[k]].rows * t.layer[t.out_layer[k]].Cout;
        if (int st = sbev::launch_grad_scale(who, grad_outs, count, n_out, gf32, ws, s)) return st;
    }
    int cur = 0;      // gbuf[cur] holds the g3 of the block being walked
    {
        const int last = t.n_layers - 1;
        const TLayer& L = t.layer[last];
        SeedArgs a;
        a.gp = L.out_k >= 0 ? grad_outs[L.out_k] : nullptr;
        a.out = act(last);
        a.g = gbuf[cur];
        a.scale = scale;
        a.items = L.rows * L.Cout / 8;
        a.f32 = gf32;
        hipLaunchKernelGGL(rb_seed_kernel, dim3((unsigned)((a.items + 255) / 256)), dim3(256), 0, s, a);
    }
    const Seg none{nullptr, 1, 1, 1, 1, 0};
    // blocks last to first: c3 is a block's last launch
    for (int c3 = t.n_layers - 1; c3 >= 2 && b.trainable[c3];) {
        const int ds = t.layer[c3 - 1].which == 2 ? c3 - 1 : -1;
        const int c2 = ds >= 0 ? c3 - 2 : c3 - 1, c1 = c2 - 1;
        const int xin = t.layer[c1].in_layer;
        const _Float16* g3 = gbuf[cur];
        params(c3, g3, act(c2));
        dgrad(seg_of(g3, t.layer[c3]), none, c3, t.layer[c2], act(c2), nullptr, nullptr, g2);
        params(c2, g2, act(c1));
        dgrad(seg_of(g2, t.layer[c2]), none, c2, t.layer[c1], act(c1), nullptr, nullptr, g1);
        params(c1, g1, act(xin));
        if (ds >= 0) params(ds, g3, act(xin));
        if (!b.dgrad[c1]) break;
        const TLayer& X = t.layer[xin];
        const void* gp = ds >= 0 && X.out_k >= 0 ? grad_outs[X.out_k] : nullptr;
        dgrad(seg_of(g1, t.layer[c1]), ds >= 0 ? seg_of(g3, t.layer[ds]) : none, c1, X, act(xin), ds >= 0 ? nullptr : g3, gp, gbuf[cur ^ 1]);
        cur ^= 1;
        c3 = xin;
    }
    return sbev::check_launch(who);
}
