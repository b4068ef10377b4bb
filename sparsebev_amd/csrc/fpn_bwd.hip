// The FPN neck's backward (include/sbev_hip.h: sbev_fpn_backward) on v_mfma_f32_32x32x16_f16: from the output gradients gP_o to the
// gradients of the inputs, the 1x1 and 3x3 weights and the biases.  Every gradient operand goes to the matrix core as fp16 in a SCALED
// domain (grad_scale.hip, shared with the backbone's backward): amax = max |gP_o| is found on the device and (2^e, 2^-e) with 2^e amax in
// [2^3, 2^4) written to the head of the workspace; every consumer reads the pair from there (no host read: the call can be captured),
// fp32 results are multiplied by 2^-e on the way out.
//
// Launches for L levels (plus grad_scale.hip's tiny launch that clears the amax word and the ticket): 4 L + 1, or 5 L + 1 with input
// gradients.
//   1            grad_scale_amax_kernel: amax over every output gradient, the last workgroup writes the pair.  A zero or non-finite
//                amax gives e = 0: an inf or NaN then travels as it is.
//   1            fpn_dgrad3_kernel: D_l = conv3x3(fp16(2^e G_l), W3_l'), the forward's convolution kernel shape (same tile table, same
//                fragment-ordered weight image, of the flipped and transposed weights).  G_l is staged from gP_l on the way into LDS:
//                fp32 (or fp16) -> + the extra levels' gradients at the pixels they were taken from (last level) -> x 2^e -> fp16.
//                Level 0 stores gM_0 = fp16(D_0) directly, the others D_l in fp32.
//   L - 1        fpn_adjoint_kernel, finest parent first: gM_l = fp16(D_l + sum of gM_{l-1} over the children of the pixel), the
//                children being the exact preimage of the forward's nearest rule (two binary searches per axis over the monotone
//                source index), summed in fp32 row-major.  Each parent gathers: no atomics.
//   L (optional) fpn_lat_dgrad_kernel: gC_l = 2^-e gM_l . Wlat_l, computed transposed (rows = input channels, columns = pixels) so a
//                lane owns 4 consecutive channels of a pixel; N = Cin_l in blocks of 32.
//   2 L          fpn_wgrad_kernel: gW3_l (9 taps x 2 x 2 tiles of 128 x 128) and gWlat_l (2 x ceil(Cin / 128) tiles), K = the level's
//                pixels split into slabs (grid.y), fp32 partial per slab.  Both operands are pixel-major, the reduction runs over
//                pixels: 32 pixels x 128 channels per operand are staged row-major into LDS and read back TRANSPOSED by
//                ds_read_b64_tr_b16 (row pitch 320 bytes: the four rows of a 16-lane block fall on disjoint bank quarters).  The
//                column sums of the A operand (the two bias gradients) ride in the workgroups of the centre tap / first column tile.
//   L            fpn_fold_kernel: partials of slab 0, 1, .. added in that order, x 2^-e, stored as gW3 [256, 256, 3, 3], gWlat, gc, gblat.
//
// Who writes what: every element of every result and intermediate is stored by exactly one lane; nothing is read-modify-written
// except the amax word (integer max) and the ticket.  The results are bit-reproducible.
#include "fpn_common.hpp"

namespace {

using namespace sbev_fpn;

// ---------------------------------------------------------------- staging of the gradient operand G_l
template <bool F32>
__device__ __forceinline__ void unpack16(const Raw<64, F32>& r, float (&v)[16]) {
    if constexpr (F32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[4 * i] = __uint_as_float(r.v[i].x); v[4 * i + 1] = __uint_as_float(r.v[i].y);
            v[4 * i + 2] = __uint_as_float(r.v[i].z); v[4 * i + 3] = __uint_as_float(r.v[i].w);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned w[4] = {r.v[i].x, r.v[i].y, r.v[i].z, r.v[i].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f16x2 h = __builtin_bit_cast(f16x2, w[j]);
                v[8 * i + 2 * j] = (float)h.x;
                v[8 * i + 2 * j + 1] = (float)h.y;
            }
        }
    }
}

// G_{L-1} = gP_{L-1} + the gradient of extra level 1, 2, .. (added in that order, fp32) at the pixels with y, x multiples of 2^e
template <bool F32>
__device__ __forceinline__ void add_extras(float (&v)[16], const void* const (&extra)[kMaxOut], int n_extra, int H, int W, int img, int y, int x,
                                           int ch) {
#pragma unroll
    for (int e = 1; e < kMaxOut; ++e) {
        if (e <= n_extra && ((y | x) & ((1 << e) - 1)) == 0) {
            const int He = (H + (1 << e) - 1) >> e, We = (W + (1 << e) - 1) >> e;
            const size_t o = (((size_t)img * He + (y >> e)) * We + (x >> e)) * kOut + ch;
            Raw<64, F32> r;
            load_raw<64, F32>(r, static_cast<const char*>(extra[e]) + o * (F32 ? 4 : 2), true);
            float t[16];
            unpack16<F32>(r, t);
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] += t[i];
        }
    }
}

// fp16(2^e v) of 16 channels -> 32 bytes of LDS
__device__ __forceinline__ void store16(const float (&v)[16], float up, _Float16* lds) {
    uint4* d = reinterpret_cast<uint4*>(lds);
#pragma unroll
    for (int i = 0; i < 2; ++i)
        d[i] = make_uint4(pack_h2(v[8 * i] * up, v[8 * i + 1] * up), pack_h2(v[8 * i + 2] * up, v[8 * i + 3] * up),
                          pack_h2(v[8 * i + 4] * up, v[8 * i + 5] * up), pack_h2(v[8 * i + 6] * up, v[8 * i + 7] * up));
}

// ---------------------------------------------------------------- 3x3 data gradient: every level and image in one launch
struct DgradArgs {
    const void* g[kMaxIn];              // gP_l [n, H, W, 256]
    const void* extra[kMaxOut];         // gP of extra level e (1 ..)
    const uint4* wp[kMaxIn];            // packed flipped / transposed 3x3 weights per level
    void* out[kMaxIn];                  // level 0: gM_0 fp16; level l > 0: D_l fp32
    const float* scale;
    int tile_end[kMaxIn];
    int pixels[kMaxIn];
    int H[kMaxIn], W[kMaxIn];
    int L, n_extra;
};

template <bool F32>
__global__ __launch_bounds__(kThreads) void fpn_dgrad3_kernel(const DgradArgs a) {
    constexpr int KC = 64, pitch = KC + 8, kPerTap = kOut / KC;
    constexpr long long esize = F32 ? 4 : 2;
    __shared__ __attribute__((aligned(16))) _Float16 tile[kTileM * pitch];
    __shared__ int rpix[kTileM];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int srow = tid >> 2, q = tid & 3;

    int level = 0;
#pragma unroll
    for (int l = 0; l < kMaxIn - 1; ++l)
        if (l + 1 < a.L && (int)blockIdx.x >= a.tile_end[l]) level = l + 1;
    level = __builtin_amdgcn_readfirstlane(level);
    const int tile0 = level > 0 ? a.tile_end[level - 1] : 0;
    const int H = a.H[level], W = a.W[level], npix = a.pixels[level];
    const uint4* wp = a.wp[level];
    const bool with_extras = level == a.L - 1 && a.n_extra > 0;
    const float up = a.scale[0];

    const long long p = (long long)((int)blockIdx.x - tile0) * kTileM + srow;
    const bool valid = p < npix;
    const int plane = H * W;
    const int img = valid ? (int)(p / plane) : 0, rem = valid ? (int)(p % plane) : 0;
    const int y = rem / W, x = rem % W;
    if (q == 0) rpix[srow] = valid ? (int)p : -1;
    const char* src = static_cast<const char*>(a.g[level]) + ((long long)(valid ? p : 0) * kOut + q * (KC / 4)) * esize;
    _Float16* dst = tile + srow * pitch + q * (KC / 4);

    f32x16 acc[2][2];
    zero_acc(acc);
    constexpr int nchunks = 9 * kPerTap;
    Raw<KC, F32> raw;
    auto fetch = [&](int c) {
        const int tap = c / kPerTap, kc = c % kPerTap;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const bool in = valid && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
        load_raw<KC, F32>(raw, src + (((long long)dy * W + dx) * kOut + kc * KC) * esize, in);
    };
    auto stage = [&](int c) {
        float v[16];
        unpack16<F32>(raw, v);
        if (with_extras) {
            const int tap = c / kPerTap, kc = c % kPerTap;
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (valid && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                add_extras<F32>(v, a.extra, a.n_extra, H, W, img, yy, xx, kc * KC + q * (KC / 4));
        }
        store16(v, up, dst);
    };
    fetch(0);
    for (int c = 0; c < nchunks; ++c) {
        stage(c);
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1);
        mma_chunk<KC>(acc, tile, wp, c * (KC / 16), wm, wn, lane);
        __syncthreads();
    }

    const int c0 = 64 * wn + 2 * (lane & 31);
    void* out = a.out[level];
    const int out_f32 = level > 0;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int px = rpix[acc_row(wm, mb, rr, lane)];
            if (px < 0) continue;
            store_pair(out, (size_t)px * kOut + c0, acc[mb][0][rr], acc[mb][1][rr], out_f32);
        }
    }
}

// ---------------------------------------------------------------- top-down adjoint: one parent level, all images
struct AdjointArgs {
    const float* d;            // D_l [n, pH, pW, 256]
    const _Float16* child;     // gM_{l-1} [n, H, W, 256]
    _Float16* gm;              // gM_l
    int pixels, pH, pW, H, W;
    float sy, sx;              // the forward's float32(pH / H), float32(pW / W)
};

// first destination index whose source index is >= t (out_size when there is none): nearest_src is monotone in dst
__device__ __forceinline__ int first_dst(int t, float scale, int in_size, int out_size) {
    int lo = 0, hi = out_size;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (nearest_src(mid, scale, in_size) >= t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void fpn_adjoint_kernel(const AdjointArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int pix = (int)(i >> 5), c8 = 8 * (int)(i & 31);
    if (pix >= a.pixels) return;
    const int plane = a.pH * a.pW;
    const int img = pix / plane, rem = pix % plane;
    const int py = rem / a.pW, px = rem % a.pW;
    const int y0 = first_dst(py, a.sy, a.pH, a.H), y1 = first_dst(py + 1, a.sy, a.pH, a.H);
    const int x0 = first_dst(px, a.sx, a.pW, a.W), x1 = first_dst(px + 1, a.sx, a.pW, a.W);
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.child + (((size_t)img * a.H + y) * a.W + x) * kOut + c8);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f16x2 h = __builtin_bit_cast(f16x2, w[j]);
                s[2 * j] += (float)h.x;
                s[2 * j + 1] += (float)h.y;
            }
        }
    const float4* dp = reinterpret_cast<const float4*>(a.d + (size_t)pix * kOut + c8);
    const float4 d0 = dp[0], d1 = dp[1];
    *reinterpret_cast<uint4*>(a.gm + (size_t)pix * kOut + c8) =
        make_uint4(pack_h2(d0.x + s[0], d0.y + s[1]), pack_h2(d0.z + s[2], d0.w + s[3]), pack_h2(d1.x + s[4], d1.y + s[5]),
                   pack_h2(d1.z + s[6], d1.w + s[7]));
}

// ---------------------------------------------------------------- lateral data gradient: gC^T = Wlat^T . gM^T
struct LatDgradArgs {
    const _Float16* gm;        // gM_l [rows, 256]
    const uint4* wp;           // [Cin / 32][16][64 lanes] fragments of Wlat^T
    void* gc;                  // [rows, Cin] fp32 or fp16
    const float* scale;
    int rows, Cin;
};

template <bool F32>
__global__ __launch_bounds__(256) void fpn_lat_dgrad_kernel(const LatDgradArgs a) {
    const int tid = (int)threadIdx.x, lane = tid & 63, fr = lane & 31, fh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long p = (long long)blockIdx.x * 128 + 32 * wave + fr;
    const long long pr = p < a.rows ? p : a.rows - 1;
    const float down = a.scale[1];
    f16x8 b[16];
    const uint4* src = reinterpret_cast<const uint4*>(a.gm + (size_t)pr * kOut + 8 * fh);
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) b[ks] = __builtin_bit_cast(f16x8, src[2 * ks]);
    const int nblk = a.Cin / 32;
    const int cb0 = 8 * (int)blockIdx.y, cb1 = min(nblk, cb0 + 8);
    for (int cb = cb0; cb < cb1; ++cb) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const uint4* w = a.wp + (size_t)cb * 16 * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w[ks * 64]), b[ks], acc, 0, 0, 0);
        if (p < a.rows) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const size_t o = (size_t)p * a.Cin + 32 * cb + 8 * g + 4 * fh;
                const float v0 = acc[4 * g] * down, v1 = acc[4 * g + 1] * down, v2 = acc[4 * g + 2] * down, v3 = acc[4 * g + 3] * down;
                if constexpr (F32)
                    *reinterpret_cast<float4*>(static_cast<float*>(a.gc) + o) = make_float4(v0, v1, v2, v3);
                else
                    *reinterpret_cast<uint2*>(static_cast<_Float16*>(a.gc) + o) = make_uint2(pack_h2(v0, v1), pack_h2(v2, v3));
            }
        }
    }
}

// ---------------------------------------------------------------- weight gradients: C[co, ci] = sum_p A[p, co] B[p (+ tap), ci]
struct WgradArgs {
    const void* a;             // MODE 0: gP_l [pixels, 256] (F32: its dtype)    MODE 1: gM_l fp16 [pixels, 256]
    const void* b;             // MODE 0: M_l fp16 [pixels, 256]                 MODE 1: C_l [pixels, N] (F32: its dtype)
    const void* extra[kMaxOut];
    const float* scale;
    float* part;               // this level's partials: [slab][part_stride]
    long long part_stride, w_off, bias_off;
    int pixels, H, W, N, slab_len, n_extra;
};

template <int MODE, bool F32>
__global__ __launch_bounds__(256) void fpn_wgrad_kernel(const WgradArgs a) {
    constexpr bool AF32 = MODE == 0 && F32, BF32 = MODE == 1 && F32;
    __shared__ __attribute__((aligned(16))) _Float16 sA[kWK * kWPitch];
    __shared__ __attribute__((aligned(16))) _Float16 sB[kWK * kWPitch];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int row = tid >> 3, seg = tid & 7;
    const int bx = (int)blockIdx.x;
    const int tap = MODE == 0 ? bx >> 2 : 0;
    const int ti = MODE == 0 ? (bx >> 1) & 1 : bx & 1, tj = MODE == 0 ? bx & 1 : bx >> 1;
    const int co0 = 128 * ti, ci0 = 128 * tj;
    const int dy = MODE == 0 ? tap / 3 - 1 : 0, dx = MODE == 0 ? tap % 3 - 1 : 0;
    const int p_begin = (int)blockIdx.y * a.slab_len, p_end = min(a.pixels, p_begin + a.slab_len);
    const int nchunks = (p_end - p_begin + kWK - 1) / kWK;
    const int H = a.H, W = a.W, plane = H * W;
    const float up = a.scale[0];
    const bool col_sums = MODE == 0 ? (tap == 4 && tj == 0) : tj == 0;

    Raw<64, AF32> ra;
    Raw<64, BF32> rb;
    auto fetch = [&](int c) {
        const int p = p_begin + kWK * c + row;
        const bool ok = p < p_end;
        load_raw<64, AF32>(ra, static_cast<const char*>(a.a) + ((size_t)(ok ? p : 0) * kOut + co0 + 16 * seg) * (AF32 ? 4 : 2), ok);
        if constexpr (MODE == 0) {
            const int rem = (ok ? p : 0) % plane;
            const int yy = rem / W + dy, xx = rem % W + dx;
            const bool in = ok && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            load_raw<64, false>(rb, static_cast<const _Float16*>(a.b) + ((long long)(in ? p + dy * W + dx : 0) * kOut + ci0 + 16 * seg), in);
        } else {
            const bool in = ok && ci0 + 16 * seg < a.N;
            load_raw<64, BF32>(rb, static_cast<const char*>(a.b) + ((size_t)(in ? p : 0) * a.N + (in ? ci0 + 16 * seg : 0)) * (BF32 ? 4 : 2), in);
        }
    };
    auto stage = [&](int c) {
        _Float16* da = sA + row * kWPitch + 16 * seg;
        if constexpr (MODE == 0) {
            float v[16];
            unpack16<AF32>(ra, v);
            const int p = p_begin + kWK * c + row;
            if (a.n_extra > 0 && p < p_end) {
                const int img = p / plane, rem = p % plane;
                add_extras<AF32>(v, a.extra, a.n_extra, H, W, img, rem / W, rem % W, co0 + 16 * seg);
            }
            store16(v, up, da);
        } else {
            store_raw<64, false>(ra, da);
        }
        store_raw<64, BF32>(rb, sB + row * kWPitch + 16 * seg);
    };

    f32x16 acc[2][2];
    zero_acc(acc);
    float colsum = 0.f;
    fetch(0);
    for (int c = 0; c < nchunks; ++c) {
        stage(c);
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
    float* wpart = part + a.w_off + (size_t)tap * kOut * kOut;
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = ci0 + 64 * wc + 32 * j + fr;
            if (ci >= a.N) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = co0 + 64 * wr + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fh;
                wpart[(size_t)co * a.N + ci] = acc[i][j][e];
            }
        }
    if (col_sums && tid < 128) part[a.bias_off + co0 + tid] = colsum;
}

// ---------------------------------------------------------------- slab 0 + slab 1 + .., x 2^-e, into the gradients' own layouts
struct FoldArgs {
    const float* part;
    const float* scale;
    float* gw3;                // [256, 256, 3, 3]
    float* gwlat;              // [256, Cin]
    float* gc;                 // [256]
    float* gblat;              // [256]
    long long stride;
    int n_slabs, Cin;
};

__global__ __launch_bounds__(256) void fpn_fold_kernel(const FoldArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n3 = 9LL * kOut * kOut, nl = (long long)kOut * a.Cin;
    if (i >= n3 + nl + 2 * kOut) return;
    float s = a.part[i];
    for (int k = 1; k < a.n_slabs; ++k) s += a.part[(size_t)k * a.stride + i];
    s *= a.scale[1];
    if (i < n3) {
        const int tap = (int)(i >> 16), rem = (int)(i & 65535);
        a.gw3[(size_t)rem * 9 + tap] = s;
    } else if (i < n3 + nl) {
        a.gwlat[i - n3] = s;
    } else if (i < n3 + nl + kOut) {
        a.gc[i - n3 - nl] = s;
    } else {
        a.gblat[i - n3 - nl - kOut] = s;
    }
}

// ---------------------------------------------------------------- weights -> the data gradients' fragment images, fp16
struct PackBwdArgs {
    const void* w;            // conv: [256, 256, 3, 3]; lateral: [256, Cin]
    uint4* dst;
    int Cin, f32, conv;
    long long frags;
};

__global__ __launch_bounds__(256) void fpn_pack_bwd_kernel(const PackBwdArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.frags) return;
    const int lane = (int)(i & 63);
    size_t elem[8];
    if (a.conv) {             // the forward's image of W3'[n][k][tap] = W3[k][n][8 - tap]
        const int nt = (int)((i >> 6) & 7);
        const long long rest = i >> 9;
        const int ks = (int)(rest % (kOut / 16)), tap = (int)(rest / (kOut / 16));
        const int n = 64 * (nt >> 1) + 2 * (lane & 31) + (nt & 1);
        const int k0 = 16 * ks + 8 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < 8; ++j) elem[j] = ((size_t)(k0 + j) * kOut + n) * 9 + (8 - tap);
    } else {                  // A operand of gC^T: row ci = 32 cb + (lane & 31), k = co = 16 ks + 8 (lane >> 5) + j
        const int ks = (int)((i >> 6) & 15), cb = (int)(i >> 10);
        const int ci = 32 * cb + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < 8; ++j) elem[j] = (size_t)(k0 + j) * a.Cin + ci;
    }
    unsigned h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
            v[t] = a.f32 ? static_cast<const float*>(a.w)[elem[2 * j + t]] : (float)static_cast<const _Float16*>(a.w)[elem[2 * j + t]];
        h[j] = pack_h2(v[0], v[1]);
    }
    a.dst[i] = make_uint4(h[0], h[1], h[2], h[3]);
}

// ---------------------------------------------------------------- the plan (pure host)
struct BwdPlan {
    Plan f;
    int slabs[kMaxIn], slab_len[kMaxIn];
    long long part_stride[kMaxIn];       // floats per slab
    long long gm_off, d_off, part_off, bytes;      // byte offsets in the workspace
    int launches;
};

int make_bwd_plan(const char* who, int n_levels, const int32_t* chw, int64_t n, int num_outs, int want_input_grads, BwdPlan* b) {
    if (int st = make_plan(who, n_levels, chw, n, num_outs, &b->f)) return st;
    SBEV_REQUIRE(want_input_grads == 0 || want_input_grads == 1, "%s: want_input_grads=%d (0 or 1)", who, want_input_grads);
    const Plan& p = b->f;
    long long part = 0;
    for (int l = 0; l < kMaxIn; ++l) b->slabs[l] = b->slab_len[l] = 0, b->part_stride[l] = 0;
    for (int l = 0; l < p.L; ++l) {
        slab_rule(p.pixels[l], &b->slabs[l], &b->slab_len[l]);
        b->part_stride[l] = 9LL * kOut * kOut + (long long)kOut * p.Cin[l] + 2 * kOut;
        part = std::max(part, b->slabs[l] * b->part_stride[l]);
    }
    b->gm_off = 256;
    b->d_off = b->gm_off + round_up(p.total * kOut * 2, 256);
    b->part_off = b->d_off + round_up((p.total - p.pixels[0]) * kOut * 4, 256);
    b->bytes = n > 0 ? b->part_off + part * 4 : 0;
    b->launches = n > 0 ? (want_input_grads ? 5 : 4) * p.L + 1 : 0;
    return SBEV_OK;
}

}  // namespace

extern "C" int sbev_fpn_backward_plan(int n_levels, const int32_t* chw, int64_t n, int num_outs, int want_input_grads, int64_t* out) {
    const char* who = "sbev_fpn_backward_plan";
    SBEV_REQUIRE(out != nullptr, "%s: null out", who);
    BwdPlan b;
    if (int st = make_bwd_plan(who, n_levels, chw, n, num_outs, want_input_grads, &b)) return st;
    for (int i = 0; i < SBEV_FPN_BWD_PLAN_WORDS; ++i) out[i] = 0;
    out[0] = b.launches;
    out[1] = b.bytes;
    out[2] = b.f.pack_halves * 2;
    for (int l = 0; l < b.f.L; ++l) {
        out[3 + l] = n > 0 ? b.slabs[l] : 0;
        out[7 + l] = b.slab_len[l];
    }
    out[11] = b.gm_off;
    out[12] = b.d_off;
    out[13] = b.part_off;
    return SBEV_OK;
}

extern "C" int sbev_fpn_pack_weights_bwd(int n_levels, const int32_t* chw, const void* const* lateral_w, const void* const* fpn_w, int w_dtype,
                                         void* pack, sbev_stream_t stream) {
    const char* who = "sbev_fpn_pack_weights_bwd";
    Plan p;
    if (int st = make_plan(who, n_levels, chw, 0, n_levels, &p)) return st;
    SBEV_REQUIRE(w_dtype == SBEV_F32 || w_dtype == SBEV_F16, "%s: w_dtype %d (SBEV_F32 or SBEV_F16)", who, w_dtype);
    SBEV_REQUIRE(lateral_w != nullptr && fpn_w != nullptr && pack != nullptr, "%s: null pointer", who);
    for (int l = 0; l < p.L; ++l) SBEV_REQUIRE(lateral_w[l] != nullptr && fpn_w[l] != nullptr, "%s: level %d: null weight", who, l);
    SBEV_REQUIRE(aligned16(pack), "%s: 16-byte alignment", who);
    for (int i = 0; i < 2 * p.L; ++i) {
        const bool conv = i >= p.L;
        const int l = conv ? i - p.L : i;
        PackBwdArgs a;
        a.w = conv ? fpn_w[l] : lateral_w[l];
        a.Cin = conv ? kOut : p.Cin[l];
        a.f32 = w_dtype == SBEV_F32;
        a.conv = conv;
        a.frags = conv ? 9LL * (kOut / 16) * 8 * 64 : (long long)p.Cin[l] * 32;
        a.dst = reinterpret_cast<uint4*>(static_cast<_Float16*>(pack) + p.pack_off[conv ? kMaxIn + l : l]);
        hipLaunchKernelGGL(fpn_pack_bwd_kernel, dim3((unsigned)((a.frags + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    }
    return sbev::check_launch(who);
}

extern "C" int sbev_fpn_backward(int n_levels, const int32_t* chw, int64_t n, int num_outs, const void* const* inputs, int in_dtype,
                                 const void* merged, const void* const* grad_outs, int g_dtype, const void* pack_bwd, void* workspace,
                                 void* const* grad_inputs, float* const* grad_lateral_w, float* const* grad_lateral_bias,
                                 float* const* grad_fpn_w, float* const* grad_fpn_bias, sbev_stream_t stream) {
    const char* who = "sbev_fpn_backward";
    BwdPlan b;
    if (int st = make_bwd_plan(who, n_levels, chw, n, num_outs, grad_inputs != nullptr, &b)) return st;
    const Plan& p = b.f;
    SBEV_REQUIRE(in_dtype == SBEV_F32 || in_dtype == SBEV_F16, "%s: in_dtype %d (SBEV_F32 or SBEV_F16)", who, in_dtype);
    SBEV_REQUIRE(g_dtype == SBEV_F32 || g_dtype == SBEV_F16, "%s: g_dtype %d (SBEV_F32 or SBEV_F16)", who, g_dtype);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(inputs != nullptr && merged != nullptr && grad_outs != nullptr && pack_bwd != nullptr && workspace != nullptr &&
                     grad_lateral_w != nullptr && grad_lateral_bias != nullptr && grad_fpn_w != nullptr && grad_fpn_bias != nullptr,
                 "%s: null pointer", who);
    for (int l = 0; l < p.L; ++l)
        SBEV_REQUIRE(inputs[l] != nullptr && grad_lateral_w[l] != nullptr && grad_lateral_bias[l] != nullptr && grad_fpn_w[l] != nullptr &&
                         grad_fpn_bias[l] != nullptr, "%s: level %d: null pointer", who, l);
    for (int o = 0; o < num_outs; ++o) SBEV_REQUIRE(grad_outs[o] != nullptr, "%s: output gradient %d: null pointer", who, o);
    bool al = aligned16(pack_bwd) && aligned16(workspace) && aligned16(merged);
    for (int l = 0; l < p.L; ++l) {
        al = al && aligned16(inputs[l]) && (grad_inputs == nullptr || aligned16(grad_inputs[l]));
        al = al && ((reinterpret_cast<uintptr_t>(grad_lateral_w[l]) | reinterpret_cast<uintptr_t>(grad_lateral_bias[l]) |
                     reinterpret_cast<uintptr_t>(grad_fpn_w[l]) | reinterpret_cast<uintptr_t>(grad_fpn_bias[l])) & 3u) == 0;
    }
    for (int o = 0; o < num_outs; ++o) al = al && aligned16(grad_outs[o]);
    SBEV_REQUIRE(al, "%s: 16-byte alignment", who);

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const float* scale = reinterpret_cast<const float*>(ws);
    _Float16* gm = reinterpret_cast<_Float16*>(ws + b.gm_off);
    float* dbuf = reinterpret_cast<float*>(ws + b.d_off);
    float* part = reinterpret_cast<float*>(ws + b.part_off);
    const _Float16* wpack = static_cast<const _Float16*>(pack_bwd);
    const _Float16* m = static_cast<const _Float16*>(merged);
    const bool gf32 = g_dtype == SBEV_F32, xf32 = in_dtype == SBEV_F32;
    auto d_of = [&](int l) { return dbuf + (p.base[l] - p.base[1 < p.L ? 1 : 0]) * kOut; };

    {
        long long count[kMaxOut];
        for (int o = 0; o < num_outs; ++o)
            count[o] = o < p.L ? p.pixels[o] * kOut : (long long)n * p.eH[o - p.L + 1] * p.eW[o - p.L + 1] * kOut;
        if (int st = sbev::launch_grad_scale(who, grad_outs, count, num_outs, gf32, ws, s)) return st;
    }
    {
        DgradArgs c;
        long long end = 0;
        for (int l = 0; l < kMaxIn; ++l) {
            const int k = l < p.L ? l : p.L - 1;
            if (l < p.L) end += p.tiles[l];
            c.g[l] = grad_outs[k];
            c.wp[l] = reinterpret_cast<const uint4*>(wpack + p.pack_off[kMaxIn + k]);
            c.out[l] = k == 0 ? static_cast<void*>(gm) : static_cast<void*>(d_of(k));
            c.tile_end[l] = (int)end;
            c.pixels[l] = (int)p.pixels[k];
            c.H[l] = p.H[k]; c.W[l] = p.W[k];
        }
        for (int e = 0; e < kMaxOut; ++e) c.extra[e] = e >= 1 && e <= p.n_extra ? grad_outs[p.L - 1 + e] : nullptr;
        c.scale = scale;
        c.L = p.L; c.n_extra = p.n_extra;
        if (gf32) hipLaunchKernelGGL(fpn_dgrad3_kernel<true>, dim3((unsigned)p.conv_tiles), dim3(kThreads), 0, s, c);
        else hipLaunchKernelGGL(fpn_dgrad3_kernel<false>, dim3((unsigned)p.conv_tiles), dim3(kThreads), 0, s, c);
    }
    for (int l = 1; l < p.L; ++l) {
        AdjointArgs a;
        a.d = d_of(l);
        a.child = gm + p.base[l - 1] * kOut;
        a.gm = gm + p.base[l] * kOut;
        a.pixels = (int)p.pixels[l];
        a.pH = p.H[l]; a.pW = p.W[l]; a.H = p.H[l - 1]; a.W = p.W[l - 1];
        a.sy = (float)a.pH / (float)a.H;
        a.sx = (float)a.pW / (float)a.W;
        hipLaunchKernelGGL(fpn_adjoint_kernel, dim3((unsigned)((p.pixels[l] * 32 + 255) / 256)), dim3(256), 0, s, a);
    }
    for (int l = 0; l < p.L && grad_inputs != nullptr; ++l) {
        if (grad_inputs[l] == nullptr) continue;
        LatDgradArgs a;
        a.gm = gm + p.base[l] * kOut;
        a.wp = reinterpret_cast<const uint4*>(wpack + p.pack_off[l]);
        a.gc = grad_inputs[l];
        a.scale = scale;
        a.rows = (int)p.pixels[l]; a.Cin = p.Cin[l];
        const dim3 grid((unsigned)p.tiles[l], (unsigned)((p.Cin[l] / 32 + 7) / 8));
        if (xf32) hipLaunchKernelGGL(fpn_lat_dgrad_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(fpn_lat_dgrad_kernel<false>, grid, dim3(256), 0, s, a);
    }
    for (int l = 0; l < p.L; ++l) {
        WgradArgs w;
        for (int e = 0; e < kMaxOut; ++e) w.extra[e] = l == p.L - 1 && e >= 1 && e <= p.n_extra ? grad_outs[p.L - 1 + e] : nullptr;
        w.scale = scale;
        w.part = part;
        w.part_stride = b.part_stride[l];
        w.pixels = (int)p.pixels[l]; w.H = p.H[l]; w.W = p.W[l];
        w.slab_len = b.slab_len[l];
        // 3x3: A = G_l from gP_l, B = M_l
        w.a = grad_outs[l];
        w.b = m + p.base[l] * kOut;
        w.N = kOut;
        w.n_extra = l == p.L - 1 ? p.n_extra : 0;
        w.w_off = 0;
        w.bias_off = 9LL * kOut * kOut + (long long)kOut * p.Cin[l];
        const dim3 g3(36, (unsigned)b.slabs[l]);
        if (gf32) hipLaunchKernelGGL((fpn_wgrad_kernel<0, true>), g3, dim3(256), 0, s, w);
        else hipLaunchKernelGGL((fpn_wgrad_kernel<0, false>), g3, dim3(256), 0, s, w);
        // lateral: A = gM_l, B = C_l
        w.a = gm + p.base[l] * kOut;
        w.b = inputs[l];
        w.N = p.Cin[l];
        w.n_extra = 0;
        w.w_off = 9LL * kOut * kOut;
        w.bias_off += kOut;
        const dim3 g1((unsigned)(2 * ((p.Cin[l] + 127) / 128)), (unsigned)b.slabs[l]);
        if (xf32) hipLaunchKernelGGL((fpn_wgrad_kernel<1, true>), g1, dim3(256), 0, s, w);
        else hipLaunchKernelGGL((fpn_wgrad_kernel<1, false>), g1, dim3(256), 0, s, w);
        FoldArgs f;
        f.part = part;
        f.scale = scale;
        f.gw3 = grad_fpn_w[l]; f.gwlat = grad_lateral_w[l]; f.gc = grad_fpn_bias[l]; f.gblat = grad_lateral_bias[l];
        f.stride = b.part_stride[l];
        f.n_slabs = b.slabs[l]; f.Cin = p.Cin[l];
        hipLaunchKernelGGL(fpn_fold_kernel, dim3((unsigned)((b.part_stride[l] + 255) / 256)), dim3(256), 0, s, f);
    }
    return sbev::check_launch(who);
}
