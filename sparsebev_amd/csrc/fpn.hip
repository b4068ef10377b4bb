// The FPN neck (mmdet's FPN forward: 1x1 laterals, top-down nearest upsample + add, 3x3 output convolutions, stride-2 extra levels) on
// v_mfma_f32_32x32x16_f16, reading the backbone's stage outputs channels-last and writing the decoder's channels-last pyramid.
// The forward (its backward: fpn_bwd.hip; the device helpers both share: fpn_common.hpp).  L + 1 launches for L input levels: one lateral + merge launch per level, coarsest first, then ONE launch for every
// output convolution of every level and image (the extra levels ride in its epilogue).
//
// Arithmetic (include/sbev_hip.h states it in full): operands fp16 (fp32 inputs rounded to nearest even on the way into LDS, weights
// when they are packed), products accumulated in fp32 on the matrix core, bias and parent added in fp32,
//   M_l = fp16(conv1x1(C_l) + b_l + float(M_{l+1}[nearest])),   P_l = conv3x3(M_l, pad 1) + b_l  (fp32, or fp16 by one rounding).
//
// Both kernels are one implicit GEMM: rows = pixels (all images of a level, 128 per workgroup), columns = the 256 output channels,
// K = taps x input channels, walked in chunks of KC channels of one tap.  8 waves: wave (wm, wn) owns rows 64 wm .. + 64 and channels
// 64 wn .. + 64 as 2 x 2 accumulators of 32 x 32.
//   (KC = 64; the lateral kernel has a KC = 32 form for channel counts that are no multiple of 64.)
//   A (pixels): thread t stages KC / 4 channels of row t / 4 -- global -> registers one chunk ahead of the MFMAs, registers -> LDS
//      (fp32 -> fp16 here) -- and the waves read their fragments back with 16-byte LDS reads (row pitch KC + 8 halves).  A row's source
//      pixel is fixed for the whole K loop; a tap outside the plane, or a row beyond the level, stages zeros: the halo never reads the
//      neighbouring row, image or level.
//   B (weights): packed once per weight version by sbev_fpn_pack_weights into fragment order, [tap][K / 16][8][64 lanes][8 halves]:
//      lane l of fragment nt holds channel co = 64 (nt / 2) + 2 (l & 31) + (nt & 1), k = 16 ks + 8 (l >> 5) + j.  A wave reads its two
//      fragments straight from global memory (16 bytes per lane, consecutive across the wave).  Interleaving the channels of a wave's
//      two column blocks puts channels c, c + 1 of one pixel into one lane: the epilogue stores 4 (fp16) or 8 (fp32) bytes per lane,
//      128 / 256 consecutive bytes per half wave.
// A workgroup never spans levels (each level has its own weights); it spans rows and images freely.  The convolution launch finds its
// level from the cumulative tile counts in its argument block (the tile table: at most 4 entries, wave-uniform).
//
// Who writes what: every element of M_l and of every output is stored by the one lane that owns it; nothing is read-modify-written.
#include "fpn_common.hpp"

namespace {

using namespace sbev_fpn;

// ---------------------------------------------------------------- lateral + merge: one level, all images
struct LatArgs {
    const void* x;            // [rows, Cin] fp16 or fp32
    const uint4* wp;          // packed 1x1 weights
    const float* bias;        // [256]
    const _Float16* parent;   // M_{l+1} [n, pH, pW, 256] or null
    _Float16* m;              // M_l [rows, 256]
    int rows, Cin, H, W, pH, pW;
    float sy, sx;             // float32(pH / H), float32(pW / W)
};

template <bool F32, int KC>
__global__ __launch_bounds__(kThreads) void fpn_lateral_kernel(const LatArgs a) {
    constexpr int pitch = KC + 8;
    __shared__ __attribute__((aligned(16))) _Float16 tile[kTileM * pitch];
    __shared__ int prow[kTileM];          // the parent's pixel of each row (-1: a row beyond the level)

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int srow = tid >> 2, q = tid & 3;
    const long long r = (long long)blockIdx.x * kTileM + srow;
    const bool valid = r < a.rows;
    if (q == 0) {
        int p = -1;
        if (valid) {
            p = 0;
            if (a.parent != nullptr) {
                const int plane = a.H * a.W;
                const int img = (int)(r / plane), rem = (int)(r % plane);
                const int y = rem / a.W, x = rem % a.W;
                p = (img * a.pH + nearest_src(y, a.sy, a.pH)) * a.pW + nearest_src(x, a.sx, a.pW);
            }
        }
        prow[srow] = p;
    }
    const size_t esize = F32 ? 4 : 2;
    const char* src = static_cast<const char*>(a.x) + ((size_t)(valid ? r : 0) * a.Cin + q * (KC / 4)) * esize;
    _Float16* dst = tile + srow * pitch + q * (KC / 4);

    f32x16 acc[2][2];
    zero_acc(acc);
    const int nchunks = a.Cin / KC;
    Raw<KC, F32> raw;
    load_raw<KC, F32>(raw, src, valid);
    for (int c = 0; c < nchunks; ++c) {
        store_raw<KC, F32>(raw, dst);
        __syncthreads();
        if (c + 1 < nchunks) load_raw<KC, F32>(raw, src + (size_t)(c + 1) * KC * esize, valid);
        mma_chunk<KC>(acc, tile, a.wp, c * (KC / 16), wm, wn, lane);
        __syncthreads();
    }

    const int c0 = 64 * wn + 2 * (lane & 31);
    const float b0 = a.bias[c0], b1 = a.bias[c0 + 1];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int row = acc_row(wm, mb, rr, lane);
            const int p = prow[row];
            if (p < 0) continue;
            float v0 = acc[mb][0][rr] + b0, v1 = acc[mb][1][rr] + b1;
            if (a.parent != nullptr) {
                const f16x2 pv = *reinterpret_cast<const f16x2*>(a.parent + (size_t)p * kOut + c0);
                v0 += (float)pv.x;
                v1 += (float)pv.y;
            }
            const size_t o = ((size_t)blockIdx.x * kTileM + row) * kOut + c0;
            *reinterpret_cast<unsigned*>(a.m + o) = pack_h2(v0, v1);
        }
    }
}

// ---------------------------------------------------------------- output convolutions: every level and image in one launch
struct ConvArgs {
    const _Float16* m;                  // the merged laterals, level after level: [total pixels, 256]
    const uint4* wp[kMaxIn];            // packed 3x3 weights per level
    const float* bias[kMaxIn];
    void* out[kMaxIn];                  // [n, H, W, 256] per level
    void* extra[kMaxOut];               // extra level e (1 ..): rows 0, 2^e, .. and columns likewise of the last level's output
    int tile_end[kMaxIn];               // cumulative tiles: level l owns workgroups [tile_end[l - 1], tile_end[l])
    int base[kMaxIn];                   // first pixel of level l in m
    int pixels[kMaxIn];                 // n * H * W
    int H[kMaxIn], W[kMaxIn];
    int L, n_extra, out_f32;
};

__global__ __launch_bounds__(kThreads) void fpn_conv_kernel(const ConvArgs a) {
    constexpr int KC = 64, pitch = KC + 8, kPerTap = kOut / KC;
    __shared__ __attribute__((aligned(16))) _Float16 tile[kTileM * pitch];
    __shared__ int rpix[kTileM];          // the row's pixel inside its level (-1: beyond the level)
    __shared__ int ryx[kTileM];           // y << 16 | x (the plan bounds a side by 32767) and the image: read where extra levels exist
    __shared__ int rimg[kTileM];

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

    const long long p = (long long)((int)blockIdx.x - tile0) * kTileM + srow;
    const bool valid = p < npix;
    const int plane = H * W;
    const int img = valid ? (int)(p / plane) : 0, rem = valid ? (int)(p % plane) : 0;
    const int y = rem / W, x = rem % W;
    if (q == 0) {
        rpix[srow] = valid ? (int)p : -1;
        ryx[srow] = (y << 16) | x;
        rimg[srow] = img;
    }
    const _Float16* src = a.m + ((size_t)a.base[level] + (size_t)(valid ? p : 0)) * kOut + q * (KC / 4);
    _Float16* dst = tile + srow * pitch + q * (KC / 4);

    f32x16 acc[2][2];
    zero_acc(acc);
    constexpr int nchunks = 9 * kPerTap;
    Raw<KC, false> raw;
    // chunk c: tap c / kPerTap = (ky, kx), channels KC (c % kPerTap) ..; the tap reads pixel (y + ky - 1, x + kx - 1) of the same image
    auto fetch = [&](int c) {
        const int tap = c / kPerTap, kc = c % kPerTap;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const bool in = valid && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
        load_raw<KC, false>(raw, src + ((long long)dy * W + dx) * kOut + kc * KC, in);
    };
    fetch(0);
    for (int c = 0; c < nchunks; ++c) {
        store_raw<KC, false>(raw, dst);
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1);
        mma_chunk<KC>(acc, tile, wp, c * (KC / 16), wm, wn, lane);
        __syncthreads();
    }

    const int c0 = 64 * wn + 2 * (lane & 31);
    const float* bias = a.bias[level];
    const float b0 = bias[c0], b1 = bias[c0 + 1];
    void* out = a.out[level];
    const int n_extra = level == a.L - 1 ? a.n_extra : 0;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int row = acc_row(wm, mb, rr, lane);
            const int px = rpix[row];
            if (px < 0) continue;
            const float v0 = acc[mb][0][rr] + b0, v1 = acc[mb][1][rr] + b1;
            store_pair(out, (size_t)px * kOut + c0, v0, v1, a.out_f32);
            if (n_extra > 0) {
                const int yx = ryx[row], ry = yx >> 16, rx = yx & 0xffff, ri = rimg[row];
#pragma unroll
                for (int e = 1; e < kMaxOut; ++e) {
                    if (e <= n_extra && ((ry | rx) & ((1 << e) - 1)) == 0) {
                        const int He = (H + (1 << e) - 1) >> e, We = (W + (1 << e) - 1) >> e;
                        const size_t o = (((size_t)ri * He + (ry >> e)) * We + (rx >> e)) * kOut + c0;
                        store_pair(a.extra[e], o, v0, v1, a.out_f32);
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------- weights -> fragment order, fp16
struct PackArgs {
    const void* w;            // [256, Cin, kh, kw] contiguous, fp32 or fp16
    uint4* dst;
    int Cin, taps, f32;
    long long frags;          // taps * (Cin / 16) * 8 * 64
};

__global__ __launch_bounds__(256) void fpn_pack_kernel(const PackArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.frags) return;
    const int lane = (int)(i & 63), nt = (int)((i >> 6) & 7);
    const long long rest = i >> 9;
    const int KS = a.Cin / 16;
    const int ks = (int)(rest % KS), tap = (int)(rest / KS);
    const int co = 64 * (nt >> 1) + 2 * (lane & 31) + (nt & 1);
    const int k0 = 16 * ks + 8 * (lane >> 5);
    unsigned h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const size_t e = ((size_t)co * a.Cin + k0 + 2 * j + t) * a.taps + tap;
            v[t] = a.f32 ? static_cast<const float*>(a.w)[e] : (float)static_cast<const _Float16*>(a.w)[e];
        }
        h[j] = pack_h2(v[0], v[1]);
    }
    a.dst[i] = make_uint4(h[0], h[1], h[2], h[3]);
}

}  // namespace

extern "C" int sbev_fpn_plan(int n_levels, const int32_t* chw, int64_t n, int num_outs, int64_t* out) {
    const char* who = "sbev_fpn_plan";
    SBEV_REQUIRE(out != nullptr, "%s: null out", who);
    Plan p;
    if (int st = make_plan(who, n_levels, chw, n, num_outs, &p)) return st;
    for (int i = 0; i < SBEV_FPN_PLAN_WORDS; ++i) out[i] = 0;
    out[0] = n > 0 ? p.L + 1 : 0;
    out[1] = p.pack_halves * 2;
    out[2] = p.total * kOut * 2;
    out[3] = p.total;
    out[4] = p.conv_tiles;
    for (int l = 0; l < p.L; ++l) out[5 + l] = p.tiles[l];
    out[9] = p.n_extra;
    for (int e = 1; e <= p.n_extra; ++e) {
        out[10 + 2 * (e - 1)] = p.eH[e];
        out[11 + 2 * (e - 1)] = p.eW[e];
    }
    return SBEV_OK;
}

extern "C" int sbev_fpn_pack_weights(int n_levels, const int32_t* chw, const void* const* lateral_w, const void* const* fpn_w, int w_dtype,
                                     void* pack, sbev_stream_t stream) {
    const char* who = "sbev_fpn_pack_weights";
    Plan p;
    if (int st = make_plan(who, n_levels, chw, 0, n_levels, &p)) return st;
    SBEV_REQUIRE(w_dtype == SBEV_F32 || w_dtype == SBEV_F16, "%s: w_dtype %d (SBEV_F32 or SBEV_F16)", who, w_dtype);
    SBEV_REQUIRE(lateral_w != nullptr && fpn_w != nullptr && pack != nullptr, "%s: null pointer", who);
    for (int l = 0; l < p.L; ++l) SBEV_REQUIRE(lateral_w[l] != nullptr && fpn_w[l] != nullptr, "%s: level %d: null weight", who, l);
    SBEV_REQUIRE(aligned16(pack), "%s: 16-byte alignment", who);
    for (int i = 0; i < 2 * p.L; ++i) {
        const bool conv = i >= p.L;
        const int l = conv ? i - p.L : i;
        PackArgs a;
        a.w = conv ? fpn_w[l] : lateral_w[l];
        a.Cin = conv ? kOut : p.Cin[l];
        a.taps = conv ? 9 : 1;
        a.f32 = w_dtype == SBEV_F32;
        a.frags = (long long)a.taps * (a.Cin / 16) * 8 * 64;
        a.dst = reinterpret_cast<uint4*>(static_cast<_Float16*>(pack) + p.pack_off[conv ? kMaxIn + l : l]);
        hipLaunchKernelGGL(fpn_pack_kernel, dim3((unsigned)((a.frags + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    }
    return sbev::check_launch(who);
}

extern "C" int sbev_fpn_forward(int n_levels, const int32_t* chw, int64_t n, int num_outs, const void* const* inputs, int in_dtype,
                                const void* pack, const float* const* lateral_bias, const float* const* fpn_bias, void* workspace,
                                void* const* outs, int out_dtype, sbev_stream_t stream) {
    const char* who = "sbev_fpn_forward";
    Plan p;
    if (int st = make_plan(who, n_levels, chw, n, num_outs, &p)) return st;
    SBEV_REQUIRE(in_dtype == SBEV_F32 || in_dtype == SBEV_F16, "%s: in_dtype %d (SBEV_F32 or SBEV_F16)", who, in_dtype);
    SBEV_REQUIRE(out_dtype == SBEV_F32 || out_dtype == SBEV_F16, "%s: out_dtype %d (SBEV_F32 or SBEV_F16)", who, out_dtype);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(inputs != nullptr && pack != nullptr && lateral_bias != nullptr && fpn_bias != nullptr && workspace != nullptr && outs != nullptr,
                 "%s: null pointer", who);
    for (int l = 0; l < p.L; ++l)
        SBEV_REQUIRE(inputs[l] != nullptr && lateral_bias[l] != nullptr && fpn_bias[l] != nullptr, "%s: level %d: null pointer", who, l);
    for (int o = 0; o < num_outs; ++o) SBEV_REQUIRE(outs[o] != nullptr, "%s: output %d: null pointer", who, o);
    bool al = aligned16(pack) && aligned16(workspace);
    for (int l = 0; l < p.L; ++l) al = al && aligned16(inputs[l]) && (reinterpret_cast<uintptr_t>(lateral_bias[l]) & 3u) == 0 &&
                                       (reinterpret_cast<uintptr_t>(fpn_bias[l]) & 3u) == 0;
    for (int o = 0; o < num_outs; ++o) al = al && aligned16(outs[o]);
    SBEV_REQUIRE(al, "%s: 16-byte alignment", who);

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const _Float16* wpack = static_cast<const _Float16*>(pack);
    _Float16* m = static_cast<_Float16*>(workspace);
    for (int l = p.L - 1; l >= 0; --l) {
        LatArgs a;
        a.x = inputs[l];
        a.wp = reinterpret_cast<const uint4*>(wpack + p.pack_off[l]);
        a.bias = lateral_bias[l];
        a.m = m + p.base[l] * kOut;
        a.rows = (int)p.pixels[l]; a.Cin = p.Cin[l]; a.H = p.H[l]; a.W = p.W[l];
        a.parent = nullptr; a.pH = a.pW = 1; a.sy = a.sx = 1.f;
        if (l + 1 < p.L) {
            a.parent = m + p.base[l + 1] * kOut;
            a.pH = p.H[l + 1]; a.pW = p.W[l + 1];
            a.sy = (float)a.pH / (float)a.H;
            a.sx = (float)a.pW / (float)a.W;
        }
        const dim3 grid((unsigned)p.tiles[l]), block(kThreads);
        const bool f32 = in_dtype == SBEV_F32;
        if (a.Cin % 64 == 0) {          // chunks of 64 channels where the level allows: half the barriers
            if (f32) hipLaunchKernelGGL((fpn_lateral_kernel<true, 64>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fpn_lateral_kernel<false, 64>), grid, block, 0, s, a);
        } else {
            if (f32) hipLaunchKernelGGL((fpn_lateral_kernel<true, 32>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((fpn_lateral_kernel<false, 32>), grid, block, 0, s, a);
        }
    }
    ConvArgs c;
    c.m = m;
    long long end = 0;
    for (int l = 0; l < kMaxIn; ++l) {
        const int k = l < p.L ? l : p.L - 1;
        if (l < p.L) end += p.tiles[l];
        c.wp[l] = reinterpret_cast<const uint4*>(wpack + p.pack_off[kMaxIn + k]);
        c.bias[l] = fpn_bias[k];
        c.out[l] = outs[k];
        c.tile_end[l] = (int)end;
        c.base[l] = (int)p.base[k];
        c.pixels[l] = (int)p.pixels[k];
        c.H[l] = p.H[k]; c.W[l] = p.W[k];
    }
    for (int e = 0; e < kMaxOut; ++e) c.extra[e] = e >= 1 && e <= p.n_extra ? outs[p.L - 1 + e] : nullptr;
    c.L = p.L; c.n_extra = p.n_extra; c.out_f32 = out_dtype == SBEV_F32;
    hipLaunchKernelGGL(fpn_conv_kernel, dim3((unsigned)p.conv_tiles), dim3(kThreads), 0, s, c);
    return sbev::check_launch(who);
}
