// What the FPN neck's forward (fpn.hip) and backward (fpn_bwd.hip) share: the staging of a pixel-major A operand through LDS, the
// 2 x 2 MFMA step of an 8-wave workgroup over a fragment-ordered weight image, the accumulator's row map, the nearest rule, and the
// host plan of the levels -- and what the neck's and the backbone's backward (resnet_bwd.hip) share beyond that: the slab rule of the
// weight gradients and their transposed LDS operand read.  Everything is internal to a translation unit (static / inline): the kernels
// of each file stay its own.
#pragma once
#include <algorithm>
#include <cmath>

#include "sbev_common.hpp"

namespace sbev_fpn {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 512;
constexpr int kTileM = 128;
constexpr int kOut = 256;               // out_channels
constexpr int kMaxIn = SBEV_FPN_MAX_IN;
constexpr int kMaxOut = SBEV_FPN_MAX_OUT;

// ---------------------------------------------------------------- staging of the A operand
template <int KC, bool F32>
struct Raw {
    uint4 v[F32 ? KC / 16 : KC / 32];
};

template <int KC, bool F32>
__device__ __forceinline__ void load_raw(Raw<KC, F32>& r, const void* p, bool valid) {
    constexpr int n = F32 ? KC / 16 : KC / 32;
#pragma unroll
    for (int i = 0; i < n; ++i) r.v[i] = make_uint4(0u, 0u, 0u, 0u);
    if (valid) {
        const uint4* q = static_cast<const uint4*>(p);
#pragma unroll
        for (int i = 0; i < n; ++i) r.v[i] = q[i];
    }
}

__device__ __forceinline__ unsigned pack_h2(float a, float b) {
    f16x2 h;
    h.x = (_Float16)a;
    h.y = (_Float16)b;
    return __builtin_bit_cast(unsigned, h);
}

template <int KC, bool F32>
__device__ __forceinline__ void store_raw(const Raw<KC, F32>& r, _Float16* lds) {
    uint4* d = reinterpret_cast<uint4*>(lds);
    if constexpr (F32) {
#pragma unroll
        for (int i = 0; i < KC / 32; ++i) {
            const uint4 a = r.v[2 * i], b = r.v[2 * i + 1];
            d[i] = make_uint4(pack_h2(__uint_as_float(a.x), __uint_as_float(a.y)), pack_h2(__uint_as_float(a.z), __uint_as_float(a.w)),
                              pack_h2(__uint_as_float(b.x), __uint_as_float(b.y)), pack_h2(__uint_as_float(b.z), __uint_as_float(b.w)));
        }
    } else {
#pragma unroll
        for (int i = 0; i < KC / 32; ++i) d[i] = r.v[i];
    }
}

// one chunk of KC reduction indices: 2 x 2 accumulators per wave, KC / 16 MFMA steps
template <int KC>
__device__ __forceinline__ void mma_chunk(f32x16 (&acc)[2][2], const _Float16* lds, const uint4* wp, int ks0, int wm, int wn, int lane) {
    constexpr int pitch = KC + 8;
    const _Float16* arow = lds + (64 * wm + (lane & 31)) * pitch + 8 * (lane >> 5);
    const uint4* bw = wp + ((size_t)ks0 * 8 + 2 * wn) * 64 + lane;
#pragma unroll
    for (int kk = 0; kk < KC / 16; ++kk) {
        const uint4 b0 = bw[(size_t)kk * 8 * 64], b1 = bw[(size_t)kk * 8 * 64 + 64];
        const uint4 a0 = *reinterpret_cast<const uint4*>(arow + 16 * kk);
        const uint4 a1 = *reinterpret_cast<const uint4*>(arow + 32 * pitch + 16 * kk);
        const f16x8 fa0 = __builtin_bit_cast(f16x8, a0), fa1 = __builtin_bit_cast(f16x8, a1);
        const f16x8 fb0 = __builtin_bit_cast(f16x8, b0), fb1 = __builtin_bit_cast(f16x8, b1);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// row of accumulator register r of row block mb inside the workgroup's 128 rows
__device__ __forceinline__ int acc_row(int wm, int mb, int r, int lane) { return 64 * wm + 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// F.interpolate(mode='nearest'): min(floor(dst * float32(in / out)), in - 1), the product rounded once in fp32
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) { return min((int)floorf((float)dst * scale), in_size - 1); }

__device__ __forceinline__ void store_pair(void* base, size_t elem, float v0, float v1, int out_f32) {
    if (out_f32)
        *reinterpret_cast<float2*>(static_cast<float*>(base) + elem) = make_float2(v0, v1);
    else
        *reinterpret_cast<unsigned*>(static_cast<_Float16*>(base) + elem) = pack_h2(v0, v1);
}

// ---------------------------------------------------------------- the plan (pure host)
struct Plan {
    int L, n_extra;
    int Cin[kMaxIn], H[kMaxIn], W[kMaxIn];
    long long pixels[kMaxIn], base[kMaxIn], tiles[kMaxIn], pack_off[2 * kMaxIn];      // pack offsets in halves: laterals, then convolutions
    long long total, conv_tiles, pack_halves;
    int eH[kMaxOut], eW[kMaxOut];          // extra level e = 1 ..
};

inline int make_plan(const char* who, int n_levels, const int32_t* chw, int64_t n, int num_outs, Plan* p) {
    SBEV_REQUIRE(chw != nullptr, "%s: null level list", who);
    SBEV_REQUIRE(n_levels >= 1 && n_levels <= kMaxIn, "%s: %d input levels (1 .. %d are built)", who, n_levels, kMaxIn);
    SBEV_REQUIRE(num_outs >= n_levels && num_outs <= kMaxOut, "%s: num_outs=%d not in %d .. %d (add_extra_convs is not built)", who, num_outs,
                 n_levels, kMaxOut);
    SBEV_REQUIRE(n >= 0 && n <= (1LL << 32), "%s: n=%lld images", who, (long long)n);
    p->L = n_levels;
    p->n_extra = num_outs - n_levels;
    p->total = 0;
    p->conv_tiles = 0;
    long long halves = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int C = chw[3 * l], H = chw[3 * l + 1], W = chw[3 * l + 2];
        SBEV_REQUIRE(C >= 32 && C % 32 == 0 && C <= 65536, "%s: level %d has %d input channels (a multiple of 32, at most 65536)", who, l, C);
        SBEV_REQUIRE(H >= 1 && W >= 1, "%s: level %d has an empty plane (%d x %d)", who, l, H, W);
        SBEV_REQUIRE(H <= 32767 && W <= 32767, "%s: level %d plane %d x %d: a side above 32767", who, l, H, W);
        p->Cin[l] = C; p->H[l] = H; p->W[l] = W;
        p->pixels[l] = (long long)n * H * W;
        p->base[l] = p->total;
        p->total += p->pixels[l];
        SBEV_REQUIRE(p->total <= 0x7fffffffLL - kTileM, "%s: %lld pixels: pixel indices are 32-bit", who, p->total);
        p->tiles[l] = (p->pixels[l] + kTileM - 1) / kTileM;
        p->conv_tiles += p->tiles[l];
        p->pack_off[l] = halves;
        halves += (long long)C * kOut;
    }
    for (int l = 0; l < n_levels; ++l) {
        p->pack_off[kMaxIn + l] = halves;
        halves += 9LL * kOut * kOut;
    }
    p->pack_halves = halves;
    for (int e = 1; e < kMaxOut; ++e) {
        p->eH[e] = (p->H[n_levels - 1] + (1 << e) - 1) >> e;
        p->eW[e] = (p->W[n_levels - 1] + (1 << e) - 1) >> e;
    }
    return SBEV_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline long long round_up(long long v, long long m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------- weight gradients (fpn_bwd.hip, resnet_bwd.hip): slabs and operand tiles
// The reduction over a convolution's output pixels is split into slabs (grid.y), one fp32 partial per slab, folded in slab order:
// slab_len = max(kMinSlab, ceil(pixels / kMaxSlabs) rounded up to kSlabRound) -- part of both backward passes' definition
// (include/sbev_hip.h: sbev_fpn_backward_plan, sbev_resnet_backward).
constexpr int kMaxSlabs = 16;            // slabs per level / layer at most
constexpr int kMinSlab = 512;            // pixels per slab at least
constexpr int kSlabRound = 256;          // a slab length is a multiple of this

inline void slab_rule(long long pixels, int* slabs, int* slab_len) {
    const long long len = std::max<long long>(kMinSlab, round_up((pixels + kMaxSlabs - 1) / kMaxSlabs, kSlabRound));
    *slab_len = (int)len;
    *slabs = (int)((pixels + len - 1) / len);
}

constexpr int kWK = 32;                  // pixels per K step of the weight gradients
constexpr int kWPitch = 160;             // halves per LDS row of a weight-gradient operand tile: 128 + 32

typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));

// operand of v_mfma_f32_32x32x16_f16 from a [pixel][channel] LDS tile: lane (fr, fh) gets channel col0 + fr, pixels k0 + 8 fh .. + 8.
// Two transposed reads of 4 pixels x 16 channels per 16-lane group; lane 4 q + pp of a group addresses pixel q, channels 4 pp .. + 4.
__device__ __forceinline__ f16x8 tr_frag(const _Float16* tile, int k0, int col0, int lane) {
    const int grp = lane >> 4, idx = lane & 15;
    const _Float16* p = tile + (k0 + 8 * (grp >> 1) + (idx >> 2)) * kWPitch + col0 + 16 * (grp & 1) + 4 * (idx & 3);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * kWPitch));
    typedef short s16x8 __attribute__((__vector_size__(8 * sizeof(short))));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(f16x8, v);
}

}  // namespace sbev_fpn
