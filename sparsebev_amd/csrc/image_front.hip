// The detector's image front end (models/sparsebev.py:61-100 with GridMask, pad_multiple and GpuPhotoMetricDistortion of
// models/utils.py) as ONE launch for all n = B * N images of a step: load (uint8 or fp32), photometric distortion, BGR -> RGB,
// normalise, zero pad to a multiple of the divisor, GridMask, store (fp32 or fp16).  Per pixel that is register work between a 1-byte
// read and a 4-byte (2-byte) write; the reference walks the fp32 tensor with a few dozen torch passes instead.
//
// Work split: a lane owns kPix = 16 consecutive pixels of one output row, in all three channels.  A workgroup owns kThreads
// consecutive (row, segment) items of ONE image, so the image's row of the parameter table (SBEV_FRONT_ROW_BYTES, layout in
// include/sbev_hip.h) is uniform: it is read with scalar loads, once.  The grid is n * ceil(Hp * ceil(Wp / 16) / kThreads) workgroups.
// The padding is written by the same lanes (zeros), so no memset precedes the launch and every output element is stored exactly once.
//
// Memory: per channel plane one 16-byte load (uint8) or four (fp32) per lane, and 16-byte stores, where the 16 pixels lie inside the
// row and their first byte is 16-byte aligned (decided per lane from the actual addresses: W is arbitrary, and with W % 16 != 0 only
// some rows start aligned); else element by element with the same bounds.  Offsets are 64-bit.
//
// Arithmetic: fp32, every operation individually rounded in the reference's order (the file is built with -ffp-contract=off; / is the
// correctly rounded division).  The channel flips (BGR -> RGB at the distortion's entry, RGB -> BGR at its exit, to_rgb) and the random
// channel permutation are not data movement: they decide which source plane a channel reads and which output plane it is stored to.
// No clamp anywhere, as in the reference: values leave [0, 255].
//
// GridMask (models/utils.py:15-46) keeps a pixel iff it lies on a row stripe or on a column stripe of the grid built on the PADDED size
// (the reference multiplies by 1 - mask).  Stripes do not overlap (l < d), so "row Y is on a stripe" is one division: with u = Y - st,
// u >= 0, u / d < hh / d (the stripe COUNT is bounded, not the extent) and u % d < l.  A lane does that once for its row and once for
// its first column, then steps the remainder along its 16 columns.
//
// Who writes what: an output element by the one lane that owns it; nothing else is written.
#include <hip/hip_fp16.h>

#include "sbev_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 16;                // pixels of one row per lane

enum { kBright = 1, kContrast = 2, kSat = 4, kHue = 8, kSwap = 16 };      // bits of Row::flags

struct Row {                   // SBEV_FRONT_ROW_BYTES per image
    int flags, mode;
    float delta, alpha, sat, hue;
    int perm[3];
    int mask_on, d, l, st_h, st_w;
    int pad[2];
};
static_assert(sizeof(Row) == SBEV_FRONT_ROW_BYTES, "the table row is part of the ABI");

struct Norm {
    float mean[3], stdv[3];
};

struct Args {
    const void* src;
    void* dst;
    const Row* table;          // null: no colour, no mask
    int n, H, W, Hp, Wp, segs, wgs_per_image;
    int to_rgb;
    Norm norm;
};

// torch.remainder for a positive divisor: fmod, then the divisor's sign.  fmod(a, b) is a itself for |a| < b, which is every value
// the chain produces from finite pixels; the library call is the rare path
__device__ __forceinline__ float rem_pos(float a, float b) {
    float r = fabsf(a) < b ? a : fmodf(a, b);
    if (r != 0.0f && r < 0.0f) r += b;
    return r;
}

__device__ __forceinline__ float pick3(int k, float a, float b, float c) { return k == 0 ? a : (k == 1 ? b : c); }

// one pixel through brightness .. contrast (mode 1): c[] in and out in the distortion's own channel order
__device__ __forceinline__ void distort(float (&c)[3], const Row& r) {
    if (r.flags & kBright) {
        c[0] += r.delta; c[1] += r.delta; c[2] += r.delta;
    }
    const bool contrast = (r.flags & kContrast) != 0;
    if (contrast && r.mode == 0) {
        c[0] *= r.alpha; c[1] *= r.alpha; c[2] *= r.alpha;
    }
    // rgb_to_hsv
    const float R = c[0] / 255.0f, G = c[1] / 255.0f, B = c[2] / 255.0f;
    float mx = R;
    int arg = 0;
    if (G > mx) { mx = G; arg = 1; }
    if (B > mx) { mx = B; arg = 2; }
    const float mn = fminf(fminf(R, G), B);
    float dc = mx - mn;
    float v = mx;
    float s = dc / (mx + 1e-8f);
    if (dc == 0.0f) dc = 1.0f;
    const float rc = mx - R, gc = mx - G, bc = mx - B;
    const float h1 = bc - gc;
    const float h2 = (rc - bc) + 2.0f * dc;
    const float h3 = (gc - rc) + 4.0f * dc;
    float h = pick3(arg, h1, h2, h3) / dc;
    h = rem_pos(h / 6.0f, 1.0f);
    h = h * 360.0f;
    v = v * 255.0f;
    if (r.flags & kSat) s *= r.sat;
    if (r.flags & kHue) h += r.hue;
    if (h > 360.0f) h -= 360.0f;
    if (h < 0.0f) h += 360.0f;
    // hsv_to_rgb
    const float hn = h / 360.0f;
    const float vn = v / 255.0f;
    const float h6 = hn * 6.0f;
    const float hi = rem_pos(floorf(h6), 6.0f);
    const float f = rem_pos(h6, 6.0f) - hi;
    const float p = vn * (1.0f - s);
    const float q = vn * (1.0f - f * s);
    const float t = vn * (1.0f - (1.0f - f) * s);
    const int k = (int)hi;
    float o0, o1, o2;
    switch (k) {
        case 0: o0 = vn; o1 = t; o2 = p; break;
        case 1: o0 = q; o1 = vn; o2 = p; break;
        case 2: o0 = p; o1 = vn; o2 = t; break;
        case 3: o0 = p; o1 = q; o2 = vn; break;
        case 4: o0 = t; o1 = p; o2 = vn; break;
        default: o0 = vn; o1 = p; o2 = q; break;
    }
    c[0] = o0 * 255.0f; c[1] = o1 * 255.0f; c[2] = o2 * 255.0f;
    if (contrast && r.mode == 1) {
        c[0] *= r.alpha; c[1] *= r.alpha; c[2] *= r.alpha;
    }
}

__device__ __forceinline__ float widen(unsigned char v) { return (float)v; }
__device__ __forceinline__ float widen(float v) { return v; }

template <typename T> struct Vec16;         // the 16-byte store of G = 16 / sizeof(T) consecutive outputs
template <> struct Vec16<float> {
    static constexpr int G = 4;
    static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    static __device__ __forceinline__ float cast(float v) { return v; }
};
template <> struct Vec16<__half> {
    static constexpr int G = 8;
    static __device__ __forceinline__ void store(__half* p, const __half* v) {
        union { __half h[8]; uint4 u; } w;
#pragma unroll
        for (int i = 0; i < 8; ++i) w.h[i] = v[i];
        *reinterpret_cast<uint4*>(p) = w.u;
    }
    static __device__ __forceinline__ __half cast(float v) { return __float2half_rn(v); }
};

// 16 pixels of one source plane -> floats; pixels outside [0, W) and rows outside [0, H) read nothing and give 0
template <typename In>
__device__ __forceinline__ void load16(const In* row, int x0, int W, bool row_valid, float (&out)[kPix]) {
#pragma unroll
    for (int j = 0; j < kPix; ++j) out[j] = 0.0f;
    if (!row_valid || x0 >= W) return;
    const In* p = row + x0;
    if (x0 + kPix <= W && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        if constexpr (sizeof(In) == 1) {
            const uint4 u = *reinterpret_cast<const uint4*>(p);
            const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int j = 0; j < kPix; ++j) out[j] = (float)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 f = reinterpret_cast<const float4*>(p)[q];
                out[4 * q] = f.x; out[4 * q + 1] = f.y; out[4 * q + 2] = f.z; out[4 * q + 3] = f.w;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPix; ++j)
            if (x0 + j < W) out[j] = widen(p[j]);
    }
}

template <typename In, typename Out, bool kColour>
__global__ __launch_bounds__(kThreads) void image_front_kernel(const Args a) {
    const int img = (int)(blockIdx.x / (unsigned)a.wgs_per_image);
    const int item = (int)(blockIdx.x % (unsigned)a.wgs_per_image) * kThreads + (int)threadIdx.x;
    const int y = item / a.segs;
    if (y >= a.Hp) return;
    const int x0 = (item - y * a.segs) * kPix;

    Row r{};
    if (a.table) r = a.table[img];                      // uniform: scalar loads

    // which source plane channel k of the chain reads, and which output plane result j is stored to
    int src_plane[3], dst_plane[3];
    if (kColour) {
        // the distortion works on RGB = planes (2, 1, 0); after it new[k] = o[P[k]], then RGB -> BGR, then to_rgb flips back:
        // output plane c holds new[to_rgb ? c : 2 - c]
#pragma unroll
        for (int k = 0; k < 3; ++k) src_plane[k] = 2 - k;
        dst_plane[0] = dst_plane[1] = dst_plane[2] = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = a.to_rgb ? c : 2 - c;
            const int j = (r.flags & kSwap) ? (k == 0 ? r.perm[0] : (k == 1 ? r.perm[1] : r.perm[2])) : k;
            if (j == 0) dst_plane[0] = c; else if (j == 1) dst_plane[1] = c; else if (j == 2) dst_plane[2] = c;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            src_plane[k] = k;
            dst_plane[k] = a.to_rgb ? 2 - k : k;
        }
    }

    // the mask: this lane's row, and the stepping state of its first column
    const bool masked = r.mask_on != 0 && r.d >= 1;
    bool row_on = false;
    int col_q = 0, col_rem = 0, col_u = 0, col_cnt = 0;
    if (masked) {
        const int hh = (int)(1.5 * (double)a.Hp), ww = (int)(1.5 * (double)a.Wp);
        const int u = y + (hh - a.Hp) / 2 - r.st_h;
        row_on = u >= 0 && u / r.d < hh / r.d && u % r.d < r.l;
        col_u = x0 + (ww - a.Wp) / 2 - r.st_w;
        col_cnt = ww / r.d;
        // floor division for a negative start: the remainder then steps up to 0 together with u
        col_q = col_u >= 0 ? col_u / r.d : -((-col_u + r.d - 1) / r.d);
        col_rem = col_u - col_q * r.d;
    }

    const bool row_valid = y < a.H;
    const long long plane_in = (long long)a.H * a.W, plane_out = (long long)a.Hp * a.Wp;
    const In* src = static_cast<const In*>(a.src) + (long long)img * 3 * plane_in + (long long)(row_valid ? y : 0) * a.W;
    Out* dst = static_cast<Out*>(a.dst) + (long long)img * 3 * plane_out + (long long)y * a.Wp + x0;

    float c[3][kPix];
#pragma unroll
    for (int k = 0; k < 3; ++k) load16<In>(src + src_plane[k] * plane_in, x0, a.W, row_valid, c[k]);

    float keep[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        float m = 1.0f;
        if (masked) {
            const bool col_on = col_u + j >= 0 && col_q < col_cnt && col_rem < r.l;
            m = (row_on || col_on) ? 1.0f : 0.0f;
            if (++col_rem == r.d) { col_rem = 0; ++col_q; }
        }
        keep[j] = m;
    }

#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        if (kColour) {
            float px[3] = {c[0][j], c[1][j], c[2][j]};
            distort(px, r);
            c[0][j] = px[0]; c[1][j] = px[1]; c[2][j] = px[2];
        }
    }

    constexpr int G = Vec16<Out>::G;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ch = dst_plane[k];
        if (ch < 0) continue;                           // a table row whose permutation is none: that result has no plane
        const float mean = pick3(ch, a.norm.mean[0], a.norm.mean[1], a.norm.mean[2]);
        const float stdv = pick3(ch, a.norm.stdv[0], a.norm.stdv[1], a.norm.stdv[2]);
        Out o[kPix];
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const float v = (row_valid && x0 + j < a.W) ? (c[k][j] - mean) / stdv : 0.0f;
            o[j] = Vec16<Out>::cast(v * keep[j]);
        }
        Out* p = dst + ch * plane_out;
        if (x0 + kPix <= a.Wp && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
#pragma unroll
            for (int g = 0; g < kPix / G; ++g) Vec16<Out>::store(p + g * G, o + g * G);
        } else {
#pragma unroll
            for (int j = 0; j < kPix; ++j)
                if (x0 + j < a.Wp) p[j] = o[j];
        }
    }
}

struct Plan {
    long long Hp, Wp, elems, table_bytes, grid;
    int segs, wgs_per_image;
};

int make_plan(int n, int H, int W, int div, Plan* p, const char* who) {
    SBEV_REQUIRE(n >= 1 && H >= 1 && W >= 1, "%s: n, H, W must be >= 1 (n=%d H=%d W=%d)", who, n, H, W);
    SBEV_REQUIRE(div >= 1, "%s: size divisor %d < 1", who, div);
    p->Hp = ((long long)H + div - 1) / div * div;
    p->Wp = ((long long)W + div - 1) / div * div;
    SBEV_REQUIRE(p->Hp <= 0x3fffffffLL && p->Wp <= 0x3fffffffLL, "%s: padded size %lld x %lld too large", who, p->Hp, p->Wp);
    const long long segs = (p->Wp + kPix - 1) / kPix;
    const long long wgs = (p->Hp * segs + kThreads - 1) / kThreads;
    SBEV_REQUIRE(wgs <= 0x7fffffffLL && wgs * n <= 0x7fffffffLL, "%s: %lld workgroups are too many for one launch", who, wgs * n);
    p->elems = (long long)n * 3 * p->Hp * p->Wp;
    p->table_bytes = (long long)n * SBEV_FRONT_ROW_BYTES;
    p->grid = wgs * n;
    p->segs = (int)segs;
    p->wgs_per_image = (int)wgs;
    return SBEV_OK;
}

template <typename In, typename Out>
void launch(const Args& a, bool colour, unsigned grid, hipStream_t s) {
    if (colour)
        hipLaunchKernelGGL((image_front_kernel<In, Out, true>), dim3(grid), dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL((image_front_kernel<In, Out, false>), dim3(grid), dim3(kThreads), 0, s, a);
}

}  // namespace

extern "C" int sbev_image_front_plan(int n, int H, int W, int div, int64_t* out) {
    SBEV_REQUIRE(out != nullptr, "sbev_image_front_plan: null out");
    Plan p;
    if (int st = make_plan(n, H, W, div, &p, "sbev_image_front_plan")) return st;
    out[0] = p.Hp;
    out[1] = p.Wp;
    out[2] = p.elems;
    out[3] = p.table_bytes;
    out[4] = p.grid;
    return SBEV_OK;
}

extern "C" int sbev_image_front(const void* src, int src_dtype, void* dst, int dst_dtype, int n, int H, int W, int div, const float* mean,
                                const float* std, int to_rgb, int colour_on, const void* table, sbev_stream_t stream) {
    SBEV_REQUIRE(src != nullptr && dst != nullptr && mean != nullptr && std != nullptr, "sbev_image_front: null pointer");
    Plan p;
    if (int st = make_plan(n, H, W, div, &p, "sbev_image_front")) return st;
    SBEV_REQUIRE(src_dtype == SBEV_U8 || src_dtype == SBEV_F32, "sbev_image_front: src_dtype %d (uint8 or fp32)", src_dtype);
    SBEV_REQUIRE(dst_dtype == SBEV_F32 || dst_dtype == SBEV_F16, "sbev_image_front: dst_dtype %d (fp32 or fp16)", dst_dtype);
    for (int c = 0; c < 3; ++c) SBEV_REQUIRE(std[c] != 0.0f, "sbev_image_front: std[%d] is 0", c);
    SBEV_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15u) == 0, "sbev_image_front: the table is not 16-byte aligned");
    SBEV_REQUIRE(table != nullptr || !colour_on, "sbev_image_front: colour_on needs a table");
    const uintptr_t in_align = src_dtype == SBEV_U8 ? 0u : 3u, out_align = dst_dtype == SBEV_F32 ? 3u : 1u;
    SBEV_REQUIRE((reinterpret_cast<uintptr_t>(src) & in_align) == 0 && (reinterpret_cast<uintptr_t>(dst) & out_align) == 0,
                 "sbev_image_front: src / dst not aligned to their element size");
    Args a;
    a.src = src;
    a.dst = dst;
    a.table = static_cast<const Row*>(table);
    a.n = n; a.H = H; a.W = W; a.Hp = (int)p.Hp; a.Wp = (int)p.Wp; a.segs = p.segs; a.wgs_per_image = p.wgs_per_image;
    a.to_rgb = to_rgb != 0;
    for (int c = 0; c < 3; ++c) {
        a.norm.mean[c] = mean[c];
        a.norm.stdv[c] = std[c];
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool colour = colour_on != 0;
    const unsigned grid = (unsigned)p.grid;
    if (src_dtype == SBEV_U8) {
        if (dst_dtype == SBEV_F32) launch<unsigned char, float>(a, colour, grid, s);
        else launch<unsigned char, __half>(a, colour, grid, s);
    } else {
        if (dst_dtype == SBEV_F32) launch<float, float>(a, colour, grid, s);
        else launch<float, __half>(a, colour, grid, s);
    }
    return sbev::check_launch("sbev_image_front");
}
