// The loader's image geometry (RandomTransformImage of loaders/pipelines/transforms.py: PIL resize with the bicubic, antialiased
// 8-bit resampler, crop with black fill, mirror, and the format bundle's HWC -> CHW) as ONE launch for all n images of a step:
// uint8 [n, H, W, 3] decoded frames in, uint8 [n, 3, fH, fW] out -- what sbev_image_front accepts.  Bit for bit what Pillow gives.
//
// Pillow's 8-bit resampler is integer arithmetic: per axis, coefficients computed in double, normalised and rounded to 22 fractional
// bits; a pass accumulates pixel * coefficient in int from 1 << 21, shifts right by 22 and clamps to 0 .. 255; the horizontal pass's
// result is stored as uint8 before the vertical pass reads it.  The kernel does exactly that with 32-bit integers (|sum| stays below
// 255 * 1.4 * 2^22 < 2^31; a coefficient fits 24 signed bits, which the plan checks, so the 24-bit multiply-add is exact).  No floating
// point in the kernel: the coefficients come from sbev_image_geom_plan, a host function, in a device table.
//
// Tables (layout in include/sbev_hip.h): one transform block per sample -- header, (first, count) per kept output column and row,
// int32 coefficients [fW, KMAX] and [fH, KMAX] -- and an int32 row that maps each image to its block.  Column j of the table is
// resized column crop_x + j; output pixel x reads j = fW - 1 - x if mirrored.  An index outside the resized image has count 0: both
// passes then give (1 << 21) >> 22 = 0, which is the crop's black fill, without a branch.
//
// Work split: a workgroup (4 waves) owns one kTileH x kTileW tile of table rows / columns of one image.
//   1. span: the source columns [c0, c1) and rows [r0, r1) its taps touch (LDS min / max over the tile's bounds);
//   2. per chunk of kChunk source rows: wave w stages rows w, w + 4, .. of [c0, c1) into LDS with aligned 4-byte loads (the tail of
//      the whole buffer byte by byte), then lane = column runs the horizontal pass over those rows, its 16 coefficients in registers,
//      and stores the uint8 results to the LDS plane mid[row][channel][column];
//   3. the vertical pass: wave w owns tile rows w, w + 4, ..: the row's bounds and coefficients are wave-uniform (fetched into LDS in
//      the prologue, one per thread, and read back as broadcasts), the taps are consecutive LDS bytes across lanes; one byte store per
//      lane and channel, 64 consecutive bytes per wave.
// Only the source rows and columns the crop's taps read are loaded, and no intermediate image goes to global memory.
//
// Capacity: KMAX = 16 taps bound the scale of an axis by 3.5 (ksize = 2 * ceil(2 * scale) + 1), so a tile's span is at most
// (kTileW - 1) * 3.5 + 17 < kSpanW columns and (kTileH - 1) * 3.5 + 17 < kSpanH rows; the plan checks the actual spans.  The kernel
// trusts no table entry with an address: a bound outside the source, a count above KMAX or a tap outside the staged span reads as
// "no taps" (zero), and a block index outside [0, n_transforms) is clamped.
//
// Who writes what: an output byte by the one lane that owns it; every output byte is stored.
#include <cmath>
#include <vector>

#include "sbev_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / sbev::kWave;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kMax = SBEV_GEOM_KMAX;
constexpr int kSpanW = 240;                          // source columns of one tile, at most
constexpr int kSpanH = 72;                           // source rows of one tile, at most
constexpr int kChunk = 16;                           // source rows staged at a time
constexpr int kRowBytes = kSpanW * 3 + 8;            // staged row: up to 3 bytes of misalignment in front, whole dwords
constexpr int kStagePad = 16;                        // dwords behind the last staged row: the uniform tap loop reads up to 13 past a lane's first
constexpr int kBits = 22;
static_assert(kTileW == sbev::kWave && kTileH * kMax == kThreads, "lane = column; one vertical coefficient per thread");
static_assert(kRowBytes % 4 == 0 && kChunk % kWaves == 0 && kTileH % kWaves == 0, "whole dwords, whole rounds");
static_assert((kTileW - 1) * 7 / 2 + kMax + 1 < kSpanW && (kTileH - 1) * 7 / 2 + kMax + 1 < kSpanH, "KMAX taps bound the span");

enum { kNewW = 0, kNewH, kCropX, kCropY, kFlip, kKsX, kKsY, kHeader = 8 };          // header words of a block

struct Layout {             // int32 word offsets inside a block
    long long xb, yb, xk, yk, words;
};
Layout __host__ __device__ inline layout(int fH, int fW) {
    Layout l;
    l.xb = kHeader;
    l.yb = l.xb + 2LL * fW;
    l.xk = (l.yb + 2LL * fH + 3) / 4 * 4;          // 16-byte aligned: a column's coefficients are four 16-byte loads
    l.yk = l.xk + (long long)kMax * fW;
    l.words = (l.yk + (long long)kMax * fH + 3) / 4 * 4;
    return l;
}

struct Args {
    const unsigned char* src;
    unsigned char* dst;
    const int* table;
    const int* image_rows;
    int n, H, W, fH, fW, n_transforms, tiles_x, tiles_y;
};

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kBits, 0), 255); }

__global__ __launch_bounds__(kThreads) void image_geom_kernel(const Args a) {
    __shared__ unsigned int stage[kChunk * kRowBytes / 4 + kStagePad];
    __shared__ unsigned char mid[kSpanH * 3 * kTileW];
    __shared__ int kyl[kTileH * kMax];                    // the tile rows' coefficients
    __shared__ int ybl[kTileH * 2];                       // and bounds (made safe)
    __shared__ int span[5];                               // c0, c1, r0, r1, the most taps of a column

    const int tiles = a.tiles_x * a.tiles_y;
    const int img = (int)(blockIdx.x / (unsigned)tiles);
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const int j0 = (tile % a.tiles_x) * kTileW, i0 = (tile / a.tiles_x) * kTileH;
    const int lane = (int)threadIdx.x & (sbev::kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / sbev::kWave);

    const Layout lay = layout(a.fH, a.fW);
    int block = a.image_rows[img];
    block = min(max(block, 0), a.n_transforms - 1);
    const int* tb = a.table + (long long)block * lay.words;
    const int flip = tb[kFlip];

    if (threadIdx.x == 0) {
        span[0] = 0x7fffffff; span[1] = 0; span[2] = 0x7fffffff; span[3] = 0; span[4] = 0;
    }
    __syncthreads();

    // this lane's column: bounds (made safe) and coefficients
    const int j = j0 + lane;
    int cfirst = 0, ccount = 0;
    int kx[kMax];
#pragma unroll
    for (int t = 0; t < kMax; ++t) kx[t] = 0;
    if (j < a.fW) {
        cfirst = tb[lay.xb + 2 * j];
        ccount = tb[lay.xb + 2 * j + 1];
        if (cfirst < 0 || ccount < 0 || ccount > kMax || cfirst > a.W - ccount) ccount = 0;
        const int4* k4 = reinterpret_cast<const int4*>(tb + lay.xk + (long long)kMax * j);
#pragma unroll
        for (int q = 0; q < kMax / 4; ++q) {
            const int4 v = k4[q];
            kx[4 * q] = v.x; kx[4 * q + 1] = v.y; kx[4 * q + 2] = v.z; kx[4 * q + 3] = v.w;
        }
    }
    if (wave == 0 && ccount > 0) {
        atomicMin(&span[0], cfirst);
        atomicMax(&span[1], cfirst + ccount);
        atomicMax(&span[4], ccount);
    }
    if (wave == 1 && lane < kTileH) {
        int rf = 0, rc = 0;
        if (i0 + lane < a.fH) {
            rf = tb[lay.yb + 2 * (i0 + lane)];
            rc = tb[lay.yb + 2 * (i0 + lane) + 1];
        }
        if (rf < 0 || rc < 0 || rc > kMax || rf > a.H - rc) rc = 0;
        if (rc > 0) {
            atomicMin(&span[2], rf);
            atomicMax(&span[3], rf + rc);
        }
        ybl[2 * lane] = rf;
        ybl[2 * lane + 1] = rc;
    }
    {   // the vertical pass's coefficients: one per thread, fetched here so that the horizontal pass hides the latency
        const int ti = (int)threadIdx.x / kMax, tt = (int)threadIdx.x % kMax;
        kyl[threadIdx.x] = i0 + ti < a.fH ? tb[lay.yk + (long long)kMax * (i0 + ti) + tt] : 0;
    }
    __syncthreads();
    const int c0 = span[0], r0 = span[2];
    const int ncols = min(max(span[1] - c0, 0), kSpanW);
    const int nrows = ncols > 0 ? min(max(span[3] - r0, 0), kSpanH) : 0;
    if (ccount > 0 && cfirst + ccount - c0 > ncols) ccount = 0;           // a tap outside the staged span: cannot happen with a planned table
    // the tap loop below is wave-uniform (groups of four taps up to the tile's largest count): a tap beyond this lane's count gets a
    // zero coefficient, so whatever staged bytes it reads do not count
#pragma unroll
    for (int t = 0; t < kMax; ++t) kx[t] = t < ccount ? kx[t] : 0;
    const int groups = __builtin_amdgcn_readfirstlane((min(span[4], kMax) + 3) / 4);

    // ---- horizontal pass over the source rows [r0, r0 + nrows), a chunk at a time
    const unsigned char* img_src = a.src + (size_t)img * a.H * a.W * 3;
    const unsigned char* src_end = a.src + (size_t)a.n * a.H * a.W * 3;
    for (int rc0 = 0; rc0 < nrows; rc0 += kChunk) {
        const int rows = min(kChunk, nrows - rc0);
        for (int r = wave; r < rows; r += kWaves) {
            const unsigned char* p = img_src + ((size_t)(r0 + rc0 + r) * a.W + c0) * 3;
            const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
            const unsigned char* q = p - mis;
            const int dwords = (mis + ncols * 3 + 3) / 4;
            for (int d = lane; d < dwords; d += sbev::kWave) {
                const unsigned char* g = q + 4 * d;
                unsigned int v;
                if (g + 4 <= src_end) {
                    v = *reinterpret_cast<const unsigned int*>(g);
                } else {
                    v = 0;
                    for (int b = 0; b < 4; ++b)
                        if (g + b < src_end) v |= (unsigned int)g[b] << (8 * b);
                }
                stage[r * (kRowBytes / 4) + d] = v;
            }
        }
        __syncthreads();
        for (int r = wave; r < rows; r += kWaves) {
            const unsigned char* p = img_src + ((size_t)(r0 + rc0 + r) * a.W + c0) * 3;
            const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
            // this lane's taps are 3 * count consecutive bytes at an arbitrary byte offset: aligned 4-byte LDS reads, realigned by
            // v_alignbyte into the byte stream R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 of four taps
            const int b = r * kRowBytes + mis + (ccount > 0 ? (cfirst - c0) * 3 : 0);
            const unsigned int* w = stage + (b >> 2);
            const unsigned int sh = (unsigned int)b & 3u;
            unsigned int lo = w[0];
            int acc0 = 1 << (kBits - 1), acc1 = acc0, acc2 = acc0;
#pragma unroll
            for (int g = 0; g < kMax / 4; ++g) {
                if (g < groups) {
                    const unsigned int d1 = w[3 * g + 1], d2 = w[3 * g + 2], d3 = w[3 * g + 3];
                    const unsigned int s0 = __builtin_amdgcn_alignbyte(d1, lo, sh), s1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                                       s2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
                    lo = d3;
                    const int k0 = kx[4 * g], k1 = kx[4 * g + 1], k2 = kx[4 * g + 2], k3 = kx[4 * g + 3];
                    acc0 += __mul24((int)(s0 & 0xffu), k0) + __mul24((int)(s0 >> 24), k1) + __mul24((int)((s1 >> 16) & 0xffu), k2) +
                            __mul24((int)((s2 >> 8) & 0xffu), k3);
                    acc1 += __mul24((int)((s0 >> 8) & 0xffu), k0) + __mul24((int)(s1 & 0xffu), k1) + __mul24((int)(s1 >> 24), k2) +
                            __mul24((int)((s2 >> 16) & 0xffu), k3);
                    acc2 += __mul24((int)((s0 >> 16) & 0xffu), k0) + __mul24((int)((s1 >> 8) & 0xffu), k1) + __mul24((int)(s2 & 0xffu), k2) +
                            __mul24((int)(s2 >> 24), k3);
                }
            }
            unsigned char* m = mid + (rc0 + r) * 3 * kTileW + lane;
            m[0] = (unsigned char)clip8(acc0);
            m[kTileW] = (unsigned char)clip8(acc1);
            m[2 * kTileW] = (unsigned char)clip8(acc2);
        }
        __syncthreads();
    }

    // ---- vertical pass
    if (j >= a.fW) return;
    const int x = flip ? a.fW - 1 - j : j;
    const size_t plane = (size_t)a.fH * a.fW;
    for (int ii = wave; ii < kTileH && i0 + ii < a.fH; ii += kWaves) {
        const int i = i0 + ii;
        int rf = ybl[2 * ii], rcount = ybl[2 * ii + 1];
        if (rf < r0 || rf + rcount - r0 > nrows) rcount = 0;
        rf = __builtin_amdgcn_readfirstlane(rf);
        rcount = __builtin_amdgcn_readfirstlane(rcount);
        const int* ky = kyl + ii * kMax;
        const unsigned char* m = mid + (rcount > 0 ? rf - r0 : 0) * 3 * kTileW + lane;
        int acc0 = 1 << (kBits - 1), acc1 = acc0, acc2 = acc0;
        for (int t = 0; t < rcount; ++t) {
            const int k = ky[t];
            acc0 += __mul24((int)m[(3 * t) * kTileW], k);
            acc1 += __mul24((int)m[(3 * t + 1) * kTileW], k);
            acc2 += __mul24((int)m[(3 * t + 2) * kTileW], k);
        }
        unsigned char* o = a.dst + (size_t)img * 3 * plane + (size_t)i * a.fW + x;
        o[0] = (unsigned char)clip8(acc0);
        o[plane] = (unsigned char)clip8(acc1);
        o[2 * plane] = (unsigned char)clip8(acc2);
    }
}

// ---------------------------------------------------------------- the host side: Pillow's coefficients
double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int ksize_of(int in_size, int out_size) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)std::ceil(2.0 * filterscale) * 2 + 1;
}

// bounds and coefficients of resized indices lo .. lo + count - 1 of one axis (in_size -> out_size); an index outside [0, out_size)
// gets (0, 0) and zeros.  Returns false if a coefficient does not fit 24 signed bits.
bool axis_tables(int in_size, int out_size, int lo, int count, int* bounds, int* kk) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    double w[kMax];
    bool fits = true;
    for (int o = 0; o < count; ++o) {
        int* b = bounds + 2 * o;
        int* k = kk + (long long)kMax * o;
        b[0] = b[1] = 0;
        for (int t = 0; t < kMax; ++t) k[t] = 0;
        const long long xx = (long long)lo + o;
        if (xx < 0 || xx >= out_size) continue;
        const double center = ((double)xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int t = 0; t < xmax; ++t) {
            w[t] = bicubic((t + xmin - center + 0.5) * ss);
            ww += w[t];
        }
        for (int t = 0; t < xmax; ++t) {
            const double v = ww != 0.0 ? w[t] / ww : w[t];
            k[t] = v < 0 ? (int)(-0.5 + v * (1 << kBits)) : (int)(0.5 + v * (1 << kBits));
            fits = fits && k[t] >= -(1 << 23) && k[t] < (1 << 23);
        }
        b[0] = xmin;
        b[1] = xmax;
    }
    return fits;
}

// the widest / tallest source span of one tile, and the number of source indices any tap reads
void spans(const int* bounds, int count, int tile, int* widest, long long* touched) {
    *widest = 0;
    int lo_all = 0x7fffffff, hi_all = 0;
    for (int t0 = 0; t0 < count; t0 += tile) {
        int lo = 0x7fffffff, hi = 0;
        for (int o = t0; o < count && o < t0 + tile; ++o) {
            if (bounds[2 * o + 1] <= 0) continue;
            lo = bounds[2 * o] < lo ? bounds[2 * o] : lo;
            hi = bounds[2 * o] + bounds[2 * o + 1] > hi ? bounds[2 * o] + bounds[2 * o + 1] : hi;
        }
        if (hi > lo && hi - lo > *widest) *widest = hi - lo;
        if (hi > lo) {
            lo_all = lo < lo_all ? lo : lo_all;
            hi_all = hi > hi_all ? hi : hi_all;
        }
    }
    *touched = hi_all > lo_all ? hi_all - lo_all : 0;
}

int check_sizes(int H, int W, int fH, int fW, const char* who) {
    SBEV_REQUIRE(H >= 1 && W >= 1 && fH >= 1 && fW >= 1, "%s: H, W, fH, fW must be >= 1 (H=%d W=%d fH=%d fW=%d)", who, H, W, fH, fW);
    SBEV_REQUIRE(H <= 0x3fffff && W <= 0x3fffff && fH <= 0x3fffff && fW <= 0x3fffff, "%s: a size above 2^22 - 1 (H=%d W=%d fH=%d fW=%d)", who, H,
                 W, fH, fW);
    return SBEV_OK;
}

}  // namespace

extern "C" int sbev_image_geom_plan(int H, int W, int fH, int fW, int resize_w, int resize_h, int crop_x, int crop_y, int flip,
                                    int32_t* table_out, int64_t* out) {
    const char* who = "sbev_image_geom_plan";
    SBEV_REQUIRE(out != nullptr, "%s: null out", who);
    if (int st = check_sizes(H, W, fH, fW, who)) return st;
    SBEV_REQUIRE(resize_w >= 1 && resize_h >= 1 && resize_w <= 0x3fffff && resize_h <= 0x3fffff, "%s: resize to %d x %d", who, resize_w,
                 resize_h);
    SBEV_REQUIRE(crop_x > -0x3fffff && crop_x < 0x3fffff && crop_y > -0x3fffff && crop_y < 0x3fffff, "%s: crop origin (%d, %d) out of range",
                 who, crop_x, crop_y);
    const int ks_x = ksize_of(W, resize_w), ks_y = ksize_of(H, resize_h);
    SBEV_REQUIRE(ks_x <= kMax && ks_y <= kMax,
                 "%s: %d x %d -> %d x %d needs %d x %d filter taps, above the capacity SBEV_GEOM_KMAX = %d (an axis can shrink by 3.5 at most)",
                 who, W, H, resize_w, resize_h, ks_x, ks_y, kMax);
    const Layout lay = layout(fH, fW);
    const long long tiles_x = (fW + kTileW - 1) / kTileW, tiles_y = (fH + kTileH - 1) / kTileH;
    SBEV_REQUIRE(tiles_x * tiles_y <= 0x7fffffffLL, "%s: %lld workgroups per image are too many", who, tiles_x * tiles_y);
    out[0] = lay.words * 4;
    out[1] = tiles_x * tiles_y;
    out[2] = ks_x;
    out[3] = ks_y;
    out[4] = 0;
    out[5] = kTileW;
    out[6] = kTileH;
    out[7] = 0;
    if (table_out == nullptr) return SBEV_OK;

    std::vector<int32_t> block((size_t)lay.words, 0);
    block[kNewW] = resize_w; block[kNewH] = resize_h; block[kCropX] = crop_x; block[kCropY] = crop_y; block[kFlip] = flip != 0;
    block[kKsX] = ks_x; block[kKsY] = ks_y;
    const bool fits_x = axis_tables(W, resize_w, crop_x, fW, &block[lay.xb], &block[lay.xk]);
    const bool fits_y = axis_tables(H, resize_h, crop_y, fH, &block[lay.yb], &block[lay.yk]);
    SBEV_REQUIRE(fits_x && fits_y, "%s: a coefficient does not fit 24 bits", who);
    int wide = 0, tall = 0;
    long long cols = 0, rows = 0;
    spans(&block[lay.xb], fW, kTileW, &wide, &cols);
    spans(&block[lay.yb], fH, kTileH, &tall, &rows);
    SBEV_REQUIRE(wide <= kSpanW && tall <= kSpanH, "%s: a tile reads %d x %d source pixels, above the kernel's %d x %d", who, wide, tall,
                 kSpanW, kSpanH);
    out[4] = rows * cols * 3;           // source bytes any tap of this transform reads, per image
    out[7] = rows;
    for (long long i = 0; i < lay.words; ++i) table_out[i] = block[(size_t)i];
    return SBEV_OK;
}

extern "C" int sbev_image_geom(const void* src, void* dst, int n, int H, int W, int fH, int fW, const void* table, const void* image_rows,
                               int n_transforms, sbev_stream_t stream) {
    const char* who = "sbev_image_geom";
    SBEV_REQUIRE(src != nullptr && dst != nullptr && table != nullptr && image_rows != nullptr, "%s: null pointer", who);
    SBEV_REQUIRE(n >= 1 && n_transforms >= 1, "%s: n and n_transforms must be >= 1 (n=%d n_transforms=%d)", who, n, n_transforms);
    if (int st = check_sizes(H, W, fH, fW, who)) return st;
    SBEV_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15u) == 0 && (reinterpret_cast<uintptr_t>(image_rows) & 3u) == 0,
                 "%s: the table is not 16-byte aligned or image_rows not 4-byte aligned", who);
    SBEV_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3u) == 0, "%s: src is not 4-byte aligned", who);
    const long long tiles_x = (fW + kTileW - 1) / kTileW, tiles_y = (fH + kTileH - 1) / kTileH;
    SBEV_REQUIRE(tiles_x * tiles_y * n <= 0x7fffffffLL, "%s: %lld workgroups are too many for one launch", who, tiles_x * tiles_y * n);
    Args a;
    a.src = static_cast<const unsigned char*>(src);
    a.dst = static_cast<unsigned char*>(dst);
    a.table = static_cast<const int*>(table);
    a.image_rows = static_cast<const int*>(image_rows);
    a.n = n; a.H = H; a.W = W; a.fH = fH; a.fW = fW; a.n_transforms = n_transforms;
    a.tiles_x = (int)tiles_x; a.tiles_y = (int)tiles_y;
    hipLaunchKernelGGL(image_geom_kernel, dim3((unsigned)(tiles_x * tiles_y * n)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch(who);
}
