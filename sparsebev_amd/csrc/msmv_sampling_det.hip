// Multi-scale multi-view bilinear sampling, BACKWARD: the feature-map gradient WITHOUT float atomics (gfx950).
//
// Replaces the grad_value atomics of ms_deformable_col2im_bilinear_gm (models/csrc/msmv_sampling/msmv_sampling_backward.cu:29-105)
// where bit-reproducible gradients are asked for; msmv_sampling_bwd.hip's kernels keep them (and stay the default).  A tap's
// contribution to grad_value is ONE scalar times a row of grad_out, so nothing has to be stored per tap but that scalar and where the
// row goes:
//   1. msmv_taps_kernel: one wave per (b', q), as the backward; for every tap i = (((b' Q + q) P + p) L + l) 4 + k of the call it
//      writes key[i] = (l << 56) | element offset of the destination row (INT64_MAX: the atomic kernel would issue nothing for this
//      tap) and coef[i] = (ch * cwid) * wl;
//   2. the caller sorts the keys, STABLY and ascending (the Python layer: torch.sort) -- integer work, the same result whatever the
//      execution order, and equal keys keep ascending i;
//   3. msmv_sum_sorted_kernel: ONE wave owns a run of equal keys (the wave in whose 64 positions the run begins), lanes are channels;
//      it walks the run front to back, acc = acc + coef_i * g_i[c] with product and sum individually rounded, and does ONE
//      read-modify-write of the destination row.
// The bits of the result depend on the inputs alone: not on the launch geometry, the number of CUs, other streams, or whether the call
// is eager or a graph replay.  No atomics, no cross-wave protocol: a run is never split, so every destination row has one writer.
// Built with -ffp-contract=off (build.py): "product rounded, then sum rounded" is the definition of the result.
#include "sbev_common.hpp"
#include "msmv_bwd_geom.hpp"

namespace {

constexpr long long KEY_DEAD = 0x7fffffffffffffffLL;      // INT64_MAX: sorts behind every live key
constexpr int KEY_LEVEL_SHIFT = 56;

struct TapArgs {
    const float* feat[SBEV_MAX_LEVELS];      // filled by fill_pyramid, never read: a tap list needs no feature VALUES
    int H[SBEV_MAX_LEVELS];
    int W[SBEV_MAX_LEVELS];
    long long stride_bo[SBEV_MAX_LEVELS];
    long long stride_v[SBEV_MAX_LEVELS];
    long long stride_g, stride_px;
    const float* loc;
    const float* w;
    long long* keys;       // [n]
    float* coefs;          // [n]
    long long n_waves;
    int N, C, Q, P, gdiv;
};

// lane = (point p0 + (lane >> 2), corner k = lane & 3): 16 points x 4 corners per trip, the level loop unrolled (H, W, strides of a
// level are wave-uniform scalars).  Every tap of the call is written, dead ones included, with plain vector stores.
template <int L>
__global__ __launch_bounds__(256) void msmv_taps_kernel(const TapArgs a) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long wave = (long long)blockIdx.x * 4 + wv;
    if (wave >= a.n_waves) return;
    const long long bp = wave / a.Q;
    const long long bo = bp / a.gdiv, gi = bp - bo * a.gdiv;
    const int P = a.P;
    const int k = lane & 3, kh = k >> 1, kw = k & 1;
    const float* __restrict__ locq = a.loc + wave * P * 3;
    const float* __restrict__ wq = a.w + wave * P * L;
    long long* __restrict__ keyq = a.keys + wave * P * (L * 4);
    float* __restrict__ coefq = a.coefs + wave * P * (L * 4);
    const float nm1 = (float)(a.N - 1);

    for (int p = lane >> 2; p < P; p += 16) {
        const float x = locq[p * 3 + 0], y = locq[p * 3 + 1];
        const int view = sbev::msmv_view(locq[p * 3 + 2], nm1, a.N);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int H = a.H[l], W = a.W[l];
            const sbev::MsmvLevelPos t = sbev::msmv_level_pos(x, y, H, W);
            const sbev::MsmvLevelFrac fr = sbev::msmv_level_frac(t);
            const int hc = (int)fr.hf + kh, wc = (int)fr.wf + kw;
            const bool live = t.lvl_ok && hc >= 0 && hc <= H - 1 && wc >= 0 && wc <= W - 1;
            const float ch = kh ? fr.lh : 1.f - fr.lh, cwid = kw ? fr.lw : 1.f - fr.lw;
            const float wl = wq[p * L + l];
            const long long off = bo * a.stride_bo[l] + gi * a.stride_g + view * a.stride_v[l] +
                                  ((long long)min(max(hc, 0), H - 1) * W + min(max(wc, 0), W - 1)) * a.stride_px;
            const int i = (p * L + l) * 4 + k;
            keyq[i] = live ? (((long long)l << KEY_LEVEL_SHIFT) | off) : KEY_DEAD;
            coefq[i] = live ? (ch * cwid) * wl : 0.f;
        }
    }
}

struct SumArgs {
    float* gfeat[SBEV_MAX_LEVELS];
    const long long* keys;     // [n] sorted ascending
    const long long* order;    // [n] tap index at sorted position j
    const float* coefs;        // [n] by tap index
    const float* gout;         // [B',Q,C,P] or [B,Q,G,T*P,C]
    long long n;
    int gout_mix, T, G;
    int L, C, Q, P;
};

// element offset of tap i's grad_out row (element c of it: + c * gs_c); I: the width the index arithmetic needs (the host picks)
template <typename I>
__device__ __forceinline__ long long tap_row_offset(const SumArgs& a, long long tap) {
    const I r = (I)tap / (I)(4 * a.L);               // (b' Q + q) P + p
    const I wave = r / (I)a.P, p = r - wave * (I)a.P;
    if (!a.gout_mix) return (long long)wave * a.C * a.P + (long long)p;
    const I bp = wave / (I)a.Q, q = wave - bp * (I)a.Q, bt = bp / (I)a.G, g = bp - bt * (I)a.G, b = bt / (I)a.T, t = bt - b * (I)a.T;
    return (((((long long)b * a.Q + q) * a.G + g) * a.T + t) * (long long)a.P + p) * a.C;
}

__device__ __forceinline__ float lane_value(float v, int lane) {      // lane: wave-uniform
    return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane));
}
__device__ __forceinline__ long long lane_value(long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// One wave per CHUNK of 64 sorted positions: it owns the runs that BEGIN in its chunk (key[j] != key[j - 1]) and follows the last of
// them past the chunk's end, block by block, for as long as it lasts -- a run is never split across waves, every destination row has
// one writer.  Per block of 64 positions the index work is done with lanes = TERMS (position -> tap -> coefficient and grad_out row:
// three dependent loads and the index divisions once per 64 terms); then lanes = CHANNELS and the wave walks the block's terms front to
// back, each term's coefficient and row handed over through v_readlane, four terms' grad_out loads requested together.  Where a run
// begins, the one before it is written (ONE read-modify-write: the row was requested when its run began) and the sum restarts at +0.
// Channels in trips of 4 x 64: the chunk is walked once per trip (C <= 256: once).  Dead, negative and foreign-level keys own nothing.
template <typename I>
__global__ __launch_bounds__(256) void msmv_sum_sorted_kernel(const SumArgs a) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long base0 = ((long long)blockIdx.x * 4 + wv) * 64;
    if (base0 >= a.n) return;
    const long long lead = base0 > 0 ? a.keys[base0 - 1] : KEY_DEAD;      // a run that began in an earlier chunk is its owner's
    const int C = a.C;
    const long long gs_c = a.gout_mix ? 1 : a.P;
    constexpr long long OFF_MASK = (1LL << KEY_LEVEL_SHIFT) - 1;

    for (int c0 = 0; c0 < C; c0 += 256) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, was[4] = {0.f, 0.f, 0.f, 0.f};
        bool cok[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) cok[m] = c0 + lane + 64 * m < C;
        float* dst = nullptr;             // wave-uniform; non-null: a run is open, `cur` its key
        long long cur = KEY_DEAD;
        for (long long base = base0;; base += 64) {
            const long long jj = base + lane;                      // lanes = terms
            const long long k = jj < a.n ? a.keys[jj] : KEY_DEAD;
            bool own, head = false;
            if (base == base0) {
                const long long prev = jj > 0 && jj < a.n ? a.keys[jj - 1] : KEY_DEAD;
                own = k != KEY_DEAD && k >= 0 && (int)(k >> KEY_LEVEL_SHIFT) < a.L && k != lead;
                head = own && prev != k;
            } else {
                own = k == cur;                                    // sorted keys: a prefix of the block
            }
            const long long tap = own ? a.order[jj] : 0;
            const bool ok = own && (unsigned long long)tap < (unsigned long long)a.n;      // not a permutation entry: no term
            const float cf = ok ? a.coefs[tap] : 0.f;
            const long long ro = ok ? tap_row_offset<I>(a, tap) : 0;
            const unsigned long long ownm = __ballot(own), okm = __ballot(ok), headm = __ballot(head);
            for (int u0 = 0; u0 < 64; u0 += 4) {                   // lanes = channels
                if (!((ownm >> u0) & 0xf)) continue;
                float coef[4], gv[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {                      // a lane that owns nothing holds row 0 and is not added
                    coef[u] = lane_value(cf, u0 + u);
                    const float* __restrict__ g = a.gout + lane_value(ro, u0 + u);
#pragma unroll
                    for (int m = 0; m < 4; ++m) gv[u][m] = cok[m] ? g[(c0 + lane + 64 * m) * gs_c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {                      // strictly in sorted order; every branch is wave-uniform
                    if ((headm >> (u0 + u)) & 1) {
                        if (dst) {
#pragma unroll
                            for (int m = 0; m < 4; ++m)
                                if (cok[m]) dst[c0 + lane + 64 * m] = was[m] + acc[m];
                        }
                        cur = lane_value(k, u0 + u);
                        dst = a.gfeat[(int)(cur >> KEY_LEVEL_SHIFT)] + (cur & OFF_MASK);
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            was[m] = cok[m] ? dst[c0 + lane + 64 * m] : 0.f;      // requested now, added when the run ends
                            acc[m] = 0.f;
                        }
                    }
                    if (!((okm >> (u0 + u)) & 1)) continue;        // a term that is not there adds nothing, not +0
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float prod = coef[u] * gv[u][m];     // rounded (no contraction in this translation unit) ...
                        acc[m] = acc[m] + prod;                    // ... then the sum, rounded
                    }
                }
            }
            // the open run goes on past this block?
            if (!(dst && (ownm >> 63) && base + 64 < a.n && a.keys[base + 64] == cur)) break;
        }
        if (dst) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (cok[m]) dst[c0 + lane + 64 * m] = was[m] + acc[m];
        }
    }
}

template <int L>
int launch_taps(const TapArgs& a, hipStream_t s) {
    const long long blocks = (a.n_waves + 3) / 4;
    hipLaunchKernelGGL(msmv_taps_kernel<L>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return sbev::check_launch("sbev_msmv_bwd_taps");
}

}  // namespace

extern "C" int64_t sbev_msmv_bwd_tap_count(int64_t Bp, int Q, int P, int L) {
    if (Bp < 0 || Q < 0 || P < 0 || P > SBEV_MAX_POINTS || L < 1 || L > SBEV_MAX_LEVELS) return -1;
    const int64_t limit = INT64_MAX / 4;
    int64_t n = 4 * (int64_t)L * P;                        // <= 640
    if (n == 0 || Q == 0 || Bp == 0) return 0;
    if ((int64_t)Q > limit / n) return -1;
    n *= Q;
    if (Bp > limit / n) return -1;
    return n * Bp;
}

extern "C" int sbev_msmv_bwd_taps(const void* const* feats, const int32_t* hw, int L,
                                  int64_t Bp, int N, int C, int Q, int P,
                                  int gdiv, const int64_t* stride_bo, int64_t stride_g, const int64_t* stride_v, int64_t stride_px,
                                  const float* loc, const float* weights, int64_t* keys, float* coefs, sbev_stream_t stream) {
    const sbev::PyramidDesc d{feats, hw, L, SBEV_F32, N, C, Q, P, gdiv, stride_bo, stride_g, stride_v, stride_px, loc, weights, nullptr, 0, nullptr};
    if (int st = sbev::check_pyramid(d, "sbev_msmv_bwd_taps")) return st;
    SBEV_REQUIRE(C >= 1 && N >= 1 && Q >= 0 && Bp >= 0 && gdiv >= 1, "sbev_msmv_bwd_taps: bad sizes");
    SBEV_REQUIRE(sbev_msmv_bwd_tap_count(Bp, Q, P, L) >= 0, "sbev_msmv_bwd_taps: B'*Q*P*L*4 too large");
    if (Bp == 0 || Q == 0) return SBEV_OK;
    SBEV_REQUIRE(loc && weights && keys && coefs, "sbev_msmv_bwd_taps: null pointer");
    SBEV_REQUIRE((Bp * Q + 3) / 4 <= 0x7fffffffLL, "sbev_msmv_bwd_taps: B'*Q too large");
    // a key is (level << 56) | offset, and every destination row [offset, offset + C) has ONE writer: offsets are non-negative,
    // below 2^56, and rows of different pixels / groups do not overlap
    SBEV_REQUIRE(stride_px >= C && stride_g >= 0 && (gdiv == 1 || stride_g >= C), "sbev_msmv_bwd_taps: pixel / group strides must be >= C=%d", C);
    const int64_t bo_last = (Bp - 1) / gdiv;
    for (int l = 0; l < L; ++l) {
        SBEV_REQUIRE(hw[2 * l] >= 1 && hw[2 * l + 1] >= 1, "sbev_msmv_bwd_taps: level %d has empty map", l);
        SBEV_REQUIRE(stride_bo[l] >= 0 && stride_v[l] >= 0, "sbev_msmv_bwd_taps: level %d has a negative stride", l);
        const __int128 last = (__int128)bo_last * stride_bo[l] + (__int128)(gdiv - 1) * stride_g + d.slab_span(l);
        SBEV_REQUIRE(last < ((__int128)1 << KEY_LEVEL_SHIFT), "sbev_msmv_bwd_taps: level %d: offsets do not fit 56 bits", l);
    }
    TapArgs a{};
    sbev::fill_pyramid(a, d);
    a.keys = reinterpret_cast<long long*>(keys);
    a.coefs = coefs;
    a.n_waves = Bp * Q;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (L) {
        case 1: return launch_taps<1>(a, s);
        case 2: return launch_taps<2>(a, s);
        case 3: return launch_taps<3>(a, s);
        case 4: return launch_taps<4>(a, s);
        default: return launch_taps<5>(a, s);
    }
}

extern "C" int sbev_msmv_bwd_sum_sorted(void* const* grad_feats, int L, const int64_t* sorted_keys, const int64_t* order,
                                        const float* coefs, int64_t n, const float* grad_out, int grad_out_layout,
                                        int64_t Bp, int C, int Q, int P, int T, int G, sbev_stream_t stream) {
    SBEV_REQUIRE(L >= 1 && L <= SBEV_MAX_LEVELS, "sbev_msmv_bwd_sum_sorted: L=%d not in 1..%d", L, SBEV_MAX_LEVELS);
    SBEV_REQUIRE(P >= 1 && P <= SBEV_MAX_POINTS, "sbev_msmv_bwd_sum_sorted: num_point exceed limits (P=%d > %d)", P, SBEV_MAX_POINTS);
    SBEV_REQUIRE(C >= 1 && Q >= 0 && Bp >= 0, "sbev_msmv_bwd_sum_sorted: bad sizes");
    SBEV_REQUIRE(grad_out_layout == SBEV_OUT_REF || grad_out_layout == SBEV_OUT_MIX, "sbev_msmv_bwd_sum_sorted: grad_out_layout %d", grad_out_layout);
    if (grad_out_layout == SBEV_OUT_MIX)
        SBEV_REQUIRE(T >= 1 && G >= 1 && Bp % ((int64_t)T * G) == 0, "sbev_msmv_bwd_sum_sorted: B'=%lld is not B*T*G (T=%d, G=%d)", (long long)Bp, T, G);
    const int64_t want = sbev_msmv_bwd_tap_count(Bp, Q, P, L);
    SBEV_REQUIRE(want >= 0 && n == want, "sbev_msmv_bwd_sum_sorted: n=%lld is not B'*Q*P*L*4 = %lld", (long long)n, (long long)want);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(grad_feats && sorted_keys && order && coefs && grad_out, "sbev_msmv_bwd_sum_sorted: null pointer");
    SBEV_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "sbev_msmv_bwd_sum_sorted: n=%lld too large for one launch", (long long)n);
    SumArgs a{};
    for (int l = 0; l < L; ++l) {
        SBEV_REQUIRE(grad_feats[l], "sbev_msmv_bwd_sum_sorted: level %d pointer is null", l);
        a.gfeat[l] = static_cast<float*>(grad_feats[l]);
    }
    a.keys = reinterpret_cast<const long long*>(sorted_keys);
    a.order = reinterpret_cast<const long long*>(order);
    a.coefs = coefs; a.gout = grad_out; a.n = n;
    a.gout_mix = grad_out_layout == SBEV_OUT_MIX; a.T = T; a.G = G;
    a.L = L; a.C = C; a.Q = Q; a.P = P;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + 255) / 256));         // 4 waves of 64 sorted positions
    if (n <= 0xffffffffLL)
        hipLaunchKernelGGL(msmv_sum_sorted_kernel<unsigned>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(msmv_sum_sorted_kernel<long long>, grid, dim3(256), 0, s, a);
    return sbev::check_launch("sbev_msmv_bwd_sum_sorted");
}
