// The ResNet backbone's two weight images -- the forward's folded fragment pack with its fp32 biases (resnet.hip:
// sbev_resnet_pack_weights) and the backward's transposed / flipped pack (resnet_bwd.hip: sbev_resnet_pack_weights_bwd) -- derived for the
// WHOLE net by ONE launch that takes no host array: a device table holds every convolution's source pointers, shape and offsets, so the
// launch records into a graph and a replay folds the weights as they are then (a training step after an optimizer update).
//
// Arithmetic: the per-layer entries', bit for bit (this unit is built with -ffp-contract=off like theirs): s = gamma / sqrtf(var + eps),
// b' = beta - mean * s, w' = fp16(fp32(w * s)), every operation rounded on its own -- resnet_train.hpp's bn_fold_scale and bn_fold_weight,
// which the pack kernels of resnet.hip and resnet_bwd.hip use too.  w' is computed ONCE per element and feeds both images.
//
// Work item = a tile of 32 output channels x 64 reduction indices (input channels; the stem: 64 of its 147 flat (c, ky, kx) indices, padded
// with zeros to 160) x all taps of one convolution.  The workgroup (256 threads)
//   1. folds the 32 scales into LDS (and, on the first K tile of a channel block, stores the 32 biases as 8 uint4);
//   2. reads the tile's 32 weight rows -- 64 taps contiguous elements each -- from global memory, one element per lane, consecutive lanes
//      on consecutive addresses, every element once per launch, and writes w' as fp16 into the LDS tile T[co][tap][ci]
//      (row pitch 64 taps + 8 halves);
//   3. stores the forward's fragments: per tap 256 uint4, thread t the piece (ks = t / 64, fragment parity, lane) -- one 16-byte LDS
//      read of 8 consecutive ci; runs of 16 threads store 256 contiguous bytes;
//   4. where the convolution has a backward image, stores its fragments: per flipped tap 256 uint4, thread t the piece (ks = t / 128,
//      fragment parity, lane) -- 8 two-byte LDS reads of 8 consecutive co; runs of 64 threads store 1 KB contiguous.
// LDS banks (64 banks of 4 bytes): step 4's reads put lanes 0 .. 31 on 32 consecutive banks and lanes 32 .. 63, 8 rows further (8 pitches =
// a multiple of 256 bytes + 128), on the other 32: conflict-free.  Step 3's 16-byte reads step 2 rows = 32 bytes (mod 256) per lane: 2-way.
// Step 2's two-byte LDS writes are the costly side for a 3 x 3: lane e goes to (e % 9) * 128 + (e / 9) * 2 bytes, so neighbouring lanes are
// 128 bytes apart and taps of equal parity share banks -- a 4- to 5-way conflict (a 1 x 1 writes consecutive halves: 2 lanes per bank word,
// no conflict).  Global loads are 4 bytes per lane (2 for fp16 weights), 256-byte segments per wave instruction, not 16-byte loads.  Nothing
// of this is measured in isolation.  The launch as a whole: 82 us for ResNet-50's 187 MB, 0.36 of the measured copy rate: not
// at the memory bound.
// Every 16-byte piece of both images has exactly one owning (item, thread, iteration) and is stored whole; no atomics; nothing outside
// the two images is written.  The grid is fixed (kGrid workgroups striding over the items): the launch needs no host copy of the table.
#include "fpn_common.hpp"
#include "resnet_train.hpp"

namespace {

using namespace sbev_fpn;

constexpr int kHead = SBEV_RESNET_REPACK_HEAD, kWords = SBEV_RESNET_REPACK_LAYER_WORDS;
constexpr int kStemK = 147, kStemKpad = 160;
constexpr int kCo = 32, kK = 64;              // the tile
constexpr int kGrid = 1024, kThreads256 = 256;
// table words of a convolution
enum { W_W = 0, W_GAMMA, W_BETA, W_MEAN, W_VAR, W_CIN, W_COUT, W_TAPS, W_FWD, W_BIAS, W_BWD, W_FIRST };

template <int TAPS, bool F32>
__device__ __forceinline__ void load_tile(const void* w, const float* sc, _Float16* tile, int co0, int k0, int klen, int Krow, int tid) {
    constexpr int pitch = kK * TAPS + 8;
    const int wave = tid >> 6, lane = tid & 63;
    const int row_len = klen * TAPS;
    for (int r = wave; r < kCo; r += 4) {
        const size_t base = ((size_t)(co0 + r) * Krow + k0) * TAPS;
        const float s = sc[r];
#pragma unroll
        for (int i = 0; i < TAPS; ++i) {
            const int e = lane + 64 * i;
            _Float16 v = (_Float16)0.f;
            if (e < row_len) {
                const float x = F32 ? static_cast<const float*>(w)[base + e] : (float)static_cast<const _Float16*>(w)[base + e];
                v = sbev_resnet::bn_fold_weight(x, s);
            }
            tile[r * pitch + (e % TAPS) * kK + e / TAPS] = v;
        }
    }
}

template <int TAPS>
__device__ __forceinline__ void store_tile(const _Float16* tile, uint4* fwd, uint4* bwd, int cob, int kb, int nks, int KS, int Cin, int Cout,
                                           int tid) {
    constexpr int pitch = kK * TAPS + 8;
    {   // the forward's fragments: [tap][KS][Cout / 32][64][8 halves], co = 64 (nt / 2) + 2 (l & 31) + (nt & 1), k = 16 ks + 8 (l >> 5) + j
        const int NF = Cout / 32;
        const int ks = tid >> 6, u = tid & 63, par = u >> 5, v = u & 31;
        const int lane = 16 * (cob & 1) + (v & 15) + 32 * (v >> 4);
        const int co_l = 2 * (v & 15) + par, k_l = 16 * ks + 8 * (v >> 4);
        const int nt = 2 * (cob >> 1) + par;
        if (ks < nks) {
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const uint4 q = *reinterpret_cast<const uint4*>(tile + co_l * pitch + tap * kK + k_l);
                fwd[(((size_t)tap * KS + (kb * 4 + ks)) * NF + nt) * 64 + lane] = q;
            }
        }
    }
    if (bwd != nullptr) {   // [tap'][Cout / 16][Cin / 32][64][8 halves], ci = 64 (nt / 2) + 2 (l & 31) + (nt & 1), co = 16 ks + 8 (l >> 5) + j
        const int NF = Cin / 32, KSB = Cout / 16;
        const int ks = tid >> 7, par = (tid >> 6) & 1, lane = tid & 63;
        const int ci_l = 2 * (lane & 31) + par, co_l = 16 * ks + 8 * (lane >> 5);
        const int nt = 2 * kb + par;
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) {
            const int tap = TAPS == 9 ? 8 - tp : 0;
            const unsigned short* src = reinterpret_cast<const unsigned short*>(tile) + co_l * pitch + tap * kK + ci_l;
            unsigned h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = (unsigned)src[(2 * j) * pitch] | ((unsigned)src[(2 * j + 1) * pitch] << 16);
            bwd[(((size_t)tp * KSB + (cob * 2 + ks)) * NF + nt) * 64 + lane] = make_uint4(h[0], h[1], h[2], h[3]);
        }
    }
}

__global__ __launch_bounds__(kThreads256) void resnet_repack_kernel(const long long* __restrict__ table, char* fwd_image, char* bwd_image,
                                                                    float eps) {
    __shared__ __attribute__((aligned(16))) _Float16 tile[kCo * (kK * 9 + 8)];
    __shared__ float sc[kCo];
    const int tid = threadIdx.x;
    const int n = (int)table[0];
    const long long items = table[1];
    const int f32 = table[4] == SBEV_F32;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        // the convolution of this item: the last one whose first item is <= item
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[kHead + kWords * mid + W_FIRST] <= item) lo = mid; else hi = mid - 1;
        }
        const long long* L = table + kHead + kWords * lo;
        const int Cin = (int)L[W_CIN], Cout = (int)L[W_COUT], taps = (int)L[W_TAPS];
        const bool stem = taps == 49;
        const int Krow = stem ? kStemK : Cin;                  // elements of a weight row per tap
        const int Kpad = stem ? kStemKpad : Cin;
        const int kblocks = (Kpad + kK - 1) / kK;
        const int local = (int)(item - L[W_FIRST]);
        const int cob = local / kblocks, kb = local % kblocks;
        const int co0 = cob * kCo, k0 = kb * kK;
        const int klen = min(kK, Krow - k0);                   // the stem's last tile: 147 - 128 = 19
        const int nks = min(4, Kpad / 16 - kb * 4);            // 16-wide K steps of this tile (the stem's last: 2)
        const float* gamma = reinterpret_cast<const float*>(L[W_GAMMA]);
        const float* var = reinterpret_cast<const float*>(L[W_VAR]);
        if (tid < kCo) sc[tid] = sbev_resnet::bn_fold_scale(gamma[co0 + tid], var[co0 + tid], eps);
        __syncthreads();
        if (kb == 0 && tid < kCo / 4) {
            const float* beta = reinterpret_cast<const float*>(L[W_BETA]);
            const float* mean = reinterpret_cast<const float*>(L[W_MEAN]);
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 4 * tid + j;
                b[j] = beta[co0 + c] - mean[co0 + c] * sc[c];
            }
            reinterpret_cast<uint4*>(fwd_image + L[W_BIAS])[cob * (kCo / 4) + tid] =
                make_uint4(__float_as_uint(b[0]), __float_as_uint(b[1]), __float_as_uint(b[2]), __float_as_uint(b[3]));
        }
        const void* w = reinterpret_cast<const void*>(L[W_W]);
        uint4* fwd = reinterpret_cast<uint4*>(fwd_image + L[W_FWD]);
        uint4* bwd = L[W_BWD] >= 0 && bwd_image != nullptr ? reinterpret_cast<uint4*>(bwd_image + L[W_BWD]) : nullptr;
        if (taps == 9) {
            if (f32) load_tile<9, true>(w, sc, tile, co0, k0, klen, Krow, tid); else load_tile<9, false>(w, sc, tile, co0, k0, klen, Krow, tid);
            __syncthreads();
            store_tile<9>(tile, fwd, bwd, cob, kb, nks, Kpad / 16, Cin, Cout, tid);
        } else {
            if (f32) load_tile<1, true>(w, sc, tile, co0, k0, klen, Krow, tid); else load_tile<1, false>(w, sc, tile, co0, k0, klen, Krow, tid);
            __syncthreads();
            store_tile<1>(tile, fwd, bwd, cob, kb, nks, Kpad / 16, Cin, Cout, tid);
        }
        __syncthreads();          // the next item overwrites sc and the tile
    }
}

}  // namespace

extern "C" int sbev_resnet_repack_plan(int depth, const int32_t* stage_blocks, int num_stages, int base_channels, int first_trainable_stage,
                                       const void* const* w, const float* const* gamma, const float* const* beta, const float* const* mean,
                                       const float* const* var, int w_dtype, int64_t* table, int64_t* out) {
    const char* who = "sbev_resnet_repack_plan";
    SBEV_REQUIRE(table != nullptr && out != nullptr, "%s: null table / out", who);
    SBEV_REQUIRE(w_dtype == SBEV_F32 || w_dtype == SBEV_F16, "%s: w_dtype %d (SBEV_F32 or SBEV_F16)", who, w_dtype);
    SBEV_REQUIRE(num_stages >= 1 && num_stages <= 4, "%s: num_stages=%d not in 1 .. 4", who, num_stages);
    // first_trainable_stage = num_stages + 1: nothing trains, no backward image
    const bool frozen = first_trainable_stage == num_stages + 1;
    const int32_t last = num_stages - 1;
    sbev_resnet::TrainNet t;
    if (int st = sbev_resnet::train_net(who, depth, stage_blocks, num_stages, base_channels, 1, 32, 32, 1, &last,
                                        frozen ? num_stages : first_trainable_stage, &t))
        return st;
    int64_t bp[SBEV_RESNET_BWD_PLAN_WORDS];
    int64_t bwd_bytes = 0;
    if (!frozen) {
        if (int st = sbev_resnet_backward_plan(depth, stage_blocks, num_stages, base_channels, 1, 32, 32, 1, &last, first_trainable_stage, bp))
            return st;
        bwd_bytes = bp[2];
    }
    SBEV_REQUIRE(w && gamma && beta && mean && var, "%s: null pointer", who);
    int n = 0;
    long long items = 0;
    for (int i = 0; i < t.n_layers; ++i) {
        const sbev_resnet::TLayer& L = t.layer[i];
        if (L.kind == 1) continue;           // the pool has no weights
        SBEV_REQUIRE(w[n] && gamma[n] && beta[n] && mean[n] && var[n], "%s: layer %d: null pointer", who, n);
        bool al = (reinterpret_cast<uintptr_t>(w[n]) & (w_dtype == SBEV_F32 ? 3u : 1u)) == 0;
        for (const float* q : {gamma[n], beta[n], mean[n], var[n]}) al = al && (reinterpret_cast<uintptr_t>(q) & 3u) == 0;
        SBEV_REQUIRE(al, "%s: layer %d: misaligned tensor", who, n);
        const long long k = L.taps == 49 ? kStemKpad : (long long)L.taps * L.Cin;      // resnet.hip: pack_bytes
        int64_t* o = table + kHead + kWords * n;
        o[W_W] = (int64_t)reinterpret_cast<uintptr_t>(w[n]);
        o[W_GAMMA] = (int64_t)reinterpret_cast<uintptr_t>(gamma[n]);
        o[W_BETA] = (int64_t)reinterpret_cast<uintptr_t>(beta[n]);
        o[W_MEAN] = (int64_t)reinterpret_cast<uintptr_t>(mean[n]);
        o[W_VAR] = (int64_t)reinterpret_cast<uintptr_t>(var[n]);
        o[W_CIN] = L.Cin; o[W_COUT] = L.Cout; o[W_TAPS] = L.taps;
        o[W_FWD] = L.pack_off;
        o[W_BIAS] = L.pack_off + k * L.Cout * 2;
        o[W_BWD] = frozen ? -1 : bp[SBEV_RESNET_BWD_PLAN_HEAD + SBEV_RESNET_BWD_LAYER_WORDS * i + 3];
        o[W_FIRST] = items;
        const long long kpad = L.taps == 49 ? kStemKpad : L.Cin;
        items += (long long)(L.Cout / kCo) * ((kpad + kK - 1) / kK);
        ++n;
    }
    for (int i = 0; i < kHead; ++i) table[i] = 0;
    table[0] = n;
    table[1] = items;
    table[2] = t.pack_bytes;
    table[3] = bwd_bytes;
    table[4] = w_dtype;
    out[0] = kHead + kWords * n;
    out[1] = items;
    out[2] = t.pack_bytes;
    out[3] = bwd_bytes;
    return SBEV_OK;
}

extern "C" int sbev_resnet_repack(const int64_t* table_dev, void* fwd_image, void* bwd_image, float eps, sbev_stream_t stream) {
    const char* who = "sbev_resnet_repack";
    SBEV_REQUIRE(eps >= 0.f && std::isfinite(eps), "%s: eps=%g", who, (double)eps);
    SBEV_REQUIRE(table_dev != nullptr && fwd_image != nullptr, "%s: null pointer", who);
    SBEV_REQUIRE((reinterpret_cast<uintptr_t>(table_dev) & 7u) == 0 && aligned16(fwd_image) && aligned16(bwd_image), "%s: 16-byte alignment", who);
    hipLaunchKernelGGL(resnet_repack_kernel, dim3(kGrid), dim3(kThreads256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(table_dev), static_cast<char*>(fwd_image), static_cast<char*>(bwd_image), eps);
    return sbev::check_launch(who);
}
