// AdamW with global-norm gradient clipping, a static loss scale and the skip of a non-finite step: one optimizer step over a LIST of
// fp32 tensors as three launches on the caller's stream, with no host synchronisation, no device -> host copy and no atomics, so the
// step can sit inside a captured graph.
//
//   optim_sumsq_kernel    one workgroup per chunk of kChunk elements: sum of (g * inv_scale)^2 -> partials[chunk]
//   optim_finish_kernel   ONE workgroup: partials added in index order -> the header (norm, clip, skip, step counter, beta powers)
//   optim_adamw_kernel    one workgroup per chunk: p, m, v updated in place from g (28 bytes per element)
//
// The update, per element, every operation an individually rounded fp32 operation in exactly this order (the file is built with
// -ffp-contract=off; sqrtf and / are correctly rounded):
//     g' = (g * inv_scale) * clip
//     p  = p * (1 - lr * wd)                      lr = lr_g * mult_g, both products and the difference rounded
//     m  = m + (g' - m) * w1                      w1 = float(1 - beta1)
//     v  = v * float(beta2) + (g' * g') * w2      w2 = float(1 - beta2)
//     p  = p - ((lr / bc1) * m) / (sqrtf(v) / bc2 + float(eps))
// bc1 = float(1 - beta1^t), bc2 = float(sqrt(1 - beta2^t)) with the powers kept as RUNNING fp64 products in the header (one
// multiplication per step by one thread): no pow per element, and the bias corrections have one definition.
//
// Chunking is fixed: a chunk is kChunk consecutive elements of ONE tensor (the last chunk of a tensor is short), whatever the device.
// Float4 index j of a chunk belongs to thread j % kThreads, on the vector path and the scalar path alike, and a workgroup's sum is a
// fixed tree; the grid is capped and strides over chunks, which changes who computes a chunk and never what it computes.  So the norm is
// the same bits from run to run, from device to device and for any alignment of the gradients.
//
// Addresses and sizes travel BY VALUE in the kernel-argument block (kMaxTensors entries, 3.1 KB of the 4 KB limit): a captured launch
// owns its table, nothing is uploaded inside the step and no device table of pointers can go stale.  The chunk -> tensor map is a binary
// search in the by-value prefix of chunk counts (wave-uniform: scalar loads from the argument segment).
//
// Who writes what: partials[c] by the workgroup that computes chunk c; the header by optim_finish_kernel only, read by
// optim_adamw_kernel only; an element of p / m / v by the one thread that owns it.  No workgroup reads what another workgroup of the
// same launch writes.
#include <cmath>

#include "sbev_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / sbev::kWave;
constexpr int kChunk = SBEV_OPTIM_CHUNK;                  // elements; 8 float4 per thread
constexpr int kMaxTensors = SBEV_OPTIM_MAX_TENSORS;
constexpr int kMaxGroups = SBEV_OPTIM_MAX_GROUPS;
constexpr int kMaxGrid = 2048;                            // 256 CUs x 8 workgroups: memory-bound launches stride beyond that
static_assert(kChunk % (4 * kThreads) == 0, "a chunk is a whole number of float4 rounds");

// what changes between steps (device, written by the caller between steps): SBEV_OPTIM_HYPER_FLOATS floats
enum { kInvScale = 0, kMaxNorm = 1, kHold = 2, kGroups = 4 };      // group g at kGroups + 4 g: lr, weight_decay, lr multiplier, -

struct Header {                // SBEV_OPTIM_HEADER_BYTES, written by optim_finish_kernel only
    double beta1_pow, beta2_pow;       // running products beta^t (1 before the first step)
    long long step, skipped;
    float norm, clip, bc1, bc2;
    int skip, pad[3];
};
static_assert(sizeof(Header) == SBEV_OPTIM_HEADER_BYTES, "header layout is part of the ABI");

struct Tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long numel;
    int group;
    int chunk_end;             // chunks of this launch up to and including this tensor
};

struct Table {
    Tensor t[kMaxTensors];
    int n;
    int chunks;
};
static_assert(sizeof(Table) + 64 <= 4096, "the table travels in the kernel-argument block");

struct Chunk {
    int tensor;
    long long first;           // first element inside the tensor
    int count;                 // 1..kChunk
};

// chunk c of the launch -> (tensor, range): binary search for the first tensor whose prefix exceeds c.  Uniform per workgroup.
__device__ inline Chunk locate(const Table& tab, int c) {
    int lo = 0, hi = tab.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab.t[mid].chunk_end > c) hi = mid;
        else lo = mid + 1;
    }
    const int before = lo == 0 ? 0 : tab.t[lo - 1].chunk_end;
    const long long first = (long long)(c - before) * kChunk;
    const long long left = tab.t[lo].numel - first;
    return Chunk{lo, first, left < kChunk ? (int)left : kChunk};
}

__device__ inline bool aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// a workgroup's sum in a fixed order: lanes by xor-shuffle inside a wave, then the waves' sums in wave order
__device__ inline double block_sum(double x, double* lds) {
    for (int off = sbev::kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, sbev::kWave);
    if ((threadIdx.x & (sbev::kWave - 1)) == 0) lds[threadIdx.x / sbev::kWave] = x;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < kWaves; ++w) s += lds[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(kThreads) void optim_sumsq_kernel(const Table tab, const float* __restrict__ hyper, float* __restrict__ partials) {
    __shared__ double lds[kWaves];
    const float inv_scale = hyper[kInvScale];
    for (int c = blockIdx.x; c < tab.chunks; c += gridDim.x) {
        const Chunk ch = locate(tab, c);
        const float* g = tab.t[ch.tensor].g + ch.first;
        const int quads = ch.count >> 2;
        double acc = 0.0;
        if (aligned16(g)) {
            for (int j = threadIdx.x; j < quads; j += kThreads) {
                const float4 q = reinterpret_cast<const float4*>(g)[j];
                const float x0 = q.x * inv_scale, x1 = q.y * inv_scale, x2 = q.z * inv_scale, x3 = q.w * inv_scale;
                acc += (double)x0 * x0;
                acc += (double)x1 * x1;
                acc += (double)x2 * x2;
                acc += (double)x3 * x3;
            }
        } else {
            for (int j = threadIdx.x; j < quads; j += kThreads)
                for (int e = 0; e < 4; ++e) {
                    const float x = g[4 * j + e] * inv_scale;
                    acc += (double)x * x;
                }
        }
        const int tail = (quads << 2) + (int)threadIdx.x;            // the < 4 elements behind the last float4: threads 0..2
        if (tail < ch.count) {
            const float x = g[tail] * inv_scale;
            acc += (double)x * x;
        }
        const double s = block_sum(acc, lds);
        if (threadIdx.x == 0) partials[c] = (float)s;
    }
}

__global__ __launch_bounds__(kThreads) void optim_finish_kernel(const float* __restrict__ partials, long long n, const float* __restrict__ hyper,
                                                                 Header* __restrict__ hdr, double beta1, double beta2) {
    __shared__ float stage[4 * kThreads];
    __shared__ double total;
    if (threadIdx.x == 0) total = 0.0;
    for (long long base = 0; base < n; base += 4 * kThreads) {      // every thread loads, ONE thread adds: index order
        __syncthreads();
        for (int i = threadIdx.x; i < 4 * kThreads && base + i < n; i += kThreads) stage[i] = partials[base + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = n - base < 4 * kThreads ? (int)(n - base) : 4 * kThreads;
            double s = total;
            for (int i = 0; i < m; ++i) s += (double)stage[i];
            total = s;
        }
    }
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(total);
    const float max_norm = hyper[kMaxNorm];
    float clip = 1.0f;
    if (max_norm > 0.0f) {                                           // clip_grad_norm_'s rule; <= 0: clipping is off
        clip = max_norm / (norm + 1e-6f);
        clip = clip < 1.0f ? clip : 1.0f;
    }
    const bool skip = !(fabsf(norm) <= 3.4028234663852886e38f) || hyper[kHold] != 0.0f;
    hdr->norm = norm;
    hdr->clip = clip;
    hdr->skip = skip ? 1 : 0;
    if (skip) {
        hdr->skipped += 1;
        return;
    }
    const double b1p = hdr->beta1_pow * beta1, b2p = hdr->beta2_pow * beta2;
    hdr->beta1_pow = b1p;
    hdr->beta2_pow = b2p;
    hdr->step += 1;
    hdr->bc1 = (float)(1.0 - b1p);
    hdr->bc2 = (float)sqrt(1.0 - b2p);
}

struct Coeffs {
    float beta2, w1, w2, eps;
};

struct Scalars {      // per chunk, uniform
    float inv_scale, clip, decay, step_size, denom_div;
};

__device__ inline void update(float& p, float g, float& m, float& v, const Scalars& s, const Coeffs& k) {
    const float gp = (g * s.inv_scale) * s.clip;
    p = p * s.decay;
    m = m + (gp - m) * k.w1;
    v = v * k.beta2 + (gp * gp) * k.w2;
    const float denom = sqrtf(v) / s.denom_div + k.eps;
    p = p - (s.step_size * m) / denom;
}

__global__ __launch_bounds__(kThreads) void optim_adamw_kernel(const Table tab, const float* __restrict__ hyper, const Header* __restrict__ hdr,
                                                                const Coeffs k) {
    if (hdr->skip != 0) return;                                      // uniform: a skipped step stores nothing
    Scalars s;
    s.inv_scale = hyper[kInvScale];
    s.clip = hdr->clip;
    s.denom_div = hdr->bc2;
    const float bc1 = hdr->bc1;
    for (int c = blockIdx.x; c < tab.chunks; c += gridDim.x) {
        const Chunk ch = locate(tab, c);
        const Tensor& t = tab.t[ch.tensor];
        const float* hg = hyper + kGroups + 4 * t.group;
        const float lr = hg[0] * hg[2];
        s.decay = 1.0f - lr * hg[1];
        s.step_size = lr / bc1;
        float* p = t.p + ch.first;
        const float* g = t.g + ch.first;
        float* m = t.m + ch.first;
        float* v = t.v + ch.first;
        const int quads = ch.count >> 2;
        if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) {
            for (int j = threadIdx.x; j < quads; j += kThreads) {
                float4 P = reinterpret_cast<float4*>(p)[j], M = reinterpret_cast<float4*>(m)[j], V = reinterpret_cast<float4*>(v)[j];
                const float4 G = reinterpret_cast<const float4*>(g)[j];
                update(P.x, G.x, M.x, V.x, s, k);
                update(P.y, G.y, M.y, V.y, s, k);
                update(P.z, G.z, M.z, V.z, s, k);
                update(P.w, G.w, M.w, V.w, s, k);
                reinterpret_cast<float4*>(p)[j] = P;
                reinterpret_cast<float4*>(m)[j] = M;
                reinterpret_cast<float4*>(v)[j] = V;
            }
        } else {
            for (int j = threadIdx.x; j < quads; j += kThreads)
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * j + e;
                    update(p[i], g[i], m[i], v[i], s, k);
                }
        }
        const int tail = (quads << 2) + (int)threadIdx.x;
        if (tail < ch.count) update(p[tail], g[tail], m[tail], v[tail], s, k);
    }
}

long long chunks_of(long long numel) { return (numel + kChunk - 1) / kChunk; }

constexpr long long kMaxNumel = 1ll << 40;

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the by-value table of one launch; tensors without elements take no chunk and stay out of it
int fill(Table& tab, void* const* p, const void* const* g, void* const* m, void* const* v, const int64_t* numel, const int32_t* group, int n,
         const char* who) {
    tab.n = 0;
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        chunks += chunks_of(numel[i]);
        SBEV_REQUIRE(chunks <= 0x7fffffffLL, "%s: too many chunks for one launch", who);
        Tensor& t = tab.t[tab.n++];
        t.p = p ? static_cast<float*>(p[i]) : nullptr;
        t.g = static_cast<const float*>(g[i]);
        t.m = m ? static_cast<float*>(m[i]) : nullptr;
        t.v = v ? static_cast<float*>(v[i]) : nullptr;
        t.numel = numel[i];
        t.group = group ? group[i] : 0;
        t.chunk_end = (int)chunks;
    }
    tab.chunks = (int)chunks;
    return SBEV_OK;
}

unsigned grid_of(int chunks) { return (unsigned)(chunks < kMaxGrid ? chunks : kMaxGrid); }

}  // namespace

extern "C" int sbev_optim_plan(const int64_t* numel, int n, int64_t* out) {
    SBEV_REQUIRE(n >= 0 && (numel != nullptr || n == 0) && out != nullptr, "sbev_optim_plan: null pointer or n=%d", n);
    long long chunks = 0, launches = 0;
    for (int first = 0; first < n; first += kMaxTensors) {
        long long here = 0;
        for (int i = first; i < n && i < first + kMaxTensors; ++i) {
            SBEV_REQUIRE(numel[i] >= 0 && numel[i] <= kMaxNumel, "sbev_optim_plan: numel[%d] = %lld", i, (long long)numel[i]);
            here += chunks_of(numel[i]);
        }
        SBEV_REQUIRE(here <= 0x7fffffffLL, "sbev_optim_plan: too many chunks for one launch");
        chunks += here;
        launches += here > 0;
    }
    out[0] = chunks;
    out[1] = launches;
    out[2] = chunks * 4;
    return SBEV_OK;
}

extern "C" int sbev_optim_sumsq(const void* const* g, const int64_t* numel, int n, const float* hyper, float* partials, sbev_stream_t stream) {
    SBEV_REQUIRE(n >= 0 && n <= kMaxTensors, "sbev_optim_sumsq: %d tensors (at most %d per call)", n, kMaxTensors);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(g != nullptr && numel != nullptr, "sbev_optim_sumsq: null array");
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        SBEV_REQUIRE(numel[i] >= 0 && numel[i] <= kMaxNumel, "sbev_optim_sumsq: numel[%d] = %lld", i, (long long)numel[i]);
        total += numel[i];
    }
    if (total == 0) return SBEV_OK;
    SBEV_REQUIRE(hyper != nullptr && partials != nullptr, "sbev_optim_sumsq: null hyper / partials");
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        SBEV_REQUIRE(g[i] != nullptr, "sbev_optim_sumsq: g[%d] is null", i);
        SBEV_REQUIRE(aligned4(g[i]), "sbev_optim_sumsq: g[%d] is not 4-byte aligned", i);
    }
    Table tab;
    if (int st = fill(tab, nullptr, g, nullptr, nullptr, numel, nullptr, n, "sbev_optim_sumsq")) return st;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(grid_of(tab.chunks)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), tab, hyper, partials);
    return sbev::check_launch("sbev_optim_sumsq");
}

extern "C" int sbev_optim_finish(const float* partials, int64_t n_partials, const float* hyper, void* header, double beta1, double beta2,
                                 sbev_stream_t stream) {
    SBEV_REQUIRE(n_partials >= 0, "sbev_optim_finish: n_partials = %lld", (long long)n_partials);
    SBEV_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "sbev_optim_finish: betas (%g, %g) not in [0, 1)", beta1, beta2);
    SBEV_REQUIRE(hyper != nullptr && header != nullptr && (partials != nullptr || n_partials == 0), "sbev_optim_finish: null pointer");
    SBEV_REQUIRE((reinterpret_cast<uintptr_t>(header) & 7u) == 0, "sbev_optim_finish: header is not 8-byte aligned");
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), partials, (long long)n_partials, hyper,
                       static_cast<Header*>(header), beta1, beta2);
    return sbev::check_launch("sbev_optim_finish");
}

extern "C" int sbev_optim_adamw(void* const* p, const void* const* g, void* const* m, void* const* v, const int64_t* numel, const int32_t* group,
                                int n, int n_groups, double beta1, double beta2, double eps, const float* hyper, const void* header,
                                sbev_stream_t stream) {
    SBEV_REQUIRE(n >= 0 && n <= kMaxTensors, "sbev_optim_adamw: %d tensors (at most %d per call)", n, kMaxTensors);
    SBEV_REQUIRE(n_groups >= 1 && n_groups <= kMaxGroups, "sbev_optim_adamw: %d groups (1..%d)", n_groups, kMaxGroups);
    SBEV_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "sbev_optim_adamw: betas (%g, %g) not in [0, 1) or eps %g < 0",
                 beta1, beta2, eps);
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(p != nullptr && g != nullptr && m != nullptr && v != nullptr && numel != nullptr && group != nullptr, "sbev_optim_adamw: null array");
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        SBEV_REQUIRE(numel[i] >= 0 && numel[i] <= kMaxNumel, "sbev_optim_adamw: numel[%d] = %lld", i, (long long)numel[i]);
        SBEV_REQUIRE(group[i] >= 0 && group[i] < n_groups, "sbev_optim_adamw: group[%d] = %d out of range (%d groups)", i, group[i], n_groups);
        total += numel[i];
    }
    if (total == 0) return SBEV_OK;
    SBEV_REQUIRE(hyper != nullptr && header != nullptr, "sbev_optim_adamw: null hyper / header");
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        SBEV_REQUIRE(p[i] != nullptr && g[i] != nullptr && m[i] != nullptr && v[i] != nullptr, "sbev_optim_adamw: tensor %d has a null pointer", i);
        SBEV_REQUIRE(aligned4(p[i]) && aligned4(g[i]) && aligned4(m[i]) && aligned4(v[i]), "sbev_optim_adamw: tensor %d is not 4-byte aligned", i);
    }
    Table tab;
    if (int st = fill(tab, p, g, m, v, numel, group, n, "sbev_optim_adamw")) return st;
    const Coeffs k{(float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
    hipLaunchKernelGGL(optim_adamw_kernel, dim3(grid_of(tab.chunks)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), tab, hyper,
                       static_cast<const Header*>(header), k);
    return sbev::check_launch("sbev_optim_adamw");
}
