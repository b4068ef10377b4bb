// Backward of the decoder layer's row-wise ops (gfx950): bias / ReLU, LayerNorm, box refinement, sample-point
// generation, camera projection + view selection, dropout.  SURVEY.md section 8f rank 4 -- the reference differentiates
// these through autograd (models/sparsebev_transformer.py:162-193,270-311; models/sparsebev_sampling.py:8-24,49-114);
// here each has one hand-written kernel behind the C ABI, and sparsebev_amd/autograd.py wires them as
// torch.autograd.Function backward passes.  All of them are HBM / latency bound and tiny next to the GEMMs.
//
// This file is compiled with -ffp-contract=off: the projection backward must re-select exactly the camera the forward
// selected, so it re-runs the forward's individually rounded expressions (project.hip) bit for bit.
#include "sbev_common.hpp"

namespace {

// ---- LayerNorm backward ---------------------------------------------------------------------------------------------
// y = relu?(xhat * gamma + beta), xhat = (x - mean) * rstd.   One wave per row (N <= 1024, N % 4 == 0):
//   g  = dY * (y_pre_relu > 0)                         dxhat = g * gamma
//   dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
// and the row's (mean, rstd) are left in `stats` for the column sums below: dgamma[n] = sum_m g * xhat, dbeta[n] = sum_m g.
struct LnBwdArgs {
    const float* dY;     // [M, N]
    const float* X;      // [M, N]   (the LayerNorm INPUT)
    const float* gamma;  // [N]
    const float* beta;   // [N]      (only read when relu)
    float* dX;           // [M, N]
    float* stats;        // [M, 2] (mean, rstd): the start of the workspace
    long long M;
    int N, relu;
    float eps;
};

__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(const LnBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.M) return;
    constexpr int MAXV = 4;
    const int nvec = a.N / 4;
    float4 x[MAXV];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXV; ++c) {
        const int i4 = lane + 64 * c;
        x[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i4 < nvec) {
            x[c] = *reinterpret_cast<const float4*>(a.X + row * a.N + i4 * 4);
            s += (x[c].x + x[c].y) + (x[c].z + x[c].w);
        }
    }
    s = sbev::wave_sum_dpp(s);
    const float mean = s / (float)a.N;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < MAXV; ++c)
        if (lane + 64 * c < nvec) {
            const float dx = x[c].x - mean, dy = x[c].y - mean, dz = x[c].z - mean, dw = x[c].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    q = sbev::wave_sum_dpp(q);
    const float rstd = rsqrtf(q / (float)a.N + a.eps);
    float dh[MAXV][4], xh[MAXV][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < MAXV; ++c) {
        const int i4 = lane + 64 * c;
        if (i4 < nvec) {
            const float4 g4 = *reinterpret_cast<const float4*>(a.dY + row * a.N + i4 * 4);
            const float4 w4 = *reinterpret_cast<const float4*>(a.gamma + i4 * 4);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, wv[4] = {w4.x, w4.y, w4.z, w4.w};
            const float xv[4] = {x[c].x, x[c].y, x[c].z, x[c].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float h = (xv[e] - mean) * rstd;
                float g = gv[e];
                if (a.relu && !(h * wv[e] + a.beta[i4 * 4 + e] > 0.f)) g = 0.f;
                xh[c][e] = h;
                dh[c][e] = g * wv[e];
                s1 += dh[c][e];
                s2 += dh[c][e] * h;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[c][e] = dh[c][e] = 0.f;
        }
    }
    s1 = sbev::wave_sum_dpp(s1) / (float)a.N;
    s2 = sbev::wave_sum_dpp(s2) / (float)a.N;
#pragma unroll
    for (int c = 0; c < MAXV; ++c) {
        const int i4 = lane + 64 * c;
        if (i4 < nvec) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = rstd * (dh[c][e] - s1 - xh[c][e] * s2);
            *reinterpret_cast<float4*>(a.dX + row * a.N + i4 * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    if (lane == 0) {
        a.stats[row * 2] = mean;
        a.stats[row * 2 + 1] = rstd;
    }
}

// ---- column sums: bias gradients, LayerNorm dgamma / dbeta ------------------------------------------------------------
// Every column reduction of the training step is  term x walk x finish, each stated once:
//   term    what row m of column n adds up.  BiasTerm: dZ = dY * (Y > 0) (Y = the forward OUTPUT of a ReLU; null -> dZ = dY), stored
//           if dZ is given, one addend.  LnTerm: g * xhat and g, the ReLU mask recomputed from the rows' (mean, rstd).  PlainTerm: a load.
//   walk    a lane takes rows rg, rg + LANES, ..: R rows per trip with their loads issued together, the trip's addends joined by
//           a pairwise halving tree or one after another in row order, then added to the running sum; tail rows one at a time.
//   finish  one launch (lane_sum_kernel): block = 64 columns x 16 row lanes, the 16 sums added in lane order from 0.f through
//           LDS, result (+)= out.  Or two passes (chunk_partial_kernel, chunk_sum_kernel): block = 64 columns x 4 row lanes
//           over a chunk of ROW_CHUNK rows writes (r0 + r1) + (r2 + r3) into one partial row, the chunks are added in order.
// The sequence of fp32 additions behind an output element is part of the contract (a step's gradients are compared bit for bit across
// changes), so R and the join belong to the entry point: bias 4 rows / tree, sbev_colsum_group 8 / tree, LayerNorm 4 / in row order.
// All of it is deterministic: no atomics.
//
// Two passes are for many rows: one block per 64 columns over ALL rows was 4 workgroups for a 256-wide Linear, 73 us for 0.9 MB.
// Up to ONE_PASS_ROWS rows (the decoder's B*Q = 900) the one launch takes 8 us instead of two of 7.9 + 7.6 (round 3: 222 of a
// training step's ~1100 launches were this pair).  The grouped entry points put up to 16 biases / 8 LayerNorms, each summed over up to 8
// segments (the layers of a decoder call that share the parameter), into one launch: per layer and bias it was one 10 us launch, 66
// of a training step's launches.  sbev_layer_norm_bwd's one launch is the grouped LayerNorm launch with one group of one segment.
constexpr int ROW_CHUNK = 32;     // rows per partial-sum block: 8 dependent iterations per thread (128 measured 13.7 us for a 900 x 256 gradient)
constexpr int ONE_PASS_ROWS = 2048;

// rows<R>(m, step, v): the addends v[i][..] of rows m + step * i, i < R, of the term's column.  (The element index stays
// (m + step * i) * ld + n: written as m * ld + n + (step * ld) * i the compiler kept the bias term's twelve pointers in SGPRs and
// advanced them with 24 scalar adds behind the trip's wait, 0.7 us on a 12 us launch.)
struct BiasTerm {
    static constexpr int K = 1;
    const float* dY;     // [M, ld]
    const float* Y;      // [M, ld] or null
    float* dZ;           // [M, ld] or null (may alias dY)
    long long ld;
    int n;
    template <int R>
    __device__ void rows(long long m, int step, float (&v)[R][K]) const {
#pragma unroll
        for (int i = 0; i < R; ++i) v[i][0] = dY[(m + step * i) * ld + n];
        if (Y) {
#pragma unroll
            for (int i = 0; i < R; ++i) if (!(Y[(m + step * i) * ld + n] > 0.f)) v[i][0] = 0.f;
        }
        if (dZ) {
#pragma unroll
            for (int i = 0; i < R; ++i) dZ[(m + step * i) * ld + n] = v[i][0];
        }
    }
};

struct LnTerm {
    static constexpr int K = 2;      // g * xhat (dgamma), g (dbeta)
    const float* dY;     // [M, N]
    const float* X;      // [M, N]
    const float* st;     // [M, 2] (mean, rstd) as ln_bwd_rows_kernel leaves them
    int N, n, relu;
    float w, bt;         // gamma[n]; beta[n] if relu
    template <int R>
    __device__ void rows(long long m, int step, float (&v)[R][K]) const {
        float h[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long long r = m + step * i;
            h[i] = (X[r * N + n] - st[r * 2]) * st[r * 2 + 1];
            v[i][1] = dY[r * N + n];
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (relu && !(h[i] * w + bt > 0.f)) v[i][1] = 0.f;
            v[i][0] = v[i][1] * h[i];
        }
    }
};

struct PlainTerm {
    static constexpr int K = 1;
    const float* p;      // [M, N]
    int N, n;
    template <int R>
    __device__ void rows(long long m, int step, float (&v)[R][K]) const {
#pragma unroll
        for (int i = 0; i < R; ++i) v[i][0] = p[(m + step * i) * N + n];
    }
};

// the pairwise halving tree over addend k of rows I0 .. I0 + R - 1.  R = 4: (v0 + v1) + (v2 + v3); R = 8: ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)).
// Depth first, as the written expression evaluates: level by level gives the same sum, but the 8-row loop's loads then lose their
// pointer chain (40 instead of 32 instructions).
template <int I0, int R, int RR, int K>
__device__ __forceinline__ float halves(const float (&v)[RR][K], int k) {
    static_assert((R & (R - 1)) == 0, "the halving tree wants a power of two");
    if constexpr (R == 1) return v[I0][k];
    else return halves<I0, R / 2>(v, k) + halves<I0 + R / 2, R / 2>(v, k);
}

// s += the addends of rows m, m + LANES, .. (R of them), joined by the tree or one after another
template <int LANES, int R, bool TREE, class Term>
__device__ __forceinline__ void trip(const Term& t, long long m, float (&s)[Term::K]) {
    float v[R][Term::K];
    t.template rows<R>(m, LANES, v);
#pragma unroll
    for (int k = 0; k < Term::K; ++k) {
        if (TREE) {
            s[k] += halves<0, R>(v, k);
        } else {
#pragma unroll
            for (int i = 0; i < R; ++i) s[k] += v[i][k];
        }
    }
}

// lane rg of LANES over the rows [m0, m1)
template <int LANES, int R, bool TREE, class Term>
__device__ __forceinline__ void walk(const Term& t, long long m0, long long m1, int rg, float (&s)[Term::K]) {
    long long m = m0 + rg;
    if constexpr (R > 1)
        for (; m + LANES * (R - 1) < m1; m += LANES * R) trip<LANES, R, TREE>(t, m, s);
    for (; m < m1; m += LANES) trip<LANES, 1, TREE>(t, m, s);
}

// A group = one parameter of N columns, summed over nseg segments of M rows each, blocks blk0 .. of its launch.  A group type names
// its term and the trip of its one-launch walk; term(n) is column n's term (what it loads of the parameter it loads once, not per
// segment: a dependent load of ~1 us each), seg(t, s) points it at segment s, dst(k) is where addend k's sums go.
template <int NSRC>
struct GroupBase {
    const float* src[NSRC][8];    // per segment: NSRC matrices
    int N, nseg, blk0, accumulate;
};
struct ColGroup : GroupBase<1> {                 // sbev_colsum_group
    using Term = PlainTerm;
    static constexpr int ROWS = 8;
    static constexpr bool TREE = true;
    float* out;
    __device__ Term term(int n) const { return {nullptr, N, n}; }
    __device__ void seg(Term& t, int s) const { t.p = src[0][s]; }
    __device__ float* dst(int) const { return out; }
};
struct LnGroup : GroupBase<3> {                  // src: dY, X, the [M, 2] row statistics
    using Term = LnTerm;
    static constexpr int ROWS = 4;
    static constexpr bool TREE = false;
    const float* gamma;
    const float* beta;
    float* dgamma;
    float* dbeta;
    int relu;
    __device__ Term term(int n) const { return {nullptr, nullptr, nullptr, N, n, relu, gamma[n], relu ? beta[n] : 0.f}; }
    __device__ void seg(Term& t, int s) const { t.dY = src[0][s]; t.X = src[1][s]; t.st = src[2][s]; }
    __device__ float* dst(int k) const { return k == 0 ? dgamma : dbeta; }
};
struct BiasGroup {                               // sbev_bias_relu_bwd: the only group of its launch, one segment
    using Term = BiasTerm;
    static constexpr int ROWS = 4;
    static constexpr bool TREE = true;
    const float* dY;
    const float* Y;
    float* dZ;
    float* out;          // db; two passes: the partial rows, null = no column sums wanted
    long long ld;
    int N, accumulate;
    static constexpr int nseg = 1, blk0 = 0;
    __device__ Term term(int n) const { return {dY, Y, dZ, ld, n}; }
    __device__ void seg(Term&, int) const {}
    __device__ float* dst(int) const { return out; }
};
template <class G, int MAXG>
struct Groups {
    G g[MAXG];
    int ng;
    long long M;
};

template <class G, int MAXG>
__global__ __launch_bounds__(1024) void lane_sum_kernel(const Groups<G, MAXG> a) {
    constexpr int K = G::Term::K;
    __shared__ float red[K][16][64];
    int gi = 0;
    if constexpr (MAXG > 1)
        for (int i = 1; i < a.ng; ++i)
            if ((int)blockIdx.x >= a.g[i].blk0) gi = i;
    const G& g = a.g[gi];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int n = ((int)blockIdx.x - g.blk0) * 64 + c;
    float s[K] = {};
    if (n < g.N) {
        auto t = g.term(n);
        for (int sgi = 0; sgi < g.nseg; ++sgi) {
            g.seg(t, sgi);
            walk<16, G::ROWS, G::TREE>(t, 0, a.M, rg, s);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][rg][c] = s[k];
    __syncthreads();
    if (rg < K && n < g.N) {                     // wave k adds addend k's 16 lanes
        float t = 0.f;
#pragma unroll
        for (int l = 0; l < 16; ++l) t += red[rg][l][c];
        float* o = g.dst(rg) + n;
        *o = g.accumulate ? *o + t : t;
    }
}

// first of two passes: partial row blockIdx.y of dst(k) [chunks, N]
template <class G>
__global__ __launch_bounds__(256) void chunk_partial_kernel(const G g, const long long M) {
    constexpr int K = G::Term::K;
    __shared__ float red[K][4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const long long m0 = (long long)blockIdx.y * ROW_CHUNK, m1 = m0 + ROW_CHUNK < M ? m0 + ROW_CHUNK : M;
    float s[K] = {};
    if (n < g.N) {
        auto t = g.term(n);
        g.seg(t, 0);
        walk<4, 1, false>(t, m0, m1, rg, s);
    }
    if (!g.dst(0)) return;                       // dZ only
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][rg][c] = s[k];
    __syncthreads();
    if (rg == 0 && n < g.N) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            g.dst(k)[(long long)blockIdx.y * g.N + n] = (red[k][0][c] + red[k][1][c]) + (red[k][2][c] + red[k][3][c]);
    }
}

// out[k][n] (+)= sum_chunks part[k][chunk][n]  for K stacked partial sets (K = 1: bias; K = 2: dgamma, dbeta)
__global__ __launch_bounds__(256) void chunk_sum_kernel(const float* __restrict__ part, float* __restrict__ out0, float* __restrict__ out1,
                                                        int chunks, int N, int accumulate) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float* out = blockIdx.y == 0 ? out0 : out1;
    const float* p = part + (long long)blockIdx.y * chunks * N;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += p[(long long)c * N + n];
    out[n] = accumulate ? out[n] + s : s;
}

// ---- refine_bbox backward (models/sparsebev_transformer.py:155-160,179-183; models/utils.py:87-102) ----------------
struct RefineBwdArgs {
    const float* gout;     // [BQ,10]  grad of the refined box
    const float* out;      // [BQ,10]  the refined box (forward output: xyz = the sigmoid)
    const float* bbox;     // [BQ,10]  the proposal
    const float* vel_div;  // [B] or null
    float* greg;           // [BQ,10]
    float* gbbox;          // [BQ,10] or null (grad of the proposal: only xyz is non-zero)
    long long BQ;
    int Q;
};

__global__ __launch_bounds__(256) void refine_bwd_kernel(const RefineBwdArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.BQ) return;
    const float* go = a.gout + i * 10;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float s = a.out[i * 10 + d];
        const float gz = go[d] * s * (1.f - s);
        a.greg[i * 10 + d] = gz;
        if (a.gbbox) {
            const float p = a.bbox[i * 10 + d];
            float g = 0.f;
            if (p >= 0.f && p <= 1.f) {                       // clamp(0, 1) passes the gradient inside the range only
                if (p >= 1e-5f) g += 1.f / p;                  // d log(max(p, eps)) / dp
                if (1.f - p >= 1e-5f) g += 1.f / (1.f - p);    // - d log(max(1 - p, eps)) / dp
            }
            a.gbbox[i * 10 + d] = gz * g;
        }
    }
    for (int d = 3; d < 10; ++d) {
        float g = go[d];
        if (d >= 8 && a.vel_div) g = g / a.vel_div[(unsigned)i / (unsigned)a.Q];
        a.greg[i * 10 + d] = g;
        if (a.gbbox) a.gbbox[i * 10 + d] = 0.f;
    }
}

// ---- projection + view selection backward (models/sparsebev_sampling.py:49-114) ------------------------------------
// One thread per (b, t, q, gp): re-run the forward's projection into the N cameras (same individually rounded
// expressions as project.hip, so the same first-hit camera is selected), then
//   u = (uh / hn) / W,  hn = max(hm, eps):   d/duh = 1 / (hn W);   d/dhm = -(uh / hn^2) / W  if hm > eps else 0
// (torch.maximum passes the gradient to the larger argument), chained through the selected camera's 4x4 matrix.
struct ProjBwdArgs {
    const float* pts;       // [B,Q,T,GP,3]
    const float* l2i;       // [B,T*N,4,4]
    const float* gloc;      // [B*T*G,Q,P,3]  (x, y used)
    float* gpts;            // [B,Q,T,GP,3]
    int B, Q, T, N, G, P;
    float image_h, image_w, eps;
};

__global__ __launch_bounds__(256) void project_bwd_kernel(const ProjBwdArgs a) {
    const int GP = a.G * a.P;
    const long long total = (long long)a.B * a.T * a.Q * GP;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const unsigned ui = (unsigned)idx;
    unsigned r = ui / (unsigned)GP;
    const int gp = (int)(ui - r * (unsigned)GP);
    const unsigned r2 = r / (unsigned)a.Q;
    const int q = (int)(r - r2 * (unsigned)a.Q);
    const int b = (int)(r2 / (unsigned)a.T);
    const int t = (int)(r2 - (unsigned)b * (unsigned)a.T);
    const long long pi = ((((long long)b * a.Q + q) * a.T + t) * GP + gp) * 3;
    const float x = a.pts[pi], y = a.pts[pi + 1], z = a.pts[pi + 2];
    int view = 0;
    bool found = false;
    float s_uh = 0.f, s_vh = 0.f, s_hm = 0.f;
    for (int n = 0; n < a.N; ++n) {
        const float* m = a.l2i + (((long long)b * a.T + t) * a.N + n) * 16;
        const float uh = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
        const float vh = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[4], x), __fmul_rn(m[5], y)), __fmul_rn(m[6], z)), m[7]);
        const float hm = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[8], x), __fmul_rn(m[9], y)), __fmul_rn(m[10], z)), m[11]);
        const float hn = fmaxf(hm, a.eps);
        const float u = __fdiv_rn(__fdiv_rn(uh, hn), a.image_w);
        const float v = __fdiv_rn(__fdiv_rn(vh, hn), a.image_h);
        const bool valid = (hm > a.eps) && (v > 0.f) && (v < 1.f) && (u > 0.f) && (u < 1.f);
        if (n == 0 || (valid && !found)) { s_uh = uh; s_vh = vh; s_hm = hm; view = n; }
        found = found || valid;
    }
    const int g = gp / a.P, p = gp - g * a.P;
    const float* gl = a.gloc + (((((long long)b * a.T + t) * a.G + g) * a.Q + q) * a.P + p) * 3;
    const float gu = gl[0], gv = gl[1];
    const float hn = fmaxf(s_hm, a.eps);
    const float g_uh = gu / (hn * a.image_w), g_vh = gv / (hn * a.image_h);
    const float g_hm = s_hm > a.eps ? -(g_uh * s_uh + g_vh * s_vh) / hn : 0.f;
    const float* m = a.l2i + (((long long)b * a.T + t) * a.N + view) * 16;
    a.gpts[pi] = g_uh * m[0] + g_vh * m[4] + g_hm * m[8];
    a.gpts[pi + 1] = g_uh * m[1] + g_vh * m[5] + g_hm * m[9];
    a.gpts[pi + 2] = g_uh * m[2] + g_vh * m[6] + g_hm * m[10];
}

// ---- sample-point generation + level softmax backward (models/sparsebev_transformer.py:270-311) ---------------------
// Per query: each of its G*P points sums its gradient over the T warped copies (which share the un-warped point) and emits
// its offset / logit gradients; the 8 box gradients (centre, log-dims, sin, cos) are summed over the points.
// Velocity is detached in the reference (:288) -> no gradient to columns 8, 9.
struct FrontBwdArgs {
    const float* bbox;      // [B,Q,10]
    const float* offset;    // [B*Q, ld_off]
    const float* logits;    // [B*Q, ld_logit]
    long long ld_off, ld_logit;
    const float* gpts;      // [B,Q,T,GP,3] or null
    const float* gw_bp;     // [B*G*T,Q,P,L] or null
    float* goffset;         // [B*Q, ld_g] (first GP*3 columns)
    float* glogits;         // [B*Q, ld_g] (first GP*L columns)
    long long ld_g;
    float* gbbox;           // [B*Q, 10] or null
    float pc_span[3];
    int B, Q, T, G, P, L;
    float rot_sign;
};

// one wave per (b, q), lane = sample point gp (G*P <= 64): per-point work in parallel, the 8 box gradients reduced over the
// wave with DPP sums (one THREAD per query walking its 16 points x T frames serially took 139 us at config 2)
__global__ __launch_bounds__(256) void front_bwd_kernel(const FrontBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const long long bq = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bq >= (long long)a.B * a.Q) return;
    const int GP = a.G * a.P;
    const int gp = lane;
    const bool act = gp < GP;
    const int b = (int)((unsigned)bq / (unsigned)a.Q), q = (int)((unsigned)bq - (unsigned)b * (unsigned)a.Q);
    const float* bb = a.bbox + bq * 10;
    float gb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (a.gpts) {
        const float s = bb[6], c = bb[7];
        // cos, sin of atan2(s, c) are c / r, s / r.  Going through the fp32 angle rounds it by up to half an ulp of pi (1.2e-7), and
        // the yaw gradient multiplies that by the un-cancelled sums over the points of g_cs, g_sn -- several times the column's own
        // rounding error.  Only where r2 leaves the normal range (or s = c = 0) the angle is taken, as the forward takes it.
        const float r2 = s * s + c * c;
        float cs, sn_raw;
        if (r2 > 1e-30f && r2 < 1e30f) {
            const float r = sqrtf(r2);
            cs = c / r; sn_raw = s / r;
        } else {
            const float yaw = atan2f(s, c);
            cs = cosf(yaw); sn_raw = sinf(yaw);
        }
        const float sn = a.rot_sign * sn_raw;
        const float ew = expf(bb[3]), el = expf(bb[4]), eh = expf(bb[5]);
        float g_yaw = 0.f;
        if (act) {
            float gx = 0.f, gy = 0.f, gz = 0.f;
            for (int t = 0; t < a.T; ++t) {
                const float* gpt = a.gpts + ((bq * a.T + t) * GP + gp) * 3;
                gx += gpt[0]; gy += gpt[1]; gz += gpt[2];
            }
            const float* of = a.offset + bq * a.ld_off + gp * 3;
            const float dx = ew * of[0], dy = el * of[1], dz = eh * of[2];
            // px = cx + (dx cs - dy sn), py = cy + (dx sn + dy cs), pz = cz + dz
            const float g_dx = gx * cs + gy * sn, g_dy = -gx * sn + gy * cs;
            float* go = a.goffset + bq * a.ld_g + gp * 3;
            go[0] = g_dx * ew; go[1] = g_dy * el; go[2] = gz * eh;
            gb[0] = gx; gb[1] = gy; gb[2] = gz;
            gb[3] = g_dx * dx; gb[4] = g_dy * dy; gb[5] = gz * dz;
            const float g_cs = gx * dx + gy * dy, g_sn = -gx * dy + gy * dx;
            g_yaw = g_cs * (-sn_raw) + g_sn * a.rot_sign * cs;
        }
#pragma unroll
        for (int d = 0; d < 6; ++d) gb[d] = sbev::wave_sum_dpp(gb[d]);
        g_yaw = sbev::wave_sum_dpp(g_yaw);
        gb[6] = g_yaw * c / r2;
        gb[7] = -g_yaw * s / r2;
        gb[0] *= a.pc_span[0]; gb[1] *= a.pc_span[1]; gb[2] *= a.pc_span[2];
    } else if (act) {
        for (int i = 0; i < 3; ++i) a.goffset[bq * a.ld_g + gp * 3 + i] = 0.f;
    }
    if (a.gbbox && lane == 0) {
#pragma unroll
        for (int d = 0; d < 8; ++d) a.gbbox[bq * 10 + d] = gb[d];
        a.gbbox[bq * 10 + 8] = 0.f;
        a.gbbox[bq * 10 + 9] = 0.f;
    }
    if (!act) return;
    float* gl = a.glogits + bq * a.ld_g + gp * a.L;
    if (!a.gw_bp) {
        for (int l = 0; l < a.L; ++l) gl[l] = 0.f;
        return;
    }
    const int g = gp / a.P, p = gp - g * a.P;
    const float* lg = a.logits + bq * a.ld_logit + gp * a.L;
    float mx = lg[0];
    for (int l = 1; l < a.L; ++l) mx = fmaxf(mx, lg[l]);
    float e[SBEV_MAX_LEVELS], gs[SBEV_MAX_LEVELS];
    float sum = 0.f;
    for (int l = 0; l < a.L; ++l) {
        e[l] = expf(lg[l] - mx);
        sum += e[l];
        gs[l] = 0.f;
    }
    // the softmax of (g, p) was replicated into the T weight rows r = (b*G + g)*T + t' (forward kernel): sum their grads
    for (int tp = 0; tp < a.T; ++tp) {
        const long long row = ((long long)b * a.G + g) * a.T + tp;
        const float* gw = a.gw_bp + ((row * a.Q + q) * a.P + p) * a.L;
        for (int l = 0; l < a.L; ++l) gs[l] += gw[l];
    }
    float dot = 0.f;
    for (int l = 0; l < a.L; ++l) dot += (e[l] / sum) * gs[l];
    for (int l = 0; l < a.L; ++l) gl[l] = (e[l] / sum) * (gs[l] - dot);
}

// ---- dropout (training only; mmcv MultiheadAttention / FFN: models/sparsebev_transformer.py:125,202) ----------------
// Counter-based: the keep decision of element i is a hash of (seed, i), so the backward regenerates the mask instead of
// storing it.  y = x * keep / (1 - p).
__device__ __forceinline__ unsigned mix32(unsigned long long z) {       // splitmix64 finaliser
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (unsigned)((z ^ (z >> 31)) >> 32);
}

__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long long n,
                                                      unsigned long long seed, const unsigned long long* seed_dev, float p, float scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned thr = (unsigned)((double)p * 4294967296.0);
    if (seed_dev) seed += *seed_dev;        // captured training steps: the part of the seed that changes from replay to replay
    y[i] = mix32(seed * 0x100000001b3ull + (unsigned long long)i) >= thr ? x[i] * scale : 0.f;
}

}  // namespace

extern "C" int64_t sbev_colsum_workspace(int64_t M, int N) {
    if (M < 0 || N < 0) return -1;
    return ((M + ROW_CHUNK - 1) / ROW_CHUNK) * (int64_t)N * (int64_t)sizeof(float);
}

static int bias_relu_bwd_impl(const float* dY, const float* Y, float* dZ, float* db, int64_t M, int N, int64_t ld,
                              float* workspace, int accumulate, sbev_stream_t stream) {
    SBEV_REQUIRE(M >= 0 && N >= 0 && ld >= N, "sbev_bias_relu_bwd: bad sizes");
    if (N == 0) return SBEV_OK;
    SBEV_REQUIRE(dY != nullptr && (!db || workspace), "sbev_bias_relu_bwd: null grad / workspace");
    const int chunks = (int)((M + ROW_CHUNK - 1) / ROW_CHUNK);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 cols((unsigned)((N + 63) / 64));
    if (db && M > 0 && M <= ONE_PASS_ROWS) {
        const Groups<BiasGroup, 1> a{{{dY, Y, dZ, db, ld, N, accumulate}}, 1, M};
        hipLaunchKernelGGL((lane_sum_kernel<BiasGroup, 1>), cols, dim3(1024), 0, s, a);
        return sbev::check_launch("sbev_bias_relu_bwd");
    }
    if (chunks > 0) {
        SBEV_REQUIRE(chunks <= 65535, "sbev_bias_relu_bwd: too many rows");
        const BiasGroup g{dY, Y, dZ, db ? workspace : nullptr, ld, N, 0};
        hipLaunchKernelGGL(chunk_partial_kernel<BiasGroup>, dim3(cols.x, (unsigned)chunks), dim3(256), 0, s, g, (long long)M);
        int st = sbev::check_launch("sbev_bias_relu_bwd");
        if (st != SBEV_OK) return st;
    }
    if (db) {
        hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)((N + 255) / 256), 1), dim3(256), 0, s, workspace, db, db, chunks, N, accumulate);
        return sbev::check_launch("sbev_bias_relu_bwd (sum)");
    }
    return SBEV_OK;
}

extern "C" int sbev_bias_relu_bwd(const float* dY, const float* Y, float* dZ, float* db, int64_t M, int N, int64_t ld,
                                  float* workspace, sbev_stream_t stream) {
    return bias_relu_bwd_impl(dY, Y, dZ, db, M, N, ld, workspace, 0, stream);
}
// the same with the column sums ADDED to db (accumulate != 0): one parameter used by several layers of a call (autograd.ParamTap)
extern "C" int sbev_bias_relu_bwd_acc(const float* dY, const float* Y, float* dZ, float* db, int64_t M, int N, int64_t ld,
                                      float* workspace, int accumulate, sbev_stream_t stream) {
    return bias_relu_bwd_impl(dY, Y, dZ, db, M, N, ld, workspace, accumulate, stream);
}

// What every group of a grouped launch has: sizes, flags, its first block (blk: the launch's block count so far) and its segments'
// pointers, from the host arrays srcs[i] [ng][8] (row b: group b's nseg_b pointers first).  own = group b's own pointers are there.
template <int NSRC>
static int fill_group(GroupBase<NSRC>& g, int& blk, const char* who, int b, bool own, const float* const* const (&srcs)[NSRC],
                      const int32_t* Ns, const int32_t* nsegs, const int32_t* accumulate) {
    SBEV_REQUIRE(Ns[b] >= 1 && nsegs[b] >= 1 && nsegs[b] <= 8 && own, "%s: group %d", who, b);
    g.N = Ns[b]; g.nseg = nsegs[b]; g.blk0 = blk; g.accumulate = accumulate[b];
    for (int s = 0; s < g.nseg; ++s)
        for (int i = 0; i < NSRC; ++i) {
            SBEV_REQUIRE(srcs[i][b * 8 + s], "%s: null segment", who);
            g.src[i][s] = srcs[i][b * 8 + s];
        }
    blk += (g.N + 63) / 64;
    return SBEV_OK;
}

// dX and the row statistics only (no dgamma / dbeta): the first half of sbev_layer_norm_bwd, for callers that sum the parameter
// gradients later with sbev_layer_norm_param_group.  workspace: >= 2 M floats, receives [M, 2] (mean, rstd).
extern "C" int sbev_layer_norm_bwd_rows(const float* dY, const float* X, const float* gamma, const float* beta, float eps, int relu,
                                        float* dX, float* workspace, int64_t M, int N, sbev_stream_t stream) {
    SBEV_REQUIRE(M >= 0 && N >= 4 && N % 4 == 0 && N <= 1024, "sbev_layer_norm_bwd_rows: N=%d must be a multiple of 4 in 4..1024", N);
    if (M == 0) return SBEV_OK;
    SBEV_REQUIRE(dY && X && gamma && dX && workspace && (!relu || beta), "sbev_layer_norm_bwd_rows: null pointer");
    LnBwdArgs a{dY, X, gamma, beta, dX, workspace, M, N, relu, eps};
    hipLaunchKernelGGL(ln_bwd_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_layer_norm_bwd_rows");
}

// dgamma_b / dbeta_b (+)= sums over the nseg_b (dY, X, stats) triples of LayerNorm b, ng <= 8 LayerNorms in one launch.
// dYs / Xs / stats: host arrays [ng][8] of device pointers; gammas / betas / dgammas / dbetas: [ng]; Ns / nsegs / relus / accumulate: [ng]
extern "C" int sbev_layer_norm_param_group(const float* const* dYs, const float* const* Xs, const float* const* stats,
                                           const float* const* gammas, const float* const* betas, float* const* dgammas, float* const* dbetas,
                                           const int32_t* Ns, const int32_t* nsegs, const int32_t* relus, const int32_t* accumulate,
                                           int ng, int64_t M, sbev_stream_t stream) {
    SBEV_REQUIRE(ng >= 0 && ng <= 8 && M >= 0, "sbev_layer_norm_param_group: at most 8 groups");
    if (ng == 0) return SBEV_OK;
    SBEV_REQUIRE(dYs && Xs && stats && gammas && betas && dgammas && dbetas && Ns && nsegs && relus && accumulate, "sbev_layer_norm_param_group: null pointer");
    Groups<LnGroup, 8> a{};
    a.ng = ng; a.M = M;
    const float* const* const srcs[3] = {dYs, Xs, stats};
    int blk = 0;
    for (int b = 0; b < ng; ++b) {
        LnGroup& g = a.g[b];
        int st = fill_group(g, blk, "sbev_layer_norm_param_group", b, gammas[b] && dgammas[b] && dbetas[b] && (!relus[b] || betas[b]),
                            srcs, Ns, nsegs, accumulate);
        if (st != SBEV_OK) return st;
        g.gamma = gammas[b]; g.beta = betas[b]; g.dgamma = dgammas[b]; g.dbeta = dbetas[b]; g.relu = relus[b];
    }
    hipLaunchKernelGGL((lane_sum_kernel<LnGroup, 8>), dim3((unsigned)blk), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_layer_norm_param_group");
}

// out_b[n] (+)= sum over the nseg_b matrices seg_b[s] [M, N_b] (row-major, contiguous) of their column sums, for ng <= 16 groups b:
// segs = host array of ng * 8 device pointers (row b: its nseg_b pointers first), outs / Ns / nsegs / accumulate = host arrays [ng]
extern "C" int sbev_colsum_group(const float* const* segs, float* const* outs, const int32_t* Ns, const int32_t* nsegs,
                                 const int32_t* accumulate, int ng, int64_t M, sbev_stream_t stream) {
    SBEV_REQUIRE(ng >= 0 && ng <= 16 && M >= 0, "sbev_colsum_group: at most 16 groups");
    if (ng == 0) return SBEV_OK;
    SBEV_REQUIRE(segs && outs && Ns && nsegs && accumulate, "sbev_colsum_group: null pointer");
    Groups<ColGroup, 16> a{};
    a.ng = ng; a.M = M;
    const float* const* const srcs[1] = {segs};
    int blk = 0;
    for (int b = 0; b < ng; ++b) {
        int st = fill_group(a.g[b], blk, "sbev_colsum_group", b, outs[b] != nullptr, srcs, Ns, nsegs, accumulate);
        if (st != SBEV_OK) return st;
        a.g[b].out = outs[b];
    }
    hipLaunchKernelGGL((lane_sum_kernel<ColGroup, 16>), dim3((unsigned)blk), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_colsum_group");
}

extern "C" int64_t sbev_layer_norm_bwd_workspace(int64_t M, int N) {
    if (M < 0 || N < 0) return -1;
    return (2 * M + 2 * ((M + ROW_CHUNK - 1) / ROW_CHUNK) * (int64_t)N) * (int64_t)sizeof(float);
}

// workspace: [M, 2] (mean, rstd), then (two passes) [2][chunks][N] partial column sums
static int layer_norm_bwd_impl(const float* dY, const float* X, const float* gamma, const float* beta, float eps, int relu,
                               float* dX, float* dgamma, float* dbeta, float* workspace, int64_t M, int N, int accumulate, sbev_stream_t stream) {
    SBEV_REQUIRE(M >= 0 && N >= 4 && N % 4 == 0 && N <= 1024, "sbev_layer_norm_bwd: N=%d must be a multiple of 4 in 4..1024", N);
    SBEV_REQUIRE(dY && X && gamma && dX && dgamma && dbeta && workspace && (!relu || beta), "sbev_layer_norm_bwd: null pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int chunks = (int)((M + ROW_CHUNK - 1) / ROW_CHUNK);
    SBEV_REQUIRE(chunks <= 65535, "sbev_layer_norm_bwd: too many rows");
    float* part = workspace + 2 * M;
    if (M > 0) {
        LnBwdArgs a{dY, X, gamma, beta, dX, workspace, M, N, relu, eps};
        hipLaunchKernelGGL(ln_bwd_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, a);
        int st = sbev::check_launch("sbev_layer_norm_bwd (rows)");
        if (st != SBEV_OK) return st;
        const bool one = M <= ONE_PASS_ROWS;      // the grouped launch over this one (dY, X, statistics) triple, or partial rows
        Groups<LnGroup, 8> ga{};
        ga.ng = 1; ga.M = M;
        LnGroup& g = ga.g[0];
        g.src[0][0] = dY; g.src[1][0] = X; g.src[2][0] = workspace;
        g.N = N; g.nseg = 1; g.blk0 = 0; g.accumulate = one ? accumulate : 0;
        g.gamma = gamma; g.beta = beta; g.relu = relu;
        g.dgamma = one ? dgamma : part; g.dbeta = one ? dbeta : part + (int64_t)chunks * N;
        const dim3 cols((unsigned)((N + 63) / 64));
        if (one) {
            hipLaunchKernelGGL((lane_sum_kernel<LnGroup, 8>), cols, dim3(1024), 0, s, ga);
            return sbev::check_launch("sbev_layer_norm_bwd (columns)");
        }
        hipLaunchKernelGGL(chunk_partial_kernel<LnGroup>, dim3(cols.x, (unsigned)chunks), dim3(256), 0, s, g, (long long)M);
        st = sbev::check_launch("sbev_layer_norm_bwd (columns)");
        if (st != SBEV_OK) return st;
    }
    hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)((N + 255) / 256), 2), dim3(256), 0, s, part, dgamma, dbeta, chunks, N, accumulate);
    return sbev::check_launch("sbev_layer_norm_bwd (sum)");
}

extern "C" int sbev_layer_norm_bwd(const float* dY, const float* X, const float* gamma, const float* beta, float eps, int relu,
                                   float* dX, float* dgamma, float* dbeta, float* workspace, int64_t M, int N, sbev_stream_t stream) {
    return layer_norm_bwd_impl(dY, X, gamma, beta, eps, relu, dX, dgamma, dbeta, workspace, M, N, 0, stream);
}
// the same with dgamma / dbeta ADDED to (accumulate != 0)
extern "C" int sbev_layer_norm_bwd_acc(const float* dY, const float* X, const float* gamma, const float* beta, float eps, int relu,
                                       float* dX, float* dgamma, float* dbeta, float* workspace, int64_t M, int N, int accumulate,
                                       sbev_stream_t stream) {
    return layer_norm_bwd_impl(dY, X, gamma, beta, eps, relu, dX, dgamma, dbeta, workspace, M, N, accumulate, stream);
}

extern "C" int sbev_refine_bbox_bwd(const float* grad_out, const float* out, const float* query_bbox, const float* vel_div,
                                    float* grad_reg, float* grad_bbox, int B, int Q, sbev_stream_t stream) {
    SBEV_REQUIRE(B >= 0 && Q >= 0 && (int64_t)B * Q < 0x7fffffffLL, "sbev_refine_bbox_bwd: bad sizes");
    if (B == 0 || Q == 0) return SBEV_OK;
    SBEV_REQUIRE(grad_out && out && query_bbox && grad_reg, "sbev_refine_bbox_bwd: null pointer");
    RefineBwdArgs a{grad_out, out, query_bbox, vel_div, grad_reg, grad_bbox, (long long)B * Q, Q};
    hipLaunchKernelGGL(refine_bwd_kernel, dim3((unsigned)((a.BQ + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_refine_bbox_bwd");
}

extern "C" int sbev_project_select_bwd(const float* sample_points, const float* lidar2img, const float* grad_loc,
                                       int B, int Q, int T, int N, int G, int P, float image_h, float image_w, float eps,
                                       float* grad_points, sbev_stream_t stream) {
    SBEV_REQUIRE(B >= 0 && Q >= 0 && T >= 1 && N >= 1 && G >= 1 && P >= 1, "sbev_project_select_bwd: bad sizes");
    const long long total = (long long)B * T * Q * G * P;
    SBEV_REQUIRE(total < 0x7fffffffLL, "sbev_project_select_bwd: too many points");
    if (total == 0) return SBEV_OK;
    SBEV_REQUIRE(sample_points && lidar2img && grad_loc && grad_points, "sbev_project_select_bwd: null pointer");
    ProjBwdArgs a{sample_points, lidar2img, grad_loc, grad_points, B, Q, T, N, G, P, image_h, image_w, eps};
    hipLaunchKernelGGL(project_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_project_select_bwd");
}

extern "C" int sbev_sampling_front_bwd(const float* query_bbox, const float* offset, int64_t ld_off, const float* logits, int64_t ld_logit,
                                       const double* pc_range, int B, int Q, int T, int G, int P, int L,
                                       const float* grad_points, const float* grad_weights_bp,
                                       float* grad_offset, float* grad_logits, int64_t ld_grad, float* grad_bbox, sbev_stream_t stream) {
    SBEV_REQUIRE(B >= 0 && Q >= 0 && T >= 1 && G >= 1 && P >= 1 && L >= 1 && L <= SBEV_MAX_LEVELS, "sbev_sampling_front_bwd: bad sizes");
    if (B == 0 || Q == 0) return SBEV_OK;
    SBEV_REQUIRE((int64_t)B * Q < 0x7fffffffLL, "sbev_sampling_front_bwd: too many queries");
    SBEV_REQUIRE(query_bbox && offset && logits && pc_range && grad_offset && grad_logits, "sbev_sampling_front_bwd: null pointer");
    FrontBwdArgs a{};
    a.bbox = query_bbox; a.offset = offset; a.logits = logits; a.ld_off = ld_off; a.ld_logit = ld_logit;
    SBEV_REQUIRE(ld_grad >= (int64_t)G * P * 3 && ld_grad >= (int64_t)G * P * L, "sbev_sampling_front_bwd: ld_grad too small");
    a.gpts = grad_points; a.gw_bp = grad_weights_bp; a.goffset = grad_offset; a.glogits = grad_logits; a.ld_g = ld_grad; a.gbbox = grad_bbox;
    for (int d = 0; d < 3; ++d) a.pc_span[d] = (float)(pc_range[3 + d] - pc_range[d]);
    a.B = B; a.Q = Q; a.T = T; a.G = G; a.P = P; a.L = L;
    a.rot_sign = sbev::box_convention() == SBEV_BOX_V0_17_1 ? -1.f : 1.f;
    SBEV_REQUIRE(G * P <= 64, "sbev_sampling_front_bwd: G*P = %d sample points per query exceed one wave", G * P);
    const long long n = (long long)B * Q;
    hipLaunchKernelGGL(front_bwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_sampling_front_bwd");
}

extern "C" int sbev_dropout_f32(const float* x, float* y, int64_t n, uint64_t seed, float p, sbev_stream_t stream) {
    return sbev_dropout_f32_ds(x, y, n, seed, nullptr, p, stream);
}

extern "C" int sbev_dropout_f32_ds(const float* x, float* y, int64_t n, uint64_t seed, const uint64_t* seed_dev, float p, sbev_stream_t stream) {
    SBEV_REQUIRE(n >= 0 && p >= 0.f && p < 1.f, "sbev_dropout_f32: need 0 <= p < 1");
    if (n == 0) return SBEV_OK;
    SBEV_REQUIRE(x && y, "sbev_dropout_f32: null pointer");
    hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y,
                       (long long)n, (unsigned long long)seed, reinterpret_cast<const unsigned long long*>(seed_dev), p, 1.f / (1.f - p));
    return sbev::check_launch("sbev_dropout_f32");
}
