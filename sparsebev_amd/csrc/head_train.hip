// Training side of the detection head on the device: everything of SparseBEVHead's training step except the decoder itself
// and the linear-sum-assignment solve, which stays on the host like the reference's (hungarian_assigner_3d.py:72-80).
//
//   dn_prepare_kernel       denoising queries + matching queries + the [pad+Q, pad+Q] attention mask, one launch
//                           (models/sparsebev_head.py:119-222 with encode_bbox, models/bbox/utils.py:46-60)
//   dn_prepare_bwd_kernel   its backward: grad of init_query_bbox.weight and label_enc.weight, one owner per output element
//   match_cost_kernel       cost[l, b, q, g] of every decoder layer and sample in one launch: FocalLossCost + BBox3DL1Cost on
//                           normalize_bbox(gt) * code_weights, nan_to_num'ed (hungarian_assigner_3d.py:54-74, match_cost.py:6-27)
//   set_loss_kernel + set_loss_finish_kernel
//                           sigmoid focal loss + L1 loss of all layers AND their gradients for unit upstream gradient
//                           (models/sparsebev_head.py:239-275,349-402; mmdet FocalLoss / L1Loss restated)
//   capacity_plan_kernel    at a fixed ground-truth capacity: the dn codes, the four averaging factors and a status word from the
//                           device's gt_offsets, so that no host value follows the per-sample counts (models/sparsebev_head.py:
//                           224-237,247,371-384)
//   lsa_solve               rectangular linear sum assignment on the host (shortest augmenting paths, Jonker-Volgenant); no GPU call
//
// fp32 throughout, plain vector stores, NO float atomics: every sum has one owner and a fixed order (a serial loop, or a
// tree over LDS whose shape depends on the launch geometry only), so loss and gradients are bit-equal from run to run.
// Built with -ffp-contract=off: the noised centre `c + (u * (wlh / 2)) * s` and the normalisation `(x - lo) / span` round
// like the reference's separate torch ops.
//
// Averaging factors: mmdet versions that divide by `avg_factor + float32 eps` differ from the plain division done here by
// 1.2e-7 relative, below every tolerance of the tests.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "sbev_common.hpp"

namespace {

// ---- denoising queries ----------------------------------------------------------------------------------------------

struct DnArgs {
    const float* init_bbox;    // [Q, 10]
    const float* label_enc;    // [NC + 1, D - 1]
    const float* gt_boxes;     // [G, 9] gravity centre, w, l, h, rot, vx, vy; samples concatenated
    const int* gt_labels;      // [G]
    const int* gt_offsets;     // [B + 1] prefix sums of the per-sample counts
    const float* u_box;        // [N * G, 3] in [-1, 1)
    const float* u_lab;        // [N * G] in [0, 1)
    const int* new_lab;        // [N * G] in [0, NC)
    float* qbbox;              // [B, pad + Q, 10]
    float* qfeat;              // [B, pad + Q, D]
    int* noised_label;         // [N * G] the label whose embedding row the known query j = r * G + i got
    unsigned char* mask;       // [pad + Q, pad + Q] 1 = may not attend
    int B, Q, D, NC, G, N, single;
    float box_scale, label_scale;
    float lo[3], span[3];
};

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }     // NaN stays NaN, like torch.clamp

__global__ void dn_prepare_kernel(const DnArgs a) {
    const int pad = a.single * a.N, T = pad + a.Q, W = 10 + a.D;
    const long long nq = (long long)a.B * T * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) {
        const long long m = i - nq;
        if (m >= (long long)T * T) return;
        const int r = (int)(m / T), c = (int)(m % T);
        // a matching row sees no dn column; a dn row sees its own group's dn columns and every matching column (:195-207)
        a.mask[m] = (c < pad && (r >= pad || r / a.single != c / a.single)) ? 1 : 0;
        return;
    }
    const int b = (int)(i / ((long long)T * W));
    const int rem = (int)(i % ((long long)T * W));
    const int row = rem / W, col = rem % W;
    float* ob = a.qbbox + ((long long)b * T + row) * 10;
    float* of = a.qfeat + ((long long)b * T + row) * a.D;
    if (row >= pad) {                                           // the eval-branch rows (sbev_head_prepare)
        const int q = row - pad;
        if (col < 10) ob[col] = a.init_bbox[q * 10 + col];
        else of[col - 10] = col - 10 < a.D - 1 ? a.label_enc[(long long)a.NC * (a.D - 1) + col - 10] : 0.f;
        return;
    }
    const int r = row / a.single, k = row % a.single;
    const int g0 = a.gt_offsets[b], gb = a.gt_offsets[b + 1] - g0;
    if (k >= gb) {                                              // unused pad row
        if (col < 10) ob[col] = 0.f;
        else of[col - 10] = 0.f;
        return;
    }
    const int gi = g0 + k, j = r * a.G + gi;
    const float* gt = a.gt_boxes + (long long)gi * 9;
    if (col < 3) {
        float c = gt[col];
        if (a.box_scale > 0.f) c = c + (a.u_box[(long long)j * 3 + col] * (gt[3 + col] / 2.f)) * a.box_scale;      // :158-160
        ob[col] = clamp01((c - a.lo[col]) / a.span[col]);       // encode_bbox + clamp_ (:164-165)
    } else if (col < 6) {
        ob[col] = logf(gt[col]);
    } else if (col == 6) {
        ob[col] = sinf(gt[6]);
    } else if (col == 7) {
        ob[col] = cosf(gt[6]);
    } else if (col < 10) {
        ob[col] = gt[col - 1];
    } else {
        const int lab = (a.label_scale > 0.f && a.u_lab[j] < a.label_scale) ? a.new_lab[j] : a.gt_labels[gi];      // :169-173
        const int d = col - 10;
        if (d < a.D - 1) {
            of[d] = (lab >= 0 && lab <= a.NC) ? a.label_enc[(long long)lab * (a.D - 1) + d] : 0.f;
        } else {
            of[d] = 1.f;                                        // the DN indicator
            a.noised_label[j] = lab;
        }
    }
}

struct DnBwdArgs {
    const float* g_qbbox;      // [B, pad + Q, 10]
    const float* g_qfeat;      // [B, pad + Q, D]
    const int* noised_label;   // [N * G]
    const int* gt_offsets;     // [B + 1]
    float* g_init;             // [Q, 10]
    float* g_label;            // [NC + 1, D - 1]
    int B, Q, D, NC, G, N, single;
};

// blocks 0 .. NC: one embedding row each (256 columns x 4 row slices, combined in a fixed order); the blocks behind them: one
// thread per element of grad init_query_bbox, a serial sum over the samples
__global__ __launch_bounds__(1024) void dn_prepare_bwd_kernel(const DnBwdArgs a) {
    __shared__ float part[4][256];
    const int pad = a.single * a.N, T = pad + a.Q;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x > a.NC) {
        const long long e = (long long)(blockIdx.x - a.NC - 1) * 1024 + tid;
        if (e >= (long long)a.Q * 10) return;
        const int q = (int)(e / 10), c = (int)(e % 10);
        float s = 0.f;
        for (int b = 0; b < a.B; ++b) s += a.g_qbbox[((long long)b * T + pad + q) * 10 + c];
        a.g_init[e] = s;
        return;
    }
    const int cls = blockIdx.x, lane = tid & 255, slice = tid >> 8;
    const int Dm = a.D - 1;
    for (int d0 = 0; d0 < Dm; d0 += 256) {
        const int d = d0 + lane;
        float s = 0.f;
        if (d < Dm) {
            if (cls == a.NC) {                                  // the matching rows of every sample
                const int n = a.B * a.Q;
                for (int t = slice; t < n; t += 4) {
                    const int b = t / a.Q, q = t % a.Q;
                    s += a.g_qfeat[((long long)b * T + pad + q) * a.D + d];
                }
            } else {                                            // the known queries whose noised label is this class
                // The known queries are the (group r, gt gi) with gi < gt_offsets[B]; rows behind that of a fixed-capacity ground truth
                // are capacity, and the forward wrote no label for them.  The slices split the USED pairs, so the order of the sum
                // does not depend on the capacity (with G == gt_offsets[B], jc is j).
                int used = a.B > 0 ? a.gt_offsets[a.B] : 0;
                used = used < 0 ? 0 : (used > a.G ? a.G : used);
                const int n = a.N * used;
                for (int jc = slice; jc < n; jc += 4) {
                    const int r = jc / used, gi = jc % used;
                    if (a.noised_label[r * a.G + gi] != cls) continue;
                    int b = 0;
                    while (b + 1 < a.B && a.gt_offsets[b + 1] <= gi) ++b;
                    const int k = gi - a.gt_offsets[b];
                    s += a.g_qfeat[((long long)b * T + r * a.single + k) * a.D + d];
                }
            }
        }
        part[slice][lane] = s;
        __syncthreads();
        if (slice == 0 && d < Dm) a.g_label[(long long)cls * Dm + d] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        __syncthreads();
    }
}

// ---- targets ----------------------------------------------------------------------------------------------------------

// normalize_bbox (models/bbox/utils.py:4-20): (cx, cy, log w, log l, cz, log h, sin, cos, vx, vy)
__device__ __forceinline__ void normalize_gt(const float* gt, float* n) {
    n[0] = gt[0]; n[1] = gt[1]; n[2] = logf(gt[3]); n[3] = logf(gt[4]); n[4] = gt[2]; n[5] = logf(gt[5]);
    n[6] = sinf(gt[6]); n[7] = cosf(gt[6]); n[8] = gt[7]; n[9] = gt[8];
}

// sigmoid and softplus(x), softplus(-x) from one exp of -|x|
struct Sig { float p, q, sp_pos, sp_neg; };      // p = sigmoid(x), q = 1 - p, sp_pos = softplus(x) = -log(1 - p), sp_neg = softplus(-x) = -log p
__device__ __forceinline__ Sig sigmoid_parts(float x) {
    const float e = expf(-fabsf(x)), inv = 1.f / (1.f + e), l = log1pf(e);
    Sig s;
    s.p = x >= 0.f ? inv : e * inv;
    s.q = x >= 0.f ? e * inv : inv;
    s.sp_pos = fmaxf(x, 0.f) + l;
    s.sp_neg = fmaxf(-x, 0.f) + l;
    return s;
}

__device__ __forceinline__ float powg(float x, float gamma) { return gamma == 2.f ? x * x : powf(x, gamma); }

struct CostArgs {
    const float* cls;          // [L, B, ld_rows, NC] logits, pointer at the first matching row
    const float* box;          // [L, B, ld_rows, 10]
    const float* gt_boxes;
    const int* gt_labels;
    const int* gt_offsets;
    const float* code_weights; // [10]
    float* cost;               // [L, B, Q, Gmax]
    int L, B, Q, NC, Gmax, ld_rows;
    float w_cls, w_reg, alpha, gamma;
};

__global__ void match_cost_kernel(const CostArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.L * a.B * a.Q * a.Gmax;
    if (i >= total) return;
    const int g = (int)(i % a.Gmax);
    const long long row = i / a.Gmax;
    const int q = (int)(row % a.Q);
    const int lb = (int)(row / a.Q), b = lb % a.B;
    const int g0 = a.gt_offsets[b], gb = a.gt_offsets[b + 1] - g0;
    if (g >= gb) {
        a.cost[i] = 0.f;
        return;
    }
    const long long src = (long long)lb * a.ld_rows + q;
    const int lab = a.gt_labels[g0 + g];
    float cc = 0.f;
    if (lab >= 0 && lab < a.NC) {                               // FocalLossCost: p = sigmoid, eps = 1e-12, as written in fp32
        const float x = a.cls[src * a.NC + lab];
        const float p = 1.f / (1.f + expf(-x));
        const float neg = -logf(1.f - p + 1e-12f) * (1.f - a.alpha) * powg(p, a.gamma);
        const float pos = -logf(p + 1e-12f) * a.alpha * powg(1.f - p, a.gamma);
        cc = (pos - neg) * a.w_cls;
    }
    float n[10];
    normalize_gt(a.gt_boxes + (long long)(g0 + g) * 9, n);
    const float* pr = a.box + src * 10;
    float rc = 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const float w = a.code_weights[k];
        rc += fabsf(pr[k] * w - n[k] * w);
    }
    float c = cc + rc * a.w_reg;
    if (c != c) c = 100.f;                                      // nan_to_num(nan=100, posinf=100, neginf=-100) (:74)
    else if (c == INFINITY) c = 100.f;
    else if (c == -INFINITY) c = -100.f;
    a.cost[i] = c;
}

// ---- set loss ---------------------------------------------------------------------------------------------------------

struct LossArgs {
    const float* cls;          // [L, B, ld_rows, NC], pointer at the first row of the range
    const float* box;          // [L, B, ld_rows, 10]
    const int* codes;          // [L (stride code_ls, 0 = shared by the layers), B, R]: -2 skip, -1 background, g >= 0 target gt g of sample b
    const float* gt_boxes;
    const int* gt_labels;
    const int* gt_offsets;
    const float* code_weights;
    const float* avg;          // [2] A_cls, A_box (clamped to >= 1 here)
    float* d_cls;              // [L, B, R, NC]
    float* d_box;              // [L, B, R, 10]
    float* partial;            // [L, nblk, 2]
    int L, B, R, NC, ld_rows, nblk;
    long long code_ls;
    float w_fl, alpha, gamma, w_l1, scale;
};

__global__ __launch_bounds__(256) void set_loss_kernel(const LossArgs a) {
    __shared__ float red[2][256];
    const int l = blockIdx.y, tid = threadIdx.x;
    const int t = blockIdx.x * 256 + tid;                       // row (b, r) of this layer
    float s_cls = 0.f, s_box = 0.f;
    if (t < a.B * a.R) {
        const int b = t / a.R, r = t % a.R;
        const float inv_cls = 1.f / fmaxf(a.avg[0], 1.f), inv_box = 1.f / fmaxf(a.avg[1], 1.f);
        const float k_cls = a.w_fl * a.scale * inv_cls, k_box = a.w_l1 * a.scale * inv_box;
        const int g0 = a.gt_offsets[b], gb = a.gt_offsets[b + 1] - g0;
        int code = a.codes[(long long)l * a.code_ls + t];
        if (code >= gb) code = -2;                              // a caller's error (documented in the header): skip, never read past the gt
        const long long src = ((long long)l * a.B + b) * a.ld_rows + r;
        const long long dst = (long long)l * a.B * a.R + t;
        const float* x = a.cls + src * a.NC;
        float* dc = a.d_cls + dst * a.NC;
        float* db = a.d_box + dst * 10;
        if (code < -1) {
            for (int c = 0; c < a.NC; ++c) dc[c] = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) db[k] = 0.f;
        } else {
            const int lab = code >= 0 ? a.gt_labels[g0 + code] : -1;
            for (int c = 0; c < a.NC; ++c) {
                const Sig s = sigmoid_parts(x[c]);
                float f, d;
                if (c == lab) {                                 // t = 1: pt = 1 - p, bce = softplus(-x)
                    const float m = a.alpha * powg(s.q, a.gamma);
                    f = m * s.sp_neg;
                    d = m * (-a.gamma * s.p * s.sp_neg - s.q);
                } else {                                        // t = 0: pt = p, bce = softplus(x)
                    const float m = (1.f - a.alpha) * powg(s.p, a.gamma);
                    f = m * s.sp_pos;
                    d = m * (a.gamma * s.q * s.sp_pos + s.p);
                }
                s_cls += f;
                dc[c] = d * k_cls;
            }
            bool use = code >= 0;
            float n[10];
            if (use) {
                normalize_gt(a.gt_boxes + (long long)(g0 + code) * 9, n);
#pragma unroll
                for (int k = 0; k < 10; ++k) use = use && isfinite(n[k]);      // isnotnan (:389): the row still counts in A_box
            }
            const float* pr = a.box + src * 10;
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                float d = 0.f;
                if (use) {
                    const float w = a.code_weights[k], e = pr[k] - n[k];
                    s_box += fabsf(e) * w;
                    d = (e > 0.f ? w : (e < 0.f ? -w : 0.f)) * k_box;
                }
                db[k] = d;
            }
        }
    }
    red[0][tid] = s_cls;
    red[1][tid] = s_box;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                         // a tree of fixed shape: the same order on every run
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
        }
        __syncthreads();
    }
    if (tid < 2) a.partial[((long long)l * a.nblk + blockIdx.x) * 2 + tid] = red[tid][0];
}

struct FinishArgs {
    const float* partial;      // [L, nblk, 2]
    const float* avg;          // [2]
    float* loss;               // [L, 2] (loss_cls, loss_bbox)
    float* finite;             // [L, 2] 1 where the loss was finite before nan_to_num (its gradient mask), else 0
    int L, nblk;
    float w_fl, w_l1, scale;
};

__global__ void set_loss_finish_kernel(const FinishArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.L * 2) return;
    const int l = i >> 1, which = i & 1;
    float s = 0.f;
    for (int k = 0; k < a.nblk; ++k) s += a.partial[((long long)l * a.nblk + k) * 2 + which];
    float v = (which ? a.w_l1 : a.w_fl) * s / fmaxf(a.avg[which], 1.f);
    const bool fin = isfinite(v);
    if (v != v) v = 0.f;                                        // torch.nan_to_num defaults
    else if (v == INFINITY) v = std::numeric_limits<float>::max();
    else if (v == -INFINITY) v = -std::numeric_limits<float>::max();
    a.loss[i] = a.scale * v;
    a.finite[i] = fin ? 1.f : 0.f;
}

// ---- the step's plan at a fixed ground-truth capacity -------------------------------------------------------------------

struct PlanArgs {
    const int* gt_offsets;     // [B + 1]
    int* codes;                // [B, N * capacity]: k for k < count[b], else -2, tiled over the N groups
    float* avg;                // [2, 2]: (A_cls, A_box) of the matching loss, (A, A) of the denoising loss
    int* status;               // [1]: 0, or kPlan* bits
    int B, Q, capacity, N;
    double bg_cls_weight;
};

constexpr int kPlanCountAboveCapacity = 1, kPlanOffsetsNotMonotone = 2, kPlanTotalAboveCapacity = 4;
constexpr int kPlanThreads = 256;

__device__ __forceinline__ int plan_count(const int* offsets, int b, int capacity) {
    const int n = offsets[b + 1] - offsets[b];
    return n < 0 ? 0 : (n > capacity ? capacity : n);          // clamped: nothing this kernel writes follows a count out of range
}

// one thread per code; thread 0 of the launch also owns the four factors and the status: a serial loop over the samples, integer
// sums, the factors formed in double and rounded once to fp32 (what numpy does with the host's python floats)
__global__ __launch_bounds__(kPlanThreads) void capacity_plan_kernel(const PlanArgs a) {
    const long long i = (long long)blockIdx.x * kPlanThreads + threadIdx.x;
    const long long row = (long long)a.N * a.capacity;
    if (i < a.B * row) {
        const int b = (int)(i / row), k = (int)((i % row) % a.capacity);
        a.codes[i] = k < plan_count(a.gt_offsets, b, a.capacity) ? k : -2;
    }
    if (i != 0) return;
    long long num_pos = 0, total = 0;
    int st = a.gt_offsets[0] != 0 ? kPlanOffsetsNotMonotone : 0;
    for (int b = 0; b < a.B; ++b) {
        const int raw = a.gt_offsets[b + 1] - a.gt_offsets[b], n = plan_count(a.gt_offsets, b, a.capacity);
        if (raw > a.capacity) st |= kPlanCountAboveCapacity;
        if (raw < 0) st |= kPlanOffsetsNotMonotone;
        num_pos += n < a.Q ? n : a.Q;
        total += n;
    }
    if ((long long)a.gt_offsets[a.B] > (long long)a.B * a.capacity) st |= kPlanTotalAboveCapacity;
    const long long num_neg = (long long)a.B * a.Q - num_pos;
    a.avg[0] = (float)((double)num_pos * 1.0 + (double)num_neg * a.bg_cls_weight);
    a.avg[1] = (float)(double)num_pos;
    a.avg[2] = a.avg[3] = (float)(double)((long long)a.N * total);
    a.status[0] = st;
}

// ---- the host solver --------------------------------------------------------------------------------------------------

// Assign every one of `nr` <= `nc` rows to its own column at minimum total cost: shortest augmenting paths with dual variables
// (Jonker-Volgenant as restated by Crouse, "On implementing 2D rectangular assignment algorithms", 2016).  at(i, j): the cost.
template <typename At>
bool lsa_rows(int nr, int nc, At at, std::vector<int>& col4row) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> u(nr, 0.0), v(nc, 0.0), shortest(nc);
    std::vector<int> path(nc, -1), row4col(nc, -1), remaining(nc);
    std::vector<char> SR(nr), SC(nc);
    col4row.assign(nr, -1);
    for (int cur = 0; cur < nr; ++cur) {
        double min_val = 0.0;
        int i = cur, sink = -1, n_rem = nc;
        for (int j = 0; j < nc; ++j) remaining[j] = nc - j - 1;
        std::fill(SR.begin(), SR.end(), 0);
        std::fill(SC.begin(), SC.end(), 0);
        std::fill(shortest.begin(), shortest.end(), inf);
        while (sink == -1) {
            int index = -1;
            double lowest = inf;
            SR[i] = 1;
            for (int it = 0; it < n_rem; ++it) {
                const int j = remaining[it];
                const double r = min_val + at(i, j) - u[i] - v[j];
                if (r < shortest[j]) {
                    path[j] = i;
                    shortest[j] = r;
                }
                // among equally short columns prefer a free one: the path ends sooner
                if (shortest[j] < lowest || (shortest[j] == lowest && row4col[j] == -1)) {
                    lowest = shortest[j];
                    index = it;
                }
            }
            min_val = lowest;
            if (index < 0 || min_val == inf) return false;
            const int j = remaining[index];
            if (row4col[j] == -1) sink = j;
            else i = row4col[j];
            SC[j] = 1;
            remaining[index] = remaining[--n_rem];
        }
        u[cur] += min_val;
        for (int r = 0; r < nr; ++r)
            if (SR[r] && r != cur) u[r] += min_val - shortest[col4row[r]];
        for (int j = 0; j < nc; ++j)
            if (SC[j]) v[j] -= min_val - shortest[j];
        int j = sink;
        while (true) {
            const int r = path[j];
            row4col[j] = r;
            std::swap(col4row[r], j);
            if (r == cur) break;
        }
    }
    return true;
}

int lsa_solve(const float* cost, int64_t ld, int n_rows, int n_cols, int32_t* col_of_row, const char* who) {
    SBEV_REQUIRE(n_rows >= 0 && n_cols >= 0, "%s: bad sizes %d x %d", who, n_rows, n_cols);
    if (n_rows == 0) return SBEV_OK;
    SBEV_REQUIRE(col_of_row != nullptr, "%s: null col_of_row", who);
    for (int i = 0; i < n_rows; ++i) col_of_row[i] = -1;
    if (n_cols == 0) return SBEV_OK;
    SBEV_REQUIRE(cost != nullptr, "%s: null cost", who);
    SBEV_REQUIRE(ld >= n_cols, "%s: leading dimension %lld < n_cols %d", who, (long long)ld, n_cols);
    for (int i = 0; i < n_rows; ++i)
        for (int j = 0; j < n_cols; ++j)
            SBEV_REQUIRE(std::isfinite(cost[(int64_t)i * ld + j]), "%s: cost[%d, %d] is not finite", who, i, j);
    std::vector<int> match;
    bool ok;
    if (n_rows <= n_cols) {
        ok = lsa_rows(n_rows, n_cols, [&](int i, int j) { return (double)cost[(int64_t)i * ld + j]; }, match);
        if (ok)
            for (int i = 0; i < n_rows; ++i) col_of_row[i] = match[i];
    } else {                                                    // more rows than columns: assign the columns
        ok = lsa_rows(n_cols, n_rows, [&](int j, int i) { return (double)cost[(int64_t)i * ld + j]; }, match);
        if (ok)
            for (int j = 0; j < n_cols; ++j) col_of_row[match[j]] = j;
    }
    SBEV_REQUIRE(ok, "%s: no feasible assignment", who);
    return SBEV_OK;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int sbev_head_dn_prepare(const float* init_query_bbox, const float* label_enc, const float* gt_boxes, const int32_t* gt_labels,
                                    const int32_t* gt_offsets, const float* u_box, const float* u_lab, const int32_t* new_lab,
                                    const double* pc_range, float box_noise_scale, float label_noise_scale, int B, int Q, int D,
                                    int num_classes, int G, int N, int single, float* query_bbox, float* query_feat,
                                    int32_t* noised_label, uint8_t* attn_mask, sbev_stream_t stream) {
    SBEV_REQUIRE(B >= 0 && Q >= 0 && D >= 2 && num_classes >= 1 && G >= 0 && N >= 1 && single >= 0,
                 "sbev_head_dn_prepare: bad sizes B=%d Q=%d D=%d NC=%d G=%d N=%d single=%d", B, Q, D, num_classes, G, N, single);
    SBEV_REQUIRE(single <= G && (G == 0) == (single == 0), "sbev_head_dn_prepare: single=%d is not the largest per-sample count of G=%d", single, G);
    const long long T = (long long)single * N + Q;
    SBEV_REQUIRE(T <= 0x7fff && T * (10 + D) <= 0x7fffffffLL, "sbev_head_dn_prepare: %lld queries per sample is too many", T);
    if (B == 0 || T == 0) return SBEV_OK;
    SBEV_REQUIRE(init_query_bbox && label_enc && gt_offsets && pc_range && query_bbox && query_feat && attn_mask, "sbev_head_dn_prepare: null pointer");
    SBEV_REQUIRE(G == 0 || (gt_boxes && gt_labels && u_box && u_lab && new_lab && noised_label), "sbev_head_dn_prepare: null ground-truth / noise pointer");
    DnArgs a{};
    a.init_bbox = init_query_bbox; a.label_enc = label_enc; a.gt_boxes = gt_boxes; a.gt_labels = gt_labels; a.gt_offsets = gt_offsets;
    a.u_box = u_box; a.u_lab = u_lab; a.new_lab = new_lab; a.qbbox = query_bbox; a.qfeat = query_feat; a.noised_label = noised_label;
    a.mask = attn_mask;
    a.B = B; a.Q = Q; a.D = D; a.NC = num_classes; a.G = G; a.N = N; a.single = single;
    a.box_scale = box_noise_scale; a.label_scale = label_noise_scale;
    for (int i = 0; i < 3; ++i) {       // python-float scalars cast to fp32 by the tensor op (models/bbox/utils.py:52-54)
        a.lo[i] = (float)pc_range[i];
        a.span[i] = (float)(pc_range[3 + i] - pc_range[i]);
    }
    const long long total = (long long)B * T * (10 + D) + T * T;
    SBEV_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "sbev_head_dn_prepare: too many elements");
    hipLaunchKernelGGL(dn_prepare_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_head_dn_prepare");
}

extern "C" int sbev_head_dn_prepare_bwd(const float* grad_query_bbox, const float* grad_query_feat, const int32_t* noised_label,
                                        const int32_t* gt_offsets, int B, int Q, int D, int num_classes, int G, int N, int single,
                                        float* grad_init_query_bbox, float* grad_label_enc, sbev_stream_t stream) {
    SBEV_REQUIRE(B >= 0 && Q >= 0 && D >= 2 && num_classes >= 1 && G >= 0 && N >= 1 && single >= 0 && single <= G,
                 "sbev_head_dn_prepare_bwd: bad sizes B=%d Q=%d D=%d NC=%d G=%d N=%d single=%d", B, Q, D, num_classes, G, N, single);
    SBEV_REQUIRE(grad_init_query_bbox && grad_label_enc, "sbev_head_dn_prepare_bwd: null output");
    SBEV_REQUIRE(B == 0 || (grad_query_bbox && grad_query_feat && gt_offsets), "sbev_head_dn_prepare_bwd: null pointer");
    SBEV_REQUIRE(G == 0 || noised_label, "sbev_head_dn_prepare_bwd: null noised_label");
    DnBwdArgs a{grad_query_bbox, grad_query_feat, noised_label, gt_offsets, grad_init_query_bbox, grad_label_enc, B, Q, D, num_classes, G, N, single};
    const unsigned grid = (unsigned)(num_classes + 1) + blocks_of((long long)Q * 10, 1024);
    hipLaunchKernelGGL(dn_prepare_bwd_kernel, dim3(grid), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_head_dn_prepare_bwd");
}

extern "C" int sbev_head_match_cost(const float* cls_scores, const float* bbox_preds, int64_t ld_rows, const float* gt_boxes,
                                    const int32_t* gt_labels, const int32_t* gt_offsets, const float* code_weights, float w_cls,
                                    float w_reg, float alpha, float gamma, int L, int B, int Q, int num_classes, int Gmax, float* cost,
                                    sbev_stream_t stream) {
    SBEV_REQUIRE(L >= 0 && B >= 0 && Q >= 0 && num_classes >= 1 && Gmax >= 0 && ld_rows >= Q && ld_rows <= 0x7fffffffLL,
                 "sbev_head_match_cost: bad sizes L=%d B=%d Q=%d NC=%d Gmax=%d ld_rows=%lld", L, B, Q, num_classes, Gmax, (long long)ld_rows);
    const long long total = (long long)L * B * Q * Gmax;
    if (total == 0) return SBEV_OK;
    SBEV_REQUIRE(cls_scores && bbox_preds && gt_boxes && gt_labels && gt_offsets && code_weights && cost, "sbev_head_match_cost: null pointer");
    SBEV_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "sbev_head_match_cost: too many elements");
    CostArgs a{cls_scores, bbox_preds, gt_boxes, gt_labels, gt_offsets, code_weights, cost, L, B, Q, num_classes, Gmax, (int)ld_rows,
               w_cls, w_reg, alpha, gamma};
    hipLaunchKernelGGL(match_cost_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_head_match_cost");
}

extern "C" int sbev_head_capacity_plan(const int32_t* gt_offsets, int B, int Q, int capacity, int N, double bg_cls_weight, int32_t* codes,
                                       float* avg_factors, int32_t* status, sbev_stream_t stream) {
    SBEV_REQUIRE(B >= 0 && Q >= 0 && capacity >= 0 && N >= 1, "sbev_head_capacity_plan: bad sizes B=%d Q=%d capacity=%d N=%d", B, Q, capacity, N);
    const long long total = (long long)B * N * capacity;
    SBEV_REQUIRE(total <= 0x7fffffffLL && (long long)B * capacity <= 0x7fffffffLL && (long long)B * Q <= 0x7fffffffLL,
                 "sbev_head_capacity_plan: B=%d Q=%d capacity=%d N=%d is too large", B, Q, capacity, N);
    SBEV_REQUIRE(gt_offsets && avg_factors && status, "sbev_head_capacity_plan: null pointer");
    SBEV_REQUIRE(total == 0 || codes, "sbev_head_capacity_plan: null codes");
    PlanArgs a{gt_offsets, codes, avg_factors, status, B, Q, capacity, N, bg_cls_weight};
    const unsigned grid = total > 0 ? blocks_of(total, kPlanThreads) : 1u;       // the factors and the status are written at any size
    hipLaunchKernelGGL(capacity_plan_kernel, dim3(grid), dim3(kPlanThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    return sbev::check_launch("sbev_head_capacity_plan");
}

extern "C" int sbev_lsa_solve(const float* cost, int64_t ld, int n_rows, int n_cols, int32_t* col_of_row) {
    return lsa_solve(cost, ld, n_rows, n_cols, col_of_row, "sbev_lsa_solve");
}

extern "C" int sbev_head_assign(const float* cost, const int32_t* gt_counts, int L, int B, int Q, int Gmax, int32_t* assign) {
    SBEV_REQUIRE(L >= 0 && B >= 0 && Q >= 0 && Gmax >= 0, "sbev_head_assign: bad sizes L=%d B=%d Q=%d Gmax=%d", L, B, Q, Gmax);
    if ((long long)L * B * Q == 0) return SBEV_OK;
    SBEV_REQUIRE(assign && gt_counts && (cost || Gmax == 0), "sbev_head_assign: null pointer");
    for (int b = 0; b < B; ++b) SBEV_REQUIRE(gt_counts[b] >= 0 && gt_counts[b] <= Gmax, "sbev_head_assign: gt_counts[%d] = %d not in 0..%d", b, gt_counts[b], Gmax);
    for (int lb = 0; lb < L * B; ++lb) {
        const int st = lsa_solve(cost + (int64_t)lb * Q * Gmax, Gmax, Q, gt_counts[lb % B], assign + (int64_t)lb * Q, "sbev_head_assign");
        if (st != SBEV_OK) return st;
    }
    return SBEV_OK;
}

extern "C" int64_t sbev_head_set_loss_workspace(int B, int rows) {
    if (B < 0 || rows < 0) return -1;
    return (int64_t)blocks_of((long long)B * rows, 256) * 2 * sizeof(float);      // per layer
}

extern "C" int sbev_head_set_loss(const float* cls_scores, const float* bbox_preds, int64_t ld_rows, const int32_t* codes,
                                  int64_t code_layer_stride, const float* gt_boxes, const int32_t* gt_labels, const int32_t* gt_offsets,
                                  const float* code_weights, const float* avg_factors, float w_focal, float alpha, float gamma,
                                  float w_l1, float scale, int L, int B, int rows, int num_classes, float* loss, float* loss_finite,
                                  float* grad_cls, float* grad_bbox, float* workspace, sbev_stream_t stream) {
    SBEV_REQUIRE(L >= 0 && L <= 65535 && B >= 0 && rows >= 0 && num_classes >= 1 && ld_rows >= rows && ld_rows <= 0x7fffffffLL,
                 "sbev_head_set_loss: bad sizes L=%d B=%d rows=%d NC=%d ld_rows=%lld", L, B, rows, num_classes, (long long)ld_rows);
    SBEV_REQUIRE(code_layer_stride == 0 || code_layer_stride >= (int64_t)B * rows, "sbev_head_set_loss: code_layer_stride %lld", (long long)code_layer_stride);
    SBEV_REQUIRE((long long)B * rows <= 0x7fffffffLL / (num_classes > 10 ? num_classes : 10), "sbev_head_set_loss: too many rows");
    if (L == 0) return SBEV_OK;
    SBEV_REQUIRE(loss && loss_finite && avg_factors, "sbev_head_set_loss: null pointer");
    const int nblk = (int)blocks_of((long long)B * rows, 256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nblk > 0) {
        SBEV_REQUIRE(cls_scores && bbox_preds && codes && gt_offsets && code_weights && grad_cls && grad_bbox && workspace,
                     "sbev_head_set_loss: null pointer");
        // codes >= 0 index the ground truth: an empty batch may pass null boxes / labels only because its offsets admit no such code
        LossArgs a{cls_scores, bbox_preds, codes, gt_boxes, gt_labels, gt_offsets, code_weights, avg_factors, grad_cls, grad_bbox, workspace,
                   L, B, rows, num_classes, (int)ld_rows, nblk, (long long)code_layer_stride, w_focal, alpha, gamma, w_l1, scale};
        hipLaunchKernelGGL(set_loss_kernel, dim3(nblk, L), dim3(256), 0, s, a);
        const int st = sbev::check_launch("sbev_head_set_loss");
        if (st != SBEV_OK) return st;
    }
    FinishArgs f{workspace, avg_factors, loss, loss_finite, L, nblk, w_focal, w_l1, scale};
    hipLaunchKernelGGL(set_loss_finish_kernel, dim3(blocks_of(2LL * L, 64)), dim3(64), 0, s, f);
    return sbev::check_launch("sbev_head_set_loss");
}
