// The training head's linear sum assignment on the device: head_train.hip's host solver (lsa_rows: shortest augmenting paths with
// dual variables, Jonker-Volgenant as restated by Crouse 2016) restated in parallel, step for step, so that the table it returns is
// the host's table BIT FOR BIT, ties included -- and the training step needs no device -> host copy and no synchronisation.
//
//   head_assign_kernel<LDS>   one workgroup per problem (layer l, sample b); the sample's count is read from the device gt_offsets
//
// What makes the tables equal:
//   * the same transposition as lsa_solve: Q <= n assigns the queries (rows) to the boxes (columns), Q > n the boxes to the queries;
//   * the reduced cost r = ((min_val + c) - u[i]) - v[j] in fp64 in the host's order, duals updated by additions and subtractions only
//     (this file is built with -ffp-contract=off like head_train.hip, though there is no product for a contraction to fuse);
//   * the host scans the `remaining` position list in order and keeps a running (lowest, index): the result is the minimum, among equal
//     minima the LAST free column in scan order if any is free, otherwise the FIRST.  As an order-free combine of keys
//     (value, free, position): lower value wins; at equal value free beats taken; both free, the larger position; both taken, the
//     smaller.  Key::rank folds the last three into one integer, so every lane's strided share of the positions and any reduction tree
//     pick the position the host's serial scan picks;
//   * the swap-removal remaining[index] = remaining[--n_rem] is the host's, so the position list evolves identically.
//
// Synchronisation: ONE barrier per Dijkstra step.  Position `it` of the list belongs to lane it % kThreads: that lane scans it, and when
// it is the chosen one that same lane does the swap-removal, so its next scan reads its own write.  Everything else a lane reads was
// written before the previous barrier.  The per-wave partial keys alternate between two LDS slots by step parity, so a fast wave's next
// write never lands on a slot a slow wave is still reading.  The chosen key comes back from LDS identical on every lane and is moved to
// SGPRs (readfirstlane), so the loop control is scalar and every barrier is reached by every lane.
//
// Every loop is bounded by the SIZES: the Dijkstra loop by nc (one column leaves the list per step), the walk-back by nr, with the
// indices it follows range-checked.  A problem that leaves a bound without a result is infeasible: status 1, its row all -1.
//
// State per problem: shortest, v (fp64), path, row4col, remaining (int32), SC (byte) per column = 29 bytes, u (fp64), col4row (int32),
// SR (byte) per row = 13 bytes.  It lives in LDS while the worst case of (Q, Gmax) fits kStateBytes -- the static per-workgroup limit
// the file is compiled with (64 KiB) less the reduction slots -- and otherwise in a per-problem slice of the caller's workspace: the
// same code over two address spaces (solve() is inlined into both instantiations).
#include <limits>

#include "sbev_common.hpp"

namespace {

// Four waves and one LDS exchange of the partial keys per step.  Measured against a single wave (no exchange) on one MI355X at Q = 900,
// 6 layers: 0.18 ms against 0.43 ms per launch at 1 x 40 boxes, 1.17 ms against 2.79 ms at 2 x 200.
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / sbev::kWave;
constexpr long long kLdsLimit = 64 * 1024;        // static LDS a workgroup may declare; NOT the CU's 160 KiB
constexpr long long kLdsFixed = 512;              // the reduction slots, the failure word and the block-wide OR's slots
constexpr long long kStateBytes = kLdsLimit - kLdsFixed;

// bytes of one problem's state for nc columns and nr <= nc rows (the carve() layout, each array on its natural alignment)
constexpr long long state_bytes(long long nc, long long nr) { return ((29 * nc + 13 * nr) + 15) / 16 * 16; }

struct State {
    double *shortest, *v, *u;
    int *path, *row4col, *remaining, *col4row;
    unsigned char *SC, *SR;
};

__device__ __forceinline__ State carve(char* base, int nc, int nr) {
    State s;
    size_t o = 0;
    s.shortest = reinterpret_cast<double*>(base + o); o += (size_t)nc * 8;
    s.v = reinterpret_cast<double*>(base + o); o += (size_t)nc * 8;
    s.u = reinterpret_cast<double*>(base + o); o += (size_t)nr * 8;
    s.path = reinterpret_cast<int*>(base + o); o += (size_t)nc * 4;
    s.row4col = reinterpret_cast<int*>(base + o); o += (size_t)nc * 4;
    s.remaining = reinterpret_cast<int*>(base + o); o += (size_t)nc * 4;
    s.col4row = reinterpret_cast<int*>(base + o); o += (size_t)nr * 4;
    s.SC = reinterpret_cast<unsigned char*>(base + o); o += (size_t)nc;
    s.SR = reinterpret_cast<unsigned char*>(base + o);
    return s;
}

// (value, free, position) of the host's scan with the column itself; j < 0: no position seen
struct Key {
    double v;
    int rank;      // free: position; taken: -1 - position.  At equal value the larger rank wins (see the file comment)
    int j;
};

// selects field by field: a Key stays in registers
__device__ __forceinline__ Key better(const Key a, const Key b) {
    const bool take_b = a.j < 0 || (b.j >= 0 && (b.v < a.v || (b.v == a.v && b.rank > a.rank)));
    Key r;
    r.v = take_b ? b.v : a.v;
    r.rank = take_b ? b.rank : a.rank;
    r.j = take_b ? b.j : a.j;
    return r;
}

__device__ __forceinline__ Key wave_best(Key k) {
#pragma unroll
    for (int m = 1; m < sbev::kWave; m <<= 1) {
        Key o;
        o.v = __shfl_xor(k.v, m);
        o.rank = __shfl_xor(k.rank, m);
        o.j = __shfl_xor(k.j, m);
        k = better(k, o);
    }
    return k;
}

__device__ __forceinline__ double uniform(double x) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = __builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

struct Slots {          // the LDS every instantiation declares
    Key red[2][kWaves];
    int failed;
};
static_assert(sizeof(Slots) <= kLdsFixed, "the fixed LDS share");

// lsa_rows for nr <= nc with at(i, j) = src[i * si + j * sj]; false: infeasible.  For Q > n a box's row is read across the queries with
// stride Gmax straight from the [Q, Gmax] block (it sits in L2: 144 KB at 900 x 40): a transposed copy staged into a workspace during
// the finiteness pass was measured and bought nothing (0.186 ms against 0.184 ms, 1.195 ms against 1.170 ms).  Called by every lane of the workgroup, after a barrier
// that follows the caller's last write of anything read here.
__device__ __forceinline__ bool solve(const State& s, Slots& lds, int nr, int nc, const float* src, long long si, long long sj) {
    const int tid = threadIdx.x, lane = tid & (sbev::kWave - 1), wave = tid / sbev::kWave;
    const double inf = std::numeric_limits<double>::infinity();
    for (int j = tid; j < nc; j += kThreads) {
        s.v[j] = 0.0;
        s.path[j] = -1;
        s.row4col[j] = -1;
        s.remaining[j] = nc - j - 1;
        s.SC[j] = 0;
        s.shortest[j] = inf;
    }
    for (int r = tid; r < nr; r += kThreads) {
        s.u[r] = 0.0;
        s.col4row[r] = -1;
        s.SR[r] = 0;
    }
    if (tid == 0) lds.failed = 0;
    __syncthreads();
    bool ok = true;
    for (int cur = 0; cur < nr && ok; ++cur) {
        double min_val = 0.0;
        int i = cur, sink = -1, n_rem = nc;
        for (int step = 0; step < nc && sink < 0; ++step) {
            if (tid == 0) s.SR[i] = 1;
            const double ui = s.u[i];
            const float* row = src + (long long)i * si;
            Key k{inf, 0, -1};
            for (int it = tid; it < n_rem; it += kThreads) {
                const int j = s.remaining[it];
                const double r = ((min_val + (double)row[(long long)j * sj]) - ui) - s.v[j];
                double sh = s.shortest[j];
                if (r < sh) {
                    s.path[j] = i;
                    s.shortest[j] = r;
                    sh = r;
                }
                const Key c{sh, s.row4col[j] == -1 ? it : -1 - it, j};
                k = better(k, c);
            }
            k = wave_best(k);
            Key* red = lds.red[step & 1];
            if (lane == 0) {
                red[wave].v = k.v;
                red[wave].rank = k.rank;
                red[wave].j = k.j;
            }
            __syncthreads();
            k = Key{red[0].v, red[0].rank, red[0].j};
#pragma unroll
            for (int w = 1; w < kWaves; ++w) k = better(k, Key{red[w].v, red[w].rank, red[w].j});
            const int j = __builtin_amdgcn_readfirstlane(k.j), rank = __builtin_amdgcn_readfirstlane(k.rank);
            min_val = uniform(k.v);
            if (j < 0 || min_val == inf) break;                 // nothing reachable: sink stays -1
            const bool is_free = rank >= 0;
            const int index = is_free ? rank : -1 - rank;
            --n_rem;
            if (index % kThreads == tid) {                      // the lane that scans this position (see the file comment)
                s.SC[j] = 1;
                s.remaining[index] = s.remaining[n_rem];
            }
            if (is_free) sink = j;
            else i = __builtin_amdgcn_readfirstlane(s.row4col[j]);
        }
        if (sink < 0) {
            ok = false;
            break;
        }
        __syncthreads();                                        // SC, shortest and path of the last step
        for (int r = tid; r < nr; r += kThreads) {
            if (r == cur) s.u[r] += min_val;
            else if (s.SR[r]) s.u[r] += min_val - s.shortest[s.col4row[r]];
        }
        for (int j = tid; j < nc; j += kThreads)
            if (s.SC[j]) s.v[j] -= min_val - s.shortest[j];
        __syncthreads();                                        // the dual updates have read col4row, SR, SC, shortest
        if (tid == 0) {                                         // augment along the path back to cur: at most one hop per row
            int j = sink;
            bool done = false;
            for (int k = 0; k < nr; ++k) {
                if (j < 0 || j >= nc) break;
                const int r = s.path[j];
                if (r < 0 || r >= nr) break;
                s.row4col[j] = r;
                const int t = s.col4row[r];
                s.col4row[r] = j;
                j = t;
                if (r == cur) {
                    done = true;
                    break;
                }
            }
            if (!done) lds.failed = 1;
        }
        for (int j = tid; j < nc; j += kThreads) {              // the next augmentation's start
            s.remaining[j] = nc - j - 1;
            s.SC[j] = 0;
            s.shortest[j] = inf;
        }
        for (int r = tid; r < nr; r += kThreads) s.SR[r] = 0;
        __syncthreads();
        ok = __builtin_amdgcn_readfirstlane(lds.failed) == 0;
    }
    return ok;
}

struct AssignArgs {
    const float* cost;         // [L, B, Q, Gmax]
    const int* gt_offsets;     // [B + 1]
    int* assign;               // [L, B, Q]
    int* status;               // [L * B] or null
    char* state;               // !LDS: slices of `slice` bytes, one per problem
    long long slice;
    int B, Q, Gmax;
};

template <bool LDS>
__global__ __launch_bounds__(kThreads) void head_assign_kernel(const AssignArgs a) {
    __shared__ Slots lds;
    const int lb = blockIdx.x, tid = threadIdx.x, b = lb % a.B;
    int n = a.gt_offsets[b + 1] - a.gt_offsets[b];
    bool bad = n < 0 || n > a.Gmax;                             // the host cannot look at the device's counts: clamp, and flag the problem
    n = n < 0 ? 0 : (n > a.Gmax ? a.Gmax : n);
    int* out = a.assign + (long long)lb * a.Q;
    if (n == 0 || bad) {                                        // uniform, before the first barrier
        for (int q = tid; q < a.Q; q += kThreads) out[q] = -1;
        if (tid == 0 && a.status) a.status[lb] = bad ? 1 : 0;
        return;
    }
    const int block = a.Q * a.Gmax;
    const float* cost = a.cost + (long long)lb * block;
    const bool rows_are_queries = a.Q <= n;                     // lsa_solve's n_rows <= n_cols
    int nonfinite = 0;
    for (long long e = tid; e < block; e += kThreads) {         // the Q x n block only: padding columns are not read
        if ((int)e % a.Gmax >= n) continue;
        nonfinite |= !(fabsf(cost[e]) <= std::numeric_limits<float>::max());
    }
    bad = __syncthreads_or(nonfinite) != 0;
    bool ok = !bad;
    State s{};
    if (ok) {                                                   // uniform
        char* base;
        if constexpr (LDS) {
            __shared__ __attribute__((aligned(16))) char state[kStateBytes];
            base = state;
        } else {
            base = a.state + (long long)lb * a.slice;
        }
        if (rows_are_queries) {
            s = carve(base, n, a.Q);
            ok = solve(s, lds, a.Q, n, cost, a.Gmax, 1);
        } else {
            s = carve(base, a.Q, n);
            ok = solve(s, lds, n, a.Q, cost, 1, a.Gmax);
        }
    }
    // one owner per element: query q's box is its column (rows are queries) or the row that holds column q
    for (int q = tid; q < a.Q; q += kThreads) out[q] = !ok ? -1 : (rows_are_queries ? s.col4row[q] : s.row4col[q]);
    if (tid == 0 && a.status) a.status[lb] = ok ? 0 : 1;
}

// Q * Gmax fits an int: the kernel indexes a problem's block with 32-bit arithmetic
bool sizes_ok(int L, int B, int Q, int Gmax) {
    return L >= 0 && B >= 0 && Q >= 0 && Gmax >= 0 && Q <= 0x7fff && (long long)Q * Gmax <= 0x7fffffffLL;
}

int plan(int Q, int Gmax) {
    const long long nc = Q > Gmax ? Q : Gmax, nr = Q > Gmax ? Gmax : Q;
    return state_bytes(nc, nr) <= kStateBytes ? 0 : 1;
}

long long slice_bytes(int Q, int Gmax) {
    const long long nc = Q > Gmax ? Q : Gmax, nr = Q > Gmax ? Gmax : Q;
    return plan(Q, Gmax) == 1 ? state_bytes(nc, nr) : 0;
}

}  // namespace

extern "C" int64_t sbev_head_assign_device_workspace(int L, int B, int Q, int Gmax) {
    if (!sizes_ok(L, B, Q, Gmax)) return -1;
    return (long long)L * B * slice_bytes(Q, Gmax);
}

extern "C" int sbev_head_assign_device_plan(int Q, int Gmax) {
    if (!sizes_ok(0, 0, Q, Gmax)) return -1;
    return plan(Q, Gmax);
}

extern "C" int sbev_head_assign_device(const float* cost, const int32_t* gt_offsets, int L, int B, int Q, int Gmax, int32_t* assign,
                                       int32_t* status, void* workspace, sbev_stream_t stream) {
    SBEV_REQUIRE(sizes_ok(L, B, Q, Gmax), "sbev_head_assign_device: bad sizes L=%d B=%d Q=%d Gmax=%d (Q <= 32767)", L, B, Q, Gmax);
    if ((long long)L * B * Q == 0) return SBEV_OK;
    SBEV_REQUIRE((long long)L * B <= 0x7fffffffLL, "sbev_head_assign_device: too many problems (L=%d B=%d)", L, B);
    SBEV_REQUIRE(assign != nullptr, "sbev_head_assign_device: null assign");
    SBEV_REQUIRE(gt_offsets != nullptr, "sbev_head_assign_device: null gt_offsets");
    SBEV_REQUIRE(cost != nullptr || Gmax == 0, "sbev_head_assign_device: null cost");
    SBEV_REQUIRE(workspace != nullptr || sbev_head_assign_device_workspace(L, B, Q, Gmax) == 0, "sbev_head_assign_device: null workspace");
    AssignArgs a{cost, gt_offsets, assign, status, static_cast<char*>(workspace), slice_bytes(Q, Gmax), B, Q, Gmax};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (plan(Q, Gmax) == 0) hipLaunchKernelGGL(head_assign_kernel<true>, dim3((unsigned)(L * B)), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(head_assign_kernel<false>, dim3((unsigned)(L * B)), dim3(kThreads), 0, s, a);
    return sbev::check_launch("sbev_head_assign_device");
}
