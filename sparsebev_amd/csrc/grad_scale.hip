// The scaled domain of the dense backward passes (fpn_bwd.hip: sbev_fpn_backward, resnet_bwd.hip: sbev_resnet_backward), once.  Every
// gradient operand goes to the matrix core as ONE fp16 value: amax = max |g| over the output gradients is found on the device and the pair
// (2^e, 2^-e) with 2^e amax in [2^W, 2^(W+1)), W = SBEV_FPN_GRAD_WINDOW_LOG2 = SBEV_RESNET_GRAD_WINDOW_LOG2, e <= 126, is written to the head
// of the caller's workspace; every consumer reads the pair from there (no host read: the call can be captured).
//
// Workspace head, four 32-bit words: [0] 2^e  [1] 2^-e  (floats)  [2] amax bits  [3] ticket.  Two launches:
//   grad_scale_clear_kernel  the four words back to zero.  A launch of its own, not a memset node: a captured 16-byte memset wrote stale
//                            bytes from the second replay of a graph on; a kernel's stores replay like any other.
//   grad_scale_amax_kernel   integer max of the absolute bit patterns (order-free; a non-finite element wins), the last workgroup (a ticket)
//                            writes the pair.  A zero or non-finite amax gives e = 0: an inf or NaN then travels as it is.
// Nothing is read-modify-written except the amax word (integer max) and the ticket: the pair is bit-reproducible.
#include <algorithm>

#include "sbev_common.hpp"

namespace {

static_assert(SBEV_FPN_GRAD_WINDOW_LOG2 == SBEV_RESNET_GRAD_WINDOW_LOG2, "the neck's and the backbone's gradient windows are one rule");
constexpr int kWindowLog2 = SBEV_FPN_GRAD_WINDOW_LOG2;      // 2^e amax in [2^3, 2^4)
constexpr int kMaxTensors = sbev::kGradScaleMaxTensors;

struct AmaxArgs {
    const void* g[kMaxTensors];
    long long count[kMaxTensors];        // elements (a multiple of 8)
    unsigned* ws;                        // the workspace head
    int n, f32;
};

__global__ __launch_bounds__(64) void grad_scale_clear_kernel(unsigned* ws) {
    if (threadIdx.x < 4) ws[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(256) void grad_scale_amax_kernel(const AmaxArgs a) {
    __shared__ unsigned smax;
    if (threadIdx.x == 0) smax = 0u;
    __syncthreads();
    unsigned m = 0u;
    const long long stride = (long long)gridDim.x * 256, t0 = (long long)blockIdx.x * 256 + threadIdx.x;
    for (int o = 0; o < a.n; ++o) {
        const uint4* p = static_cast<const uint4*>(a.g[o]);
        const long long nv = a.f32 ? a.count[o] / 4 : a.count[o] / 8;
        for (long long i = t0; i < nv; i += stride) {
            const uint4 v = p[i];
            if (a.f32) {
                m = max(m, max(max(v.x & 0x7fffffffu, v.y & 0x7fffffffu), max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
            } else {
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned h = max(w[j] & 0x7fffu, (w[j] >> 16) & 0x7fffu);
                    m = max(m, __float_as_uint((float)__builtin_bit_cast(_Float16, (unsigned short)h)));
                }
            }
        }
    }
    atomicMax(&smax, m);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(a.ws + 2, smax);
        __threadfence();
        const unsigned ticket = atomicAdd(a.ws + 3, 1u);
        if (ticket == gridDim.x - 1) {
            __threadfence();
            const unsigned bits = atomicMax(a.ws + 2, 0u);
            int e = 0;
            if (bits != 0u && bits < 0x7f800000u) e = min(kWindowLog2 - ilogbf(__uint_as_float(bits)), 126);
            a.ws[0] = (unsigned)(127 + e) << 23;
            a.ws[1] = (unsigned)(127 - e) << 23;
        }
    }
}

}  // namespace

int sbev::launch_grad_scale(const char* who, const void* const* grads, const long long* counts, int n, bool f32, void* ws_head, hipStream_t s) {
    SBEV_REQUIRE(n >= 1 && n <= kMaxTensors, "%s: %d gradient tensors (1 .. %d)", who, n, kMaxTensors);
    unsigned* ws = static_cast<unsigned*>(ws_head);
    hipLaunchKernelGGL(grad_scale_clear_kernel, dim3(1), dim3(64), 0, s, ws);
    if (int st = sbev::check_launch(who)) return st;          // the scale words are cleared or nothing else is enqueued
    AmaxArgs a;
    long long most = 0;
    for (int o = 0; o < kMaxTensors; ++o) {
        a.g[o] = o < n ? grads[o] : nullptr;
        a.count[o] = o < n ? counts[o] : 0;
        most = std::max(most, a.count[o]);
    }
    a.ws = ws;
    a.n = n;
    a.f32 = f32;
    const long long blocks = std::min<long long>(1024, std::max<long long>(1, most / (256 * 8 * 4)));
    hipLaunchKernelGGL(grad_scale_amax_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return sbev::check_launch(who);
}
