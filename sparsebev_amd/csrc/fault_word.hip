// The decoder's sticky fault word (host only, no kernel here): 64 bytes of pinned host memory mapped into the device, one per process (a
// process drives one GPU: one process per GPU is the deployment model; with several devices the word is shared -- a fault on any of them
// stops pair mode everywhere).  A hand-off that times out inside a launch -- the tail chain's pair mode (row_chain.hip), the
// out-projection's in-launch fold (gemm_bf16s.hip) -- bumps it with a system-scope atomic, so sbev_decoder_forward / sbev_graph_launch see
// the fault WITHOUT synchronising the device and refuse with SBEV_EFAULT until it is acknowledged.  Each of those kernel files keeps its
// own __device__ pointer and timeout counter (no relocatable device code: a symbol lives with its kernel) and exports two functions --
// install this device address, read your counter; this unit owns the word, installs it on every device, and keeps the acknowledged count.
#include "sbev_common.hpp"
#include <mutex>
#include <atomic>

namespace {

std::atomic<unsigned> g_fault_acked{0};
std::atomic<int> g_fault_warned{0};

// nullptr when the allocation fails (the device-side counters still work)
volatile unsigned* fault_word_host() {
    // NOT a function-local static initialised by the first call: that call may run where hipHostMalloc is illegal (a caller's stream
    // capture around its first decoder call) and the failure would be cached for the life of the process -- a failed
    // attempt is retried by the next call; sbev_init() (called when the Python binding loads the library) makes the first attempt early
    static std::atomic<volatile unsigned*> word{nullptr};
    static std::mutex mu;
    volatile unsigned* w = word.load(std::memory_order_acquire);
    if (w) return w;
    std::lock_guard<std::mutex> lk(mu);
    w = word.load(std::memory_order_acquire);
    if (w) return w;
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess || !h) {
        const hipError_t e = hipGetLastError();
        if (g_fault_warned.exchange(1) == 0) {
            sbev::set_error("pair-mode fault word: hipHostMalloc failed (%s) -- pair mode stays off until a later call succeeds (stream capture active? call sbev_init() first)",
                            hipGetErrorString(e));
            fprintf(stderr, "sparsebev_amd: %s\n", sbev_last_error());
        }
        return nullptr;
    }
    *static_cast<volatile unsigned*>(h) = 0u;
    word.store(static_cast<volatile unsigned*>(h), std::memory_order_release);
    return static_cast<volatile unsigned*>(h);
}

// the word's device address into every kernel file that reports into it; once per device, before the first pair-mode launch on it
bool fault_word_install() {
    static std::atomic<int> done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (done[dev & 63].load(std::memory_order_acquire)) return true;
    volatile unsigned* h = fault_word_host();
    if (!h) return false;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<unsigned*>(h), 0) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (!sbev::chain_pair_install(d) || !sbev::out_fold_install(d)) { (void)hipGetLastError(); return false; }
    done[dev & 63].store(1, std::memory_order_release);
    return true;
}

}  // namespace

namespace sbev {

bool chain_fault_word_ready() { return fault_word_install(); }

// Install the fault word for the current device NOW (hipHostMalloc + hipMemcpyToSymbol: neither is legal under stream capture, and a
// caller's first pair-mode launch may be a captured one): sbev_decoder_workspace_bytes calls this, which every caller runs before its
// first forward / capture.  Quiet without a device.
void chain_pair_prepare() {
    if (chain_pair_enabled()) (void)fault_word_install();
}

// hand-offs that timed out and were not acknowledged yet (host memory: no device synchronisation)
unsigned chain_pair_faults_pending() {
    volatile unsigned* h = fault_word_host();
    return h ? *h - g_fault_acked.load(std::memory_order_relaxed) : 0u;
}

}  // namespace sbev

// partners that did not show up within the poll bound since the library was loaded (0 unless the GPU was shared with something
// that kept half of a pair from being scheduled for about a second); synchronises the device
extern "C" int64_t sbev_decoder_chain_pair_timeouts(void) {
    const long long v = sbev::chain_pair_timeouts();
    if (v < 0) return -1;
    const long long f = sbev::out_fold_timeouts();          // (+ row tiles of the out-projection's in-launch fold that never completed)
    if (f < 0) return -1;
    return (int64_t)v + f;
}

// the sticky fault word: timed-out hand-offs since the last acknowledgement, read from pinned host memory (NO synchronisation; a fault
// becomes visible once the faulting launch has run, ~1 s after its partner went missing)
extern "C" int64_t sbev_decoder_chain_pair_faults(void) { return (int64_t)sbev::chain_pair_faults_pending(); }
// One-time per-device setup that must not happen inside a caller's stream capture: the host-mapped fault word (hipHostMalloc +
// hipMemcpyToSymbol).  The Python binding calls it when it loads the library on a GPU box; C callers call it once per device before their
// first capture (sbev_decoder_workspace_bytes still does the same lazily, and a failed attempt is retried by later calls).
extern "C" int sbev_init(void) {
    if (!sbev::chain_pair_enabled()) return SBEV_OK;
    if (!fault_word_install()) {
        sbev::set_error("sbev_init: could not install the pair-mode fault word on the current device (pair mode stays off until a later attempt succeeds)");
        return SBEV_ELAUNCH;
    }
    return SBEV_OK;
}
// acknowledge them (the caller has dealt with the invalid step): sbev_decoder_forward accepts calls again.  Returns how many there were.
extern "C" int64_t sbev_decoder_chain_pair_faults_ack(void) {
    volatile unsigned* h = fault_word_host();
    if (!h) return 0;
    const unsigned now = *h;
    return (int64_t)(now - g_fault_acked.exchange(now));
}
