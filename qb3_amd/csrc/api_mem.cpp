// qb3_amd/csrc/api_mem.cpp -- device memory and host <-> device copies of the C ABI: the pool released device buffers wait in,
// DevBuf, the waits (wait_stream, fetch_small), upload / download of pageable host memory through the pinned ring, and the
// three streams of a pipelined host call (Pipe).
#include <chrono>
#include <mutex>
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

// ---------------------------------------------------------------- device buffers owned by a handle
// Device buffers of destroyed handles wait in a small per-process pool for the next handle: a caller that opens, decodes and
// closes a container per tile (the reference's calling pattern) would otherwise pay tens of milliseconds of hipMalloc / hipFree
// around a fraction of a millisecond of kernels.  Bounded (POOL_ITEMS buffers, POOL_BYTES bytes); qb3x_trim() empties it.
struct DevPool {
    struct Item { void *p; size_t cap; int dev; };
    static constexpr size_t POOL_ITEMS = 24;
    const size_t POOL_BYTES = [] { const char *e = getenv("QB3_POOL_MB"); return (e && e[0] ? (size_t)strtoull(e, nullptr, 10) : (size_t)3072) << 20; }();   // (0: nothing is kept)
    std::mutex mu;
    std::vector<Item> items;
    size_t bytes = 0;
    void *take(size_t n, int dev, size_t *cap) {           // the smallest pooled buffer of this device that holds n and is not more than twice that
        std::lock_guard<std::mutex> l(mu);
        size_t best = items.size();
        for (size_t i = 0; i < items.size(); i++)
            if (items[i].dev == dev && items[i].cap >= n && items[i].cap / 2 <= n && (best == items.size() || items[i].cap < items[best].cap)) best = i;
        if (best == items.size()) return nullptr;
        void *p = items[best].p;
        *cap = items[best].cap;
        bytes -= items[best].cap;
        items.erase(items.begin() + (long)best);
        return p;
    }
    bool give(void *p, size_t cap, int dev) {
        std::lock_guard<std::mutex> l(mu);
        if (items.size() >= POOL_ITEMS || bytes + cap > POOL_BYTES) return false;
        items.push_back({p, cap, dev});
        bytes += cap;
        return true;
    }
    void trim() {
        std::vector<Item> out;
        { std::lock_guard<std::mutex> l(mu); out.swap(items); bytes = 0; }
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (auto &it : out) { (void)hipSetDevice(it.dev); (void)hipFree(it.p); }
        (void)hipSetDevice(cur);
    }
};
static DevPool &dev_pool() { static DevPool *g = new DevPool(); return *g; }      // (never destroyed: the HIP runtime may be gone before static destructors run)

bool DevBuf::ensure(size_t n) {
    if (n <= cap) return true;
    release();
    (void)hipGetDevice(&dev);
    try {
        if ((p = dev_pool().take(n, dev, &cap)) != nullptr) return true;
    } catch (...) { p = nullptr; }
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {                              // out of memory with buffers idle in the pool: give them back and try once more
        (void)hipGetLastError();
        dev_pool().trim();
        e = hipMalloc(&p, n);
    }
    if (e != hipSuccess) { set_error("hipMalloc", (int)e); p = nullptr; cap = 0; return false; }
    cap = n;
    return true;
}
// hipFree waits for the device; a buffer that goes to the pool instead may be handed to another handle on another stream
// at once, so the same wait comes first -- unless the caller has just made it (`idle`: a handle's buffers go one after
// the other).  An error return in the middle of a call leaves kernels in flight; they end here, not in the next owner.
void DevBuf::release(bool idle) {
    if (p) {
        if (!idle) (void)hipDeviceSynchronize();
        bool kept = false;
        try { kept = dev_pool().give(p, cap, dev); } catch (...) { kept = false; }
        if (!kept) (void)hipFree(p);
    }
    p = nullptr; cap = 0;
}
void qb3api::release_all(std::initializer_list<DevBuf *> bufs) {
    bool any = false;
    for (DevBuf *b : bufs) any = any || b->p != nullptr;
    if (any) (void)hipDeviceSynchronize();
    for (DevBuf *b : bufs) b->release(true);
}
// returns the device buffers that destroyed handles left in the library's pool to the runtime
QB3_API void qb3x_trim(void) { try { dev_pool().trim(); qb3host::ring_trim(); } catch (...) {} }

bool qb3api::device_ok() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { set_error("no usable HIP device (the block codec has no CPU fallback)", (int)e); return false; }
    return true;
}

// Waiting for a stream whose work is short: the runtime's blocking wait costs tens of microseconds to wake up, a kernel
// sequence of this library takes a few hundred.  Poll for a bounded time first.
hipError_t qb3api::wait_stream(hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 0;; i++) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if ((i & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(4)) break;
    }
    return hipStreamSynchronize(st);
}
// A few result bytes from the device, then the wait: through pinned memory of the calling thread (a copy into pageable
// memory goes through the runtime's staging path)
hipError_t qb3api::fetch_small(void *dst, const void *d_src, size_t n, hipStream_t st) {
    static thread_local void *pinned = nullptr;
    if (!pinned && hipHostMalloc(&pinned, 1024, hipHostMallocDefault) != hipSuccess) pinned = nullptr;
    if (!pinned || n > 1024) {
        hipError_t e = hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    }
    hipError_t e = hipMemcpyAsync(pinned, d_src, n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = wait_stream(st);
    if (e == hipSuccess) memcpy(dst, pinned, n);
    return e;
}

// ---------------------------------------------------------------- host <-> device copies of the host-pointer API
static void parallel_memcpy(uint8_t *dst, const uint8_t *src, size_t n) {
    try { qb3host::CopyPool::get().copy(dst, src, n); }
    catch (...) { memcpy(dst, src, n); }                    // (a pool that cannot be had: the caller's thread copies)
}
// host -> device; returns once the host bytes have been consumed (the last slices may still be on the link)
bool qb3api::upload(Stager &sg, void *d_dst, const void *h_src, size_t bytes, hipStream_t st) {
    if (bytes < Stager::MIN_BYTES || !sg.init()) {
        hipError_t e = hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { set_error("upload", (int)e); return false; }
        return true;
    }
    size_t i = 0;
    for (size_t off = 0; off < bytes; off += Stager::SLICE, i++) {
        const size_t n = std::min(Stager::SLICE, bytes - off);
        if (i >= Stager::NSLOT && hipEventSynchronize(sg.ev(i)) != hipSuccess) { set_error("upload: slot wait", 0); return false; }
        parallel_memcpy(sg.slot(i), (const uint8_t *)h_src + off, n);
        hipError_t e = hipMemcpyAsync((uint8_t *)d_dst + off, sg.slot(i), n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(sg.ev(i), st);
        if (e != hipSuccess) { set_error("upload", (int)e); return false; }
    }
    return true;
}
// device -> host; returns when the bytes are in h_dst (synchronises the stream)
bool qb3api::download(Stager &sg, void *h_dst, const void *d_src, size_t bytes, hipStream_t st) {
    if (bytes < Stager::MIN_BYTES || !sg.init()) {
        hipError_t e = hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { set_error("download", (int)e); return false; }
        return true;
    }
    const size_t nsl = (bytes + Stager::SLICE - 1) / Stager::SLICE;
    auto issue = [&](size_t i) -> hipError_t {
        const size_t off = i * Stager::SLICE, n = std::min(Stager::SLICE, bytes - off);
        hipError_t e = hipMemcpyAsync(sg.slot(i), (const uint8_t *)d_src + off, n, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipEventRecord(sg.ev(i), st) : e;
    };
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < std::min(nsl, (size_t)Stager::NSLOT) && e == hipSuccess; i++) e = issue(i);
    for (size_t i = 0; i < nsl && e == hipSuccess; i++) {
        e = hipEventSynchronize(sg.ev(i));
        if (e != hipSuccess) break;
        const size_t off = i * Stager::SLICE, n = std::min(Stager::SLICE, bytes - off);
        parallel_memcpy((uint8_t *)h_dst + off, sg.slot(i), n);
        if (i + Stager::NSLOT < nsl) e = issue(i + Stager::NSLOT);
    }
    if (e != hipSuccess) { set_error("download", (int)e); return false; }
    return true;
}

// ---------------------------------------------------------------- the streams and events of a pipelined host call
bool Pipe::init() {
    if (up) return true;
    if (failed) return false;
    if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&k, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&dn, hipStreamNonBlocking) != hipSuccess || hipHostMalloc((void **)&words, 8 * WORDS, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); release(); failed = true; return false;
    }
    return true;
}
bool Pipe::events(size_t n) {
    while (ev.size() < n) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
        ev.push_back(e);
    }
    return true;
}
void Pipe::release() {
    for (auto e : ev) (void)hipEventDestroy(e);
    ev.clear();
    if (up) (void)hipStreamDestroy(up);
    if (k) (void)hipStreamDestroy(k);
    if (dn) (void)hipStreamDestroy(dn);
    if (words) (void)hipHostFree(words);
    up = k = dn = nullptr; words = nullptr;
}
